// Calibration on the device: the reliability counts, NLL and Brier sums of class probabilities against a ground truth, the
// temperature transform of the probabilities, and the NLL of that transform with its first two derivatives in beta = 1 / T.
// The definitions are in include/oct_unet.h (oct_calibration_counts, oct_temperature_apply, oct_temperature_nll) and restated
// in numpy by evaluation/calibration.py; every per-pixel step is one IEEE fp32 operation in class order, none contracted with
// another, logf / expf are OCML's (as in kernels_mc.hpp), and every sum over pixels is fp64.
//
//   calib_counts_k<VC>      probs (B, npix, C) f32, labels (B, npix) u8 -> one partial row per block in the workspace.
//   temperature_nll_k<VC>   the same inputs and K <= 8 betas             -> one partial row per block in the workspace.
//                   grid (G, B): blockIdx.y is the image, the G blocks of an image stride over its items.  The work is
//                   memory-bound and the item is kernels_mc.hpp's: 4 adjacent pixels = VC float4 loads (mc_load4, VC = C in
//                   2..8, chosen by the launcher where every image's base is 16-byte aligned), every cache line used whole; the
//                   pixels behind the last whole item, and every pixel with VC = 0 (any C <= 32, any alignment), take the scalar
//                   path: the same operations in the same order, one class at a time, no arrays.
//                   The histogram of a block lives in LDS (uint64 words, integer atomics: order-free).  A thread keeps the
//                   words of the bin it is in in registers and only flushes them when the bin changes: a confident network puts
//                   nearly every pixel into the last bin, which 256 threads would otherwise fight over three atomics a pixel.
//                   The fp64 sums go thread -> wave (shuffles) -> block (LDS) in a fixed order, and the block stores its row
//                   with plain stores.  No global atomics: nothing depends on the order blocks arrive in.
//   calib_rows_sum_k        adds the G rows of an image into the outputs in a fixed order: a block per image and 64 words, each
//                   wave a quarter of the rows with eight loads in flight, the quarters added in order.
//   temperature_apply_k<VC> probs -> softmax(beta * log p): one launch, grid-stride over items, a pixel owned by one thread (so
//                   the output may be the input).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels_mc.hpp"

namespace oct {

constexpr int kCalThreads = 256;
constexpr int kCalMaxBlocks = 2048;      // as kMcMaxBlocks: 8 blocks per CU over all images; larger inputs stride
constexpr int kCalMaxBins = 64;
constexpr int kCalMaxBetas = 8;
constexpr float kCalEps = 1e-7f;         // FOCAL_EPS of common/custom_losses.py
constexpr float kCalScale = 268435456.f; // 2^28: confidences in fixed point

// blocks per image for `items` items in each of B images
inline unsigned cal_blocks_per_image(int B, size_t items) {
    const size_t want = (items + kCalThreads - 1) / kCalThreads, cap = (size_t)(kCalMaxBlocks / B > 1 ? kCalMaxBlocks / B : 1);
    return (unsigned)(want < 1 ? 1 : want < cap ? want : cap);
}

struct CalArgs {
    const float* probs;              // (B, npix, C)
    const unsigned char* labels;     // (B, npix)
    unsigned long long* ws;          // (B, G, row) 8-byte words
    size_t npix;
    int C, ignore, M;
    int lab4;                        // the labels of an item may be loaded as one uchar4
};

struct CalBetas { float b[kCalMaxBetas]; int K; };

// the sum of v over the block, in every thread: lanes by shuffles, then the four waves in order
__device__ __forceinline__ double cal_block_sum(double v, double* red) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    __syncthreads();                 // red may still be read from the sum before
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

__device__ __forceinline__ float cal_log(float p) { return logf(fmaxf(p, kCalEps)); }

// the labels of pixels px0..px0+3 of an image
__device__ __forceinline__ void cal_labels4(const CalArgs& A, const unsigned char* Y, size_t px0, int (&y)[4]) {
    if (A.lab4) {
        const uchar4 v = *reinterpret_cast<const uchar4*>(Y + px0);
        y[0] = v.x; y[1] = v.y; y[2] = v.z; y[3] = v.w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) y[j] = Y[px0 + j];
    }
}

// ---- reliability counts -----------------------------------------------------------------------------------------------
// what one class adds to a pixel's state: the arg-max as the lowest index of the maximum, p_y, the Brier sum in class order
struct CalPixel {
    float best, py, brier; int bi;
    __device__ __forceinline__ void add(int c, float p, int y) {
#pragma clang fp contract(off)
        if (c == 0 || p > best) { best = p; bi = c; }
        if (c == y) py = p;
        const float d = p - (c == y ? 1.f : 0.f);
        const float t = d * d;
        brier = c == 0 ? t : brier + t;
    }
};

// a thread's sums: fp64 over its pixels, and the histogram words of the bin it is in
struct CalAcc {
    double nll, brier;
    unsigned cnt, bad;
    int bin; unsigned n, ok; unsigned long long sk;
    __device__ __forceinline__ void flush(unsigned long long* hist) {
        if (n) {
            atomicAdd(&hist[3 * bin], (unsigned long long)n);
            atomicAdd(&hist[3 * bin + 1], (unsigned long long)ok);
            atomicAdd(&hist[3 * bin + 2], sk);
        }
        n = ok = 0; sk = 0;
    }
};

__device__ __forceinline__ void cal_finish(const CalArgs& A, const CalPixel& st, int y, CalAcc& acc, unsigned long long* hist) {
#pragma clang fp contract(off)
    if (y == A.ignore) return;
    if (y >= A.C) { ++acc.bad; return; }
    const float conf = fminf(fmaxf(st.best, 0.f), 1.f);
    const unsigned k = (unsigned)floorf(conf * kCalScale);
    const int top = (int)(((unsigned long long)k * (unsigned)A.M) >> 28);
    const int bin = top < A.M - 1 ? top : A.M - 1;
    const float pc = fminf(fmaxf(st.py, kCalEps), 1.0f - kCalEps);
    acc.nll += (double)(-logf(pc));
    acc.brier += (double)st.brier;
    ++acc.cnt;
    if (bin != acc.bin) { acc.flush(hist); acc.bin = bin; }
    ++acc.n; acc.ok += st.bi == y ? 1u : 0u; acc.sk += k;
}

__device__ __forceinline__ void cal_pixel(const CalArgs& A, const float* p, int y, CalAcc& acc, unsigned long long* hist) {
    CalPixel st{0.f, 0.f, 0.f, 0};
    for (int c = 0; c < A.C; ++c) st.add(c, p[c], y);
    cal_finish(A, st, y, acc, hist);
}

// items = ceil(npix / 4) with VC > 0, npix with VC == 0; row = 3 M histogram words, then nll, brier, counted, bad as doubles
template <int VC>
__global__ void __launch_bounds__(kCalThreads) calib_counts_k(const CalArgs A, size_t items) {
    __shared__ unsigned long long hist[3 * kCalMaxBins];
    __shared__ double red[4];
    const int b = blockIdx.y, tid = threadIdx.x, nh = 3 * A.M;
    const float* P = A.probs + (size_t)b * A.npix * A.C;
    const unsigned char* Y = A.labels + (size_t)b * A.npix;
    for (int i = tid; i < nh; i += kCalThreads) hist[i] = 0;
    __syncthreads();
    CalAcc acc{0.0, 0.0, 0u, 0u, 0, 0u, 0u, 0ull};
    const size_t stride = (size_t)gridDim.x * kCalThreads;
    for (size_t it = (size_t)blockIdx.x * kCalThreads + tid; it < items; it += stride) {
        if constexpr (VC == 0) {
            cal_pixel(A, P + it * A.C, Y[it], acc, hist);
        } else {
            const size_t px0 = it * 4;
            if (px0 + 4 > A.npix) {      // the pixels behind the last whole item
                for (size_t px = px0; px < A.npix; ++px) cal_pixel(A, P + px * VC, Y[px], acc, hist);
                continue;
            }
            float pv[4 * VC]; int y[4];
            mc_load4<VC>(P + px0 * VC, pv);
            cal_labels4(A, Y, px0, y);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                CalPixel st{0.f, 0.f, 0.f, 0};
#pragma unroll
                for (int c = 0; c < VC; ++c) st.add(c, pv[j * VC + c], y[j]);
                cal_finish(A, st, y[j], acc, hist);
            }
        }
    }
    acc.flush(hist);
    const double s0 = cal_block_sum(acc.nll, red), s1 = cal_block_sum(acc.brier, red);
    const double s2 = cal_block_sum((double)acc.cnt, red), s3 = cal_block_sum((double)acc.bad, red);   // (the syncs inside order the flushes too)
    unsigned long long* row = A.ws + ((size_t)b * gridDim.x + blockIdx.x) * (size_t)(nh + 4);
    for (int i = tid; i < nh; i += kCalThreads) row[i] = hist[i];
    if (tid == 0) {
        double* d = reinterpret_cast<double*>(row + nh);
        d[0] = s0; d[1] = s1; d[2] = s2; d[3] = s3;
    }
}

// the sum of word i of rows g0..g1-1 in row order; T is the word's type.  Eight loads are issued before the first add: a
// load -> wait -> add loop pays one memory round trip per row
template <class T>
__device__ __forceinline__ T cal_sum_rows(const unsigned long long* rows, int w, int i, int g0, int g1) {
    T s = 0;
    int g = g0;
    for (; g + 8 <= g1; g += 8) {
        T v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = reinterpret_cast<const T*>(rows)[(size_t)(g + u) * w + i];
#pragma unroll
        for (int u = 0; u < 8; ++u) s += v[u];
    }
    for (; g < g1; ++g) s += reinterpret_cast<const T*>(rows)[(size_t)g * w + i];
    return s;
}

// out_u[b][i] = sum over the G rows of image b of word i < nu (uint64), out_d likewise of the nd doubles behind them.  With
// out_tail the last double of a row goes to out_tail[b] and out_d has nd - 1 columns.  Grid (B, ceil((nu + nd) / 64)): a block
// takes 64 words of image blockIdx.x; wave r sums the r-th quarter of the rows in row order, and the four quarters are added in
// order: the order is fixed, so the fp64 sums are reproducible.
__global__ void __launch_bounds__(kCalThreads) calib_rows_sum_k(const unsigned long long* ws, int G, int nu, int nd,
                                                                unsigned long long* out_u, double* out_d, double* out_tail) {
    __shared__ unsigned long long part[4][64];
    const int b = blockIdx.x, w = nu + nd, lane = threadIdx.x & 63, r = threadIdx.x >> 6;
    const int i = blockIdx.y * 64 + lane, q = (G + 3) / 4;
    const int g0 = r * q < G ? r * q : G, g1 = (r + 1) * q < G ? (r + 1) * q : G;
    const unsigned long long* rows = ws + (size_t)b * G * w;
    if (i < w) {
        if (i < nu) part[r][lane] = cal_sum_rows<unsigned long long>(rows, w, i, g0, g1);
        else reinterpret_cast<double*>(part[r])[lane] = cal_sum_rows<double>(rows, w, i, g0, g1);
    }
    __syncthreads();
    if (r != 0 || i >= w) return;
    if (i < nu) {
        out_u[(size_t)b * nu + i] = ((part[0][lane] + part[1][lane]) + part[2][lane]) + part[3][lane];
    } else {
        const double s = ((reinterpret_cast<double*>(part[0])[lane] + reinterpret_cast<double*>(part[1])[lane]) +
                          reinterpret_cast<double*>(part[2])[lane]) + reinterpret_cast<double*>(part[3])[lane];
        const int j = i - nu;
        if (out_tail && j == nd - 1) out_tail[b] = s;
        else out_d[(size_t)b * (out_tail ? nd - 1 : nd) + j] = s;
    }
}

// ---- temperature ------------------------------------------------------------------------------------------------------
// q_c = expf(beta (l_c - L)) / S of one pixel with n classes; lf(c) is l_c = logf(max(p_c, EPS)), put(c, q) takes q_c.  The
// scalar path hands in functions that read memory and recompute l_c (no arrays), the float4 path ones that index registers.
template <class LF, class PUT>
__device__ __forceinline__ void temp_pixel(int n, float beta, LF lf, PUT put) {
#pragma clang fp contract(off)
    float L = 0.f, S = 0.f;
    for (int c = 0; c < n; ++c) { const float l = lf(c); L = c == 0 ? l : fmaxf(L, l); }
    for (int c = 0; c < n; ++c) { const float e = expf(beta * (lf(c) - L)); S = c == 0 ? e : S + e; }
    for (int c = 0; c < n; ++c) put(c, expf(beta * (lf(c) - L)) / S);
}

// items as in calib_counts_k, over all npix pixels of the batch
template <int VC>
__global__ void __launch_bounds__(kCalThreads) temperature_apply_k(const float* in, float* out, size_t npix, int C, float beta,
                                                                   size_t items) {
#pragma clang fp contract(off)
    const size_t stride = (size_t)gridDim.x * kCalThreads;
    auto scalar = [&](size_t px) {
        const float* p = in + px * C; float* q = out + px * C;
        temp_pixel(C, beta, [&](int c) { return cal_log(p[c]); }, [&](int c, float v) { q[c] = v; });   // q[c] is written after p[c] is last read
    };
    for (size_t it = (size_t)blockIdx.x * kCalThreads + threadIdx.x; it < items; it += stride) {
        if constexpr (VC == 0) {
            scalar(it);
        } else {
            const size_t px0 = it * 4;
            if (px0 + 4 > npix) {
                for (size_t px = px0; px < npix; ++px) scalar(px);
                continue;
            }
            float pv[4 * VC];
            mc_load4<VC>(in + px0 * VC, pv);
#pragma unroll
            for (int i = 0; i < 4 * VC; ++i) pv[i] = cal_log(pv[i]);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float L = pv[j * VC], e[VC];
#pragma unroll
                for (int c = 1; c < VC; ++c) L = fmaxf(L, pv[j * VC + c]);
                float S = 0.f;
#pragma unroll
                for (int c = 0; c < VC; ++c) { e[c] = expf(beta * (pv[j * VC + c] - L)); S = c == 0 ? e[c] : S + e[c]; }
#pragma unroll
                for (int c = 0; c < VC; ++c) pv[j * VC + c] = e[c] / S;
            }
            float4* o4 = reinterpret_cast<float4*>(out + px0 * VC);
#pragma unroll
            for (int q = 0; q < VC; ++q) o4[q] = make_float4(pv[4 * q], pv[4 * q + 1], pv[4 * q + 2], pv[4 * q + 3]);
        }
    }
}

// nll, g, h of one pixel with n classes and label y at one beta; lf(c) is l_c, L their maximum, ly = l_y
template <class LF>
__device__ __forceinline__ void temp_nll_terms(int n, float beta, float L, float ly, LF lf, float& nll, float& g, float& h) {
#pragma clang fp contract(off)
    float S = 0.f, m = 0.f, v = 0.f;
    for (int c = 0; c < n; ++c) { const float e = expf(beta * (lf(c) - L)); S = c == 0 ? e : S + e; }
    for (int c = 0; c < n; ++c) {
        const float l = lf(c);
        const float t = (expf(beta * (l - L)) / S) * l;
        m = c == 0 ? t : m + t;
    }
    for (int c = 0; c < n; ++c) {
        const float l = lf(c);
        const float r = l - m;
        const float t = (expf(beta * (l - L)) / S) * (r * r);
        v = c == 0 ? t : v + t;
    }
    nll = logf(S) - beta * (ly - L);
    g = m - ly;
    h = v;
}

struct CalNllAcc { double s[kCalMaxBetas][3]; unsigned cnt; };

// one counted pixel into the thread's sums, for every beta (the loop is unrolled: the sums stay in registers)
template <class LF>
__device__ __forceinline__ void temp_nll_pixel(int n, const CalBetas& bt, LF lf, int y, CalNllAcc& acc) {
    float L = 0.f, ly = 0.f;
    for (int c = 0; c < n; ++c) { const float l = lf(c); L = c == 0 ? l : fmaxf(L, l); if (c == y) ly = l; }
    ++acc.cnt;
#pragma unroll
    for (int k = 0; k < kCalMaxBetas; ++k) {
        if (k < bt.K) {
            float nll, g, h;
            temp_nll_terms(n, bt.b[k], L, ly, lf, nll, g, h);
            acc.s[k][0] += (double)nll; acc.s[k][1] += (double)g; acc.s[k][2] += (double)h;
        }
    }
}

// items as in calib_counts_k; row = K x (nll, g, h), then counted, as doubles
template <int VC>
__global__ void __launch_bounds__(kCalThreads) temperature_nll_k(const CalArgs A, const CalBetas bt, size_t items) {
    __shared__ double red[4];
    const int b = blockIdx.y, tid = threadIdx.x;
    const float* P = A.probs + (size_t)b * A.npix * A.C;
    const unsigned char* Y = A.labels + (size_t)b * A.npix;
    CalNllAcc acc;
#pragma unroll
    for (int k = 0; k < kCalMaxBetas; ++k) acc.s[k][0] = acc.s[k][1] = acc.s[k][2] = 0.0;
    acc.cnt = 0;
    auto scalar = [&](size_t px) {
        const int y = Y[px];
        if (y == A.ignore || y >= A.C) return;
        const float* p = P + px * A.C;
        temp_nll_pixel(A.C, bt, [&](int c) { return cal_log(p[c]); }, y, acc);
    };
    const size_t stride = (size_t)gridDim.x * kCalThreads;
    for (size_t it = (size_t)blockIdx.x * kCalThreads + tid; it < items; it += stride) {
        if constexpr (VC == 0) {
            scalar(it);
        } else {
            const size_t px0 = it * 4;
            if (px0 + 4 > A.npix) {
                for (size_t px = px0; px < A.npix; ++px) scalar(px);
                continue;
            }
            float pv[4 * VC]; int y[4];
            mc_load4<VC>(P + px0 * VC, pv);
            cal_labels4(A, Y, px0, y);
#pragma unroll
            for (int i = 0; i < 4 * VC; ++i) pv[i] = cal_log(pv[i]);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (y[j] == A.ignore || y[j] >= A.C) continue;
                float l[VC];
#pragma unroll
                for (int c = 0; c < VC; ++c) l[c] = pv[j * VC + c];
                // (a function of c over registers: every loop over c in temp_nll_pixel has the constant trip count VC)
                temp_nll_pixel(VC, bt, [&](int c) {
                    float r = l[0];
#pragma unroll
                    for (int i = 1; i < VC; ++i) r = c == i ? l[i] : r;
                    return r;
                }, y[j], acc);
            }
        }
    }
    const int w = 3 * bt.K + 1;
    double* row = reinterpret_cast<double*>(A.ws) + ((size_t)b * gridDim.x + blockIdx.x) * (size_t)w;
#pragma unroll
    for (int k = 0; k < kCalMaxBetas; ++k) {
        if (k < bt.K) {
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const double s = cal_block_sum(acc.s[k][i], red);
                if (tid == 0) row[3 * k + i] = s;
            }
        }
    }
    const double n = cal_block_sum((double)acc.cnt, red);
    if (tid == 0) row[w - 1] = n;
}

}  // namespace oct
