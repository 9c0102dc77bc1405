// Surface-distance metrics on the device: average surface distance and robust (percentile) Hausdorff distance of every
// foreground class of (B,H,W) uint8 class maps, a restatement of google-deepmind/surface-distance's 2D path
// (compute_surface_distances / compute_average_surface_distance / compute_robust_hausdorff) as called by the reference's
// evaluation (evaluation/evaluation.py:207-262).  PARITY UNPINNED: the package is not vendored; the restatement is
// checked against a brute-force pairwise oracle and against scipy (tests/test_surface_distance.py).
//
// Per (image b, class c) and mask m in {gt, pred}, the (H+1) x (W+1) grid of 2x2 cells of the zero-padded mask:
//   code(i,j) = 8 m[i-1,j-1] + 4 m[i-1,j] + 2 m[i,j-1] + m[i,j]; border cell iff code not in {0, 15};
//   contour length by kind: d = sqrt(v^2+h^2)/2 (one corner in or out), h (horizontal edge), v (vertical edge), 2d (saddle).
// Three launches, no device allocation:
//   surf_col_k     one thread per (b, c, m, cell column): cell kinds + nearest border row above/below in the column
//                  (uint16 row distance, 0xFFFF = none in that column); also flags labels >= n_cls.  Its masked
//                  instantiation (an ignore label in the ground truth) drops the cells that touch an ignored pixel.
//   surf_row_k     one block per (b, c, m, cell row): for each border cell of m, the exact nearest border cell of the other
//                  mask -- min over columns of (v*dy)^2 + (h*dx)^2, searched outward from the cell's column and stopped once
//                  (h*dx)^2 alone reaches the best so far (O(dx of the nearest) per cell, O(W) at worst).  fp64 with FMA
//                  contraction off, the same expression scipy's distance_transform_edt evaluates.
//   surf_select_k  one block per (b, c, m): fixed-order length-weighted sum (average distance) and an exact weighted
//                  percentile by an 8-pass radix select on the fp64 bit pattern (distances are >= 0, so the pattern orders
//                  like the value), counting border cells per length kind as integers so the cumulative length
//                  n_d d + n_h h + n_v v + n_2d 2d at every candidate is one fixed expression: deterministic.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace oct {

constexpr unsigned short kSurfNone = 0xFFFF;   // no border cell in this column
constexpr unsigned char kSurfNotBorder = 255;
constexpr int kSurfSelectThreads = 1024;

struct SurfGeom {
    int B, H, W, n_cls;
    int Hc, Wc;          // H + 1, W + 1
    size_t N;            // Hc * Wc cells per (b, c, m)
    size_t KS;           // stride of the kind planes (N rounded up to 16)
};

// code -> length kind: 0 = d, 1 = h, 2 = v, 3 = 2d, 255 = not a border cell
__device__ inline unsigned char surf_kind(int code) {
    switch (code) {
        case 0: case 15: return kSurfNotBorder;
        case 3: case 12: return 1;
        case 5: case 10: return 2;
        case 6: case 9: return 3;
        default: return 0;
    }
}

// plane index of (b, c, m): ((b * (n_cls-1) + c-1) * 2 + m)
// kMasked (oct_surface_distances_masked): a ground-truth pixel equal to `ignore` (a value in n_cls..255) is unknown.  A
// cell with such a pixel among its in-image pixels is no border cell, in the gt plane and in the pred plane alike -- the
// pred planes read the ground-truth bytes beside their own -- and the label check passes that value in the ground truth.
template <bool kMasked>
__global__ void __launch_bounds__(256) surf_col_k(const unsigned char* __restrict__ gt, const unsigned char* __restrict__ pred,
                                                  SurfGeom g, int ignore, unsigned char* __restrict__ kind,
                                                  unsigned short* __restrict__ dy, unsigned int* __restrict__ bad) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int nc = g.n_cls - 1;
    if (t >= (size_t)g.B * nc * 2 * g.Wc) return;
    const int j = (int)(t % g.Wc);
    const size_t plane = t / g.Wc;
    const int m = (int)(plane & 1);
    const size_t seg = plane >> 1;
    const int b = (int)(seg / nc), c = (int)(seg % nc) + 1;
    const unsigned char* lab = (m == 0 ? gt : pred) + (size_t)b * g.H * g.W;
    unsigned char* kp = kind + plane * g.KS + j;
    unsigned short* dp = dy + plane * g.N + j;
    const bool check = (c == 1) && j < g.W;   // one thread per pixel column and map checks the labels
    unsigned int badv = 0;
    // forward: kinds, distance to the nearest border row at or above
    int tl = 0, tr = 0, last = -1;
    int ti = 0;                               // kMasked: a pixel of the row above, left or right, is ignored
    const unsigned char* gtb = gt + (size_t)b * g.H * g.W;
    constexpr int U = 8;
    for (int i0 = 0; i0 < g.Hc; i0 += U) {
        unsigned char l[U], r[U], gl[U], gr[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int i = i0 + u;
            l[u] = (i < g.H && j >= 1) ? lab[(size_t)i * g.W + j - 1] : 0;
            r[u] = (i < g.H && j < g.W) ? lab[(size_t)i * g.W + j] : 0;
            if (kMasked) {                    // the ground-truth bytes: the plane's own for m == 0 (the padding is 0: known)
                gl[u] = m == 0 ? l[u] : (i < g.H && j >= 1) ? gtb[(size_t)i * g.W + j - 1] : 0;
                gr[u] = m == 0 ? r[u] : (i < g.H && j < g.W) ? gtb[(size_t)i * g.W + j] : 0;
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int i = i0 + u;
            if (i >= g.Hc) break;
            if (check && i < g.H && r[u] >= g.n_cls && !(kMasked && m == 0 && r[u] == ignore)) badv = 1;
            const int bl = l[u] == c, br = r[u] == c;
            unsigned char k = surf_kind(8 * tl + 4 * tr + 2 * bl + br);
            if (kMasked) {
                const int bi = (gl[u] == ignore) | (gr[u] == ignore);
                if (ti | bi) k = kSurfNotBorder;
                ti = bi;
            }
            kp[(size_t)i * g.Wc] = k;
            if (k != kSurfNotBorder) last = i;
            dp[(size_t)i * g.Wc] = last < 0 ? kSurfNone : (unsigned short)(i - last);
            tl = bl; tr = br;
        }
    }
    if (badv) atomicOr(bad, 1u);
    // backward: combine with the nearest border row below
    int next = -1;
    for (int i1 = g.Hc - 1; i1 >= 0; i1 -= U) {
        unsigned short up[U];
#pragma unroll
        for (int u = 0; u < U; ++u) { const int i = i1 - u; up[u] = i >= 0 ? dp[(size_t)i * g.Wc] : kSurfNone; }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int i = i1 - u;
            if (i < 0) break;
            if (up[u] == 0) next = i;
            if (next >= 0 && (unsigned)(next - i) < up[u]) dp[(size_t)i * g.Wc] = (unsigned short)(next - i);
        }
    }
}

// grid (Hc, planes); dynamic LDS: Wc uint16 (the other mask's row of column distances)
__global__ void __launch_bounds__(256) surf_row_k(SurfGeom g, const unsigned char* __restrict__ kind,
                                                  const unsigned short* __restrict__ dy, double* __restrict__ dist,
                                                  double sv, double sh) {
#pragma clang fp contract(off)
    extern __shared__ unsigned short s_dy[];
    const int i = blockIdx.x;
    const size_t plane = blockIdx.y, other = plane ^ 1;
    const unsigned short* drow = dy + other * g.N + (size_t)i * g.Wc;
    for (int j = threadIdx.x; j < g.Wc; j += blockDim.x) s_dy[j] = drow[j];
    __syncthreads();
    const unsigned char* krow = kind + plane * g.KS + (size_t)i * g.Wc;
    double* orow = dist + plane * g.N + (size_t)i * g.Wc;
    for (int j = threadIdx.x; j < g.Wc; j += blockDim.x) {
        if (krow[j] == kSurfNotBorder) continue;
        double best = __builtin_inf();
        for (int s = 0;; ++s) {
            const double bx = sh * (double)s;
            const double bb = bx * bx;
            if (bb >= best) break;                 // every column at |dx| >= s costs at least bb
            const int jl = j - s, jr = j + s;
            if (jl < 0 && jr >= g.Wc) break;
            if (jl >= 0 && s_dy[jl] != kSurfNone) {
                const double a = sv * (double)s_dy[jl];
                const double q = a * a + bb;
                best = q < best ? q : best;
            }
            if (s > 0 && jr < g.Wc && s_dy[jr] != kSurfNone) {
                const double a = sv * (double)s_dy[jr];
                const double q = a * a + bb;
                best = q < best ? q : best;
            }
        }
        orow[j] = __builtin_sqrt(best);           // +inf when the other mask has no border cell
    }
}

// cumulative contour length of counts per kind: one fixed expression (host restatement: common/custom_metrics.py)
__device__ inline double surf_len(const unsigned int* n, double ld, double lh, double lv, double l2) {
#pragma clang fp contract(off)
    return (((double)n[0] * ld + (double)n[1] * lh) + (double)n[2] * lv) + (double)n[3] * l2;
}

// grid (planes); out[(b*(n_cls-1) + c-1)*6 + {0,2,4} + m] = {average distance, percentile distance, surfel count}
__global__ void __launch_bounds__(kSurfSelectThreads) surf_select_k(SurfGeom g, const unsigned char* __restrict__ kind,
                                                                    const double* __restrict__ dist, double ld, double lh,
                                                                    double lv, double l2, double q, double* __restrict__ out) {
#pragma clang fp contract(off)
    constexpr int NT = kSurfSelectThreads;
    __shared__ unsigned int s_hist[4][256];
    __shared__ unsigned int s_cum[2][4][256];
    __shared__ double s_red[NT];
    __shared__ unsigned int s_total[4], s_below[4];
    __shared__ unsigned long long s_prefix;
    __shared__ int s_sel;
    const int tid = threadIdx.x;
    const size_t plane = blockIdx.x;
    const int m = (int)(plane & 1);
    const uchar4* kp = reinterpret_cast<const uchar4*>(kind + plane * g.KS);
    const double* dp = dist + plane * g.N;
    const size_t groups = (g.N + 3) / 4;
    const int hk = tid >> 8, hd = tid & 255;     // this thread's (kind, digit) slot of the histogram
    if (tid < 4) s_below[tid] = 0;
    if (tid == 0) s_prefix = 0;
    double acc = 0.0;                            // fixed-order partial sum of dist * length
    for (int pass = 0; pass < 8; ++pass) {
        const int shift = 56 - 8 * pass;
        s_hist[hk][hd] = 0;
        if (tid == 0) s_sel = 256;
        __syncthreads();
        const unsigned long long want = pass == 0 ? 0ull : s_prefix >> (shift + 8);
        for (size_t gi = tid; gi < groups; gi += NT) {
            const uchar4 k4 = kp[gi];
            const unsigned char ks[4] = {k4.x, k4.y, k4.z, k4.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const size_t idx = gi * 4 + e;
                if (idx >= g.N || ks[e] == kSurfNotBorder) continue;
                const double dv = dp[idx];
                const unsigned long long key = (unsigned long long)__double_as_longlong(dv);
                if (pass == 0) acc += dv * (ks[e] == 0 ? ld : ks[e] == 1 ? lh : ks[e] == 2 ? lv : l2);
                if (pass == 0 || (key >> (shift + 8)) == want) atomicAdd(&s_hist[ks[e]][(key >> shift) & 255], 1u);
            }
        }
        __syncthreads();
        // inclusive prefix sums of the four count rows over the 256 digits (Hillis-Steele, ping-pong)
        int src = 0;
        s_cum[0][hk][hd] = s_hist[hk][hd];
        __syncthreads();
        for (int off = 1; off < 256; off <<= 1) {
            unsigned int x = s_cum[src][hk][hd];
            if (hd >= off) x += s_cum[src][hk][hd - off];
            s_cum[src ^ 1][hk][hd] = x;
            __syncthreads();
            src ^= 1;
        }
        if (pass == 0) {
            if (tid < 4) s_total[tid] = s_cum[src][tid][255];
            __syncthreads();
            if (s_total[0] + s_total[1] + s_total[2] + s_total[3] == 0u) break;
        }
        const double wtot = surf_len(s_total, ld, lh, lv, l2);
        if (tid < 256) {
            unsigned int n[4];
            bool nonempty = false;
#pragma unroll
            for (int k = 0; k < 4; ++k) { n[k] = s_below[k] + s_cum[src][k][tid]; nonempty |= s_hist[k][tid] != 0u; }
            if (nonempty && surf_len(n, ld, lh, lv, l2) / wtot >= q) atomicMin(&s_sel, tid);
        }
        __syncthreads();
        if (tid == 0) {
            const int sel = s_sel < 256 ? s_sel : 255;   // (the last non-empty digit always qualifies: ratio 1)
            for (int k = 0; k < 4; ++k) s_below[k] += s_cum[src][k][sel] - s_hist[k][sel];
            s_prefix |= (unsigned long long)sel << shift;
        }
        __syncthreads();
    }
    // fixed-order tree sum of the per-thread partials
    s_red[tid] = acc;
    __syncthreads();
    for (int w = NT / 2; w > 0; w >>= 1) {
        if (tid < w) s_red[tid] = s_red[tid] + s_red[tid + w];
        __syncthreads();
    }
    if (tid == 0) {
        const unsigned int n = s_total[0] + s_total[1] + s_total[2] + s_total[3];
        double* o = out + (plane >> 1) * 6;
        o[0 + m] = s_red[0] / surf_len(s_total, ld, lh, lv, l2);    // 0/0 = NaN without border cells, as numpy
        o[2 + m] = n ? __longlong_as_double((long long)s_prefix) : __builtin_inf();
        o[4 + m] = (double)n;
    }
}

}  // namespace oct
