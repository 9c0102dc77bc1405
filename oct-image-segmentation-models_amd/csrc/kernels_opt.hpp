// The Keras optimizer family on flat buffers (oct_opt_step, include/oct_unet.h): one streaming kernel per kind and the two
// launches that turn the gradient's squared norms into clipping scales.  Formulas: DESIGN.md section 13.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "common.hpp"

namespace oct {

enum { K_SGD = 0, K_ADAM = 1, K_ADAMAX = 2, K_RMSPROP = 3, K_ADAGRAD = 4, K_ADADELTA = 5 };
enum { CLIP_NONE = 0, CLIP_VALUE = 1, CLIP_NORM = 2, CLIP_GLOBAL = 3 };
// kernel variant bits (template parameter V): SGD: V_A = momentum buffer, V_B = nesterov; Adam: V_A = amsgrad;
// RMSprop: V_A = momentum buffer, V_B = centered
enum { V_A = 1, V_B = 2 };

constexpr int kNormParts = 16;       // stage-1 blocks per variable (OCT_CLIP_NORM)
constexpr int kNormPartsGlobal = 256;  // at most this many stage-1 blocks over the whole buffer (OCT_CLIP_GLOBAL_NORM)

struct OptArgs {
    float* p; const float* g; float* s[3];
    size_t n;
    size_t head, nvec;       // elements [0, head) and [head + 4*nvec, n) take scalar accesses, the middle float4 ones
    float lr;                // Adam: lr_t (both bias corrections); Adamax: lr / (1 - beta1^t); else the step's learning rate
    float b1, b2, rho, mu, eps;
    int clip_mode; float clip;
    const unsigned long long* var_off; int n_vars;   // CLIP_NORM: n_vars + 1 ascending offsets
    const float* scale;                              // CLIP_NORM: one scale per variable; CLIP_GLOBAL: scale[0]
};

// index of the variable that holds element i: the last k with var_off[k] <= i (offsets are clamped to n by the reader)
static __device__ __forceinline__ int var_of(const OptArgs& a, size_t i) {
    int lo = 0, hi = a.n_vars - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (a.var_off[mid] <= i) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// One element of one step: w the parameter, g the clipped gradient, s0..s2 the state values in the ABI's slot order.
// Every product and sum is rounded on its own (no contraction into FMAs): the result of an element must not depend on
// whether the float4 body or a scalar edge computed it, and the SGD / Adam expressions then give the bits of sgd_k / adam_k
// (kernels_bwd.hpp), whose momentum and moment updates the compiler emits unfused and whose plain-SGD line it fuses.
template <int KIND, int V>
static __device__ __forceinline__ void opt_update(float& w, const float g, float& s0, float& s1, float& s2, const OptArgs& a) {
#pragma clang fp contract(off)
    if constexpr (KIND == K_SGD) {
        if constexpr (V & V_A) {
            const float vi = a.mu * s0 - a.lr * g;
            s0 = vi;
            if constexpr (V & V_B) w += a.mu * vi - a.lr * g; else w += vi;
        } else {
            w = fmaf(-a.lr, g, w);
        }
    } else if constexpr (KIND == K_ADAM) {
        const float mi = a.b1 * s0 + (1.f - a.b1) * g;
        const float vi = a.b2 * s1 + (1.f - a.b2) * g * g;
        s0 = mi; s1 = vi;
        if constexpr (V & V_A) {
            const float vh = fmaxf(s2, vi);
            s2 = vh;
            w -= a.lr * mi / (sqrtf(vh) + a.eps);
        } else {
            w -= a.lr * mi / (sqrtf(vi) + a.eps);
        }
    } else if constexpr (KIND == K_ADAMAX) {
        const float mi = a.b1 * s0 + (1.f - a.b1) * g;
        const float ui = fmaxf(a.b2 * s1, fabsf(g));
        s0 = mi; s1 = ui;
        w -= a.lr * mi / (ui + a.eps);
    } else if constexpr (KIND == K_RMSPROP) {
        // slots: rms, then mom (V_A), then mg (V_B)
        const float rms = a.rho * s0 + (1.f - a.rho) * g * g;
        s0 = rms;
        float d = rms;
        if constexpr (V & V_B) {
            float& mgs = (V & V_A) ? s2 : s1;
            const float mg = a.rho * mgs + (1.f - a.rho) * g;
            mgs = mg;
            d = rms - mg * mg;
        }
        if constexpr (V & V_A) {
            const float mom = a.mu * s1 + a.lr * g / sqrtf(d + a.eps);
            s1 = mom;
            w -= mom;
        } else {
            w -= a.lr * g / (sqrtf(d) + a.eps);
        }
    } else if constexpr (KIND == K_ADAGRAD) {
        const float acc = s0 + g * g;
        s0 = acc;
        w -= a.lr * g / (sqrtf(acc) + a.eps);
    } else {   // K_ADADELTA
        const float acc = a.rho * s0 + (1.f - a.rho) * g * g;
        const float u = g * sqrtf(s1 + a.eps) / sqrtf(acc + a.eps);
        s0 = acc;
        s1 = a.rho * s1 + (1.f - a.rho) * u * u;
        w -= a.lr * u;
    }
}

template <int KIND, int V>
constexpr int opt_slots() {
    return KIND == K_SGD ? (V & V_A ? 1 : 0) : KIND == K_ADAM ? (V & V_A ? 3 : 2) : KIND == K_ADAMAX ? 2
         : KIND == K_RMSPROP ? 1 + ((V & V_A) ? 1 : 0) + ((V & V_B) ? 1 : 0) : KIND == K_ADAGRAD ? 1 : 2;
}

static __device__ __forceinline__ float clip_one(const OptArgs& a, float g, float sc) {
    if (a.clip_mode == CLIP_VALUE) return fminf(fmaxf(g, -a.clip), a.clip);
    return a.clip_mode == CLIP_NONE ? g : g * sc;
}

// The step: 16-byte accesses over [head, head + 4*nvec) -- the host picks `head` so that every buffer is 16-byte aligned
// there, or nvec = 0 where the buffers' alignments differ -- and 4-byte accesses over the two edges.
template <int KIND, int V>
static __global__ __launch_bounds__(kBlock) void opt_k(const OptArgs a) {
    constexpr int NS = opt_slots<KIND, V>();
    const size_t tid = (size_t)blockIdx.x * kBlock + threadIdx.x, nthr = (size_t)gridDim.x * kBlock;
    const float gsc = a.clip_mode == CLIP_GLOBAL ? a.scale[0] : 1.f;
    for (size_t q = tid; q < a.nvec; q += nthr) {
        const size_t i = a.head + 4 * q;
        float4 w = *reinterpret_cast<const float4*>(a.p + i);
        const float4 g4 = *reinterpret_cast<const float4*>(a.g + i);
        float4 s[3] = {};
#pragma unroll
        for (int k = 0; k < NS; ++k) s[k] = *reinterpret_cast<const float4*>(a.s[k] + i);
        float sc[4] = {gsc, gsc, gsc, gsc};
        if (a.clip_mode == CLIP_NORM) {
            int k = var_of(a, i);
            size_t end = min((size_t)a.var_off[k + 1], a.n);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                while (i + j >= end && k + 1 < a.n_vars) { ++k; end = min((size_t)a.var_off[k + 1], a.n); }
                sc[j] = a.scale[k];
            }
        }
        float* wv = reinterpret_cast<float*>(&w);
        const float* gv = reinterpret_cast<const float*>(&g4);
#pragma unroll
        for (int j = 0; j < 4; ++j)
            opt_update<KIND, V>(wv[j], clip_one(a, gv[j], sc[j]), reinterpret_cast<float*>(&s[0])[j],
                                reinterpret_cast<float*>(&s[1])[j], reinterpret_cast<float*>(&s[2])[j], a);
        *reinterpret_cast<float4*>(a.p + i) = w;
#pragma unroll
        for (int k = 0; k < NS; ++k) *reinterpret_cast<float4*>(a.s[k] + i) = s[k];
    }
    const size_t body_end = a.head + 4 * a.nvec, nedge = a.head + (a.n - body_end);
    for (size_t e = tid; e < nedge; e += nthr) {
        const size_t i = e < a.head ? e : body_end + (e - a.head);
        float w = a.p[i], s[3] = {0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < NS; ++k) s[k] = a.s[k][i];
        const float sc = a.clip_mode == CLIP_NORM ? a.scale[var_of(a, i)] : gsc;
        opt_update<KIND, V>(w, clip_one(a, a.g[i], sc), s[0], s[1], s[2], a);
        a.p[i] = w;
#pragma unroll
        for (int k = 0; k < NS; ++k) a.s[k][i] = s[k];
    }
}

// ---- clipping by norm: sum of squares per variable, in a fixed order ------------------------------------------------
// Stage 1, grid (parts, n_vars): block (c, k) adds the squares of variable k's elements c*kBlock + t, (c + parts)*kBlock + t,
// ... per thread in float -- four independent sums, so that four loads are in flight, combined as (s0 + s1) + (s2 + s3) --
// then the block's 256 sums in double (a tree over LDS: the same order every run), into part[k * parts + c].
// var_off == nullptr: one variable, the whole buffer.
static __device__ __forceinline__ double block_sum(double v, double* sh) {
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int w = kBlock / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
        __syncthreads();
    }
    return sh[0];
}

static __global__ __launch_bounds__(kBlock) void opt_sqnorm_k(const float* __restrict__ g, size_t n,
                                                              const unsigned long long* __restrict__ var_off,
                                                              double* __restrict__ part) {
    __shared__ double sh[kBlock];
    const int k = blockIdx.y, parts = gridDim.x;
    const size_t lo = var_off ? min((size_t)var_off[k], n) : 0, hi = var_off ? min((size_t)var_off[k + 1], n) : n;
    const size_t stride = (size_t)parts * kBlock;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    size_t i = lo + (size_t)blockIdx.x * kBlock + threadIdx.x;
    for (; i + 3 * stride < hi; i += 4 * stride) {
        const float v0 = g[i], v1 = g[i + stride], v2 = g[i + 2 * stride], v3 = g[i + 3 * stride];
        s0 += v0 * v0; s1 += v1 * v1; s2 += v2 * v2; s3 += v3 * v3;
    }
    for (; i < hi; i += stride) { const float v = g[i]; s0 += v * v; }
    const double t = block_sum((double)((s0 + s1) + (s2 + s3)), sh);
    if (threadIdx.x == 0) part[(size_t)k * parts + blockIdx.x] = t;
}

// Stage 2, one block per variable: its partials (parts <= kBlock) summed in double by the same tree,
// scale = clip / max(norm, clip) -- 1 for a zero (or NaN) norm.
static __global__ __launch_bounds__(kBlock) void opt_scale_k(const double* __restrict__ part, int parts, float clip,
                                                             float* __restrict__ scale) {
    __shared__ double sh[kBlock];
    const int k = blockIdx.x;
    const double t = block_sum((int)threadIdx.x < parts ? part[(size_t)k * parts + threadIdx.x] : 0.0, sh);
    if (threadIdx.x == 0) scale[k] = clip / fmaxf((float)sqrt(t), clip);
}

}  // namespace oct
