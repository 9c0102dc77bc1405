// Monte-Carlo dropout reduction on the device: fold the softmax output of stochastic sample t into running sums and, on
// the last sample, turn the sums into the mean class probabilities, their arg-max, the predictive entropy and the mutual
// information (BALD).  The definition is in include/oct_unet.h (oct_mc_update) and restated in numpy by
// common/utils.py::mc_reduce_reference; every step is one IEEE fp32 operation and none is contracted with another.
//
//   mc_update_k<VC, FIRST, LAST>  probs (npix, C) f32, workspace S (npix, C) + E (npix) f32 -> at LAST the four maps.
//                   FIRST = (t == 0): the sums are assigned, not added to, so the workspace needs no memset.
//                   LAST = (t == T - 1): the sums are finished in registers and NOT written back (nothing reads them again).
//                   The kernel is memory-bound: per pixel and sample it reads p and S and writes S (3 C floats) and reads
//                   and writes E (2 floats).  S has the layout of probs, so a work item is 4 adjacent pixels = 4 C
//                   consecutive floats of both: VC = C float4 loads each (VC = C in 2..8, chosen by the launcher where the
//                   bases are 16-byte aligned and npix * C % 4 == 0, which keeps E aligned behind S).  The VC loads of a
//                   lane are 16 bytes apart and lanes are 16 C bytes apart, so the VC load instructions of a wave together
//                   cover one contiguous stretch of 64 x 16 C bytes: every cache line fetched is used whole.  E, entropy and
//                   mutual_info are one float4 per item, the arg-max one uchar4.  The pixels behind the last whole item,
//                   and every pixel with VC = 0 (any C <= 32, any alignment), take the scalar path mc_pixel: the same
//                   operations in the same order, one class at a time, no arrays.
//                   One launch, grid-stride over items, no atomics: a pixel is owned by one thread.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace oct {

constexpr int kMcThreads = 256;
constexpr int kMcMaxBlocks = 2048;       // 8 blocks per CU; larger batches stride
constexpr int kMcMaxClasses = 32;
constexpr int kMcMaxSamples = 64;
constexpr int kMcMaxVec = 8;             // widest class count of the float4 path (4 * 8 floats of p and of S in registers)

struct McArgs {
    const float* probs;      // (npix, C)
    float* S;                // (npix, C) running sum of p
    float* E;                // (npix)    running sum of the per-sample entropies
    float* mean;             // LAST: (npix, C) or nullptr
    unsigned char* am;       // LAST: (npix)    or nullptr
    float* ent;              // LAST: (npix)    or nullptr
    float* mi;               // LAST: (npix)    or nullptr
    size_t npix;
    int C;
    float inv_t;             // float(1.0f / T)
};

// p ln p with the limit 0 at p == 0 (OCML logf: the correctly rounded-to-1-ulp one, not the fast intrinsic)
__device__ __forceinline__ float mc_plogp(float p) {
#pragma clang fp contract(off)
    return p > 0.f ? p * logf(p) : 0.f;
}

// what one class adds to a pixel's state: the entropy sums in class order, the arg-max as the lowest index of the maximum
struct McPixel {
    float h, hm, best; int bi;
    template <bool LAST>
    __device__ __forceinline__ void add(int c, float p, float m) {
#pragma clang fp contract(off)
        const float t = mc_plogp(p);
        h = c == 0 ? t : h + t;
        if constexpr (LAST) {
            const float u = mc_plogp(m);
            hm = c == 0 ? u : hm + u;
            if (c == 0 || m > best) { best = m; bi = c; }
        }
    }
};

// pixel px of the sums and the outputs takes the sample's classes at p (oct_mc_update: the same pixel of probs; oct_tta_update:
// the mirrored one, kernels_tta.hpp)
template <bool FIRST, bool LAST>
__device__ __forceinline__ void mc_pixel_from(const McArgs& A, size_t px, const float* p) {
#pragma clang fp contract(off)
    float* s = A.S + px * A.C;
    McPixel st{0.f, 0.f, 0.f, 0};
    for (int c = 0; c < A.C; ++c) {
        const float pc = p[c];
        const float sc = FIRST ? pc : s[c] + pc;
        float m = 0.f;
        if constexpr (LAST) {
            m = sc * A.inv_t;
            if (A.mean) A.mean[px * A.C + c] = m;
        } else {
            s[c] = sc;
        }
        st.add<LAST>(c, pc, m);
    }
    const float ht = -st.h;
    const float e = FIRST ? ht : A.E[px] + ht;
    if constexpr (LAST) {
        const float ent = -st.hm;
        if (A.am) A.am[px] = (unsigned char)st.bi;
        if (A.ent) A.ent[px] = ent;
        if (A.mi) A.mi[px] = fmaxf(ent - e * A.inv_t, 0.f);
    } else {
        A.E[px] = e;
    }
}

template <bool FIRST, bool LAST>
__device__ __forceinline__ void mc_pixel(const McArgs& A, size_t px) { mc_pixel_from<FIRST, LAST>(A, px, A.probs + px * A.C); }

// load VC float4s = 4 pixels x VC classes of one sample
template <int VC>
__device__ __forceinline__ void mc_load4(const float* p, float (&pv)[4 * VC]) {
    const float4* p4 = reinterpret_cast<const float4*>(p);
#pragma unroll
    for (int q = 0; q < VC; ++q) {
        const float4 a = p4[q];
        pv[4 * q] = a.x; pv[4 * q + 1] = a.y; pv[4 * q + 2] = a.z; pv[4 * q + 3] = a.w;
    }
}

// the float4 item: pixels px0..px0+3 of the sums and the outputs take the sample values pv (pixel j, class c at pv[j * VC + c])
template <int VC, bool FIRST, bool LAST>
__device__ __forceinline__ void mc_item4(const McArgs& A, size_t px0, const float (&pv)[4 * VC]) {
#pragma clang fp contract(off)
    float4* s4 = reinterpret_cast<float4*>(A.S + px0 * VC);
    float sv[4 * VC];
    if constexpr (FIRST) {
#pragma unroll
        for (int i = 0; i < 4 * VC; ++i) sv[i] = pv[i];
    } else {
#pragma unroll
        for (int q = 0; q < VC; ++q) {
            const float4 a = s4[q];
            sv[4 * q] = a.x + pv[4 * q]; sv[4 * q + 1] = a.y + pv[4 * q + 1];
            sv[4 * q + 2] = a.z + pv[4 * q + 2]; sv[4 * q + 3] = a.w + pv[4 * q + 3];
        }
    }
    if constexpr (LAST) {
#pragma unroll
        for (int i = 0; i < 4 * VC; ++i) sv[i] = sv[i] * A.inv_t;      // sv is now the mean m
        if (A.mean) {
            float4* m4 = reinterpret_cast<float4*>(A.mean + px0 * VC);
#pragma unroll
            for (int q = 0; q < VC; ++q) m4[q] = make_float4(sv[4 * q], sv[4 * q + 1], sv[4 * q + 2], sv[4 * q + 3]);
        }
    } else {
#pragma unroll
        for (int q = 0; q < VC; ++q) s4[q] = make_float4(sv[4 * q], sv[4 * q + 1], sv[4 * q + 2], sv[4 * q + 3]);
    }
    float e[4], ent[4]; unsigned char bi[4];
    float4 e_in = make_float4(0.f, 0.f, 0.f, 0.f);
    if constexpr (!FIRST) e_in = *reinterpret_cast<const float4*>(A.E + px0);
    const float ev[4] = {e_in.x, e_in.y, e_in.z, e_in.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        McPixel st{0.f, 0.f, 0.f, 0};
#pragma unroll
        for (int c = 0; c < VC; ++c) st.add<LAST>(c, pv[j * VC + c], sv[j * VC + c]);
        const float ht = -st.h;
        e[j] = FIRST ? ht : ev[j] + ht;
        ent[j] = -st.hm; bi[j] = (unsigned char)st.bi;
    }
    if constexpr (LAST) {
        if (A.am) *reinterpret_cast<uchar4*>(A.am + px0) = make_uchar4(bi[0], bi[1], bi[2], bi[3]);
        if (A.ent) *reinterpret_cast<float4*>(A.ent + px0) = make_float4(ent[0], ent[1], ent[2], ent[3]);
        if (A.mi) {
            float v[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = fmaxf(ent[j] - e[j] * A.inv_t, 0.f);
            *reinterpret_cast<float4*>(A.mi + px0) = make_float4(v[0], v[1], v[2], v[3]);
        }
    } else {
        *reinterpret_cast<float4*>(A.E + px0) = make_float4(e[0], e[1], e[2], e[3]);
    }
}

// items = ceil(npix / 4) with VC > 0, npix with VC == 0
template <int VC, bool FIRST, bool LAST>
__global__ void __launch_bounds__(kMcThreads) mc_update_k(const McArgs A, size_t items) {
#pragma clang fp contract(off)
    const size_t stride = (size_t)gridDim.x * kMcThreads;
    for (size_t it = (size_t)blockIdx.x * kMcThreads + threadIdx.x; it < items; it += stride) {
        if constexpr (VC == 0) {
            mc_pixel<FIRST, LAST>(A, it);
        } else {
            const size_t px0 = it * 4;
            if (px0 + 4 > A.npix) {      // the pixels behind the last whole item
                for (size_t px = px0; px < A.npix; ++px) mc_pixel<FIRST, LAST>(A, px);
                continue;
            }
            float pv[4 * VC];
            mc_load4<VC>(A.probs + px0 * VC, pv);
            mc_item4<VC, FIRST, LAST>(A, px0, pv);
        }
    }
}

}  // namespace oct
