// Training augmentations on the device (reference: common/data_generator.py:140-283 picks an augmentation per sample,
// common/augmentation.py:43-103 applies it): (B,H,W,C) uint8 images -> float32 in [0,1], flipped or with noise added, and
// (B,H,W) uint8 labels flipped alongside.  One streaming kernel in front of the first conv; the host only decides WHICH
// augmentation a sample gets (one 32-byte oct_aug_op per sample).
//
// The random stream is the library's own and fully specified (include/oct_unet.h, oct_augment_batch): Philox4x32-10
// (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11) with key = seed and counter =
// (e >> 1, 0, noise_id): element e of a sample -- its OUTPUT position (y*W + x)*C + c -- owns words 2(e&1), 2(e&1)+1 of
// that block.  Nothing depends on the batch position or the launch geometry; common/augmentation.py restates it in numpy.
//
// augment_k<VEC>: grid (blocks per sample, B): a block never spans two samples, so the sample's descriptor is one scalar
// load and the branch on its kind is uniform.  A thread owns 4 consecutive elements per pass (grid-stride inside the
// sample): one 4-byte load, two Philox blocks, one 16-byte store.  VEC = the sample size is a multiple of 4 and the
// pointers are aligned; otherwise the same thread does guarded byte loads / float stores.  Flips read the mirrored source:
// up-down keeps the 4-byte load when a row is a multiple of 4 bytes, left-right when C == 1 and W % 4 == 0 (the mirrored
// group is contiguous: loaded as one word and byte-reversed, so a wave still reads one contiguous 256-byte run per row
// segment); other shapes gather bytes.  Labels go through a second pass of the same thread layout, 4 bytes per lane.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/oct_unet.h"
#include "philox.hpp"

namespace oct {

enum { AUG_NONE = 0, AUG_FLIP_UD = 1, AUG_FLIP_LR = 2, AUG_GAUSSIAN = 3, AUG_SPECKLE = 4, AUG_SP = 5 };

// float32(i / 255.0), the engine's uint8 input definition (common.hpp c_u8_lut; that table is filled per handle, this
// entry point has none, so its copy is a compile-time constant)
struct AugLut {
    float v[256];
    constexpr AugLut() : v() {
        for (int i = 0; i < 256; ++i) v[i] = (float)((double)i / 255.0);
    }
};
static __constant__ const AugLut c_aug_lut{};

struct AugGeom {
    int H, W, C;
    unsigned n;        // H*W*C elements of one image
    unsigned nl;       // H*W elements of one label map
    unsigned row;      // W*C
};

// source element of output element e under a flip
__device__ __forceinline__ unsigned aug_src(unsigned e, int kind, unsigned H, unsigned W, unsigned C) {
    if (kind == AUG_FLIP_UD) {
        const unsigned row = W * C, y = e / row;
        return (H - 1 - y) * row + (e - y * row);
    }
    if (kind == AUG_FLIP_LR) {
        const unsigned p = e / C, c = e - p * C, y = p / W, x = p - y * W;
        return (y * W + (W - 1 - x)) * C + c;
    }
    return e;
}

// the 4 source bytes of output elements e0..e0+3 (e0 % 4 == 0) of one sample; bytes past n are 0
template <bool VEC>
__device__ __forceinline__ uint32_t aug_load4(const unsigned char* __restrict__ s, unsigned e0, unsigned n, int kind,
                                              unsigned H, unsigned W, unsigned C) {
    const unsigned row = W * C;
    if constexpr (VEC) {
        if (kind != AUG_FLIP_UD && kind != AUG_FLIP_LR) return *reinterpret_cast<const uint32_t*>(s + e0);
        if (kind == AUG_FLIP_UD && (row & 3u) == 0) {
            const unsigned y = e0 / row;
            return *reinterpret_cast<const uint32_t*>(s + (H - 1 - y) * row + (e0 - y * row));
        }
        if (kind == AUG_FLIP_LR && C == 1 && (W & 3u) == 0) {
            const unsigned y = e0 / W, x = e0 - y * W;
            return __builtin_bswap32(*reinterpret_cast<const uint32_t*>(s + y * W + (W - 4 - x)));
        }
    }
    uint32_t v = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (e0 + j < n) v |= (uint32_t)s[aug_src(e0 + j, kind, H, W, C)] << (8 * j);
    return v;
}

template <bool VEC>
__global__ __launch_bounds__(256) void augment_k(const unsigned char* __restrict__ x, const unsigned char* __restrict__ lab,
                                                 const oct_aug_op* __restrict__ ops, AugGeom g, uint32_t k0, uint32_t k1,
                                                 float* __restrict__ out, unsigned char* __restrict__ lab_out) {
    const unsigned b = blockIdx.y;
    const oct_aug_op op = ops[b];
    const int kind = (unsigned)op.kind > (unsigned)AUG_SP ? AUG_NONE : op.kind;      // unknown kinds pass through
    const uint32_t id0 = (uint32_t)op.noise_id, id1 = (uint32_t)(op.noise_id >> 32);
    const unsigned char* xs = x + (size_t)b * g.n;
    float* os = out + (size_t)b * g.n;
    const unsigned stride = gridDim.x * blockDim.x;

    for (unsigned e0 = (blockIdx.x * blockDim.x + threadIdx.x) * 4u; e0 < g.n; e0 += stride * 4u) {
        const uint32_t src = aug_load4<VEC>(xs, e0, g.n, kind, g.H, g.W, g.C);
        float o[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = c_aug_lut.v[(src >> (8 * j)) & 255u];
        if (kind >= AUG_GAUSSIAN) {
            const Philox4 r0 = philox4x32_10(e0 >> 1, 0u, id0, id1, k0, k1);
            const Philox4 r1 = philox4x32_10((e0 >> 1) + 1u, 0u, id0, id1, k0, k1);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const Philox4& r = j < 2 ? r0 : r1;
                const uint32_t w0 = r.w[2 * (j & 1)], w1 = r.w[2 * (j & 1) + 1];
                const float u2 = (float)(w1 >> 8) * 0x1p-24f;
                if (kind == AUG_SP) {
                    const float u1 = (float)(w0 >> 8) * 0x1p-24f;
                    if (u2 <= op.p0) o[j] = u1 <= op.p1 ? 1.f : 0.f;
                } else {
                    const float u1 = (float)((w0 >> 8) + 1u) * 0x1p-24f;
                    const float z = sqrtf(-2.f * logf(u1)) * cospif(2.f * u2);
                    const float nz = op.p0 + op.p1 * z;
                    const float v = kind == AUG_SPECKLE ? o[j] + o[j] * nz : o[j] + nz;
                    o[j] = fminf(fmaxf(v, 0.f), 1.f);
                }
            }
        }
        if constexpr (VEC) {
            *reinterpret_cast<float4*>(os + e0) = make_float4(o[0], o[1], o[2], o[3]);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (e0 + j < g.n) os[e0 + j] = o[j];
        }
    }

    if (lab_out == nullptr) return;
    const unsigned char* ls = lab + (size_t)b * g.nl;
    unsigned char* lo = lab_out + (size_t)b * g.nl;
    const int lkind = kind == AUG_FLIP_UD || kind == AUG_FLIP_LR ? kind : AUG_NONE;
    // VEC also promises 4-byte aligned label pointers and nl % 4 == 0 (tu_augment.hip)
    for (unsigned e0 = (blockIdx.x * blockDim.x + threadIdx.x) * 4u; e0 < g.nl; e0 += stride * 4u) {
        const uint32_t src = aug_load4<VEC>(ls, e0, g.nl, lkind, g.H, g.W, 1u);
        if constexpr (VEC) {
            *reinterpret_cast<uint32_t*>(lo + e0) = src;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (e0 + j < g.nl) lo[e0 + j] = (unsigned char)(src >> (8 * j));
        }
    }
}

}  // namespace oct
