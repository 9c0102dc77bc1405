// Geometric training augmentations on the device: (B,H,W,C) uint8 images -> uint8 images, each sample shifted per column
// (depth position, tilt, curvature of the retina) or mapped through an affine transform (rotation, zoom, translation), and
// (B,H,W) uint8 labels moved alongside.  The stage runs in front of augment_k (kernels_augment.hpp), whose flips and noise
// then apply to its output.  The definition is include/oct_unet.h, oct_warp_batch; common/augmentation.py warp_reference
// restates it in numpy.  Integer arithmetic only: 64-bit where the definition needs it (the column shift's numerator, the
// affine source position), 32-bit everywhere else -- every source index fits an int32 inside the header's parameter ranges.
//
// warp_k<VEC>: grid (blocks per sample, B): a block never spans two samples, so the sample's descriptor is one uniform load
// and the branch on its kind and border is uniform.  A thread produces 4 adjacent output bytes per pass (grid-stride inside
// the sample) and stores them as one 32-bit word.  VEC = the sample size is a multiple of 4 and the pointers are 4-byte
// aligned; otherwise the same thread does guarded byte stores.  Source bytes are gathered straight from global memory (a
// 256x512 scan is 128 KB: it lives in L2).  Column shift with C == 1 and W % 4 == 0: the 4 output bytes are 4 columns of one
// row; when they share one shift the source is one aligned word.  Labels go through a second pass of the same thread layout.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/oct_unet.h"

namespace oct {

enum { WARP_NONE = 0, WARP_COLUMN_SHIFT = 1, WARP_AFFINE = 2 };
enum { WARP_REPLICATE = 0, WARP_WRAP = 1, WARP_CONSTANT = 2 };

struct WarpGeom {
    int H, W, C;
    unsigned n;        // H*W*C elements of one image
    unsigned nl;       // H*W elements of one label map
};

// source index of i on an axis of length n under the border rule; -1 = outside (constant border only)
__device__ __forceinline__ int warp_border(int i, int n, int border) {
    if (border == WARP_REPLICATE) return min(max(i, 0), n - 1);
    if (border == WARP_WRAP) {
        const int r = i % n;
        return r < 0 ? r + n : r;
    }
    return (unsigned)i < (unsigned)n ? i : -1;
}

// s(x) of the column shift: floor((a D^2 + b t D + c t^2 + 128 D^2) / (256 D^2)), t = 2x - (W-1), D = max(W-1, 1)
__device__ __forceinline__ int warp_shift(int x, int W, int a, int b, int c) {
    const int64_t D = W > 1 ? W - 1 : 1, t = 2 * (int64_t)x - (W - 1);
    const int64_t num = ((int64_t)a + 128) * D * D + (int64_t)b * t * D + (int64_t)c * t * t, den = 256 * D * D;
    int64_t q = num / den;
    if (num % den < 0) --q;          // C++ truncates: floor for a negative numerator
    return (int)q;
}

// one output byte of the column shift: plane of `ch` interleaved channels, element e = (y*W + x)*ch + c
__device__ __forceinline__ unsigned warp_shift_byte(const unsigned char* __restrict__ s, unsigned e, int H, int W, unsigned ch,
                                                    const oct_warp_op& op, unsigned fill) {
    const unsigned p = e / ch, c = e - p * ch, y = p / (unsigned)W, x = p - y * (unsigned)W;
    const int sy = warp_border((int)y - warp_shift((int)x, W, op.p[0], op.p[1], op.p[2]), H, op.border);
    return sy < 0 ? fill : s[((unsigned)sy * (unsigned)W + x) * ch + c];
}

// Q16 source position of output pixel (x, y) under the affine inverse map
__device__ __forceinline__ void warp_affine_src(int x, int y, int H, int W, const oct_warp_op& op, int64_t& sx, int64_t& sy) {
    const int64_t X = 2 * (int64_t)x - (W - 1), Y = 2 * (int64_t)y - (H - 1);
    const int64_t U = (int64_t)op.p[0] * X + (int64_t)op.p[1] * Y + op.p[4];
    const int64_t V = (int64_t)op.p[2] * X + (int64_t)op.p[3] * Y + op.p[5];
    sx = (U + (int64_t)(W - 1) * 65536) >> 1;
    sy = (V + (int64_t)(H - 1) * 65536) >> 1;
}

// one output byte of the affine map, bilinear in 8-bit fractions
__device__ __forceinline__ unsigned warp_affine_byte(const unsigned char* __restrict__ s, unsigned e, int H, int W, unsigned C,
                                                     const oct_warp_op& op, unsigned fill) {
    const unsigned p = e / C, c = e - p * C, y = p / (unsigned)W, x = p - y * (unsigned)W;
    int64_t sx, sy;
    warp_affine_src((int)x, (int)y, H, W, op, sx, sy);
    const int ix = (int)(sx >> 16), iy = (int)(sy >> 16);
    const unsigned fx = (unsigned)(sx >> 8) & 255u, fy = (unsigned)(sy >> 8) & 255u;
    const int x0 = warp_border(ix, W, op.border), x1 = warp_border(ix + 1, W, op.border);
    const int y0 = warp_border(iy, H, op.border), y1 = warp_border(iy + 1, H, op.border);
    auto tap = [&](int yy, int xx) -> unsigned {
        return (yy | xx) < 0 ? fill : s[((unsigned)yy * (unsigned)W + (unsigned)xx) * C + c];
    };
    const unsigned acc = (256u - fx) * (256u - fy) * tap(y0, x0) + fx * (256u - fy) * tap(y0, x1) +
                         (256u - fx) * fy * tap(y1, x0) + fx * fy * tap(y1, x1);
    return (acc + 32768u) >> 16;
}

// one label of the affine map: the nearest source pixel
__device__ __forceinline__ unsigned warp_affine_label(const unsigned char* __restrict__ s, unsigned e, int H, int W,
                                                      const oct_warp_op& op, unsigned fill) {
    const unsigned y = e / (unsigned)W, x = e - y * (unsigned)W;
    int64_t sx, sy;
    warp_affine_src((int)x, (int)y, H, W, op, sx, sy);
    const int xx = warp_border((int)((sx + 32768) >> 16), W, op.border), yy = warp_border((int)((sy + 32768) >> 16), H, op.border);
    return (yy | xx) < 0 ? fill : s[(unsigned)yy * (unsigned)W + (unsigned)xx];
}

// the 4 output bytes e0..e0+3 (e0 % 4 == 0) of one plane of `ch` channels (ch = 1 and LABELS for the label map); bytes past n
// are 0
template <bool VEC, bool LABELS>
__device__ __forceinline__ uint32_t warp_out4(const unsigned char* __restrict__ s, unsigned e0, unsigned n, int kind, int H, int W,
                                              unsigned ch, const oct_warp_op& op, unsigned fill) {
    if constexpr (VEC) {
        if (kind == WARP_NONE) return *reinterpret_cast<const uint32_t*>(s + e0);
        if (kind == WARP_COLUMN_SHIFT && ch == 1 && (W & 3) == 0) {
            // 4 columns of one row: one aligned source word when they share the shift
            const unsigned y = e0 / (unsigned)W, x = e0 - y * (unsigned)W;
            int sh[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) sh[j] = warp_shift((int)x + j, W, op.p[0], op.p[1], op.p[2]);
            if (sh[0] == sh[1] && sh[0] == sh[2] && sh[0] == sh[3]) {
                const int sy = warp_border((int)y - sh[0], H, op.border);
                return sy < 0 ? fill * 0x01010101u : *reinterpret_cast<const uint32_t*>(s + (unsigned)sy * (unsigned)W + x);
            }
            uint32_t v = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int sy = warp_border((int)y - sh[j], H, op.border);
                v |= (sy < 0 ? fill : (unsigned)s[(unsigned)sy * (unsigned)W + x + j]) << (8 * j);
            }
            return v;
        }
    }
    uint32_t v = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const unsigned e = e0 + j;
        if (e >= n) break;
        unsigned byte;
        if (kind == WARP_COLUMN_SHIFT) byte = warp_shift_byte(s, e, H, W, ch, op, fill);
        else if (kind == WARP_AFFINE) byte = LABELS ? warp_affine_label(s, e, H, W, op, fill) : warp_affine_byte(s, e, H, W, ch, op, fill);
        else byte = s[e];
        v |= byte << (8 * j);
    }
    return v;
}

template <bool VEC>
__device__ __forceinline__ void warp_store4(unsigned char* __restrict__ o, unsigned e0, unsigned n, uint32_t v) {
    if constexpr (VEC) {
        *reinterpret_cast<uint32_t*>(o + e0) = v;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (e0 + j < n) o[e0 + j] = (unsigned char)(v >> (8 * j));
    }
}

template <bool VEC>
__global__ __launch_bounds__(256) void warp_k(const unsigned char* __restrict__ x, const unsigned char* __restrict__ lab,
                                              const oct_warp_op* __restrict__ ops, WarpGeom g, unsigned char* __restrict__ out,
                                              unsigned char* __restrict__ lab_out) {
    const unsigned b = blockIdx.y;
    const oct_warp_op op = ops[b];
    // unknown kinds and borders pass through
    const int kind = (unsigned)op.kind > (unsigned)WARP_AFFINE || (unsigned)op.border > (unsigned)WARP_CONSTANT ? WARP_NONE : op.kind;
    const unsigned stride = gridDim.x * blockDim.x;
    const unsigned first = (blockIdx.x * blockDim.x + threadIdx.x) * 4u;

    const unsigned char* xs = x + (size_t)b * g.n;
    unsigned char* os = out + (size_t)b * g.n;
    const unsigned fill = (unsigned)op.fill & 255u;
    for (unsigned e0 = first; e0 < g.n; e0 += stride * 4u)
        warp_store4<VEC>(os, e0, g.n, warp_out4<VEC, false>(xs, e0, g.n, kind, g.H, g.W, (unsigned)g.C, op, fill));

    if (lab_out == nullptr) return;
    // VEC also promises 4-byte aligned label pointers and nl % 4 == 0 (tu_warp.hip)
    const unsigned char* ls = lab + (size_t)b * g.nl;
    unsigned char* lo = lab_out + (size_t)b * g.nl;
    const unsigned lfill = (unsigned)op.fill_label & 255u;
    for (unsigned e0 = first; e0 < g.nl; e0 += stride * 4u)
        warp_store4<VEC>(lo, e0, g.nl, warp_out4<VEC, true>(ls, e0, g.nl, kind, g.H, g.W, 1u, op, lfill));
}

}  // namespace oct
