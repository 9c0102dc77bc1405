// Test-time augmentation on the device: the four flips of a batch and the mirrored fold of their softmax outputs.  The
// definitions are include/oct_unet.h (oct_flip_batch, oct_tta_update); common/utils.py flip_reference / tta_reduce_reference
// restate them in numpy.  A view code v: bit 0 mirrors columns (x -> W-1-x), bit 1 mirrors rows (y -> H-1-y).
//
//   flip_k<DW>      dst[b, y, x] = src[b, yv, xv] over pixels of pb bytes: the kernel only moves bytes.  Grid (x: units of a
//                   destination row, y: rows, z: images), a grid-stride loop on each axis.  DW: the unit is one aligned dword
//                   of the destination -- the launcher picks it where a row is a whole number of dwords and both bases are
//                   4-byte aligned, so every row of both buffers starts on a dword.  With pb >= 4 a dword is part k of pixel
//                   x and comes from part k of pixel xv; with pb 1 or 2 it holds 4 or 2 whole pixels, which come from ONE
//                   source dword, the mirrored one of the row, with their order reversed (byte swap / half swap).  Lanes walk
//                   the destination row forwards and the source row forwards or backwards: both sides use whole cache lines.
//                   !DW: one byte per unit, for rows and bases of any alignment (a store never leaves the row).
//   tta_update_k<VC, FIRST, LAST>   mc_update_k (kernels_mc.hpp) with one change: pixel (b, y, x) of the sums and of the
//                   outputs takes the sample's pixel (b, yv, xv).  The arithmetic is mc_pixel_from / mc_item4 themselves.
//                   VC = C in 2..8 where W % 4 == 0 and the bases are 16-byte aligned: an item is 4 adjacent output pixels
//                   of one row; its 4 source pixels are adjacent too and start at a multiple of 4 (W-4-x0), so they are the
//                   same VC float4 loads from the mirrored address, followed by a permutation of the pixels in registers.
//                   VC = 0: any C <= 32, W and alignment, one pixel per item.  One thread owns an output pixel: no atomics.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels_mc.hpp"

namespace oct {

constexpr int kTtaMaxViews = 4;

struct FlipArgs {
    const unsigned char* src; unsigned char* dst;
    int B, H, W, pb;           // pb: bytes of a pixel
    int fx, fy;                // mirror columns / rows
};

template <bool DW>
__global__ __launch_bounds__(256) void flip_k(FlipArgs a) {
    const int rb = a.W * a.pb;                              // bytes of a row (< 2^30, the host checks)
    const int units = DW ? rb >> 2 : rb;
    const int q = DW ? (a.pb >= 4 ? a.pb >> 2 : 1) : a.pb;  // units of a pixel (pb < 4 under DW: several pixels per unit)
    for (int b = blockIdx.z; b < a.B; b += gridDim.z) {
        for (int y = blockIdx.y * blockDim.y + threadIdx.y; y < a.H; y += gridDim.y * blockDim.y) {
            const int sy = a.fy ? a.H - 1 - y : y;
            unsigned char* drow = a.dst + ((size_t)b * a.H + y) * (size_t)rb;
            const unsigned char* srow = a.src + ((size_t)b * a.H + sy) * (size_t)rb;
            for (int u = blockIdx.x * blockDim.x + threadIdx.x; u < units; u += gridDim.x * blockDim.x) {
                int su = u;
                if (a.fx) {
                    if (DW && a.pb < 4) {
                        su = units - 1 - u;
                    } else {
                        const int x = u / q, k = u - x * q;
                        su = (a.W - 1 - x) * q + k;
                    }
                }
                if constexpr (DW) {
                    uint32_t v = reinterpret_cast<const uint32_t*>(srow)[su];
                    if (a.fx && a.pb == 1) v = __builtin_bswap32(v);
                    if (a.fx && a.pb == 2) v = (v >> 16) | (v << 16);
                    reinterpret_cast<uint32_t*>(drow)[u] = v;
                } else {
                    drow[u] = srow[su];
                }
            }
        }
    }
}

struct TtaArgs {
    McArgs m;
    unsigned H, W;
    int fx, fy;
};

// the sample's pixel that output pixel px (< 2^31) takes
__device__ __forceinline__ unsigned tta_src_pixel(const TtaArgs& T, unsigned px) {
    const unsigned row = px / T.W, x = px - row * T.W;
    const unsigned b = row / T.H, y = row - b * T.H;
    return (b * T.H + (T.fy ? T.H - 1 - y : y)) * T.W + (T.fx ? T.W - 1 - x : x);
}

// items = npix / 4 with VC > 0 (W % 4 == 0: an item never leaves its row), npix with VC == 0
template <int VC, bool FIRST, bool LAST>
__global__ void __launch_bounds__(kMcThreads) tta_update_k(const TtaArgs T, size_t items) {
#pragma clang fp contract(off)
    const size_t stride = (size_t)gridDim.x * kMcThreads;
    for (size_t it = (size_t)blockIdx.x * kMcThreads + threadIdx.x; it < items; it += stride) {
        if constexpr (VC == 0) {
            mc_pixel_from<FIRST, LAST>(T.m, it, T.m.probs + (size_t)tta_src_pixel(T, (unsigned)it) * T.m.C);
        } else {
            const unsigned px0 = (unsigned)it * 4;
            const unsigned row = px0 / T.W, x0 = px0 - row * T.W;
            const unsigned b = row / T.H, y = row - b * T.H;
            const size_t spx = (size_t)(b * T.H + (T.fy ? T.H - 1 - y : y)) * T.W + (T.fx ? T.W - 4 - x0 : x0);
            float raw[4 * VC], pv[4 * VC];
            mc_load4<VC>(T.m.probs + spx * VC, raw);
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int c = 0; c < VC; ++c) pv[j * VC + c] = T.fx ? raw[(3 - j) * VC + c] : raw[j * VC + c];
            mc_item4<VC, FIRST, LAST>(T.m, px0, pv);
        }
    }
}

}  // namespace oct
