// Photometric augmentation on the device: (B,H,W,C) uint8 images -> uint8 images through a separable integer blur with a
// replicate border, column shadows and a 256-entry intensity table, per sample and in that order.  The stage runs directly
// behind elastic_k (kernels_elastic.hpp) and in front of warp_k.  The definition is include/oct_unet.h, oct_photo_batch;
// common/augmentation.py photometric_reference restates it in numpy.  Integer arithmetic only; no atomics.
//
// photo_k<VEC>: grid (tiles per sample, B): a block owns one PH_TH x PH_TW pixel tile of one sample, so the sample's
// descriptor is one uniform load and the branches on its flags are uniform.  The shadow gains of the tile's columns (one
// uint16 per shadow and column) and the table go into LDS once per block.  A thread finishes 4 adjacent pixels of a row:
// gains, table, store.  Where they come from:
//   no blur: straight from global memory (one dword with VEC);
//   blur, per channel, three phases:
//     1. the tile's bytes plus a halo of R rows and R4 = R rounded up to 4 columns into LDS, rows and columns clamped at the
//        image edges; with VEC every staged dword lies wholly inside a row or wholly outside it, so it is one dword load or
//        one byte splat;
//     2. the horizontal pass: a thread reads the 2 R4 / 4 + 1 dwords around its 4 pixels of one staged row and writes 4
//        uint16 sums (<= 65280: exact) into the plane s_h, (PH_TH + 2 R) x PH_TW.  The taps beyond R have weight 0 by the
//        descriptor's rule, so the pass is unrolled for R4 = 4 and R4 = 8 only;
//     3. the vertical pass: 2 R + 1 reads of 4 uint16 from s_h, the weights broadcast from LDS.
// LDS traffic by the bank rules (ds_read_b32: groups of 32 lanes, banks mod 32; ds_read_b64: 32 lanes, banks mod 64;
// ds_write_b64: 16 lanes): PH_TW = 128 makes a row 32 groups of 4 pixels, so the 32 lanes of a group read or write
// consecutive dwords (phase 2 reads), consecutive 8-byte words covering one 256-byte row of s_h (phase 2 writes, phase 3
// reads): no conflicts.  The staged rows are packed (pitch PH_TW + 2 R4 bytes), so phase 1 writes consecutive dwords too.
// VEC = C == 1, W % 4 == 0 and 4-byte aligned pointers: the 4 pixels are one 32-bit store; otherwise guarded byte stores.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/oct_unet.h"

#ifndef OCT_PHOTO_TILE_ROWS
#define OCT_PHOTO_TILE_ROWS 32      // rows of a tile (DESIGN.md section 39 has the times at 16, 32 and 64)
#endif

namespace oct {

enum {
    PH_TH = OCT_PHOTO_TILE_ROWS, PH_TW = 128, PH_GROUPS = PH_TW / 4, PH_THREADS = 256,
    PH_ROWS = PH_TH + 2 * OCT_PHOTO_MAX_RADIUS,      // staged rows at R = 8
    PH_PITCH = PH_TW + 2 * OCT_PHOTO_MAX_RADIUS,     // staged bytes per row at R4 = 8
};
static_assert(PH_GROUPS == 32, "a row of the tile is one 32-lane group of the LDS bank rules");
static_assert(OCT_PHOTO_MAX_RADIUS == 8 && OCT_PHOTO_MAX_SHADOWS == 4, "the passes are unrolled for R4 in {4, 8}, the gains for 4 shadows");

struct PhotoGeom {
    int H, W, C;
    unsigned n;        // H*W*C elements of one image
    unsigned tiles_x;  // tiles across one row of tiles
};

// phase 2 for one staged row and group: NW = R4 / 4.  src: the row's first staged dword of this group (the pixel group
// itself starts NW dwords further); w[k]: the weights.
template <int NW>
__device__ __forceinline__ uint2 photo_hpass(const uint32_t* __restrict__ src, const unsigned (&w)[9]) {
    unsigned b[8 * NW + 4];
#pragma unroll
    for (int i = 0; i < 2 * NW + 1; ++i) {
        const uint32_t d = src[i];
#pragma unroll
        for (int e = 0; e < 4; ++e) b[4 * i + e] = (d >> (8 * e)) & 255u;
    }
    unsigned acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        acc[j] = w[0] * b[4 * NW + j];
#pragma unroll
        for (int k = 1; k <= 4 * NW; ++k) acc[j] += w[k] * (b[4 * NW + j - k] + b[4 * NW + j + k]);
    }
    return make_uint2(acc[0] | (acc[1] << 16), acc[2] | (acc[3] << 16));
}

template <bool VEC>
__global__ __launch_bounds__(PH_THREADS) void photo_k(const unsigned char* __restrict__ x, const oct_photo_op* __restrict__ ops,
                                                      PhotoGeom g, unsigned char* __restrict__ out) {
    __shared__ __align__(16) unsigned char s_src[PH_ROWS * PH_PITCH];          // staged bytes, pitch PH_TW + 2 R4
    __shared__ __align__(16) unsigned short s_h[PH_ROWS * PH_TW];              // horizontal sums
    __shared__ __align__(8) unsigned short s_g[OCT_PHOTO_MAX_SHADOWS][PH_TW];  // g_s of the tile's columns
    __shared__ __align__(4) unsigned char s_lut[256];
    __shared__ unsigned s_w[OCT_PHOTO_MAX_RADIUS + 1];

    const unsigned b = blockIdx.y, tid = threadIdx.x;
    const oct_photo_op* __restrict__ op = ops + b;
    const int H = g.H, W = g.W;
    const unsigned C = (unsigned)g.C;
    const int R = op->radius, ns = op->n_shadows;
    int kind = op->kind;
    int y0s[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) y0s[s] = op->y0[s];
    {   // descriptors outside the definition pass through (the host refuses them before upload)
        bool ok = (unsigned)kind <= 7u && (unsigned)R <= (unsigned)OCT_PHOTO_MAX_RADIUS && ns <= OCT_PHOTO_MAX_SHADOWS;
#pragma unroll
        for (int s = 0; s < 4; ++s) ok = ok && (s >= ns || op->hw[s] >= 1);
        if (!ok) kind = 0;
    }
    const bool blur = (kind & OCT_PHOTO_BLUR) && R > 0;         // R = 0: w[0] = 256, the identity
    const bool shadow = (kind & OCT_PHOTO_SHADOW) && ns > 0, table = (kind & OCT_PHOTO_LUT) != 0;
    const int ty0 = (int)(blockIdx.x / g.tiles_x) * PH_TH, tx0 = (int)(blockIdx.x % g.tiles_x) * PH_TW;
    const int th = min((int)PH_TH, H - ty0), tw = min((int)PH_TW, W - tx0);      // the tile's rows and columns inside the image

    if (table && tid < 64) reinterpret_cast<uint32_t*>(s_lut)[tid] = reinterpret_cast<const uint32_t*>(op->lut)[tid];
    if (shadow)
        for (int t = (int)tid; t < ns * PH_TW; t += PH_THREADS) {
            const int s = t / PH_TW, xl = t % PH_TW, hw = op->hw[s];
            const int d = abs(tx0 + xl - (int)op->cx[s]);
            // strength above 256 (refused on the host) would leave 0..256: the store keeps 16 bits, the reads below mask
            s_g[s][xl] = (unsigned short)(256 - ((int)op->strength[s] * max(0, hw - d)) / hw);
        }
    if (blur && tid <= (unsigned)OCT_PHOTO_MAX_RADIUS) s_w[tid] = op->w[tid];
    __syncthreads();

    const unsigned char* xs = x + (size_t)b * g.n;
    unsigned char* os = out + (size_t)b * g.n;

    // v (4 pixels of row y from column xg, group gi of the tile) through the shadows and the table
    auto finish = [&](unsigned (&v)[4], int y, int gi) {
        if (shadow) {
            unsigned gg[4] = {256u, 256u, 256u, 256u};
#pragma unroll
            for (int s = 0; s < 4; ++s)
                if (s < ns && y >= y0s[s]) {
                    const uint2 q = *reinterpret_cast<const uint2*>(&s_g[s][4 * gi]);
                    gg[0] = min(gg[0], q.x & 0xffffu); gg[1] = min(gg[1], q.x >> 16);
                    gg[2] = min(gg[2], q.y & 0xffffu); gg[3] = min(gg[3], q.y >> 16);
                }
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = (v[j] * gg[j] + 128u) >> 8;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = table ? s_lut[v[j] & 255u] : (v[j] & 255u);
    };

    if (!blur) {
        for (int it = (int)tid; it < PH_TH * PH_GROUPS; it += PH_THREADS) {
            const int ly = it / PH_GROUPS, gi = it % PH_GROUPS;
            if (ly >= th || 4 * gi >= tw) continue;
            const int y = ty0 + ly, xg = tx0 + 4 * gi;
            const unsigned p0 = (unsigned)y * (unsigned)W + (unsigned)xg;      // the group's first pixel inside the sample
            unsigned v[4];
            if constexpr (VEC) {
                const uint32_t d = *reinterpret_cast<const uint32_t*>(xs + p0);
                if (kind) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) v[j] = (d >> (8 * j)) & 255u;
                    finish(v, y, gi);
                    *reinterpret_cast<uint32_t*>(os + p0) = v[0] | (v[1] << 8) | (v[2] << 16) | (v[3] << 24);
                } else {
                    *reinterpret_cast<uint32_t*>(os + p0) = d;
                }
            } else {
                const int np = min(4, W - xg);
                for (unsigned c = 0; c < C; ++c) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) v[j] = j < np ? xs[(p0 + j) * C + c] : 0u;
                    if (kind) finish(v, y, gi);
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (j < np) os[(p0 + j) * C + c] = (unsigned char)v[j];
                }
            }
        }
        return;
    }

    const int R4 = (R + 3) & ~3, NW = R4 >> 2;          // 4 or 8; 1 or 2
    const int rows = th + 2 * R, ndw = PH_GROUPS + 2 * NW;      // staged rows; dwords per staged row
    unsigned w[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) w[k] = op->w[k];
    uint32_t* src32 = reinterpret_cast<uint32_t*>(s_src);

    for (unsigned c = 0; c < C; ++c) {
        if (c) __syncthreads();         // the last channel's readers of s_src and s_h are done
        // phase 1: staged row r is image row clamp(ty0 - R + r), staged dword d starts at column tx0 - R4 + 4 d
        for (int t = (int)tid; t < rows * ndw; t += PH_THREADS) {
            const int r = t / ndw, d = t - r * ndw;
            const int y = min(max(ty0 - R + r, 0), H - 1), xg = tx0 - R4 + 4 * d;
            const unsigned row = (unsigned)y * (unsigned)W;
            uint32_t v;
            if constexpr (VEC) {        // W % 4 == 0 and xg % 4 == 0: the dword is inside the row, or outside it
                if (xg >= 0 && xg < W) v = *reinterpret_cast<const uint32_t*>(xs + row + (unsigned)xg);
                else v = 0x01010101u * xs[row + (xg < 0 ? 0u : (unsigned)(W - 1))];
            } else {
                v = 0;
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    v |= (uint32_t)xs[(row + (unsigned)min(max(xg + e, 0), W - 1)) * C + c] << (8 * e);
            }
            src32[t] = v;
        }
        __syncthreads();
        // phase 2
        for (int t = (int)tid; t < rows * PH_GROUPS; t += PH_THREADS) {
            const int r = t / PH_GROUPS, gi = t % PH_GROUPS;
            if (4 * gi >= tw) continue;
            const uint32_t* p = src32 + r * ndw + gi;
            *reinterpret_cast<uint2*>(&s_h[r * PH_TW + 4 * gi]) = NW == 1 ? photo_hpass<1>(p, w) : photo_hpass<2>(p, w);
        }
        __syncthreads();
        // phase 3: output row ly is staged row ly + R
        for (int it = (int)tid; it < PH_TH * PH_GROUPS; it += PH_THREADS) {
            const int ly = it / PH_GROUPS, gi = it % PH_GROUPS;
            if (ly >= th || 4 * gi >= tw) continue;
            const int y = ty0 + ly, xg = tx0 + 4 * gi;
            unsigned v[4] = {32768u, 32768u, 32768u, 32768u};
            for (int j = -R; j <= R; ++j) {
                const unsigned wj = s_w[abs(j)];
                const uint2 q = *reinterpret_cast<const uint2*>(&s_h[(ly + R + j) * PH_TW + 4 * gi]);
                v[0] += wj * (q.x & 0xffffu); v[1] += wj * (q.x >> 16);
                v[2] += wj * (q.y & 0xffffu); v[3] += wj * (q.y >> 16);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] >>= 16;
            finish(v, y, gi);
            const unsigned p0 = (unsigned)y * (unsigned)W + (unsigned)xg;
            if constexpr (VEC) {
                *reinterpret_cast<uint32_t*>(os + p0) = v[0] | (v[1] << 8) | (v[2] << 16) | (v[3] << 24);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (xg + j < W) os[(p0 + j) * C + c] = (unsigned char)v[j];
            }
        }
    }
}

}  // namespace oct
