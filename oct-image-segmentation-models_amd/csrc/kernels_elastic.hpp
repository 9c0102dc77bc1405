// Elastic deformation on the device: (B,H,W,C) uint8 images -> uint8 images sampled bilinearly through a smooth random
// displacement field (a cubic B-spline over Philox-drawn control points every S pixels), and (B,H,W) uint8 labels moved
// alongside by nearest pixel.  The stage runs in front of warp_k (kernels_warp.hpp).  The definition is include/oct_unet.h,
// oct_elastic_batch; common/augmentation.py elastic_reference restates it in numpy.  Integer arithmetic only.
//
// elastic_k<VEC>: grid (tiles per sample, B): a block owns one EL_TH x EL_TW pixel tile of one sample, so the sample's
// descriptor is one uniform load and the branches on its kind, border and axes are uniform.  Three phases, two barriers:
//   1. the tile's own control points (at most EL_NYC x EL_NXC: the cells the tile touches, + 3) by Philox straight into LDS;
//      beside them, one thread per tile column and tile row works out that position's cell and its four weight numerators
//      (the only integer divisions by S);
//   2. the column interpolation, once per (control row, tile column): t = sum_b bx_b d[r][cx + b] for both axes, an int64
//      pair stored as [r][x % 4][x / 4] so that the 32 lanes of a row read 512 contiguous bytes (ds_read_b128) in phase 3;
//   3. a thread owns 4 adjacent pixels of a row: per pixel and axis four 32 x 64-bit multiply-adds over the control rows and
//      one floor division, then the image's bilinear gather (source bytes straight from global memory, as warp_k) for each
//      channel and the label's nearest-pixel gather with the SAME displacement.
// The floor division by 36 S^6 (< 2^48) is a multiply by the reciprocal in double precision and one exact integer correction:
// the quotient is at most 2^13 in magnitude, so the estimate is off by far less than one and a single step repairs it.
// VEC = C == 1, W % 4 == 0 and 4-byte aligned pointers: the 4 pixels are one 32-bit store; otherwise guarded byte stores.
// A sample that is not deformed is copied.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/oct_unet.h"
#include "kernels_warp.hpp"
#include "philox.hpp"

namespace oct {

enum { ELASTIC_NONE = 0, ELASTIC_ON = 1 };
enum {
    EL_TH = 16, EL_TW = 128, EL_GROUPS = EL_TW / 4,
    // floor((p0 + n - 1) / S) - floor(p0 / S) <= ceil((n - 1) / S): control rows / columns a tile can touch at the smallest S
    EL_NYC = (EL_TH - 1) / OCT_ELASTIC_MIN_SPACING + 5,
    EL_NXC = (EL_TW - 1) / OCT_ELASTIC_MIN_SPACING + 5,
};
static_assert((EL_TH - 1) % OCT_ELASTIC_MIN_SPACING == 1 && (EL_TW - 1) % OCT_ELASTIC_MIN_SPACING == 1,
              "EL_NYC / EL_NXC round (n - 1) / S up by adding one: n - 1 must not divide by the smallest S");

struct ElasticGeom {
    int H, W, C;
    unsigned n;        // H*W*C elements of one image
    unsigned nl;       // H*W elements of one label map
    unsigned tiles_x;  // tiles across one row of tiles
};

// the four weight numerators over 6 S^3 at offset k of a cell: all >= 0, their sum is 6 S^3 <= 2^24
__device__ __forceinline__ void elastic_weights(int k, int S, int w[4]) {
    const int k2 = k * k, k3 = k2 * k, S2 = S * S, S3 = S2 * S, m = S - k;
    w[0] = m * m * m;
    w[1] = 3 * k3 - 6 * S * k2 + 4 * S3;
    w[2] = -3 * k3 + 3 * S * k2 + 3 * S2 * k + S3;
    w[3] = k3;
}

// floor((N + D/2) / D) for |N| <= 2^13 D, D = 36 S^6 < 2^48, rD = 1.0 / D
__device__ __forceinline__ int elastic_round_div(int64_t N, int64_t D, double rD) {
    const int64_t n = N + (D >> 1);
    int q = __double2int_rd((double)n * rD);
    const int64_t r = n - (int64_t)q * D;
    if (r < 0) --q;
    else if (r >= D) ++q;
    return q;
}

// one output byte of the image at pixel (x, y) displaced by (dx, dy) 1/256 pixel: bilinear in 8-bit fractions
__device__ __forceinline__ unsigned elastic_byte(const unsigned char* __restrict__ s, int x, int y, int dx, int dy, int H, int W,
                                                 unsigned C, unsigned c, int border, unsigned fill) {
    const int sx = 256 * x + dx, sy = 256 * y + dy;
    const int ix = sx >> 8, iy = sy >> 8;
    const unsigned fx = (unsigned)sx & 255u, fy = (unsigned)sy & 255u;
    const int x0 = warp_border(ix, W, border), x1 = warp_border(ix + 1, W, border);
    const int y0 = warp_border(iy, H, border), y1 = warp_border(iy + 1, H, border);
    auto tap = [&](int yy, int xx) -> unsigned {
        return (yy | xx) < 0 ? fill : s[((unsigned)yy * (unsigned)W + (unsigned)xx) * C + c];
    };
    const unsigned acc = (256u - fx) * (256u - fy) * tap(y0, x0) + fx * (256u - fy) * tap(y0, x1) +
                         (256u - fx) * fy * tap(y1, x0) + fx * fy * tap(y1, x1);
    return (acc + 32768u) >> 16;
}

// one label: the nearest source pixel
__device__ __forceinline__ unsigned elastic_label(const unsigned char* __restrict__ s, int x, int y, int dx, int dy, int H, int W,
                                                  int border, unsigned fill) {
    const int xx = warp_border((256 * x + dx + 128) >> 8, W, border), yy = warp_border((256 * y + dy + 128) >> 8, H, border);
    return (yy | xx) < 0 ? fill : s[(unsigned)yy * (unsigned)W + (unsigned)xx];
}

template <bool VEC>
__global__ __launch_bounds__(256) void elastic_k(const unsigned char* __restrict__ x, const unsigned char* __restrict__ lab,
                                                 const oct_elastic_op* __restrict__ ops, ElasticGeom g,
                                                 unsigned char* __restrict__ out, unsigned char* __restrict__ lab_out) {
    __shared__ int2 s_ctrl[EL_NYC][EL_NXC];                             // (dx, dy) of the tile's control points
    __shared__ __align__(16) int64_t s_t[EL_NYC][4][EL_GROUPS][2];      // column-interpolated (x, y) sums, [r][x % 4][x / 4]
    __shared__ int s_wx[EL_TW][4], s_wy[EL_TH][4];                      // weight numerators of the tile's columns and rows
    __shared__ int s_cx[EL_TW], s_cy[EL_TH];                            // ... and their first control column / row in s_ctrl

    const unsigned b = blockIdx.y, tid = threadIdx.x;
    const oct_elastic_op op = ops[b];
    const int S = op.spacing, H = g.H, W = g.W;
    // unknown kinds, borders, spacings and amplitudes pass through
    const bool on = op.kind == ELASTIC_ON && (unsigned)op.border <= (unsigned)WARP_CONSTANT && S >= OCT_ELASTIC_MIN_SPACING &&
                    S <= OCT_ELASTIC_MAX_SPACING && (unsigned)op.amp_x <= (unsigned)OCT_ELASTIC_MAX_AMP &&
                    (unsigned)op.amp_y <= (unsigned)OCT_ELASTIC_MAX_AMP;
    const int ty0 = (int)(blockIdx.x / g.tiles_x) * EL_TH, tx0 = (int)(blockIdx.x % g.tiles_x) * EL_TW;
    const int th = min((int)EL_TH, H - ty0), tw = min((int)EL_TW, W - tx0);      // the tile's rows and columns inside the image

    int64_t D = 1;
    double rD = 1.0;
    if (on) {
        const int cx0 = tx0 / S, cy0 = ty0 / S;
        const int nxc = (tx0 + tw - 1) / S - cx0 + 4, nyc = (ty0 + th - 1) / S - cy0 + 4;       // <= EL_NXC, EL_NYC
        for (int t = (int)tid; t < nyc * nxc; t += 256) {
            const int r = t / nxc, c = t - r * nxc;
            const Philox4 w = philox4x32_10((uint32_t)(cx0 + c), (uint32_t)(cy0 + r), 0u, 0x454C4153u, op.seed_lo, op.seed_hi);
            s_ctrl[r][c] = make_int2((int)(((uint64_t)w.w[0] * (uint32_t)(2 * op.amp_x + 1)) >> 32) - op.amp_x,
                                     (int)(((uint64_t)w.w[1] * (uint32_t)(2 * op.amp_y + 1)) >> 32) - op.amp_y);
        }
        if ((int)tid < tw + th) {       // one thread per column, then per row, of the tile
            const bool row = (int)tid >= tw;
            const int l = row ? (int)tid - tw : (int)tid, p = (row ? ty0 : tx0) + l, cell = p / S;
            int w[4];
            elastic_weights(p - cell * S, S, w);
            int* dst = row ? s_wy[l] : s_wx[l];
#pragma unroll
            for (int a = 0; a < 4; ++a) dst[a] = w[a];
            if (row) s_cy[l] = cell - cy0;
            else s_cx[l] = cell - cx0;
        }
        __syncthreads();
        for (int t = (int)tid; t < nyc * EL_TW; t += 256) {
            const int r = t / EL_TW, q = t % EL_TW, j = q / EL_GROUPS, gi = q % EL_GROUPS, xl = 4 * gi + j;
            if (xl >= tw) continue;
            const int c = s_cx[xl];
            int64_t ax = 0, ay = 0;
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                const int2 d = s_ctrl[r][c + a];
                const int w = s_wx[xl][a];
                ax += (int64_t)w * d.x;
                ay += (int64_t)w * d.y;
            }
            s_t[r][j][gi][0] = ax;
            s_t[r][j][gi][1] = ay;
        }
        __syncthreads();
        const int64_t S3 = (int64_t)S * S * S;
        D = 36 * S3 * S3;
        rD = 1.0 / (double)D;
    }

    const unsigned C = (unsigned)g.C;
    const unsigned char* xs = x + (size_t)b * g.n;
    unsigned char* os = out + (size_t)b * g.n;
    const unsigned char* ls = lab_out ? lab + (size_t)b * g.nl : nullptr;
    unsigned char* lo = lab_out ? lab_out + (size_t)b * g.nl : nullptr;
    const unsigned fill = (unsigned)op.fill & 255u, lfill = (unsigned)op.fill_label & 255u;

    for (int it = (int)tid; it < EL_TH * EL_GROUPS; it += 256) {
        const int ly = it / EL_GROUPS, gi = it % EL_GROUPS;
        if (ly >= th || 4 * gi >= tw) continue;
        const int y = ty0 + ly, xg = tx0 + 4 * gi;
        const unsigned p0 = (unsigned)y * (unsigned)W + (unsigned)xg;      // the group's first pixel inside the sample
        if (!on) {
            if constexpr (VEC) {
                *reinterpret_cast<uint32_t*>(os + p0) = *reinterpret_cast<const uint32_t*>(xs + p0);
                if (lo) *reinterpret_cast<uint32_t*>(lo + p0) = *reinterpret_cast<const uint32_t*>(ls + p0);
            } else {
                const int np = min(4, W - xg);
                for (unsigned e = p0 * C; e < (p0 + (unsigned)np) * C; ++e) os[e] = xs[e];
                if (lo)
                    for (int j = 0; j < np; ++j) lo[p0 + j] = ls[p0 + j];
            }
            continue;
        }
        int dx[4], dy[4];
        {
            const int r0 = s_cy[ly];
            int wy[4];
#pragma unroll
            for (int a = 0; a < 4; ++a) wy[a] = s_wy[ly][a];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                int64_t nx = 0, ny = 0;
                if (4 * gi + j < tw) {
#pragma unroll
                    for (int a = 0; a < 4; ++a) {
                        nx += (int64_t)wy[a] * s_t[r0 + a][j][gi][0];
                        ny += (int64_t)wy[a] * s_t[r0 + a][j][gi][1];
                    }
                }
                // an axis of amplitude 0 has a zero field: its pixels stay in their column (row)
                dx[j] = op.amp_x ? elastic_round_div(nx, D, rD) : 0;
                dy[j] = op.amp_y ? elastic_round_div(ny, D, rD) : 0;
            }
        }
        if constexpr (VEC) {
            uint32_t v = 0, lv = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) v |= elastic_byte(xs, xg + j, y, dx[j], dy[j], H, W, 1u, 0u, op.border, fill) << (8 * j);
            *reinterpret_cast<uint32_t*>(os + p0) = v;
            if (lo) {
#pragma unroll
                for (int j = 0; j < 4; ++j) lv |= elastic_label(ls, xg + j, y, dx[j], dy[j], H, W, op.border, lfill) << (8 * j);
                *reinterpret_cast<uint32_t*>(lo + p0) = lv;
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (xg + j >= W) break;
                for (unsigned c = 0; c < C; ++c)
                    os[(p0 + j) * C + c] = (unsigned char)elastic_byte(xs, xg + j, y, dx[j], dy[j], H, W, C, c, op.border, fill);
                if (lo) lo[p0 + j] = (unsigned char)elastic_label(ls, xg + j, y, dx[j], dy[j], H, W, op.border, lfill);
            }
        }
    }
}

}  // namespace oct
