// The evaluation / prediction pictures on the device: a base layer (the scan, or a class map through a palette) and K
// anti-aliased polylines over it, rasterised into (B,H,W,4) uint8 RGBA.  The rule is in include/oct_unet.h
// (oct_render_rgba) and restated in numpy by common/plotting.py::render_reference; it is integer arithmetic throughout, so
// the bytes equal numpy's.
//
//   render_rgba_k   A block owns kRenderCols columns x kRenderRows rows of one image; a thread owns one column of the tile
//                   and walks kRenderRows / (kRenderThreads / kRenderCols) of its rows, so a wave's store is 64 adjacent
//                   pixels = 256 contiguous bytes of an output row (one dword per lane where out is 4-byte aligned).
//                   The block stages rows[k][c] of every line for its columns plus a halo of ceil((R+3)/8)+1 columns on
//                   either side into LDS as uint16, with 0 wherever the column holds no vertex (outside the image, outside
//                   [col_lo, col_hi], row 0, row >= H): a segment exists where two neighbouring entries are non-zero.
//                   A sample at x can only be within R of a segment between columns j and j+1 when 8j - R <= x <= 8j + 8 + R,
//                   which for a pixel of column c (x in 8c-3..8c+3) leaves j in c-1-hw .. c+hw, hw = ceil((R+3)/8).
//                   Per line the thread walks those segments, rejects one by its row range (32-bit) and only then tests the
//                   16 samples in int64; the hits of all segments are OR-ed into a 16-bit mask, whose popcount is the
//                   coverage.  The blend runs in registers, line after line.  With K = 0 the block is a streaming copy.
//                   The palette, line colours and styles sit in the kernel's arguments (RenderArgs, by value).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/oct_unet.h"

namespace oct {

constexpr int kRenderThreads = 256;
constexpr int kRenderCols = 64;                                   // columns per block: one wave per row of threads
constexpr int kRenderRows = 16;                                   // rows per block: 4 per thread
constexpr int kRenderMaxR = 64;                                   // half_width, eighths of a pixel
constexpr int kRenderMaxHalo = (kRenderMaxR + 3 + 7) / 8 + 1;     // 10 columns on either side
constexpr int kRenderMaxH = 4096;                                 // keeps every product of the sample test inside int64

struct RenderArgs {
    const unsigned char* base;
    const unsigned short* rows;
    unsigned char* out;
    int mode, ic, H, W;
    oct_render_style st;
};

// is sample (wx, wy) -- relative to P0 -- within R of the segment P0 -> P0 + (8, dy)?  (include/oct_unet.h, "on")
__device__ __forceinline__ bool render_on_segment(int wx, int wy, int dy, long long RR) {
    const long long t = 8LL * wx + (long long)wy * dy;
    const long long den = 64LL + (long long)dy * dy;
    const long long ww = (long long)wx * wx + (long long)wy * wy;
    if (t <= 0) return ww <= RR;
    if (t >= den) {
        const long long ex = wx - 8, ey = wy - dy;
        return ex * ex + ey * ey <= RR;
    }
    return ww * den - t * t <= RR * den;
}

__global__ void __launch_bounds__(kRenderThreads) render_rgba_k(const RenderArgs a) {
    __shared__ unsigned short s_rows[OCT_RENDER_MAX_LINES][kRenderCols + 2 * kRenderMaxHalo];
    const int H = a.H, W = a.W, K = a.st.n_lines, R = a.st.half_width;
    const int hw = (R + 3 + 7) / 8, halo = hw + 1;
    const int span = kRenderCols + 2 * halo;
    const int c0 = (int)blockIdx.x * kRenderCols, r0 = (int)blockIdx.y * kRenderRows;
    const size_t b = blockIdx.z;
    if (K > 0) {
        const unsigned short* rows = a.rows + b * (size_t)K * W;
        for (int i = threadIdx.x; i < K * span; i += kRenderThreads) {
            const int k = i / span, j = i - k * span;
            const int c = c0 - halo + j;
            unsigned short v = 0;
            if (c >= 0 && c < W && c >= a.st.col_lo && c <= a.st.col_hi) {
                v = rows[(size_t)k * W + c];
                if ((int)v >= H) v = 0;
            }
            s_rows[k][j] = v;
        }
        __syncthreads();
    }
    const int tx = threadIdx.x % kRenderCols, ty = threadIdx.x / kRenderCols;
    const int c = c0 + tx;
    if (c >= W) return;
    // the dotted pattern depends on the sample's x alone: 4 bits by ox, repeated for the 4 values of oy
    unsigned dot4 = 0;
#pragma unroll
    for (int ix = 0; ix < 4; ++ix) {
        int m = (8 * (c - a.st.col_lo) + 2 * ix - 3) % 120;
        if (m < 0) m += 120;
        if (m < 48) dot4 |= 1u << ix;
    }
    const unsigned dot16 = dot4 * 0x1111u;
    const long long RR = (long long)R * R;
    const bool dword = ((uintptr_t)a.out & 3) == 0;
    for (int r = r0 + ty; r < r0 + kRenderRows && r < H; r += kRenderThreads / kRenderCols) {
        const size_t pix = (b * H + r) * (size_t)W + c;
        int cr, cg, cb;
        if (a.mode == OCT_RENDER_BASE_LABELS) {
            const int lab = a.base[pix];
            if (lab < a.st.n_cls) {
                cr = a.st.palette[3 * lab]; cg = a.st.palette[3 * lab + 1]; cb = a.st.palette[3 * lab + 2];
            } else {
                cr = cg = cb = 0;
            }
        } else {
            const unsigned char* p = a.base + pix * (size_t)a.ic;
            cr = p[0];
            if (a.ic == 3) { cg = p[1]; cb = p[2]; } else { cg = cb = cr; }
        }
        for (int k = 0; k < K; ++k) {
            unsigned mask = 0;
            // segment j -> j+1 for j = c + d, d in -1-hw .. hw; s_rows index of column j is j - c0 + halo = tx + d + halo
            int prev = s_rows[k][tx + halo - 1 - hw];
            for (int d = -1 - hw; d <= hw; ++d) {
                const int next = s_rows[k][tx + halo + d + 1];
                const int v0 = prev, v1 = next;
                prev = next;
                if (v0 == 0 || v1 == 0) continue;
                const int lo = v0 < v1 ? v0 : v1, hi = v0 < v1 ? v1 : v0;
                if (8 * r + 3 < 8 * lo - R || 8 * r - 3 > 8 * hi + R) continue;         // no sample can be within R
                const int dy = 8 * (v1 - v0);
#pragma unroll
                for (int iy = 0; iy < 4; ++iy) {
                    const int wy = 8 * (r - v0) + 2 * iy - 3;
#pragma unroll
                    for (int ix = 0; ix < 4; ++ix) {
                        const int wx = 2 * ix - 3 - 8 * d;
                        if (render_on_segment(wx, wy, dy, RR)) mask |= 1u << (4 * iy + ix);
                    }
                }
            }
            if (a.st.line_style[k]) mask &= dot16;
            const int cov = __popc(mask);
            if (cov) {
                cr = (cov * a.st.line_rgb[3 * k] + (16 - cov) * cr + 8) >> 4;
                cg = (cov * a.st.line_rgb[3 * k + 1] + (16 - cov) * cg + 8) >> 4;
                cb = (cov * a.st.line_rgb[3 * k + 2] + (16 - cov) * cb + 8) >> 4;
            }
        }
        unsigned char* q = a.out + pix * 4;
        if (dword) {
            *reinterpret_cast<uchar4*>(q) = make_uchar4((unsigned char)cr, (unsigned char)cg, (unsigned char)cb, 255);
        } else {
            q[0] = (unsigned char)cr; q[1] = (unsigned char)cg; q[2] = (unsigned char)cb; q[3] = 255;
        }
    }
}

}  // namespace oct
