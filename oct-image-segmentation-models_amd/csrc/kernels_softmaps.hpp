// Soft boundary maps on the device: the reference's convert_predictions_to_maps_semantic (common/utils.py:115-168) on the
// class PROBABILITIES, i.e. on what perform_argmax(bin=False) hands it, where boundary_maps_k (kernels_fwd.hpp) takes the
// one-hot of the arg-max.  The definition is in include/oct_unet.h (oct_boundary_maps_soft) and restated in numpy by
// common/utils.py::soft_boundary_maps_reference; every step is one IEEE fp32 operation, so the bytes equal numpy's.
//
//   soft_maps_k<VC> probs (B,H,W,C) f32 -> maps (B, C-1, H, W) u8.  A work item is 4 adjacent columns of a strip of
//                   kSoftRows rows of one image; items are numbered (b, strip, column group) with the column group
//                   fastest, so a wave walks along a row: its loads cover one contiguous stretch of the row (64 x 4 pixels
//                   x C floats) and its stores are 256 adjacent bytes of a map row.  The item walks down its strip with
//                   g of the current row in registers and computes g of the next row ((r+1) mod H: the last row of an
//                   image takes row 0's), which reads the two rows around that one -- 2 (kSoftRows + 1) row reads for
//                   kSoftRows output rows; what neighbouring strips and the item itself read twice is left to the cache,
//                   nothing is staged in LDS.
//                   VC = C in 2..4, chosen by the launcher where W % 4 == 0 and probs is 16-byte aligned: the 4 pixels of
//                   a row are VC float4 loads and carry every channel, so all maps come from one pass.  VC = 0: any C, W
//                   and alignment; one pass per map with dword loads of the map's channel.
//                   The 4 bytes of a map row are one dword store where the address is 4-byte aligned and the group is
//                   whole, single bytes otherwise (any W, any base).  The grid is capped (kSoftMaxBlocks); the items
//                   beyond it are reached by the grid stride.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace oct {

constexpr int kSoftThreads = 256;
constexpr int kSoftCols = 4;             // columns per work item: one dword of a map row
constexpr int kSoftRows = 4;             // rows per work item
constexpr int kSoftMaxBlocks = 2048;     // 8 blocks per CU; larger batches stride
constexpr int kSoftMaxClasses = 32;

// the two rows np.gradient reads for `row` (one-sided at the edges, the same row twice where H == 1) and whether it halves
__device__ __forceinline__ void soft_rows(int row, int H, int& lo, int& hi, bool& mid) {
    lo = row > 0 ? row - 1 : 0;
    hi = row + 1 < H ? row + 1 : H - 1;
    mid = row > 0 && row + 1 < H;
}

// g = 2 * max(+-d, 0) from the two rows' values
__device__ __forceinline__ float soft_g(float f_lo, float f_hi, bool mid, bool flip) {
#pragma clang fp contract(off)
    float d = f_hi - f_lo;
    if (mid) d = d / 2.0f;
    if (flip) d = -d;
    return 2.0f * fmaxf(d, 0.f);
}

// one map row's 4 bytes from g of the row and of the next one; numpy's float32 -> uint8 cast truncates, then wraps
__device__ __forceinline__ void soft_store(unsigned char* q, int nc, const float (&g0)[kSoftCols], const float (&g1)[kSoftCols]) {
#pragma clang fp contract(off)
    unsigned char v8[kSoftCols];
#pragma unroll
    for (int j = 0; j < kSoftCols; ++j) {
        const float v = fmaxf(g0[j] - g1[j], 0.f);
        v8[j] = (unsigned char)((int)(v * 255.0f) & 255);
    }
    if (nc == kSoftCols && ((uintptr_t)q & 3) == 0) {
        *reinterpret_cast<uchar4*>(q) = make_uchar4(v8[0], v8[1], v8[2], v8[3]);
    } else {
#pragma unroll
        for (int j = 0; j < kSoftCols; ++j)
            if (j < nc) q[j] = v8[j];
    }
}

// items = B * ceil(H / kSoftRows) * ceil(W / 4)
template <int VC>
__global__ void __launch_bounds__(kSoftThreads) soft_maps_k(const float* __restrict__ probs, unsigned char* __restrict__ maps,
                                                            size_t items, int H, int W, int C, int bg_ilm, int bg_csi) {
    const int groups = (W + kSoftCols - 1) / kSoftCols;
    const int strips = (H + kSoftRows - 1) / kSoftRows;
    const size_t stride = (size_t)gridDim.x * kSoftThreads;
    for (size_t it = (size_t)blockIdx.x * kSoftThreads + threadIdx.x; it < items; it += stride) {
        const int c0 = (int)(it % groups) * kSoftCols;
        const size_t t = it / groups;
        const int r0 = (int)(t % strips) * kSoftRows;
        const size_t b = t / strips;
        const float* img = probs + b * (size_t)H * W * C;
        unsigned char* out = maps + b * (size_t)(C - 1) * H * W + c0;             // + (m - 1) H W + r W
        const int nc = W - c0 < kSoftCols ? W - c0 : kSoftCols;                  // columns of this item inside the image
        if constexpr (VC > 0) {
            // every channel of the 4 pixels of a row: VC float4 (W % 4 == 0 and a 16-byte aligned base: the launcher)
            auto g_row = [&](int row, float (&g)[VC - 1][kSoftCols]) {
                int lo, hi; bool mid;
                soft_rows(row, H, lo, hi, mid);
                const float4* p_lo = reinterpret_cast<const float4*>(img + ((size_t)lo * W + c0) * VC);
                const float4* p_hi = reinterpret_cast<const float4*>(img + ((size_t)hi * W + c0) * VC);
                float f_lo[kSoftCols * VC], f_hi[kSoftCols * VC];
#pragma unroll
                for (int q = 0; q < VC; ++q) {
                    const float4 a = p_lo[q], c = p_hi[q];
                    f_lo[4 * q] = a.x; f_lo[4 * q + 1] = a.y; f_lo[4 * q + 2] = a.z; f_lo[4 * q + 3] = a.w;
                    f_hi[4 * q] = c.x; f_hi[4 * q + 1] = c.y; f_hi[4 * q + 2] = c.z; f_hi[4 * q + 3] = c.w;
                }
#pragma unroll
                for (int m = 1; m < VC; ++m) {
                    const bool flip = (m == 1 && bg_ilm) || (m == VC - 1 && bg_csi);
#pragma unroll
                    for (int j = 0; j < kSoftCols; ++j) {
                        // (k = flip ? m - 1 : m, selected between two compile-time indices)
                        const float a = flip ? f_lo[j * VC + m - 1] : f_lo[j * VC + m];
                        const float c = flip ? f_hi[j * VC + m - 1] : f_hi[j * VC + m];
                        g[m - 1][j] = soft_g(a, c, mid, flip);
                    }
                }
            };
            float g0[VC - 1][kSoftCols], g1[VC - 1][kSoftCols];
            g_row(r0, g0);
#pragma unroll
            for (int i = 0; i < kSoftRows; ++i) {
                const int r = r0 + i;
                if (r >= H) break;
                g_row(r + 1 == H ? 0 : r + 1, g1);
#pragma unroll
                for (int m = 1; m < VC; ++m) {
                    soft_store(out + ((size_t)(m - 1) * H + r) * W, nc, g0[m - 1], g1[m - 1]);
#pragma unroll
                    for (int j = 0; j < kSoftCols; ++j) g0[m - 1][j] = g1[m - 1][j];
                }
            }
        } else {
            for (int m = 1; m < C; ++m) {
                const bool flip = (m == 1 && bg_ilm) || (m == C - 1 && bg_csi);
                const int k = flip ? m - 1 : m;
                auto g_row = [&](int row, float (&g)[kSoftCols]) {
                    int lo, hi; bool mid;
                    soft_rows(row, H, lo, hi, mid);
                    const float* p_lo = img + ((size_t)lo * W + c0) * C + k;
                    const float* p_hi = img + ((size_t)hi * W + c0) * C + k;
#pragma unroll
                    for (int j = 0; j < kSoftCols; ++j)
                        g[j] = j < nc ? soft_g(p_lo[(size_t)j * C], p_hi[(size_t)j * C], mid, flip) : 0.f;
                };
                float g0[kSoftCols], g1[kSoftCols];
                g_row(r0, g0);
                for (int i = 0; i < kSoftRows; ++i) {
                    const int r = r0 + i;
                    if (r >= H) break;
                    g_row(r + 1 == H ? 0 : r + 1, g1);
                    soft_store(out + ((size_t)(m - 1) * H + r) * W, nc, g0, g1);
#pragma unroll
                    for (int j = 0; j < kSoftCols; ++j) g0[j] = g1[j];
                }
            }
        }
    }
}

}  // namespace oct
