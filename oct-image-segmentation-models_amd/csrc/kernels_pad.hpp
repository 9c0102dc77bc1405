// Pad and crop on the device, for scans whose size is no multiple of 2^pool_layers: pad_k places a (B,H,W,ch) batch at
// (top, left) of a (B,Hp,Wp,ch) one and fills the frame by the border rule; crop_k takes the (B,H,W) window at (top, left)
// out of (B,Hp,Wp) pixels of `pb` bytes each.  The definitions are include/oct_unet.h, oct_pad_batch / oct_crop_batch;
// common/utils.py pad_reference / crop_reference restate them in numpy.  Both kernels only move bytes: nothing depends on
// the element type beyond the width of the constant.
//
// Layout of the work.  Grid (x: 16-byte chunks of a destination row, y: rows of an image, z: images), a grid-stride loop on
// each axis, so no index is ever divided.  A destination row is cut at ABSOLUTE 16-byte addresses: chunk j of a row that
// starts at address a covers [16 j - (a & 15), +16) of the row, clipped to the row.  A whole chunk is one 16-byte store;
// the clipped chunks at the two ends of a row (rows of W * pb bytes start anywhere) are byte stores.  A whole chunk whose
// bytes all come from one contiguous run of the source -- every chunk of crop_k, the chunks inside the image of pad_k -- is
// loaded by load16: one 16-byte load where the source address is a multiple of 4 (global multi-dword loads need dword
// alignment only), else five aligned dwords shifted into place, else 16 byte loads next to the ends of the source buffer,
// where the dwords would reach outside it.  Every other chunk (the frame of pad_k, the clipped ends) gathers byte by
// byte through the border rule.  No LDS.  Addresses are size_t; positions inside a row are 32-bit (the host refuses rows of
// 2^31 bytes or more).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/oct_unet.h"

namespace oct {

struct PadArgs {
    const unsigned char* src; unsigned char* dst;
    size_t src_bytes;          // of the whole source buffer: load16 stays inside it
    int B, H, W, Hp, Wp, top, left, mode;
    int pb, es;                // bytes of a pixel (ch * es) and of an element (1 or 4)
    unsigned value;            // the constant's bytes, little endian (es of them count)
};

struct CropArgs {
    const unsigned char* src; unsigned char* dst;
    size_t src_bytes;
    int B, Hp, Wp, H, W, top, left, pb;
};

struct __attribute__((packed, aligned(4))) PadDwords4 { uint32_t v[4]; };

// source index of i on an axis of length n: edge clamps, reflect mirrors about the border pixel without repeating it
// (|pad| < n, checked on the host, so one mirror is enough), constant answers -1 outside
__device__ __forceinline__ int pad_index(int i, int n, int mode) {
    if (mode == OCT_PAD_EDGE) return min(max(i, 0), n - 1);
    if (mode == OCT_PAD_REFLECT) return i < 0 ? -i : (i >= n ? 2 * (n - 1) - i : i);
    return (unsigned)i < (unsigned)n ? i : -1;
}

// 16 contiguous bytes at p, which need no alignment; [base, base + bytes) is the buffer p points into
__device__ __forceinline__ uint4 load16(const unsigned char* p, const unsigned char* base, size_t bytes) {
    const unsigned s = (unsigned)((uintptr_t)p & 3);
    uint4 r;
    if (s == 0) {
        const PadDwords4 d = *reinterpret_cast<const PadDwords4*>(p);
        r = make_uint4(d.v[0], d.v[1], d.v[2], d.v[3]);
    } else if (p - s >= base && p - s + 20 <= base + bytes) {
        const uint32_t* q = reinterpret_cast<const uint32_t*>(p - s);
        const uint32_t w0 = q[0], w1 = q[1], w2 = q[2], w3 = q[3], w4 = q[4];
        const unsigned lo = 8 * s, hi = 32 - lo;       // s in 1..3: neither shift is by 0 or 32
        r = make_uint4((w0 >> lo) | (w1 << hi), (w1 >> lo) | (w2 << hi), (w2 >> lo) | (w3 << hi), (w3 >> lo) | (w4 << hi));
    } else {
        uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
        for (int k = 0; k < 16; ++k) w[k >> 2] |= (uint32_t)p[k] << (8 * (k & 3));
        r = make_uint4(w[0], w[1], w[2], w[3]);
    }
    return r;
}

// bytes k of w (16 of them, little endian) for which c0 + k lies in [0, row_bytes) -> d[c0 + k]
__device__ __forceinline__ void store_clipped(unsigned char* d, int c0, int row_bytes, const uint32_t (&w)[4]) {
#pragma unroll
    for (int k = 0; k < 16; ++k)
        if ((unsigned)(c0 + k) < (unsigned)row_bytes) d[c0 + k] = (unsigned char)(w[k >> 2] >> (8 * (k & 3)));
}

__global__ __launch_bounds__(256) void pad_k(PadArgs a) {
    const int rb_dst = a.Wp * a.pb, rb_src = a.W * a.pb;
    const int in_lo = a.left * a.pb, in_hi = in_lo + rb_src;        // the image's bytes inside a destination row
    for (int b = blockIdx.z; b < a.B; b += gridDim.z) {
        for (int y = blockIdx.y * blockDim.y + threadIdx.y; y < a.Hp; y += gridDim.y * blockDim.y) {
            unsigned char* drow = a.dst + ((size_t)b * a.Hp + y) * (size_t)rb_dst;
            const int a0 = (int)((uintptr_t)drow & 15), chunks = (a0 + rb_dst + 15) >> 4;
            const int sy = pad_index(y - a.top, a.H, a.mode);
            const unsigned char* srow = a.src + ((size_t)b * a.H + (sy < 0 ? 0 : sy)) * (size_t)rb_src;
            for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < chunks; j += gridDim.x * blockDim.x) {
                const int c0 = 16 * j - a0;                          // row position of the chunk's first byte (may be < 0)
                const bool whole = c0 >= 0 && c0 + 16 <= rb_dst;
                if (whole && sy >= 0 && c0 >= in_lo && c0 + 16 <= in_hi) {
                    *reinterpret_cast<uint4*>(drow + c0) = load16(srow + (c0 - in_lo), a.src, a.src_bytes);
                    continue;
                }
                // gather: pixel px, byte kk of it; one division for the first byte, then counted up
                const int first = max(c0, 0);
                int px = first / a.pb, kk = first - px * a.pb;
                uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
                for (int k = 0; k < 16; ++k) {
                    if ((unsigned)(c0 + k) >= (unsigned)rb_dst) continue;
                    const int sx = pad_index(px - a.left, a.W, a.mode);
                    const unsigned v = (sy < 0 || sx < 0) ? (a.value >> (8 * (kk % a.es))) & 255u : srow[(size_t)sx * a.pb + kk];
                    w[k >> 2] |= v << (8 * (k & 3));
                    if (++kk == a.pb) { kk = 0; ++px; }
                }
                if (whole) *reinterpret_cast<uint4*>(drow + c0) = make_uint4(w[0], w[1], w[2], w[3]);
                else store_clipped(drow, c0, rb_dst, w);
            }
        }
    }
}

__global__ __launch_bounds__(256) void crop_k(CropArgs a) {
    const int rb_dst = a.W * a.pb;
    const size_t rb_src = (size_t)a.Wp * a.pb;
    for (int b = blockIdx.z; b < a.B; b += gridDim.z) {
        for (int y = blockIdx.y * blockDim.y + threadIdx.y; y < a.H; y += gridDim.y * blockDim.y) {
            unsigned char* drow = a.dst + ((size_t)b * a.H + y) * (size_t)rb_dst;
            const unsigned char* srow = a.src + ((size_t)b * a.Hp + y + a.top) * rb_src + (size_t)a.left * a.pb;
            const int a0 = (int)((uintptr_t)drow & 15), chunks = (a0 + rb_dst + 15) >> 4;
            for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < chunks; j += gridDim.x * blockDim.x) {
                const int c0 = 16 * j - a0;
                if (c0 >= 0 && c0 + 16 <= rb_dst) {
                    *reinterpret_cast<uint4*>(drow + c0) = load16(srow + c0, a.src, a.src_bytes);
                    continue;
                }
                uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
                for (int k = 0; k < 16; ++k)
                    if ((unsigned)(c0 + k) < (unsigned)rb_dst) w[k >> 2] |= (uint32_t)srow[c0 + k] << (8 * (k & 3));
                store_clipped(drow, c0, rb_dst, w);
            }
        }
    }
}

}  // namespace oct
