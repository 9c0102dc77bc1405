// One translation unit of liboct_unet_hip.so (see host.hpp): pad and crop on the device (kernels_pad.hpp) and their C ABI,
// oct_pad_batch / oct_crop_batch (include/oct_unet.h).  The calls allocate nothing and never wait for the stream.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>

#include "../../include/oct_unet.h"
#include "host.hpp"
#include "kernels_pad.hpp"

using namespace oct;
using namespace octh;

namespace {

constexpr int kPadMaxDim = 1 << 30;                    // B, rows of an image, bytes of a row: the kernels' 32-bit loop counters
constexpr size_t kPadMaxBytes = (size_t)1 << 62;       // a whole buffer: its byte offsets are size_t

bool overlap(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + nb && b0 < a0 + na;
}

// B * rows * cols * pb bytes, or 0 where a row or the whole leaves the kernels' indexing
size_t checked_bytes(int B, int rows, int cols, int pb) {
    if (B > kPadMaxDim || rows > kPadMaxDim || (uint64_t)cols * (uint64_t)pb > (uint64_t)kPadMaxDim) return 0;
    size_t n = (size_t)cols * (size_t)pb;
    if (__builtin_mul_overflow(n, (size_t)rows, &n) || __builtin_mul_overflow(n, (size_t)B, &n) || n >= kPadMaxBytes) return 0;
    return n;
}

// Block (tx, 256 / tx): tx = the power of two in 16..256 that covers a row's chunks (a 768-byte row is 48 chunks: 64 x 4).
// Grid: the row's remaining chunks by x, rows by y, images by z, about 8192 blocks at the most; the loops do the rest.
void launch_shape(int row_bytes, int rows, int B, dim3& grid, dim3& block) {
    const int chunks = row_bytes / 16 + 2;
    int tx = 16;
    while (tx < 256 && tx < chunks) tx *= 2;
    const int ty = 256 / tx;
    const unsigned gx = (unsigned)std::min(cdiv(chunks, tx), 64), gz = (unsigned)std::min(B, 65535);
    const unsigned gy = (unsigned)std::max(1, std::min(cdiv(rows, ty), (int)std::max(1u, 8192u / (gx * gz))));
    grid = dim3(gx, std::min(gy, 65535u), gz);
    block = dim3((unsigned)tx, (unsigned)ty);
}

}  // namespace

int oct_pad_batch(const void* src_dev, int is_u8, int B, int H, int W, int ch, int Hp, int Wp, int top, int left, int mode,
                  float value, void* dst_dev, oct_stream_t stream) {
    if (!src_dev || !dst_dev) return fail(-1, "pad_batch: null pointer (src_dev, dst_dev)");
    if (B < 1 || H < 1 || W < 1 || ch < 1 || Hp < 1 || Wp < 1) return fail(-1, "pad_batch: B, H, W, ch, Hp, Wp must be positive");
    if (top < 0 || left < 0 || (int64_t)top + H > Hp || (int64_t)left + W > Wp)
        return fail(-1, "pad_batch: the image does not fit: need 0 <= top, top + H <= Hp, 0 <= left, left + W <= Wp");
    if (mode != OCT_PAD_EDGE && mode != OCT_PAD_REFLECT && mode != OCT_PAD_CONSTANT)
        return fail(-1, "pad_batch: unknown mode " + std::to_string(mode) + " (0 edge, 1 reflect, 2 constant)");
    if (mode == OCT_PAD_REFLECT && (top >= H || Hp - top - H >= H || left >= W || Wp - left - W >= W))
        return fail(-1, "pad_batch: reflect needs every pad smaller than the image's dimension on that axis");
    const int es = is_u8 ? 1 : 4;
    unsigned vbits = 0;
    if (mode == OCT_PAD_CONSTANT) {
        if (is_u8) {
            if (!(value >= 0.0f && value <= 255.0f) || value != std::floor(value))
                return fail(-1, "pad_batch: the constant of a uint8 batch must be a whole number in 0..255");
            vbits = (unsigned)value;
        } else {
            std::memcpy(&vbits, &value, sizeof(vbits));
        }
    }
    if ((uint64_t)ch * (uint64_t)es > (uint64_t)kPadMaxDim) return fail(-1, "pad_batch: element counts overflow the kernel's indexing");
    const int pb = ch * es;
    const size_t nsrc = checked_bytes(B, H, W, pb), ndst = checked_bytes(B, Hp, Wp, pb);
    if (!nsrc || !ndst)
        return fail(-1, "pad_batch: element counts overflow the kernel's indexing (B, Hp and the bytes of a row <= 2^30, a buffer < 2^62 bytes)");
    if (!is_u8 && (((uintptr_t)src_dev | (uintptr_t)dst_dev) & 3)) return fail(-1, "pad_batch: float32 buffers must be 4-byte aligned");
    if (overlap(src_dev, nsrc, dst_dev, ndst)) return fail(-1, "pad_batch: the destination overlaps the source");

    PadArgs a{};
    a.src = (const unsigned char*)src_dev; a.dst = (unsigned char*)dst_dev; a.src_bytes = nsrc;
    a.B = B; a.H = H; a.W = W; a.Hp = Hp; a.Wp = Wp; a.top = top; a.left = left; a.mode = mode;
    a.pb = pb; a.es = es; a.value = vbits;
    dim3 grid, block;
    launch_shape(Wp * pb, Hp, B, grid, block);
    hipStream_t st = (hipStream_t)stream;
    ProfScope ps(st, "pad_k", "pad", 0.0, (double)nsrc + (double)ndst);
    pad_k<<<grid, block, 0, st>>>(a);
    HIP_OK(hipGetLastError());
    return 0;
}

int oct_crop_batch(const void* src_dev, int B, int Hp, int Wp, int pixel_bytes, int H, int W, int top, int left, void* dst_dev,
                   oct_stream_t stream) {
    if (!src_dev || !dst_dev) return fail(-1, "crop_batch: null pointer (src_dev, dst_dev)");
    if (B < 1 || H < 1 || W < 1 || Hp < 1 || Wp < 1) return fail(-1, "crop_batch: B, Hp, Wp, H, W must be positive");
    const int pb = pixel_bytes;
    if (!(pb == 1 || pb == 2 || (pb >= 4 && pb <= 32 && pb % 4 == 0)))
        return fail(-1, "crop_batch: pixel_bytes must be 1, 2 or a multiple of 4 in 4..32, not " + std::to_string(pb));
    if (top < 0 || left < 0 || (int64_t)top + H > Hp || (int64_t)left + W > Wp)
        return fail(-1, "crop_batch: the window does not fit: need 0 <= top, top + H <= Hp, 0 <= left, left + W <= Wp");
    const size_t nsrc = checked_bytes(B, Hp, Wp, pb), ndst = checked_bytes(B, H, W, pb);
    if (!nsrc || !ndst)
        return fail(-1, "crop_batch: element counts overflow the kernel's indexing (B, Hp and the bytes of a row <= 2^30, a buffer < 2^62 bytes)");
    if (overlap(src_dev, nsrc, dst_dev, ndst)) return fail(-1, "crop_batch: the destination overlaps the source");

    CropArgs a{};
    a.src = (const unsigned char*)src_dev; a.dst = (unsigned char*)dst_dev; a.src_bytes = nsrc;
    a.B = B; a.Hp = Hp; a.Wp = Wp; a.H = H; a.W = W; a.top = top; a.left = left; a.pb = pb;
    dim3 grid, block;
    launch_shape(W * pb, H, B, grid, block);
    hipStream_t st = (hipStream_t)stream;
    ProfScope ps(st, "crop_k", "crop", 0.0, 2.0 * (double)ndst);
    crop_k<<<grid, block, 0, st>>>(a);
    HIP_OK(hipGetLastError());
    return 0;
}
