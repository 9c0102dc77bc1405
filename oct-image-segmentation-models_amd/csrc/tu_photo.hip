// One translation unit of liboct_unet_hip.so (see host.hpp): the photometric augmentation on the device (kernels_photo.hpp)
// and its C ABI, oct_photo_batch (include/oct_unet.h).
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <string>

#include "../../include/oct_unet.h"
#include "host.hpp"
#include "kernels_photo.hpp"

using namespace oct;
using namespace octh;

static_assert(sizeof(oct_photo_op) == 320 && offsetof(oct_photo_op, w) == 8 && offsetof(oct_photo_op, n_shadows) == 26 &&
                  offsetof(oct_photo_op, cx) == 28 && offsetof(oct_photo_op, strength) == 52 &&
                  offsetof(oct_photo_op, reserved) == 60 && offsetof(oct_photo_op, lut) == 64,
              "oct_photo_op is 320 bytes (common/augmentation.py PHOTO_OP_DTYPE)");

namespace {
bool overlap(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + nb && b0 < a0 + na;
}
}  // namespace

int oct_photo_batch(const unsigned char* x_dev, const oct_photo_op* ops_dev, int B, int H, int W, int C, unsigned char* out_dev,
                    oct_stream_t stream) {
    if (!x_dev || !ops_dev || !out_dev) return fail(-1, "photo_batch: null pointer (x_dev, ops_dev, out_dev)");
    if ((uintptr_t)ops_dev % 4) return fail(-1, "photo_batch: ops_dev must be 4-byte aligned");
    if (B < 1 || H < 1 || W < 1 || C < 1) return fail(-1, "photo_batch: B, H, W, C must be positive");
    if (B > 65535 || H > OCT_PHOTO_MAX_DIM || W > OCT_PHOTO_MAX_DIM || C > OCT_PHOTO_MAX_DIM || (uint64_t)H * W * C > 0x7fffffffull)
        return fail(-1, "photo_batch: need B <= 65535, H, W and C <= 16384 and H*W*C < 2^31");
    const size_t n = (size_t)H * W * C, xb = B * n, ob = (size_t)B * sizeof(oct_photo_op);
    if (overlap(out_dev, xb, x_dev, xb) || overlap(out_dev, xb, ops_dev, ob))
        return fail(-1, "photo_batch: out_dev overlaps x_dev or ops_dev (the stage cannot run in place)");

    PhotoGeom g;
    g.H = H; g.W = W; g.C = C; g.n = (unsigned)n;
    g.tiles_x = (unsigned)((W + PH_TW - 1) / PH_TW);
    const unsigned tiles = g.tiles_x * (unsigned)((H + PH_TH - 1) / PH_TH);     // <= 128 * 512
    // one 32-bit load and store per 4 pixels: one channel, rows of whole words, aligned pointers
    const bool vec = C == 1 && W % 4 == 0 && (uintptr_t)x_dev % 4 == 0 && (uintptr_t)out_dev % 4 == 0;
    hipStream_t st = (hipStream_t)stream;
    ProfScope ps(st, vec ? "photo_k<true>" : "photo_k<false>", "photometric", 0.0, (double)(2 * xb));
    if (vec) photo_k<true><<<dim3(tiles, (unsigned)B), PH_THREADS, 0, st>>>(x_dev, ops_dev, g, out_dev);
    else photo_k<false><<<dim3(tiles, (unsigned)B), PH_THREADS, 0, st>>>(x_dev, ops_dev, g, out_dev);
    HIP_OK(hipGetLastError());
    return 0;
}
