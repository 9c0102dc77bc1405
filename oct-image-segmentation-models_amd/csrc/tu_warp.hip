// One translation unit of liboct_unet_hip.so (see host.hpp): the geometric training augmentations on the device
// (kernels_warp.hpp) and their C ABI, oct_warp_batch (include/oct_unet.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <string>

#include "../../include/oct_unet.h"
#include "host.hpp"
#include "kernels_warp.hpp"

using namespace oct;
using namespace octh;

static_assert(sizeof(oct_warp_op) == 40, "oct_warp_op is 40 bytes (common/augmentation.py WARP_OP_DTYPE)");

namespace {
bool overlap(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a && b && a0 < b0 + nb && b0 < a0 + na;
}
}  // namespace

int oct_warp_batch(const unsigned char* x_u8_dev, const unsigned char* labels_dev, const oct_warp_op* ops_dev, int B, int H,
                   int W, int C, unsigned char* x_out_dev, unsigned char* labels_out_dev, oct_stream_t stream) {
    if (!x_u8_dev || !ops_dev || !x_out_dev) return fail(-1, "warp_batch: null pointer (x_u8_dev, ops_dev, x_out_dev)");
    if (B < 1 || H < 1 || W < 1 || C < 1) return fail(-1, "warp_batch: B, H, W, C must be positive");
    if (B > 65535 || H > OCT_WARP_MAX_DIM || W > OCT_WARP_MAX_DIM || (uint64_t)H * W * C > 0x7fffffffull)
        return fail(-1, "warp_batch: need B <= 65535, H and W <= 16384 and H*W*C < 2^31");
    if (labels_out_dev && !labels_dev) return fail(-1, "warp_batch: labels_out_dev without labels_dev");
    const size_t n = (size_t)H * W * C, nl = (size_t)H * W;
    const size_t xb = B * n, lb = B * nl, ob = (size_t)B * sizeof(oct_warp_op);
    if (overlap(x_out_dev, xb, x_u8_dev, xb) || overlap(x_out_dev, xb, labels_dev, lb) || overlap(x_out_dev, xb, ops_dev, ob) ||
        overlap(labels_out_dev, lb, x_u8_dev, xb) || overlap(labels_out_dev, lb, labels_dev, lb) ||
        overlap(labels_out_dev, lb, ops_dev, ob) || overlap(labels_out_dev, lb, x_out_dev, xb))
        return fail(-1, "warp_batch: an output range overlaps an input range or the other output");

    WarpGeom g;
    g.H = H; g.W = W; g.C = C; g.n = (unsigned)n; g.nl = (unsigned)nl;
    const bool with_labels = labels_dev && labels_out_dev;
    const bool vec = n % 4 == 0 && (uintptr_t)x_u8_dev % 4 == 0 && (uintptr_t)x_out_dev % 4 == 0 &&
                     (!with_labels || (nl % 4 == 0 && (uintptr_t)labels_dev % 4 == 0 && (uintptr_t)labels_out_dev % 4 == 0));
    // 4 bytes per thread and pass; about 2048 blocks over the batch (8 per CU), the rest by the grid-stride loop
    const unsigned groups = (unsigned)((n + 3) / 4);
    const unsigned gx = std::max(1u, std::min((groups + 255u) / 256u, std::max(1u, 2048u / (unsigned)B)));
    hipStream_t st = (hipStream_t)stream;
    unsigned char* lo = with_labels ? labels_out_dev : nullptr;
    ProfScope ps(st, vec ? "warp_k<true>" : "warp_k<false>", "warp", 0.0, (double)(2 * xb + (lo ? 2 * lb : 0)));
    if (vec) warp_k<true><<<dim3(gx, (unsigned)B), 256, 0, st>>>(x_u8_dev, labels_dev, ops_dev, g, x_out_dev, lo);
    else warp_k<false><<<dim3(gx, (unsigned)B), 256, 0, st>>>(x_u8_dev, labels_dev, ops_dev, g, x_out_dev, lo);
    HIP_OK(hipGetLastError());
    return 0;
}
