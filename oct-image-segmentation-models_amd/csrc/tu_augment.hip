// One translation unit of liboct_unet_hip.so (see host.hpp): the training augmentations on the device
// (kernels_augment.hpp) and their C ABI, oct_augment_batch (include/oct_unet.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <string>

#include "../../include/oct_unet.h"
#include "host.hpp"
#include "kernels_augment.hpp"

using namespace oct;
using namespace octh;

static_assert(sizeof(oct_aug_op) == 32, "oct_aug_op is 32 bytes (common/augmentation.py AUG_OP_DTYPE)");

namespace {
bool overlap(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a && b && a0 < b0 + nb && b0 < a0 + na;
}
}  // namespace

int oct_augment_batch(const unsigned char* x_u8_dev, const unsigned char* labels_dev, const oct_aug_op* ops_dev, int B, int H,
                      int W, int C, unsigned long long seed, float* x_out_dev, unsigned char* labels_out_dev,
                      oct_stream_t stream) {
    if (!x_u8_dev || !ops_dev || !x_out_dev) return fail(-1, "augment_batch: null pointer (x_u8_dev, ops_dev, x_out_dev)");
    if (B < 1 || H < 1 || W < 1 || C < 1) return fail(-1, "augment_batch: B, H, W, C must be positive");
    if (B > 65535 || (uint64_t)H * W * C > 0x7fffffffull)
        return fail(-1, "augment_batch: need B <= 65535 and H*W*C < 2^31");
    if (labels_out_dev && !labels_dev) return fail(-1, "augment_batch: labels_out_dev without labels_dev");
    const size_t n = (size_t)H * W * C, nl = (size_t)H * W;
    const size_t xin = B * n, xout = B * n * sizeof(float), lb = B * nl, ob = (size_t)B * sizeof(oct_aug_op);
    if (overlap(x_out_dev, xout, x_u8_dev, xin) || overlap(x_out_dev, xout, labels_dev, lb) ||
        overlap(x_out_dev, xout, ops_dev, ob) || overlap(labels_out_dev, lb, x_u8_dev, xin) ||
        overlap(labels_out_dev, lb, labels_dev, lb) || overlap(labels_out_dev, lb, ops_dev, ob) ||
        overlap(labels_out_dev, lb, x_out_dev, xout))
        return fail(-1, "augment_batch: an output range overlaps an input range or the other output");

    AugGeom g;
    g.H = H; g.W = W; g.C = C; g.n = (unsigned)n; g.nl = (unsigned)nl; g.row = (unsigned)(W * C);
    const bool with_labels = labels_dev && labels_out_dev;
    const bool vec = n % 4 == 0 && (uintptr_t)x_u8_dev % 4 == 0 && (uintptr_t)x_out_dev % 16 == 0 &&
                     (!with_labels || (nl % 4 == 0 && (uintptr_t)labels_dev % 4 == 0 && (uintptr_t)labels_out_dev % 4 == 0));
    // 4 elements per thread and pass; about 2048 blocks over the batch (8 per CU), the rest by the grid-stride loop
    const unsigned groups = (unsigned)((n + 3) / 4);
    const unsigned gx = std::max(1u, std::min((groups + 255u) / 256u, std::max(1u, 2048u / (unsigned)B)));
    hipStream_t st = (hipStream_t)stream;
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    unsigned char* lo = with_labels ? labels_out_dev : nullptr;
    ProfScope ps(st, vec ? "augment_k<true>" : "augment_k<false>", "augment", 0.0, (double)(xin + xout + (lo ? 2 * lb : 0)));
    if (vec) augment_k<true><<<dim3(gx, (unsigned)B), 256, 0, st>>>(x_u8_dev, labels_dev, ops_dev, g, k0, k1, x_out_dev, lo);
    else augment_k<false><<<dim3(gx, (unsigned)B), 256, 0, st>>>(x_u8_dev, labels_dev, ops_dev, g, k0, k1, x_out_dev, lo);
    HIP_OK(hipGetLastError());
    return 0;
}
