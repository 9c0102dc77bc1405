// One translation unit of liboct_unet_hip.so (see host.hpp): the elastic deformation on the device (kernels_elastic.hpp)
// and its C ABI, oct_elastic_batch (include/oct_unet.h).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "../../include/oct_unet.h"
#include "host.hpp"
#include "kernels_elastic.hpp"

using namespace oct;
using namespace octh;

static_assert(sizeof(oct_elastic_op) == 40, "oct_elastic_op is 40 bytes (common/augmentation.py ELASTIC_OP_DTYPE)");

namespace {
bool overlap(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a && b && a0 < b0 + nb && b0 < a0 + na;
}
}  // namespace

int oct_elastic_batch(const unsigned char* x_u8_dev, const unsigned char* labels_dev, const oct_elastic_op* ops_dev, int B, int H,
                      int W, int C, unsigned char* x_out_dev, unsigned char* labels_out_dev, oct_stream_t stream) {
    if (!x_u8_dev || !ops_dev || !x_out_dev) return fail(-1, "elastic_batch: null pointer (x_u8_dev, ops_dev, x_out_dev)");
    if (B < 1 || H < 1 || W < 1 || C < 1) return fail(-1, "elastic_batch: B, H, W, C must be positive");
    if (B > 65535 || H > OCT_ELASTIC_MAX_DIM || W > OCT_ELASTIC_MAX_DIM || (uint64_t)H * W * C > 0x7fffffffull)
        return fail(-1, "elastic_batch: need B <= 65535, H and W <= 16384 and H*W*C < 2^31");
    if (labels_out_dev && !labels_dev) return fail(-1, "elastic_batch: labels_out_dev without labels_dev");
    const size_t n = (size_t)H * W * C, nl = (size_t)H * W;
    const size_t xb = B * n, lb = B * nl, ob = (size_t)B * sizeof(oct_elastic_op);
    if (overlap(x_out_dev, xb, x_u8_dev, xb) || overlap(x_out_dev, xb, labels_dev, lb) || overlap(x_out_dev, xb, ops_dev, ob) ||
        overlap(labels_out_dev, lb, x_u8_dev, xb) || overlap(labels_out_dev, lb, labels_dev, lb) ||
        overlap(labels_out_dev, lb, ops_dev, ob) || overlap(labels_out_dev, lb, x_out_dev, xb))
        return fail(-1, "elastic_batch: an output range overlaps an input range or the other output");

    ElasticGeom g;
    g.H = H; g.W = W; g.C = C; g.n = (unsigned)n; g.nl = (unsigned)nl;
    g.tiles_x = (unsigned)((W + EL_TW - 1) / EL_TW);
    const unsigned tiles = g.tiles_x * (unsigned)((H + EL_TH - 1) / EL_TH);     // <= 128 * 1024
    const bool with_labels = labels_dev && labels_out_dev;
    // one 32-bit store per 4 pixels: one channel, rows of whole words, aligned pointers
    const bool vec = C == 1 && W % 4 == 0 && (uintptr_t)x_u8_dev % 4 == 0 && (uintptr_t)x_out_dev % 4 == 0 &&
                     (!with_labels || ((uintptr_t)labels_dev % 4 == 0 && (uintptr_t)labels_out_dev % 4 == 0));
    hipStream_t st = (hipStream_t)stream;
    unsigned char* lo = with_labels ? labels_out_dev : nullptr;
    ProfScope ps(st, vec ? "elastic_k<true>" : "elastic_k<false>", "elastic", 0.0, (double)(2 * xb + (lo ? 2 * lb : 0)));
    if (vec) elastic_k<true><<<dim3(tiles, (unsigned)B), 256, 0, st>>>(x_u8_dev, labels_dev, ops_dev, g, x_out_dev, lo);
    else elastic_k<false><<<dim3(tiles, (unsigned)B), 256, 0, st>>>(x_u8_dev, labels_dev, ops_dev, g, x_out_dev, lo);
    HIP_OK(hipGetLastError());
    return 0;
}
