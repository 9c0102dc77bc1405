// One translation unit of liboct_unet_hip.so (see host.hpp): the edge weight map on the device (kernels_edge_weight.hpp)
// and its C ABI, oct_edge_weight_map (include/oct_unet.h).  One launch, no workspace, no allocation, no wait.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "../../include/oct_unet.h"
#include "host.hpp"
#include "kernels_edge_weight.hpp"

using namespace oct;
using namespace octh;

static_assert(OCT_EDGE_WEIGHT_MAX_RADIUS == EW_MAX_R, "header and kernel agree on the largest radius");
static_assert(ew_lds_bytes(EW_MAX_R) <= 64 * 1024, "the three planes of the largest radius fit a block's LDS");
static_assert(EW_MAX_R < EW_NONE, "a vertical distance fits a byte beside the 'none' mark");

int oct_edge_weight_map(const unsigned char* labels_dev, int B, int H, int W, int n_cls, int radius, const float* lut_dev,
                        float* weights_dev, oct_stream_t stream) {
    if (!labels_dev || !lut_dev || !weights_dev) return fail(-1, "edge_weight_map: null pointer (labels_dev, lut_dev, weights_dev)");
    if (B < 1 || H < 1 || W < 1) return fail(-1, "edge_weight_map: B, H, W must be positive");
    if (n_cls < 1 || n_cls > 255) return fail(-1, "edge_weight_map: n_cls must be in 1..255 (a byte >= n_cls is unknown)");
    if (radius < 1 || radius > OCT_EDGE_WEIGHT_MAX_RADIUS)
        return fail(-1, "edge_weight_map: radius must be in 1..32: got " + std::to_string(radius));
    if (B > 65535 || H > OCT_EDGE_WEIGHT_MAX_DIM || W > OCT_EDGE_WEIGHT_MAX_DIM)
        return fail(-1, "edge_weight_map: need B <= 65535 and H, W <= 16384");
    const size_t n = (size_t)B * H * W;
    const uintptr_t l0 = (uintptr_t)labels_dev, w0 = (uintptr_t)weights_dev;
    if (w0 % 4 || (uintptr_t)lut_dev % 4) return fail(-1, "edge_weight_map: lut_dev and weights_dev must be 4-byte aligned");
    if (l0 < w0 + 4 * n && w0 < l0 + n) return fail(-1, "edge_weight_map: weights_dev overlaps labels_dev");

    EdgeWeightGeom g;
    g.H = H; g.W = W; g.n_cls = n_cls; g.R = radius;
    g.tiles_x = (unsigned)((W + EW_TW - 1) / EW_TW);
    const unsigned tiles = g.tiles_x * (unsigned)((H + EW_TH - 1) / EW_TH);      // <= 256 * 512
    hipStream_t st = (hipStream_t)stream;
    ProfScope ps(st, "edge_weight_k", "edge_weight", 0.0, 5.0 * (double)n);
    edge_weight_k<<<dim3(tiles, (unsigned)B), 256, (size_t)ew_lds_bytes(radius), st>>>(labels_dev, lut_dev, g, weights_dev);
    HIP_OK(hipGetLastError());
    return 0;
}
