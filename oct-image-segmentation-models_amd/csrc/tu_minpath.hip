// One translation unit of liboct_unet_hip.so (see host.hpp): the min-path boundary search on the device
// (kernels_minpath.hpp) and its C ABI, oct_minpath_workspace_bytes / oct_minpath_device (include/oct_unet.h).
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/oct_unet.h"
#include "host.hpp"
#include "kernels_minpath.hpp"

using namespace oct;
using namespace octh;

namespace {
constexpr size_t kMinWorkspace = 256;       // a supported shape never reports 0

// H and W must fit the uint16 rows; the two live columns and one map tile must fit LDS (H <= ~1600)
bool shape_ok(int B, int M, int H, int W, int max_grad) {
    if (B < 1 || M < 1 || H < 1 || W < 1 || H > 65535 || W > 65535) return false;
    if (max_grad < 1 || max_grad > kMpMaxGrad) return false;
    if ((size_t)B * M > 0x7fffffffu) return false;
    return minpath_lds_base(H) <= kMpLdsLimit;
}
bool choice_in_lds(int H, int W) { return minpath_lds_base(H) + minpath_lds_choice(H, W) <= kMpLdsLimit; }
size_t workspace_need(int B, int M, int H, int W) {
    return choice_in_lds(H, W) ? kMinWorkspace : kMinWorkspace + (size_t)B * M * H * W;
}

const MinpathTable& table() {
    static const MinpathTable t = [] {
        MinpathTable x;
        for (int k = 0; k < 256; ++k) x.p[k] = (double)k / 255.0;     // numpy's maps / 255
        return x;
    }();
    return t;
}

// dynamic LDS beyond the 64 KiB default has to be announced once per device and kernel
template <bool LDS_CHOICE>
int raise_lds_limit(size_t bytes) {
    static size_t raised[64] = {};
    int dev = 0;
    HIP_OK(hipGetDevice(&dev));
    if (dev < 0 || dev >= 64) return fail(-1, "minpath_device: device index out of range");
    if (bytes > raised[dev]) {
        HIP_OK(hipFuncSetAttribute((const void*)minpath_k<LDS_CHOICE>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kMpLdsLimit));
        raised[dev] = kMpLdsLimit;
    }
    return 0;
}
}  // namespace

size_t oct_minpath_workspace_bytes(int B, int M, int H, int W, int max_grad) {
    return shape_ok(B, M, H, W, max_grad) ? workspace_need(B, M, H, W) : 0;
}

int oct_minpath_device(const unsigned char* maps_dev, int B, int M, int H, int W, int max_grad, void* workspace_dev,
                       size_t workspace_bytes, unsigned short* rows_out_dev, double* cost_out_dev,
                       unsigned char* tied_out_dev, oct_stream_t stream) {
    if (!maps_dev || !workspace_dev || !rows_out_dev || !cost_out_dev || !tied_out_dev)
        return fail(-1, "minpath_device: null pointer");
    if (max_grad < 1 || max_grad > kMpMaxGrad) return fail(-1, "minpath_device: max_grad must lie in 1..16");
    if (!shape_ok(B, M, H, W, max_grad))
        return fail(-1, "minpath_device: need B, M >= 1, 1 <= H, W <= 65535 (uint16 rows) and H small enough for two "
                        "fp64 column pairs and one map tile in LDS (H <= about 1600)");
    const size_t need = workspace_need(B, M, H, W);
    if (workspace_bytes < need)
        return fail(-1, "minpath_device: workspace too small (" + std::to_string(workspace_bytes) + " < " +
                        std::to_string(need) + " bytes)");
    MinpathArgs a;
    a.maps = maps_dev;
    a.choice = (unsigned char*)workspace_dev + kMinWorkspace;
    a.rows = rows_out_dev; a.cost = cost_out_dev; a.tied = tied_out_dev;
    a.H = H; a.W = W; a.G = max_grad;
    a.vec4 = (W % 4 == 0 && ((uintptr_t)maps_dev & 3) == 0) ? 1 : 0;
    const int threads = H <= 64 ? 64 : H <= 128 ? 128 : kMpMaxThreads;      // a power of two (the end reduction halves it)
    const unsigned grid = (unsigned)((size_t)B * M);
    hipStream_t st = (hipStream_t)stream;
    if (choice_in_lds(H, W)) {
        const size_t lds = minpath_lds_base(H) + minpath_lds_choice(H, W);
        if (lds > 64 * 1024) { const int rc = raise_lds_limit<true>(lds); if (rc) return rc; }
        minpath_k<true><<<grid, threads, lds, st>>>(a, table());
    } else {
        const size_t lds = minpath_lds_base(H);
        if (lds > 64 * 1024) { const int rc = raise_lds_limit<false>(lds); if (rc) return rc; }
        minpath_k<false><<<grid, threads, lds, st>>>(a, table());
    }
    HIP_OK(hipGetLastError());
    return 0;
}
