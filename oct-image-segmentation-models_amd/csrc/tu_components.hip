// One translation unit of liboct_unet_hip.so (see host.hpp): connected components of a class map and the component filter
// (kernels_components.hpp) behind their C ABI, oct_components_workspace_bytes / oct_components / oct_component_filter
// (include/oct_unet.h).  Neither call allocates or waits for the stream.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "../../include/oct_unet.h"
#include "host.hpp"
#include "kernels_components.hpp"

using namespace oct;
using namespace octh;

namespace {

bool cc_shape_ok(int B, int H, int W) {
    return B >= 1 && B <= kCcMaxBatch && H >= 1 && W >= 1 && (size_t)B * H * W < ((size_t)1 << 31);
}

bool overlap(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + nb && y < x + na;
}

// workspace: (B, 32) uint64 best-root keys of the filter, then B*H*W uint32 -- the size words of oct_components when the
// caller wants none, the removal flags (a byte each) of the filter's fill mode 1
size_t cc_best_bytes(int B) { return (size_t)B * kCcMaxClasses * sizeof(unsigned long long); }

// blocks of an image for the kernels that stride over it: 8 pixels to a thread
unsigned cc_image_blocks(size_t hw) { return (unsigned)((hw + kCcThreads * 8 - 1) / (kCcThreads * 8)); }

}  // namespace

size_t oct_components_workspace_bytes(int B, int H, int W) {
    if (!cc_shape_ok(B, H, W)) return 0;
    return cc_best_bytes(B) + ((size_t)B * H * W * sizeof(unsigned) + 255) / 256 * 256;
}

int oct_components(const unsigned char* labels_dev, int B, int H, int W, int n_cls, int connectivity, void* ws_dev, size_t ws_bytes,
                   unsigned int* root_out_dev, unsigned int* size_out_dev, unsigned int* stats_out_dev, oct_stream_t stream) {
    if (!labels_dev || !root_out_dev || !ws_dev) return fail(-1, "components: null labels, root or workspace");
    if (!cc_shape_ok(B, H, W))
        return fail(-1, "components: need 1 <= B <= " + std::to_string(kCcMaxBatch) + ", H, W >= 1 and B*H*W < 2^31");
    if (n_cls < 1 || n_cls > kCcMaxClasses) return fail(-1, "components: need 1 <= n_cls <= " + std::to_string(kCcMaxClasses));
    if (connectivity != 4 && connectivity != 8) return fail(-1, "components: connectivity must be 4 or 8");
    const size_t need = oct_components_workspace_bytes(B, H, W);
    if (ws_bytes < need) return fail(-4, "components: workspace too small: need " + std::to_string(need) + " bytes");
    if (((uintptr_t)ws_dev & 7) || ((uintptr_t)root_out_dev & 3) || ((uintptr_t)size_out_dev & 3) || ((uintptr_t)stats_out_dev & 3))
        return fail(-1, "components: root, size and stats must be 4-byte and the workspace 8-byte aligned");
    const size_t npx = (size_t)B * H * W;
    const void* ptr[5] = {labels_dev, ws_dev, root_out_dev, size_out_dev, stats_out_dev};
    const size_t len[5] = {npx, need, npx * sizeof(unsigned), npx * sizeof(unsigned), (size_t)B * n_cls * 2 * sizeof(unsigned)};
    for (int i = 2; i < 5; ++i)
        for (int j = 0; j < i; ++j)
            if (ptr[i] && ptr[j] && overlap(ptr[i], len[i], ptr[j], len[j]))
                return fail(-1, "components: an output range overlaps the input, the workspace or another output");
    if (overlap(labels_dev, npx, ws_dev, need)) return fail(-1, "components: the workspace overlaps the input");

    CcArgs a{};
    a.labels = labels_dev; a.root = root_out_dev; a.stats = stats_out_dev;
    a.size = size_out_dev ? size_out_dev : (unsigned*)((char*)ws_dev + cc_best_bytes(B));
    a.B = B; a.H = H; a.W = W; a.n_cls = n_cls; a.conn8 = connectivity == 8;
    hipStream_t st = (hipStream_t)stream;
    const int ntx = cdiv(W, kCcTile), nty = cdiv(H, kCcTile);      // ntx * nty <= H * W < 2^31: the tiles of an image are grid.x
    a.ntx = ntx;
    const int n_row = (nty - 1) * W, n_all = n_row + (ntx - 1) * H;      // < 2 * H * W / 64
    ProfScope ps(st, "cc_tile_k + cc_border_k + cc_flatten_k", "components", 0.0, (double)npx * (1 + 4 + 4));
    if (stats_out_dev) HIP_OK(hipMemsetAsync(stats_out_dev, 0, len[4], st));
    cc_tile_k<<<dim3((unsigned)ntx * (unsigned)nty, 1, B), kCcThreads, 0, st>>>(a);
    if (n_all > 0) cc_border_k<<<dim3(cdiv(n_all, kCcThreads), 1, B), kCcThreads, 0, st>>>(a, n_row, n_all);
    cc_flatten_k<<<(unsigned)((npx + kCcThreads - 1) / kCcThreads), kCcThreads, 0, st>>>(a, (unsigned)((size_t)H * W), npx);
    if (stats_out_dev) cc_stats_k<<<dim3(cc_image_blocks((size_t)H * W), 1, B), kCcThreads, 0, st>>>(a);
    HIP_OK(hipGetLastError());
    return 0;
}

int oct_component_filter(const unsigned char* labels_dev, const unsigned int* root_dev, const unsigned int* size_dev, int B, int H,
                         int W, int n_cls, const oct_component_rule* rule, void* ws_dev, size_t ws_bytes,
                         unsigned char* labels_out_dev, unsigned int* removed_out_dev, oct_stream_t stream) {
    if (!labels_dev || !root_dev || !size_dev || !rule || !ws_dev || !labels_out_dev)
        return fail(-1, "component_filter: null labels, root, size, rule, workspace or output");
    if (!cc_shape_ok(B, H, W))
        return fail(-1, "component_filter: need 1 <= B <= " + std::to_string(kCcMaxBatch) + ", H, W >= 1 and B*H*W < 2^31");
    if (n_cls < 1 || n_cls > kCcMaxClasses) return fail(-1, "component_filter: need 1 <= n_cls <= " + std::to_string(kCcMaxClasses));
    if (rule->fill_mode < 0 || rule->fill_mode > 1) return fail(-1, "component_filter: fill_mode must be 0 (constant) or 1 (column)");
    if (rule->fill_label < 0 || rule->fill_label > 255) return fail(-1, "component_filter: fill_label must be in 0..255");
    if (n_cls < 32 && (rule->keep_largest >> n_cls)) return fail(-1, "component_filter: keep_largest has bits at or above n_cls");
    const size_t need = oct_components_workspace_bytes(B, H, W);
    if (ws_bytes < need) return fail(-4, "component_filter: workspace too small: need " + std::to_string(need) + " bytes");
    if (((uintptr_t)ws_dev & 7) || ((uintptr_t)root_dev & 3) || ((uintptr_t)size_dev & 3) || ((uintptr_t)removed_out_dev & 3))
        return fail(-1, "component_filter: root, size and removed must be 4-byte and the workspace 8-byte aligned");
    const size_t npx = (size_t)B * H * W;
    const void* ptr[6] = {labels_dev, root_dev, size_dev, ws_dev, labels_out_dev, removed_out_dev};
    const size_t len[6] = {npx, npx * sizeof(unsigned), npx * sizeof(unsigned), need, npx, (size_t)B * n_cls * sizeof(unsigned)};
    for (int i = 4; i < 6; ++i)
        for (int j = 0; j < i; ++j)
            if (ptr[i] && overlap(ptr[i], len[i], ptr[j], len[j]))
                return fail(-1, "component_filter: an output range overlaps an input, the workspace or the other output");
    for (int j = 0; j < 3; ++j)
        if (overlap(ptr[j], len[j], ws_dev, need)) return fail(-1, "component_filter: the workspace overlaps an input");

    CcFilterArgs a{};
    a.labels = labels_dev; a.root = root_dev; a.size = size_dev;
    a.best = (unsigned long long*)ws_dev; a.flags = (unsigned char*)ws_dev + cc_best_bytes(B);
    a.out = labels_out_dev; a.removed = removed_out_dev;
    a.B = B; a.H = H; a.W = W; a.n_cls = n_cls; a.fill_mode = rule->fill_mode; a.fill_label = rule->fill_label;
    a.keep_largest = rule->keep_largest;
    for (int c = 0; c < kCcMaxClasses; ++c) a.min_pixels[c] = c < n_cls ? rule->min_pixels[c] : 0u;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(cc_image_blocks((size_t)H * W), 1, B);
    ProfScope ps(st, "cc_best_k + cc_filter_k + cc_column_fill_k", "component_filter", 0.0, (double)npx * (1 + 4 + 4 + 1));
    // the launches depend on the rule alone, never on the data: the best roots only if a class keeps its largest component,
    // the column walk only under fill mode 1
    if (removed_out_dev) HIP_OK(hipMemsetAsync(removed_out_dev, 0, len[5], st));
    if (a.keep_largest) {
        HIP_OK(hipMemsetAsync(a.best, 0, cc_best_bytes(B), st));
        cc_best_k<<<grid, kCcThreads, 0, st>>>(a);
    }
    cc_filter_k<<<grid, kCcThreads, 0, st>>>(a);
    if (a.fill_mode == 1)
        cc_column_fill_k<<<(unsigned)(((size_t)B * W + kCcColThreads - 1) / kCcColThreads), kCcColThreads, 0, st>>>(a);
    HIP_OK(hipGetLastError());
    return 0;
}
