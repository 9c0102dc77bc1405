// One translation unit of liboct_unet_hip.so (see host.hpp): the Monte-Carlo dropout reduction (kernels_mc.hpp) and its C
// ABI, oct_mc_workspace_bytes / oct_mc_update (include/oct_unet.h).  The calls allocate nothing and never wait for the stream.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <string>

#include "../../include/oct_unet.h"
#include "host.hpp"
#include "kernels_mc.hpp"

using namespace oct;
using namespace octh;

namespace {

bool mc_shape_ok(int B, int H, int W, int n_cls) {
    return B >= 1 && H >= 1 && W >= 1 && n_cls >= 2 && n_cls <= kMcMaxClasses && (size_t)B * H * W < ((size_t)1 << 31);
}

template <int VC>
void mc_launch(const McArgs& a, size_t items, unsigned grid, bool first, bool last, hipStream_t st) {
    if (first && last) mc_update_k<VC, true, true><<<grid, kMcThreads, 0, st>>>(a, items);
    else if (first) mc_update_k<VC, true, false><<<grid, kMcThreads, 0, st>>>(a, items);
    else if (last) mc_update_k<VC, false, true><<<grid, kMcThreads, 0, st>>>(a, items);
    else mc_update_k<VC, false, false><<<grid, kMcThreads, 0, st>>>(a, items);
}

}  // namespace

namespace octh {

// every argument error of oct_mc_update, without launching: oct_unet_infer asks before its first launch
int mc_validate(const float* probs, int B, int H, int W, int n_cls, int t, int T, const void* ws, size_t ws_bytes,
                const oct_mc_out* out) {
    if (!probs || !ws) return fail(-1, "mc_update: null pointer");
    if (B < 1 || H < 1 || W < 1) return fail(-1, "mc_update: B, H, W must be positive");
    if (n_cls < 2 || n_cls > kMcMaxClasses) return fail(-1, "mc_update: need 2 <= n_cls <= " + std::to_string(kMcMaxClasses));
    if ((size_t)B * H * W >= ((size_t)1 << 31)) return fail(-1, "mc_update: B*H*W must be below 2^31");
    if (T < 1 || T > kMcMaxSamples) return fail(-1, "mc_update: need 1 <= T <= " + std::to_string(kMcMaxSamples));
    if (t < 0 || t >= T) return fail(-1, "mc_update: need 0 <= t < T");
    const size_t need = oct_mc_workspace_bytes(B, H, W, n_cls);
    if (ws_bytes < need) return fail(-4, "mc_update: workspace too small: need " + std::to_string(need) + " bytes");
    if (((uintptr_t)probs & 3) || ((uintptr_t)ws & 3)) return fail(-1, "mc_update: probs and workspace must be 4-byte aligned");
    const size_t npix = (size_t)B * H * W, nin = npix * n_cls * sizeof(float);
    auto overlap = [](const void* a, size_t na, const void* b, size_t nb) {
        const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
        return x < y + nb && y < x + na;
    };
    if (overlap(probs, nin, ws, need)) return fail(-1, "mc_update: the workspace overlaps the input");
    if (t != T - 1) return 0;
    if (!out) return fail(-1, "mc_update: null out on the last sample");
    const void* o[4] = {out->mean_probs, out->argmax, out->entropy, out->mutual_info};
    const size_t on[4] = {nin, npix, npix * sizeof(float), npix * sizeof(float)};
    for (int i = 0; i < 4; ++i) {
        if (!o[i]) continue;
        if (i != 1 && ((uintptr_t)o[i] & 3)) return fail(-1, "mc_update: float outputs must be 4-byte aligned");
        if (overlap(o[i], on[i], probs, nin) || overlap(o[i], on[i], ws, need))
            return fail(-1, "mc_update: an output range overlaps the input or the workspace");
        for (int j = 0; j < i; ++j)
            if (o[j] && overlap(o[i], on[i], o[j], on[j])) return fail(-1, "mc_update: two output ranges overlap");
    }
    return 0;
}

}  // namespace octh

size_t oct_mc_workspace_bytes(int B, int H, int W, int n_cls) {
    if (!mc_shape_ok(B, H, W, n_cls)) return 0;
    return (size_t)B * H * W * (size_t)(n_cls + 1) * sizeof(float);
}

int oct_mc_update(const float* probs_dev, int B, int H, int W, int n_cls, int t, int T, void* ws_dev, size_t ws_bytes,
                  const oct_mc_out* out, oct_stream_t stream) {
    if (int rc = mc_validate(probs_dev, B, H, W, n_cls, t, T, ws_dev, ws_bytes, out)) return rc;
    const bool first = t == 0, last = t == T - 1;
    McArgs a{};
    a.npix = (size_t)B * H * W; a.C = n_cls; a.inv_t = 1.0f / (float)T;
    a.probs = probs_dev; a.S = (float*)ws_dev; a.E = a.S + a.npix * n_cls;
    if (last) { a.mean = out->mean_probs; a.am = out->argmax; a.ent = out->entropy; a.mi = out->mutual_info; }
    // float4 items of 4 pixels where every base allows it (E sits behind S: aligned iff npix * C % 4 == 0); else per pixel
    const uintptr_t al16 = (uintptr_t)a.probs | (uintptr_t)a.S | (uintptr_t)a.mean | (uintptr_t)a.ent | (uintptr_t)a.mi;
    const bool vec = n_cls <= kMcMaxVec && (a.npix * n_cls) % 4 == 0 && (al16 & 15) == 0 && ((uintptr_t)a.am & 3) == 0;
    const int vc = vec ? n_cls : 0;
    const size_t items = vec ? (a.npix + 3) / 4 : a.npix;
    const unsigned grid = (unsigned)std::min<size_t>((items + kMcThreads - 1) / kMcThreads, (size_t)kMcMaxBlocks);
    hipStream_t st = (hipStream_t)stream;
    // bytes: p once; S read unless first, written unless last; E likewise; the maps written on the last sample
    double by = (double)a.npix * n_cls * 4 * (1 + (first ? 0 : 1) + (last ? 0 : 1)) + (double)a.npix * 4 * ((first ? 0 : 1) + (last ? 0 : 1));
    if (last) by += (double)a.npix * ((a.mean ? n_cls * 4 : 0) + (a.am ? 1 : 0) + (a.ent ? 4 : 0) + (a.mi ? 4 : 0));
    ProfScope ps(st, vec ? "mc_update_k<C>" : "mc_update_k<0>", "mc_update", 0.0, by);
    switch (vc) {
        case 2: mc_launch<2>(a, items, grid, first, last, st); break;
        case 3: mc_launch<3>(a, items, grid, first, last, st); break;
        case 4: mc_launch<4>(a, items, grid, first, last, st); break;
        case 5: mc_launch<5>(a, items, grid, first, last, st); break;
        case 6: mc_launch<6>(a, items, grid, first, last, st); break;
        case 7: mc_launch<7>(a, items, grid, first, last, st); break;
        case 8: mc_launch<8>(a, items, grid, first, last, st); break;
        default: mc_launch<0>(a, items, grid, first, last, st); break;
    }
    HIP_OK(hipGetLastError());
    return 0;
}
