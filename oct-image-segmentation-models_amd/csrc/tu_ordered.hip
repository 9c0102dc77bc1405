// One translation unit of liboct_unet_hip.so (see host.hpp): the ordered layer decode (kernels_ordered.hpp) and its C ABI,
// oct_ordered_workspace_bytes / oct_ordered_decode (include/oct_unet.h).  The call allocates nothing and never waits for the stream.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "../../include/oct_unet.h"
#include "host.hpp"
#include "kernels_ordered.hpp"

using namespace oct;
using namespace octh;

namespace {

bool od_shape_ok(int B, int H, int W, int n_cls) {
    return B >= 1 && H >= 1 && W >= 1 && n_cls >= kOdMinClasses && n_cls <= kOdMaxClasses && H <= kOdMaxH &&
           (size_t)B * H * W < ((size_t)1 << 31);
}

bool overlap(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + nb && y < x + na;
}

template <int C>
void od_launch(const OdArgs& a, bool vec, unsigned grid, hipStream_t st) {
    if constexpr (C <= kOdMaxVec) {
        if (vec) { ordered_decode_k<C, true><<<grid, kOdThreads, 0, st>>>(a); return; }
    }
    ordered_decode_k<C, false><<<grid, kOdThreads, 0, st>>>(a);
}

}  // namespace

size_t oct_ordered_workspace_bytes(int B, int H, int W, int n_cls) {
    if (!od_shape_ok(B, H, W, n_cls)) return 0;
    return (size_t)B * H * (size_t)((W + 3) / 4 * 4) * sizeof(unsigned short);
}

int oct_ordered_decode(const float* probs_dev, int B, int H, int W, int n_cls, void* ws_dev, size_t ws_bytes,
                       unsigned char* labels_out_dev, unsigned short* rows_out_dev, unsigned int* score_out_dev, oct_stream_t stream) {
    if (!probs_dev || !ws_dev) return fail(-1, "ordered_decode: null pointer");
    if (!labels_out_dev && !rows_out_dev && !score_out_dev) return fail(-1, "ordered_decode: all three outputs are null");
    if (!od_shape_ok(B, H, W, n_cls))
        return fail(-1, "ordered_decode: need B, H, W >= 1, H <= " + std::to_string(kOdMaxH) + ", B*H*W < 2^31 and " +
                            std::to_string(kOdMinClasses) + " <= n_cls <= " + std::to_string(kOdMaxClasses));
    const size_t need = oct_ordered_workspace_bytes(B, H, W, n_cls);
    if (ws_bytes < need) return fail(-4, "ordered_decode: workspace too small: need " + std::to_string(need) + " bytes");
    if (((uintptr_t)probs_dev & 3) || ((uintptr_t)ws_dev & 7) || ((uintptr_t)rows_out_dev & 1) || ((uintptr_t)score_out_dev & 3))
        return fail(-1, "ordered_decode: probs and score must be 4-byte, rows 2-byte and the workspace 8-byte aligned");
    const size_t npx = (size_t)B * H * W;
    const void* ptr[5] = {probs_dev, ws_dev, labels_out_dev, rows_out_dev, score_out_dev};
    const size_t len[5] = {npx * n_cls * sizeof(float), need, npx, (size_t)B * (n_cls - 1) * W * sizeof(unsigned short),
                           (size_t)B * W * sizeof(unsigned int)};
    for (int i = 2; i < 5; ++i)
        for (int j = 0; j < i; ++j)
            if (ptr[i] && overlap(ptr[i], len[i], ptr[j], len[j]))
                return fail(-1, "ordered_decode: an output range overlaps the input, the workspace or another output");
    if (overlap(probs_dev, len[0], ws_dev, need)) return fail(-1, "ordered_decode: the workspace overlaps the input");

    OdArgs a{};
    a.probs = probs_dev; a.bits = (unsigned short*)ws_dev; a.labels = labels_out_dev; a.rows = rows_out_dev; a.score = score_out_dev;
    a.B = B; a.H = H; a.W = W; a.Wp = (W + 3) / 4 * 4;
    // one column per thread; under option "ordered_float4" items of 4 adjacent columns where every row of every image starts
    // on a float4
    const bool vec = g_opt.ordered_float4 && n_cls <= kOdMaxVec && ((size_t)W * n_cls) % 4 == 0 && ((uintptr_t)probs_dev & 15) == 0;
    a.ipr = vec ? (W + 3) / 4 : W;
    a.lab4 = vec && W % 4 == 0 && ((uintptr_t)labels_out_dev & 3) == 0;
    const unsigned grid = (unsigned)(((size_t)B * a.ipr + kOdThreads - 1) / kOdThreads);
    hipStream_t st = (hipStream_t)stream;
    ProfScope ps(st, vec ? "ordered_decode_k<C,4>" : "ordered_decode_k<C,1>", "ordered_decode", 0.0,
                 (double)npx * (n_cls * 4 + 2 * 2 + 1));
    switch (n_cls) {
#define OD_CASE(N) case N: od_launch<N>(a, vec, grid, st); break;
        OD_CASE(2) OD_CASE(3) OD_CASE(4) OD_CASE(5) OD_CASE(6) OD_CASE(7) OD_CASE(8) OD_CASE(9) OD_CASE(10) OD_CASE(11)
        OD_CASE(12) OD_CASE(13) OD_CASE(14) OD_CASE(15) OD_CASE(16)
#undef OD_CASE
        default: return fail(-1, "ordered_decode: n_cls");
    }
    HIP_OK(hipGetLastError());
    return 0;
}
