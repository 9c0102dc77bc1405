// One translation unit of liboct_unet_hip.so (see host.hpp): test-time augmentation (kernels_tta.hpp) and its C ABI,
// oct_flip_batch / oct_tta_update (include/oct_unet.h).  The calls allocate nothing and never wait for the stream.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <string>

#include "../../include/oct_unet.h"
#include "host.hpp"
#include "kernels_tta.hpp"

using namespace oct;
using namespace octh;

namespace {

constexpr int kFlipMaxDim = 1 << 30;                    // B, rows of an image, bytes of a row: the kernel's 32-bit loop counters
constexpr size_t kFlipMaxBytes = (size_t)1 << 62;       // a whole buffer: its byte offsets are size_t

template <int VC>
void tta_launch(const TtaArgs& a, size_t items, unsigned grid, bool first, bool last, hipStream_t st) {
    if (first && last) tta_update_k<VC, true, true><<<grid, kMcThreads, 0, st>>>(a, items);
    else if (first) tta_update_k<VC, true, false><<<grid, kMcThreads, 0, st>>>(a, items);
    else if (last) tta_update_k<VC, false, true><<<grid, kMcThreads, 0, st>>>(a, items);
    else tta_update_k<VC, false, false><<<grid, kMcThreads, 0, st>>>(a, items);
}

}  // namespace

namespace octh {

// every argument error of oct_flip_batch, without launching; *bytes (optional) = the size of either buffer
int flip_validate(const void* src, int B, int H, int W, int pb, int view, const void* dst, size_t* bytes) {
    if (!src || !dst) return fail(-1, "flip_batch: null pointer (src_dev, dst_dev)");
    if (B < 1 || H < 1 || W < 1) return fail(-1, "flip_batch: B, H, W must be positive");
    if (!(pb == 1 || pb == 2 || (pb >= 4 && pb <= 32 && pb % 4 == 0)))
        return fail(-1, "flip_batch: pixel_bytes must be 1, 2 or a multiple of 4 in 4..32, not " + std::to_string(pb));
    if (view < 0 || view > 3) return fail(-1, "flip_batch: view must be in 0..3 (bit 0 mirrors columns, bit 1 rows), not " + std::to_string(view));
    size_t n = (size_t)W * (size_t)pb;
    if (B > kFlipMaxDim || H > kFlipMaxDim || n > (size_t)kFlipMaxDim || __builtin_mul_overflow(n, (size_t)H, &n) ||
        __builtin_mul_overflow(n, (size_t)B, &n) || n >= kFlipMaxBytes)
        return fail(-1, "flip_batch: element counts overflow the kernel's indexing (B, H and the bytes of a row <= 2^30, a buffer < 2^62 bytes)");
    const uintptr_t a0 = (uintptr_t)src, b0 = (uintptr_t)dst;
    if (a0 < b0 + n && b0 < a0 + n) return fail(-1, "flip_batch: the destination overlaps the source (the flip is out of place)");
    if (bytes) *bytes = n;
    return 0;
}

// every argument error of oct_tta_update, without launching: oct_unet_infer asks before its first launch
int tta_validate(const float* probs, int B, int H, int W, int n_cls, int view, int t, int T, const void* ws, size_t ws_bytes,
                 const oct_mc_out* out) {
    if (view < 0 || view > 3) return fail(-1, "tta_update: view must be in 0..3 (bit 0 mirrors columns, bit 1 rows), not " + std::to_string(view));
    if (T < 1 || T > kTtaMaxViews) return fail(-1, "tta_update: need 1 <= T <= " + std::to_string(kTtaMaxViews));
    if (int rc = mc_validate(probs, B, H, W, n_cls, t, T, ws, ws_bytes, out)) {
        std::string msg = oct_last_error();           // the shared checks speak as the call that was made
        if (msg.rfind("mc_update", 0) == 0) msg.replace(0, 9, "tta_update");
        return fail(rc, msg);
    }
    return 0;
}

}  // namespace octh

int oct_flip_batch(const void* src_dev, int B, int H, int W, int pixel_bytes, int view, void* dst_dev, oct_stream_t stream) {
    size_t n = 0;
    if (int rc = flip_validate(src_dev, B, H, W, pixel_bytes, view, dst_dev, &n)) return rc;
    FlipArgs a{};
    a.src = (const unsigned char*)src_dev; a.dst = (unsigned char*)dst_dev;
    a.B = B; a.H = H; a.W = W; a.pb = pixel_bytes; a.fx = view & 1; a.fy = (view >> 1) & 1;
    const int rb = W * pixel_bytes;
    // dwords where every row of both buffers starts on one; else bytes
    const bool dw = rb % 4 == 0 && (((uintptr_t)src_dev | (uintptr_t)dst_dev) & 3) == 0;
    // block (tx, 256 / tx): tx = the power of two in 16..256 that covers a row's units; grid: about 8192 blocks at the most
    const int units = dw ? rb / 4 : rb;
    int tx = 16;
    while (tx < 256 && tx < units) tx *= 2;
    const int ty = 256 / tx;
    const unsigned gx = (unsigned)std::min(cdiv(units, tx), 64), gz = (unsigned)std::min(B, 65535);
    const unsigned gy = (unsigned)std::max(1, std::min(cdiv(H, ty), (int)std::max(1u, 8192u / (gx * gz))));
    const dim3 grid(gx, std::min(gy, 65535u), gz), block((unsigned)tx, (unsigned)ty);
    hipStream_t st = (hipStream_t)stream;
    ProfScope ps(st, dw ? "flip_k<1>" : "flip_k<0>", "flip", 0.0, 2.0 * (double)n);
    if (dw) flip_k<true><<<grid, block, 0, st>>>(a);
    else flip_k<false><<<grid, block, 0, st>>>(a);
    HIP_OK(hipGetLastError());
    return 0;
}

int oct_tta_update(const float* probs_dev, int B, int H, int W, int n_cls, int view, int t, int T, void* ws_dev, size_t ws_bytes,
                   const oct_mc_out* out, oct_stream_t stream) {
    if (int rc = tta_validate(probs_dev, B, H, W, n_cls, view, t, T, ws_dev, ws_bytes, out)) return rc;
    const bool first = t == 0, last = t == T - 1;
    TtaArgs a{};
    McArgs& m = a.m;
    m.npix = (size_t)B * H * W; m.C = n_cls; m.inv_t = 1.0f / (float)T;
    m.probs = probs_dev; m.S = (float*)ws_dev; m.E = m.S + m.npix * n_cls;
    if (last) { m.mean = out->mean_probs; m.am = out->argmax; m.ent = out->entropy; m.mi = out->mutual_info; }
    a.H = (unsigned)H; a.W = (unsigned)W; a.fx = view & 1; a.fy = (view >> 1) & 1;
    // float4 items of 4 pixels of one row where W and every base allow it (E sits behind S: aligned as npix % 4 == 0); else per pixel
    const uintptr_t al16 = (uintptr_t)m.probs | (uintptr_t)m.S | (uintptr_t)m.mean | (uintptr_t)m.ent | (uintptr_t)m.mi;
    const bool vec = n_cls <= kMcMaxVec && W % 4 == 0 && (al16 & 15) == 0 && ((uintptr_t)m.am & 3) == 0;
    const int vc = vec ? n_cls : 0;
    const size_t items = vec ? m.npix / 4 : m.npix;
    const unsigned grid = (unsigned)std::min<size_t>((items + kMcThreads - 1) / kMcThreads, (size_t)kMcMaxBlocks);
    hipStream_t st = (hipStream_t)stream;
    // the bytes of oct_mc_update: p once; S read unless first, written unless last; E likewise; the maps on the last sample
    double by = (double)m.npix * n_cls * 4 * (1 + (first ? 0 : 1) + (last ? 0 : 1)) + (double)m.npix * 4 * ((first ? 0 : 1) + (last ? 0 : 1));
    if (last) by += (double)m.npix * ((m.mean ? n_cls * 4 : 0) + (m.am ? 1 : 0) + (m.ent ? 4 : 0) + (m.mi ? 4 : 0));
    ProfScope ps(st, vec ? "tta_update_k<C>" : "tta_update_k<0>", "tta_update", 0.0, by);
    switch (vc) {
        case 2: tta_launch<2>(a, items, grid, first, last, st); break;
        case 3: tta_launch<3>(a, items, grid, first, last, st); break;
        case 4: tta_launch<4>(a, items, grid, first, last, st); break;
        case 5: tta_launch<5>(a, items, grid, first, last, st); break;
        case 6: tta_launch<6>(a, items, grid, first, last, st); break;
        case 7: tta_launch<7>(a, items, grid, first, last, st); break;
        case 8: tta_launch<8>(a, items, grid, first, last, st); break;
        default: tta_launch<0>(a, items, grid, first, last, st); break;
    }
    HIP_OK(hipGetLastError());
    return 0;
}
