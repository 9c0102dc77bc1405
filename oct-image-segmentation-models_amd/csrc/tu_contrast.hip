// One translation unit of liboct_unet_hip.so (see host.hpp): contrast normalisation on the device (kernels_contrast.hpp) and
// its C ABI, oct_contrast_workspace_bytes / oct_contrast_batch (include/oct_unet.h).  One memset and three launches; the call
// allocates nothing and never waits for the stream.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <string>

#include "../../include/oct_unet.h"
#include "host.hpp"
#include "kernels_contrast.hpp"

using namespace oct;
using namespace octh;

static_assert(OCT_CONTRAST_CLAHE == CT_CLAHE && OCT_CONTRAST_STRETCH == CT_STRETCH, "header and kernel agree on the methods");
static_assert(OCT_CONTRAST_MAX_TILES == CT_MAX_TILES && OCT_CONTRAST_MIN_TILE == CT_MIN_TILE && OCT_CONTRAST_MAX_DIM == CT_MAX_DIM,
              "header and kernel agree on the limits");

namespace {

// empty when the call is accepted, else what is wrong with it
std::string ct_refusal(int B, int H, int W, int ch, const oct_contrast_desc* d) {
    if (!d) return "null descriptor";
    if (B < 1 || B > 65535) return "B must be in 1..65535";
    if (H < 1 || W < 1 || H > CT_MAX_DIM || W > CT_MAX_DIM) return "H and W must be in 1..4096";
    if (ch < 1 || ch > 4) return "ch must be in 1..4";
    if (d->method != CT_CLAHE && d->method != CT_STRETCH) return "method must be OCT_CONTRAST_CLAHE or OCT_CONTRAST_STRETCH";
    if (d->tiles_y < 1 || d->tiles_y > CT_MAX_TILES || d->tiles_x < 1 || d->tiles_x > CT_MAX_TILES) return "tiles must be in 1..16";
    if (H / d->tiles_y < CT_MIN_TILE || W / d->tiles_x < CT_MIN_TILE)
        return "tiles of " + std::to_string(H / d->tiles_y) + " x " + std::to_string(W / d->tiles_x) + " pixels: need at least 8 x 8";
    if (d->method == CT_CLAHE && d->clip_q8 != 0 && (d->clip_q8 < 256 || d->clip_q8 > 65535))
        return "clip_q8 must be 0 (no limit) or in 256..65535";
    if (d->method == CT_STRETCH && !(0 <= d->lo_bp && d->lo_bp < d->hi_bp && d->hi_bp <= 10000))
        return "need 0 <= lo_bp < hi_bp <= 10000";
    return "";
}

size_t ct_lut_bytes(int B, int ch, const oct_contrast_desc* d) { return (size_t)B * ch * d->tiles_y * d->tiles_x * CT_BINS; }

bool overlap(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + nb && y < x + na;
}

}  // namespace

size_t oct_contrast_workspace_bytes(int B, int H, int W, int ch, const oct_contrast_desc* d) {
    if (!ct_refusal(B, H, W, ch, d).empty()) return 0;
    return ct_lut_bytes(B, ch, d) * (1 + sizeof(unsigned));      // the LUTs, then the uint32 histograms
}

int oct_contrast_batch(const unsigned char* x_dev, int B, int H, int W, int ch, const oct_contrast_desc* d, void* ws_dev,
                       size_t ws_bytes, unsigned char* out_dev, oct_stream_t stream) {
    if (!x_dev || !d || !ws_dev || !out_dev) return fail(-1, "contrast_batch: null pointer (x_dev, d, ws_dev, out_dev)");
    const std::string why = ct_refusal(B, H, W, ch, d);
    if (!why.empty()) return fail(-1, "contrast_batch: " + why);
    const size_t need = oct_contrast_workspace_bytes(B, H, W, ch, d), nlut = ct_lut_bytes(B, ch, d);
    if (ws_bytes < need) return fail(-4, "contrast_batch: workspace too small: need " + std::to_string(need) + " bytes");
    if ((uintptr_t)ws_dev & 3) return fail(-1, "contrast_batch: the workspace must be 4-byte aligned");
    const size_t n = (size_t)B * H * W * ch;
    if (out_dev != x_dev && overlap(x_dev, n, out_dev, n)) return fail(-1, "contrast_batch: out_dev must be x_dev itself or not overlap it");
    if (overlap(out_dev, n, ws_dev, need)) return fail(-1, "contrast_batch: out_dev overlaps the workspace");
    if (overlap(x_dev, n, ws_dev, need)) return fail(-1, "contrast_batch: the workspace overlaps the input");

    ContrastGeom g{};
    g.H = H; g.W = W; g.ch = ch; g.ty = d->tiles_y; g.tx = d->tiles_x;
    g.method = d->method; g.clip_q8 = d->clip_q8; g.lo_bp = d->lo_bp; g.hi_bp = d->hi_bp;
    // blocks per tile: a tile's rows are shared out until about 1024 blocks are in flight; never more bands than the
    // lowest tile has rows
    const int ntiles = g.ty * g.tx;
    const size_t slots = (size_t)B * ch * ntiles;
    g.split = slots >= 1024 ? 1 : (int)std::min<size_t>((1024 + slots - 1) / slots, (size_t)std::min(H / g.ty, (int)CT_MAX_SPLIT));
    unsigned char* lut = (unsigned char*)ws_dev;
    unsigned* hist = (unsigned*)(lut + nlut);
    hipStream_t st = (hipStream_t)stream;
    {
        ProfScope ps(st, "contrast_hist_k", "contrast", 0.0, (double)n + 4.0 * (double)nlut);
        HIP_OK(hipMemsetAsync(hist, 0, nlut * sizeof(unsigned), st));
        contrast_hist_k<<<dim3((unsigned)(ntiles * g.split), (unsigned)ch, (unsigned)B), CT_THREADS, 0, st>>>(x_dev, g, hist);
        HIP_OK(hipGetLastError());
    }
    {
        ProfScope ps(st, "contrast_lut_k", "contrast", 0.0, 5.0 * (double)nlut);
        contrast_lut_k<<<dim3((unsigned)ntiles, (unsigned)ch, (unsigned)B), CT_THREADS, 0, st>>>(hist, g, lut);
        HIP_OK(hipGetLastError());
    }
    // four bytes per thread where every row of every image, in and out, starts on a 4-byte boundary
    const size_t rowb = (size_t)W * ch;
    const bool vec = rowb % 4 == 0 && (((uintptr_t)x_dev | (uintptr_t)out_dev) & 3) == 0;
    const unsigned upr = (unsigned)(vec ? rowb / 4 : rowb);
    const dim3 grid((unsigned)(((size_t)H * upr + CT_THREADS - 1) / CT_THREADS), (unsigned)B);
    ProfScope ps(st, vec ? "contrast_apply_k<4>" : "contrast_apply_k<1>", "contrast", 0.0, 2.0 * (double)n);
    if (vec) contrast_apply_k<4><<<grid, CT_THREADS, 0, st>>>(x_dev, lut, g, upr, out_dev);
    else contrast_apply_k<1><<<grid, CT_THREADS, 0, st>>>(x_dev, lut, g, upr, out_dev);
    HIP_OK(hipGetLastError());
    return 0;
}
