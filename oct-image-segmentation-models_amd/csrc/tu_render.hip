// One translation unit of liboct_unet_hip.so (see host.hpp): the picture rasteriser (kernels_render.hpp) and its C ABI,
// oct_render_rgba (include/oct_unet.h).  The call allocates nothing and never waits for the stream; the style struct is
// copied into the kernel's arguments.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "../../include/oct_unet.h"
#include "host.hpp"
#include "kernels_render.hpp"

using namespace oct;
using namespace octh;

static_assert(kRenderMaxR == 64 && kRenderMaxHalo == 10, "the halo of render_rgba_k follows the largest half_width");

int oct_render_rgba(int base_mode, const unsigned char* base_dev, int ic, const unsigned short* rows_dev,
                    const oct_render_style* style, int B, int H, int W, unsigned char* out_dev, oct_stream_t stream) {
    if (!base_dev || !out_dev || !style) return fail(-1, "render_rgba: null pointer");
    if (B < 1 || H < 1 || W < 1) return fail(-1, "render_rgba: B, H, W must be positive");
    if (B > 65535) return fail(-1, "render_rgba: B above 65535");
    if (W > (1 << 24)) return fail(-1, "render_rgba: W above 2^24");
    if (H > kRenderMaxH) return fail(-1, "render_rgba: H above " + std::to_string(kRenderMaxH));
    if (base_mode != OCT_RENDER_BASE_IMAGE && base_mode != OCT_RENDER_BASE_LABELS)
        return fail(-1, "render_rgba: unknown base mode " + std::to_string(base_mode));
    if (base_mode == OCT_RENDER_BASE_IMAGE && ic < 1) return fail(-1, "render_rgba: the image needs ic >= 1 channels");
    if (base_mode == OCT_RENDER_BASE_LABELS && (style->n_cls < 1 || style->n_cls > OCT_RENDER_MAX_CLASSES))
        return fail(-1, "render_rgba: need 1 <= n_cls <= " + std::to_string(OCT_RENDER_MAX_CLASSES));
    const int K = style->n_lines;
    if (K < 0 || K > OCT_RENDER_MAX_LINES)
        return fail(-1, "render_rgba: need 0 <= n_lines <= " + std::to_string(OCT_RENDER_MAX_LINES));
    if (K > 0 && !rows_dev) return fail(-1, "render_rgba: null pointer (rows_dev with n_lines > 0)");
    if (style->half_width < 1 || style->half_width > kRenderMaxR)
        return fail(-1, "render_rgba: need 1 <= half_width <= " + std::to_string(kRenderMaxR));
    if (style->col_lo > style->col_hi || style->col_lo < 0 || style->col_hi > W - 1)
        return fail(-1, "render_rgba: need 0 <= col_lo <= col_hi <= W - 1");
    for (int k = 0; k < K; ++k)
        if (style->line_style[k] > 1) return fail(-1, "render_rgba: line_style must be 0 (solid) or 1 (dotted)");
    const size_t npix = (size_t)B * H * W;
    const size_t nbase = npix * (size_t)(base_mode == OCT_RENDER_BASE_IMAGE ? ic : 1), nout = npix * 4;
    const size_t nrows = (size_t)B * K * W * sizeof(unsigned short);
    const uintptr_t b0 = (uintptr_t)base_dev, r0 = (uintptr_t)rows_dev, o0 = (uintptr_t)out_dev;
    if ((b0 < o0 + nout && o0 < b0 + nbase) || (K > 0 && r0 < o0 + nout && o0 < r0 + nrows))
        return fail(-1, "render_rgba: the output range overlaps an input");
    RenderArgs a;
    a.base = base_dev; a.rows = rows_dev; a.out = out_dev;
    a.mode = base_mode; a.ic = base_mode == OCT_RENDER_BASE_IMAGE ? ic : 1; a.H = H; a.W = W;
    a.st = *style;
    const dim3 grid((unsigned)((W + kRenderCols - 1) / kRenderCols), (unsigned)((H + kRenderRows - 1) / kRenderRows), (unsigned)B);
    hipStream_t st = (hipStream_t)stream;
    // bytes: the base and the line rows read once, the picture written
    ProfScope ps(st, "render_rgba_k", "render_rgba", 0.0, (double)(nbase + nrows + nout));
    render_rgba_k<<<grid, kRenderThreads, 0, st>>>(a);
    HIP_OK(hipGetLastError());
    return 0;
}
