// One translation unit of liboct_unet_hip.so (see host.hpp): surface-distance metrics of class maps
// (kernels_surface.hpp) and their C ABI, oct_surface_workspace_bytes / oct_surface_distances /
// oct_surface_distances_masked (include/oct_unet.h).
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "../../include/oct_unet.h"
#include "host.hpp"
#include "kernels_surface.hpp"

using namespace oct;
using namespace octh;

namespace {
constexpr size_t kAlign = 256;
size_t align_up(size_t x) { return (x + kAlign - 1) / kAlign * kAlign; }

bool geom(int B, int H, int W, int n_cls, SurfGeom* g) {
    if (B < 1 || H < 1 || W < 1 || H > 32767 || W > 16383 || n_cls < 2 || n_cls > 256) return false;
    g->B = B; g->H = H; g->W = W; g->n_cls = n_cls; g->Hc = H + 1; g->Wc = W + 1;
    g->N = (size_t)g->Hc * g->Wc;
    g->KS = (g->N + 15) / 16 * 16;
    return (size_t)B * (n_cls - 1) * 2 <= 65535;    // one grid row per (image, class, mask) in the row pass
}

// workspace: [error word | kinds (planes x KS u8) | column distances (planes x N u16) | distances (planes x N f64)]
struct Layout { size_t kind, dy, dist, total; };
Layout layout(const SurfGeom& g) {
    const size_t planes = (size_t)g.B * (g.n_cls - 1) * 2;
    Layout l;
    l.kind = kAlign;
    l.dy = l.kind + align_up(planes * g.KS);
    l.dist = l.dy + align_up(planes * g.N * sizeof(unsigned short));
    l.total = l.dist + align_up(planes * g.N * sizeof(double));
    return l;
}
}  // namespace

size_t oct_surface_workspace_bytes(int B, int H, int W, int n_cls) {
    SurfGeom g;
    return geom(B, H, W, n_cls, &g) ? layout(g).total : 0;
}

namespace {
// ignore_label < 0: oct_surface_distances; else the masked column pass in front of the same row and select passes
int surface_distances(const unsigned char* pred, const unsigned char* gt, int B, int H, int W, int n_cls, int ignore_label,
                      double spacing_row, double spacing_col, double percent, void* workspace, size_t workspace_bytes,
                      double* out, oct_stream_t stream) {
    SurfGeom g;
    if (!pred || !gt || !workspace || !out) return fail(-1, "surface_distances: null pointer");
    if (!geom(B, H, W, n_cls, &g))
        return fail(-1, "surface_distances: need B >= 1, 1 <= H <= 32767, 1 <= W <= 16383, 2 <= n_cls <= 256, "
                        "B*(n_cls-1)*2 <= 65535");
    if (!(spacing_row > 0.0) || !(spacing_col > 0.0) || !std::isfinite(spacing_row) || !std::isfinite(spacing_col))
        return fail(-1, "surface_distances: spacings must be positive and finite");
    if (!(percent >= 0.0 && percent <= 100.0)) return fail(-1, "surface_distances: percent must lie in [0, 100]");
    const Layout l = layout(g);
    if (workspace_bytes < l.total)
        return fail(-1, "surface_distances: workspace too small (" + std::to_string(workspace_bytes) + " < " +
                        std::to_string(l.total) + " bytes)");
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    unsigned int* bad = (unsigned int*)ws;
    unsigned char* kind = (unsigned char*)(ws + l.kind);
    unsigned short* dy = (unsigned short*)(ws + l.dy);
    double* dist = (double*)(ws + l.dist);
    const unsigned planes = (unsigned)((size_t)B * (n_cls - 1) * 2);

    HIP_OK(hipMemsetAsync(bad, 0, sizeof(unsigned int), st));
    const size_t ncol = (size_t)planes * g.Wc;
    if (ignore_label >= 0)
        surf_col_k<true><<<(unsigned)((ncol + 255) / 256), 256, 0, st>>>(gt, pred, g, ignore_label, kind, dy, bad);
    else
        surf_col_k<false><<<(unsigned)((ncol + 255) / 256), 256, 0, st>>>(gt, pred, g, -1, kind, dy, bad);
    HIP_OK(hipGetLastError());
    // labels >= n_cls are an argument error: the column pass flags them and the call reports it before the distance passes
    unsigned int flag = 0;
    HIP_OK(hipMemcpyAsync(&flag, bad, sizeof(flag), hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    if (flag)
        return fail(-2, "surface_distances: a label is >= n_cls=" + std::to_string(n_cls) +
                        (ignore_label >= 0 ? " and not the ignore label " + std::to_string(ignore_label) : std::string()));

    surf_row_k<<<dim3((unsigned)g.Hc, planes), 256, (size_t)g.Wc * sizeof(unsigned short), st>>>(g, kind, dy, dist,
                                                                                                spacing_row, spacing_col);
    HIP_OK(hipGetLastError());
    double ld, lh = spacing_col, lv = spacing_row, l2;
    {
#pragma clang fp contract(off)
        ld = 0.5 * std::sqrt(spacing_row * spacing_row + spacing_col * spacing_col);
        l2 = 2.0 * ld;
    }
    surf_select_k<<<planes, kSurfSelectThreads, 0, st>>>(g, kind, dist, ld, lh, lv, l2, percent / 100.0, out);
    HIP_OK(hipGetLastError());
    return 0;
}
}  // namespace

int oct_surface_distances(const unsigned char* pred, const unsigned char* gt, int B, int H, int W, int n_cls,
                          double spacing_row, double spacing_col, double percent, void* workspace, size_t workspace_bytes,
                          double* out, oct_stream_t stream) {
    return surface_distances(pred, gt, B, H, W, n_cls, -1, spacing_row, spacing_col, percent, workspace, workspace_bytes, out,
                             stream);
}

int oct_surface_distances_masked(const unsigned char* pred, const unsigned char* gt, int B, int H, int W, int n_cls,
                                 int ignore_label, double spacing_row, double spacing_col, double percent, void* workspace,
                                 size_t workspace_bytes, double* out, oct_stream_t stream) {
    if (ignore_label < n_cls || ignore_label < 0 || ignore_label > 255)
        return fail(-1, "surface_distances_masked: ignore_label must lie in n_cls..255");
    return surface_distances(pred, gt, B, H, W, n_cls, ignore_label, spacing_row, spacing_col, percent, workspace,
                             workspace_bytes, out, stream);
}
