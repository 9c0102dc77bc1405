// One translation unit of liboct_unet_hip.so (see host.hpp): the calibration kernels (kernels_calibration.hpp) and their C ABI,
// oct_calibration_workspace_bytes / oct_calibration_counts / oct_temperature_apply / oct_temperature_workspace_bytes /
// oct_temperature_nll (include/oct_unet.h).  The calls allocate nothing and never wait for the stream.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>

#include "../../include/oct_unet.h"
#include "host.hpp"
#include "kernels_calibration.hpp"

using namespace oct;
using namespace octh;

namespace {

bool cal_shape_ok(int B, size_t npix, int n_cls) {
    return B >= 1 && B <= 65535 && npix >= 1 && n_cls >= 2 && n_cls <= kMcMaxClasses && npix < ((size_t)1 << 31) &&
           (size_t)B * npix < ((size_t)1 << 31);
}

bool overlap(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + nb && y < x + na;
}

// rows of the workspace: the blocks per image of the scalar path, which no launch of the shape exceeds
size_t cal_rows(int B, size_t npix) { return (size_t)B * cal_blocks_per_image(B, npix); }

// what the counts and the NLL call share: the argument errors, then the item form and the grid
struct CalPlan { int vc; size_t items; unsigned G; };
int cal_plan(const char* who, const float* probs, const unsigned char* labels, int B, size_t npix, int n_cls, int ignore_label,
             const void* ws, size_t ws_bytes, size_t need, CalArgs* a, CalPlan* p) {
    const std::string w(who);
    if (!probs || !labels || !ws) return fail(-1, w + ": null pointer");
    if (!cal_shape_ok(B, npix, n_cls))
        return fail(-1, w + ": need 1 <= B <= 65535, npix >= 1, B*npix < 2^31 and 2 <= n_cls <= " + std::to_string(kMcMaxClasses));
    if (ignore_label < -1 || ignore_label > 255) return fail(-1, w + ": ignore_label must be -1 (none) or in 0..255");
    if (ws_bytes < need) return fail(-4, w + ": workspace too small: need " + std::to_string(need) + " bytes");
    if (((uintptr_t)probs & 3) || ((uintptr_t)ws & 7)) return fail(-1, w + ": probs must be 4-byte and the workspace 8-byte aligned");
    const size_t nin = (size_t)B * npix * n_cls * sizeof(float);
    if (overlap(probs, nin, ws, need) || overlap(labels, (size_t)B * npix, ws, need))
        return fail(-1, w + ": the workspace overlaps an input");
    a->probs = probs; a->labels = labels; a->ws = (unsigned long long*)ws; a->npix = npix; a->C = n_cls; a->ignore = ignore_label;
    // float4 items of 4 pixels where every image's base allows it; else per pixel
    const bool vec = n_cls <= kMcMaxVec && (npix * n_cls) % 4 == 0 && ((uintptr_t)probs & 15) == 0;
    a->lab4 = ((uintptr_t)labels & 3) == 0 && npix % 4 == 0;
    p->vc = vec ? n_cls : 0;
    p->items = vec ? (npix + 3) / 4 : npix;
    p->G = cal_blocks_per_image(B, p->items);
    return 0;
}

#define CAL_SWITCH(vc, STMT)                                                                     \
    switch (vc) {                                                                                \
        case 2: { constexpr int VC = 2; STMT; } break;  case 3: { constexpr int VC = 3; STMT; } break; \
        case 4: { constexpr int VC = 4; STMT; } break;  case 5: { constexpr int VC = 5; STMT; } break; \
        case 6: { constexpr int VC = 6; STMT; } break;  case 7: { constexpr int VC = 7; STMT; } break; \
        case 8: { constexpr int VC = 8; STMT; } break;  default: { constexpr int VC = 0; STMT; } break; \
    }

}  // namespace

size_t oct_calibration_workspace_bytes(int B, size_t npix, int n_cls, int n_bins) {
    if (!cal_shape_ok(B, npix, n_cls) || n_bins < 1 || n_bins > kCalMaxBins) return 0;
    return cal_rows(B, npix) * (size_t)(3 * n_bins + 4) * 8;
}

int oct_calibration_counts(const float* probs_dev, const unsigned char* labels_dev, int B, size_t npix, int n_cls, int ignore_label,
                           int n_bins, unsigned long long* counts_dev, double* sums_dev, void* ws_dev, size_t ws_bytes,
                           oct_stream_t stream) {
    if (n_bins < 1 || n_bins > kCalMaxBins) return fail(-1, "calibration_counts: need 1 <= n_bins <= " + std::to_string(kCalMaxBins));
    if (!counts_dev || !sums_dev) return fail(-1, "calibration_counts: null pointer");
    if (((uintptr_t)counts_dev & 7) || ((uintptr_t)sums_dev & 7)) return fail(-1, "calibration_counts: outputs must be 8-byte aligned");
    CalArgs a{}; CalPlan p{};
    const size_t need = oct_calibration_workspace_bytes(B, npix, n_cls, n_bins);
    if (int rc = cal_plan("calibration_counts", probs_dev, labels_dev, B, npix, n_cls, ignore_label, ws_dev, ws_bytes, need, &a, &p))
        return rc;
    const size_t nc = (size_t)B * n_bins * 3 * 8, ns = (size_t)B * 4 * 8, nin = (size_t)B * npix * n_cls * sizeof(float);
    if (overlap(counts_dev, nc, sums_dev, ns) || overlap(counts_dev, nc, ws_dev, need) || overlap(sums_dev, ns, ws_dev, need) ||
        overlap(counts_dev, nc, probs_dev, nin) || overlap(sums_dev, ns, probs_dev, nin) ||
        overlap(counts_dev, nc, labels_dev, (size_t)B * npix) || overlap(sums_dev, ns, labels_dev, (size_t)B * npix))
        return fail(-1, "calibration_counts: an output range overlaps an input, the workspace or the other output");
    a.M = n_bins;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(p.G, (unsigned)B);
    {
        ProfScope ps(st, p.vc ? "calib_counts_k<C>" : "calib_counts_k<0>", "calibration_counts", 0.0,
                     (double)B * npix * (n_cls * 4 + 1));
        CAL_SWITCH(p.vc, (calib_counts_k<VC><<<grid, kCalThreads, 0, st>>>(a, p.items)));
        HIP_OK(hipGetLastError());
    }
    ProfScope ps(st, "calib_rows_sum_k", "calibration_counts", 0.0, (double)B * p.G * (3 * n_bins + 4) * 8);
    calib_rows_sum_k<<<dim3((unsigned)B, (3 * n_bins + 4 + 63) / 64), kCalThreads, 0, st>>>(a.ws, (int)p.G, 3 * n_bins, 4, counts_dev, sums_dev, nullptr);
    HIP_OK(hipGetLastError());
    return 0;
}

int oct_temperature_apply(const float* probs_in_dev, float* probs_out_dev, size_t npix_total, int n_cls, float beta,
                          oct_stream_t stream) {
    if (!probs_in_dev || !probs_out_dev) return fail(-1, "temperature_apply: null pointer");
    if (npix_total < 1 || npix_total >= ((size_t)1 << 31) || n_cls < 2 || n_cls > kMcMaxClasses)
        return fail(-1, "temperature_apply: need 1 <= npix_total < 2^31 and 2 <= n_cls <= " + std::to_string(kMcMaxClasses));
    if (!std::isfinite(beta) || !(beta > 0.f)) return fail(-1, "temperature_apply: beta must be finite and positive");
    if (((uintptr_t)probs_in_dev & 3) || ((uintptr_t)probs_out_dev & 3)) return fail(-1, "temperature_apply: buffers must be 4-byte aligned");
    const size_t n = npix_total * n_cls * sizeof(float);
    if ((const float*)probs_out_dev != probs_in_dev && overlap(probs_in_dev, n, probs_out_dev, n))
        return fail(-1, "temperature_apply: the output must be the input itself or not overlap it");
    const bool vec = n_cls <= kMcMaxVec && (((uintptr_t)probs_in_dev | (uintptr_t)probs_out_dev) & 15) == 0;
    const int vc = vec ? n_cls : 0;
    const size_t items = vec ? (npix_total + 3) / 4 : npix_total;
    const unsigned grid = (unsigned)std::min<size_t>((items + kCalThreads - 1) / kCalThreads, (size_t)kCalMaxBlocks);
    hipStream_t st = (hipStream_t)stream;
    ProfScope ps(st, vec ? "temperature_apply_k<C>" : "temperature_apply_k<0>", "temperature_apply", 0.0, 2.0 * n);
    CAL_SWITCH(vc, (temperature_apply_k<VC><<<grid, kCalThreads, 0, st>>>(probs_in_dev, probs_out_dev, npix_total, n_cls, beta, items)));
    HIP_OK(hipGetLastError());
    return 0;
}

size_t oct_temperature_workspace_bytes(int B, size_t npix, int n_cls, int n_betas) {
    if (!cal_shape_ok(B, npix, n_cls) || n_betas < 1 || n_betas > kCalMaxBetas) return 0;
    return cal_rows(B, npix) * (size_t)(3 * n_betas + 1) * 8;
}

int oct_temperature_nll(const float* probs_dev, const unsigned char* labels_dev, int B, size_t npix, int n_cls, int ignore_label,
                        const float* betas, int n_betas, double* out_dev, void* ws_dev, size_t ws_bytes, oct_stream_t stream) {
    if (n_betas < 1 || n_betas > kCalMaxBetas) return fail(-1, "temperature_nll: need 1 <= n_betas <= " + std::to_string(kCalMaxBetas));
    if (!betas || !out_dev) return fail(-1, "temperature_nll: null pointer");
    if ((uintptr_t)out_dev & 7) return fail(-1, "temperature_nll: out must be 8-byte aligned");
    CalBetas bt{};
    bt.K = n_betas;
    for (int k = 0; k < n_betas; ++k) {
        if (!std::isfinite(betas[k]) || !(betas[k] > 0.f)) return fail(-1, "temperature_nll: every beta must be finite and positive");
        bt.b[k] = betas[k];
    }
    CalArgs a{}; CalPlan p{};
    const size_t need = oct_temperature_workspace_bytes(B, npix, n_cls, n_betas);
    if (int rc = cal_plan("temperature_nll", probs_dev, labels_dev, B, npix, n_cls, ignore_label, ws_dev, ws_bytes, need, &a, &p)) return rc;
    const size_t no = (size_t)B * (3 * n_betas + 1) * 8;
    if (overlap(out_dev, no, ws_dev, need) || overlap(out_dev, no, probs_dev, (size_t)B * npix * n_cls * sizeof(float)) ||
        overlap(out_dev, no, labels_dev, (size_t)B * npix))
        return fail(-1, "temperature_nll: out overlaps an input or the workspace");
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(p.G, (unsigned)B);
    {
        ProfScope ps(st, p.vc ? "temperature_nll_k<C>" : "temperature_nll_k<0>", "temperature_nll", 0.0, (double)B * npix * (n_cls * 4 + 1));
        CAL_SWITCH(p.vc, (temperature_nll_k<VC><<<grid, kCalThreads, 0, st>>>(a, bt, p.items)));
        HIP_OK(hipGetLastError());
    }
    ProfScope ps(st, "calib_rows_sum_k", "temperature_nll", 0.0, (double)B * p.G * (3 * n_betas + 1) * 8);
    calib_rows_sum_k<<<dim3((unsigned)B, 1), kCalThreads, 0, st>>>(a.ws, (int)p.G, 0, 3 * n_betas + 1, nullptr, out_dev, out_dev + (size_t)B * 3 * n_betas);
    HIP_OK(hipGetLastError());
    return 0;
}
