// One translation unit of liboct_unet_hip.so (see host.hpp): the confusion counts behind the evaluation's Dice metrics
// and the class map of graph-search delineations (kernels_dice.hpp), with their C ABI, oct_confusion_counts /
// oct_confusion_counts_masked / oct_area_labels (include/oct_unet.h).  Neither call allocates or waits for the stream.
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/oct_unet.h"
#include "host.hpp"
#include "kernels_dice.hpp"

using namespace oct;
using namespace octh;

namespace {
// ignore_label < 0: oct_confusion_counts (rows of n_cls^2 + 1 words); else the masked kernel (rows of n_cls^2 + 2)
int confusion_counts(const char* who, const unsigned char* pred, const unsigned char* gt, int B, int H, int W, int n_cls,
                     int ignore_label, unsigned int* counts, oct_stream_t stream) {
    const std::string name(who);
    if (!pred || !gt || !counts) return fail(-1, name + ": null pointer");
    if (B < 1 || B > 65535 || H < 1 || W < 1 || n_cls < 2 || n_cls > kDiceMaxClasses ||
        (unsigned long long)H * (unsigned long long)W >= (1ull << 32))
        return fail(-1, name + ": need 1 <= B <= 65535, H, W >= 1, H*W < 2^32, 2 <= n_cls <= " +
                        std::to_string(kDiceMaxClasses));
    const bool masked = ignore_label >= 0;
    hipStream_t st = (hipStream_t)stream;
    const size_t npix = (size_t)H * W, nk = (size_t)n_cls * n_cls + (masked ? 2 : 1);
    HIP_OK(hipMemsetAsync(counts, 0, (size_t)B * nk * sizeof(unsigned int), st));
    // four 16-byte steps per thread, at most 1024 chunks per image
    size_t chunks = (npix / 16 + 4 * kDiceThreads - 1) / (4 * kDiceThreads);
    chunks = chunks < 1 ? 1 : chunks > 1024 ? 1024 : chunks;
    const dim3 grid((unsigned)chunks, (unsigned)B);
    if (masked)
        confusion_masked_k<<<grid, kDiceThreads, 0, st>>>(pred, gt, npix, n_cls, (unsigned)ignore_label, counts);
    else
        confusion_k<<<grid, kDiceThreads, 0, st>>>(pred, gt, npix, n_cls, counts);
    HIP_OK(hipGetLastError());
    return 0;
}
}  // namespace

int oct_confusion_counts(const unsigned char* pred, const unsigned char* gt, int B, int H, int W, int n_cls,
                         unsigned int* counts, oct_stream_t stream) {
    return confusion_counts("confusion_counts", pred, gt, B, H, W, n_cls, -1, counts, stream);
}

int oct_confusion_counts_masked(const unsigned char* pred, const unsigned char* gt, int B, int H, int W, int n_cls,
                                int ignore_label, unsigned int* counts, oct_stream_t stream) {
    if (n_cls >= 2 && (ignore_label < n_cls || ignore_label > 255))
        return fail(-1, "confusion_counts_masked: ignore_label must lie in n_cls..255");
    return confusion_counts("confusion_counts_masked", pred, gt, B, H, W, n_cls, ignore_label < 0 ? 0 : ignore_label, counts,
                            stream);
}

int oct_area_labels(const unsigned short* segs, int B, int H, int W, int n_cls, unsigned char* labels,
                    oct_stream_t stream) {
    if (!segs || !labels) return fail(-1, "area_labels: null pointer");
    if (B < 1 || B > 65535 || H < 1 || H > 65535 || W < 1 || n_cls < 2 || n_cls > kDiceMaxClasses ||
        (unsigned long long)H * (unsigned long long)W >= (1ull << 32))
        return fail(-1, "area_labels: need 1 <= B <= 65535, 1 <= H <= 65535 (uint16 rows), W >= 1, H*W < 2^32, "
                        "2 <= n_cls <= " + std::to_string(kDiceMaxClasses));
    const unsigned gx = (unsigned)(((size_t)W + kAreaTileW - 1) / kAreaTileW), gy = (unsigned)((H + kAreaTileH - 1) / kAreaTileH);
    area_labels_k<<<dim3(gx, gy, (unsigned)B), kDiceThreads, 0, (hipStream_t)stream>>>(segs, H, W, n_cls - 1, labels);
    HIP_OK(hipGetLastError());
    return 0;
}
