// One translation unit of liboct_unet_hip.so (see host.hpp): the soft boundary maps (kernels_softmaps.hpp) and their C
// ABI, oct_boundary_maps_soft (include/oct_unet.h).  The call allocates nothing and never waits for the stream.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <string>

#include "../../include/oct_unet.h"
#include "host.hpp"
#include "kernels_softmaps.hpp"

using namespace oct;
using namespace octh;

int oct_boundary_maps_soft(const float* probs_dev, int B, int H, int W, int n_cls, int bg_ilm, int bg_csi,
                           unsigned char* maps_dev, oct_stream_t stream) {
    if (!probs_dev || !maps_dev) return fail(-1, "boundary_maps_soft: null pointer");
    if (B < 1 || H < 1 || W < 1) return fail(-1, "boundary_maps_soft: B, H, W must be positive");
    if (n_cls < 2 || n_cls > kSoftMaxClasses)
        return fail(-1, "boundary_maps_soft: need 2 <= n_cls <= " + std::to_string(kSoftMaxClasses));
    const size_t npix = (size_t)B * H * W;
    const size_t nin = npix * n_cls * sizeof(float), nout = npix * (size_t)(n_cls - 1);
    const uintptr_t p0 = (uintptr_t)probs_dev, m0 = (uintptr_t)maps_dev;
    if (p0 < m0 + nout && m0 < p0 + nin) return fail(-1, "boundary_maps_soft: the output range overlaps the input");
    const size_t items = (size_t)B * (size_t)((H + kSoftRows - 1) / kSoftRows) * (size_t)((W + kSoftCols - 1) / kSoftCols);
    const unsigned grid = (unsigned)std::min<size_t>((items + kSoftThreads - 1) / kSoftThreads, (size_t)kSoftMaxBlocks);
    hipStream_t st = (hipStream_t)stream;
    // float4 rows carrying every channel where the shape and the base allow it (2..4 classes); else a pass per map
    const int vc = (n_cls <= 4 && W % kSoftCols == 0 && p0 % 16 == 0) ? n_cls : 0;
    // bytes: one read of the probabilities (every channel: the rows are contiguous in memory) + the maps written
    ProfScope ps(st, vc ? "soft_maps_k<C>" : "soft_maps_k<0>", "boundary_maps_soft", 0.0, (double)(nin + nout));
    const int ilm = bg_ilm != 0, csi = bg_csi != 0;
    switch (vc) {
        case 2: soft_maps_k<2><<<grid, kSoftThreads, 0, st>>>(probs_dev, maps_dev, items, H, W, n_cls, ilm, csi); break;
        case 3: soft_maps_k<3><<<grid, kSoftThreads, 0, st>>>(probs_dev, maps_dev, items, H, W, n_cls, ilm, csi); break;
        case 4: soft_maps_k<4><<<grid, kSoftThreads, 0, st>>>(probs_dev, maps_dev, items, H, W, n_cls, ilm, csi); break;
        default: soft_maps_k<0><<<grid, kSoftThreads, 0, st>>>(probs_dev, maps_dev, items, H, W, n_cls, ilm, csi); break;
    }
    HIP_OK(hipGetLastError());
    return 0;
}
