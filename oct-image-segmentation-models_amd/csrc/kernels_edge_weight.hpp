// Edge weight maps on the device: (B,H,W) uint8 labels -> (B,H,W) f32 per-pixel loss weights w(x) = lut[d2(x)], d2 the
// capped exact squared Euclidean distance to the nearest class border of the same image.  The definition is
// include/oct_unet.h, oct_edge_weight_map; common/utils.py edge_weight_reference restates it in numpy.  The distances are
// integers, so device and numpy agree bit for bit; the only floats are the table's.
//
// edge_weight_k: grid (tiles per image, B), one launch, no workspace.  A block owns one EW_TH x EW_TW tile of one image and
// holds everything it needs in LDS (sized at launch from R), three byte planes and three barriers:
//   1. labels of the tile with a halo of R + 1 on every side (255 = unknown outside the image);
//   2. the edge flags of the tile with a halo of R: a known pixel with a known 4-neighbour of another label;
//   3. column pass: v <= R, the vertical distance of each pixel of the tile's rows (halo of R columns) to the nearest edge
//      pixel of its column, or EW_NONE;
//   4. row pass: a thread owns one pixel, d2 = min over |dx| <= R of dx^2 + v(x + dx)^2 where that is <= R^2, else R^2 + 1.
// O(R) work per pixel in 3 and 4, the pattern of the column and row passes of kernels_surface.hpp.  Every LDS access of a
// wave is along a row: 64 lanes read 64 consecutive bytes = 16 words in 16 banks, four lanes sharing each word (a
// broadcast); no plane is read column-wise by neighbouring lanes, so the byte planes need no padding against conflicts.
// No atomics, no block waits on another, every loop bounded by R or the tile.
#pragma once
#include <hip/hip_runtime.h>

namespace oct {

enum { EW_TH = 32, EW_TW = 64, EW_MAX_R = 32, EW_NONE = 255 };

struct EdgeWeightGeom {
    int H, W, n_cls, R;
    unsigned tiles_x;   // tiles across one row of tiles
};

// row pitches of the three planes (multiples of 4 bytes) and the bytes of LDS a block takes at radius R
__host__ __device__ constexpr int ew_pitch_lab(int R) { return (EW_TW + 2 * R + 2 + 3) & ~3; }
__host__ __device__ constexpr int ew_pitch_edge(int R) { return (EW_TW + 2 * R + 3) & ~3; }
__host__ __device__ constexpr int ew_lds_bytes(int R) {
    return (EW_TH + 2 * R + 2) * ew_pitch_lab(R) + (EW_TH + 2 * R) * ew_pitch_edge(R) + EW_TH * ew_pitch_edge(R);
}

__global__ __launch_bounds__(256) void edge_weight_k(const unsigned char* __restrict__ lab, const float* __restrict__ lut,
                                                     const EdgeWeightGeom g, float* __restrict__ out) {
    extern __shared__ __align__(16) unsigned char ew_lds[];
    const int R = g.R, H = g.H, W = g.W, n_cls = g.n_cls, tid = (int)threadIdx.x;
    const int LH = EW_TH + 2 * R + 2, LW = EW_TW + 2 * R + 2, pL = ew_pitch_lab(R);      // labels: halo R + 1
    const int EH = EW_TH + 2 * R, EWd = EW_TW + 2 * R, pE = ew_pitch_edge(R);            // edge flags: halo R
    unsigned char* const s_lab = ew_lds;
    unsigned char* const s_edge = s_lab + LH * pL;
    unsigned char* const s_v = s_edge + EH * pE;
    const int ty0 = (int)(blockIdx.x / g.tiles_x) * EW_TH, tx0 = (int)(blockIdx.x % g.tiles_x) * EW_TW;
    const size_t img = (size_t)blockIdx.y * (size_t)H * (size_t)W;
    const unsigned char* const ls = lab + img;

    for (int t = tid; t < LH * LW; t += 256) {
        const int r = t / LW, c = t - r * LW, y = ty0 - R - 1 + r, x = tx0 - R - 1 + c;
        const bool in = (unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W;
        s_lab[r * pL + c] = in ? ls[(size_t)y * W + x] : (unsigned char)255;
    }
    __syncthreads();
    for (int t = tid; t < EH * EWd; t += 256) {
        const int r = t / EWd, c = t - r * EWd;
        const unsigned char* p = s_lab + (r + 1) * pL + c + 1;
        const int a = p[0], up = p[-pL], dn = p[pL], lf = p[-1], rt = p[1];
        const bool e = a < n_cls && ((up < n_cls && up != a) || (dn < n_cls && dn != a) || (lf < n_cls && lf != a) || (rt < n_cls && rt != a));
        s_edge[r * pE + c] = e ? 1 : 0;
    }
    __syncthreads();
    for (int t = tid; t < EW_TH * EWd; t += 256) {
        const int r = t / EWd, c = t - r * EWd;
        const unsigned char* p = s_edge + (r + R) * pE + c;
        int v = EW_NONE;
        for (int d = 0; d <= R; ++d)
            if (p[-d * pE] | p[d * pE]) { v = d; break; }
        s_v[r * pE + c] = (unsigned char)v;
    }
    __syncthreads();
    const int R2 = R * R;
    for (int t = tid; t < EW_TH * EW_TW; t += 256) {
        const int r = t / EW_TW, c = t % EW_TW, y = ty0 + r, x = tx0 + c;
        if (y >= H || x >= W) continue;
        float w = 0.f;
        if (s_lab[(r + R + 1) * pL + c + R + 1] < n_cls) {
            const unsigned char* p = s_v + r * pE + c + R;
            int best = R2 + 1;
            for (int dx = -R; dx <= R; ++dx) {
                const int v = p[dx], d2 = dx * dx + v * v;      // EW_NONE^2 > R^2: a column without an edge never wins
                best = d2 < best ? d2 : best;
            }
            w = lut[best];
        }
        out[img + (size_t)y * W + x] = w;
    }
}

}  // namespace oct
