// Evaluation Dice on the device: the per-image confusion matrix of two (B,H,W) uint8 class maps, and the class map that
// a set of graph-search delineations encloses (common/utils.py::labels_from_delineations, built on create_area_mask;
// reference dataset_construction.py:654-708, evaluation.py:317-333, prediction.py:143-156).  Every Dice metric of the
// evaluation is a function of the confusion matrix (evaluation/dice_device.py::dice_from_counts); both kernels produce
// integers, so their results do not depend on the order of accumulation.
//
//   confusion_k     grid (chunks, B), 256 threads.  key = gt * n_cls + pred, or n_cls^2 where either label is >= n_cls.
//                   A thread loads 16 bytes of each map per step and counts RUNS of equal keys in registers, across its
//                   steps: class maps are spatially coherent, so a thread issues one LDS atomic per run, not per pixel
//                   (a constant map: one per thread and launch).  The block's LDS row is added to the image's row of
//                   `counts` with integer global atomics, non-zero words only; the caller zeroes `counts` before.
//                   The 16-byte loads start at the first 16-byte boundary of the image's pred map; the pixels before it
//                   and after the last whole vector are read as bytes.  Where the two maps of an image sit at different
//                   offsets from a 16-byte boundary, the whole image is read as bytes.
//   confusion_masked_k  the same body with one more compare on the ground-truth byte: gt == ignore_label goes to a word
//                   of its own, n_cls^2 + 1 (rows of n_cls^2 + 2 words), and to no other.
//   area_labels_k   grid (ceil(W / 256), ceil(H / 32), B), 256 threads: a tile of 256 columns x 32 rows.  The block
//                   stages the tile's boundaries into LDS after the zero replacement (going up in i, s_i == 0 becomes the
//                   first non-zero s_j, j > i, or H); a thread then labels 4 adjacent columns of 8 rows,
//                       label(r) = M if r >= s_{M-1}, else the largest k in 1..M-1 with s_{k-1} <= r < s_k, else 0
//                   (what the host loop's sequential overwrites leave), walking k downwards and keeping the first hit,
//                   and stores each row's 4 labels as one uchar4 where the address allows it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace oct {

constexpr int kDiceMaxClasses = 32;
constexpr int kDiceThreads = 256;
constexpr int kAreaTileW = 256;       // columns of an area_labels_k tile: 64 lanes x uchar4
constexpr int kAreaRowsPerThread = 8;
constexpr int kAreaTileH = (kDiceThreads / 64) * kAreaRowsPerThread;

// npix = H * W < 2^32; counts rows of n_cls^2 + 1 words (kMasked: + 2), zeroed by the caller.  kMasked: a pixel with
// gt == ignore (a value in n_cls..255) goes to word n_cls^2 + 1 and nowhere else, whatever its prediction.
template <bool kMasked>
__device__ __forceinline__ void confusion_body(const unsigned char* __restrict__ pred, const unsigned char* __restrict__ gt,
                                               size_t npix, int n_cls, unsigned ignore, unsigned int* __restrict__ counts) {
    __shared__ unsigned int s_cnt[kDiceMaxClasses * kDiceMaxClasses + (kMasked ? 2 : 1)];
    const int tid = threadIdx.x;
    const unsigned bad = (unsigned)(n_cls * n_cls);
    const int nk = (int)bad + (kMasked ? 2 : 1);
    for (int k = tid; k < nk; k += kDiceThreads) s_cnt[k] = 0u;
    __syncthreads();
    const size_t b = blockIdx.y;
    const unsigned char* p = pred + b * npix;
    const unsigned char* g = gt + b * npix;
    size_t head = 0, nvec = 0;
    if ((((uintptr_t)p ^ (uintptr_t)g) & 15) == 0) {
        head = (16 - ((uintptr_t)p & 15)) & 15;
        if (head > npix) head = npix;
        nvec = (npix - head) / 16;
    }
    unsigned cur = bad, run = 0;      // the open run of this thread
    auto add = [&](unsigned pv, unsigned gv) {
        unsigned key = (pv < (unsigned)n_cls && gv < (unsigned)n_cls) ? gv * (unsigned)n_cls + pv : bad;
        if (kMasked && gv == ignore) key = bad + 1u;
        if (key == cur) {
            ++run;
        } else {
            if (run) atomicAdd(&s_cnt[cur], run);
            cur = key;
            run = 1;
        }
    };
    const size_t t = (size_t)blockIdx.x * kDiceThreads + tid, stride = (size_t)gridDim.x * kDiceThreads;
    const uint4* p4 = reinterpret_cast<const uint4*>(p + head);
    const uint4* g4 = reinterpret_cast<const uint4*>(g + head);
    for (size_t v = t; v < nvec; v += stride) {
        const uint4 a = p4[v], c = g4[v];
        const unsigned pw[4] = {a.x, a.y, a.z, a.w}, gw[4] = {c.x, c.y, c.z, c.w};
#pragma unroll
        for (int w = 0; w < 4; ++w) {
#pragma unroll
            for (int e = 0; e < 4; ++e) add((pw[w] >> (8 * e)) & 255u, (gw[w] >> (8 * e)) & 255u);
        }
    }
    // the pixels outside the whole vectors: [0, head) and [head + 16 nvec, npix)
    const size_t nscalar = npix - 16 * nvec;
    for (size_t s = t; s < nscalar; s += stride) {
        const size_t i = s < head ? s : s + 16 * nvec;
        add(p[i], g[i]);
    }
    if (run) atomicAdd(&s_cnt[cur], run);
    __syncthreads();
    unsigned int* row = counts + b * (size_t)nk;
    for (int k = tid; k < nk; k += kDiceThreads) {
        const unsigned int v = s_cnt[k];
        if (v) atomicAdd(&row[k], v);
    }
}

__global__ void __launch_bounds__(kDiceThreads) confusion_k(const unsigned char* __restrict__ pred,
                                                            const unsigned char* __restrict__ gt, size_t npix, int n_cls,
                                                            unsigned int* __restrict__ counts) {
    confusion_body<false>(pred, gt, npix, n_cls, 0u, counts);
}

__global__ void __launch_bounds__(kDiceThreads) confusion_masked_k(const unsigned char* __restrict__ pred,
                                                                   const unsigned char* __restrict__ gt, size_t npix,
                                                                   int n_cls, unsigned ignore,
                                                                   unsigned int* __restrict__ counts) {
    confusion_body<true>(pred, gt, npix, n_cls, ignore, counts);
}

// segs (B, M, W) uint16, labels (B, H, W) uint8; M = n_cls - 1 in 1..31, H <= 65535
__global__ void __launch_bounds__(kDiceThreads) area_labels_k(const unsigned short* __restrict__ segs, int H, int W, int M,
                                                              unsigned char* __restrict__ labels) {
    __shared__ __attribute__((aligned(8))) unsigned short s_seg[(kDiceMaxClasses - 1) * kAreaTileW];
    const int tid = threadIdx.x;
    const int col0 = blockIdx.x * kAreaTileW;
    const size_t b = blockIdx.z;
    {   // one thread per column of the tile: zero replacement, from the last boundary down
        const int col = col0 + tid;
        const unsigned short* sp = segs + b * (size_t)M * W + col;
        unsigned short next = (unsigned short)H;
        for (int i = M - 1; i >= 0; --i) {
            unsigned short v = col < W ? sp[(size_t)i * W] : (unsigned short)0;
            if (v == 0) v = next;
            next = v;
            s_seg[i * kAreaTileW + tid] = v;
        }
    }
    __syncthreads();
    const int lane = tid & 63, wy = tid >> 6;
    const int c0 = col0 + 4 * lane;
    if (c0 >= W) return;
    const int r0 = blockIdx.y * kAreaTileH + wy;           // this thread's rows: r0 + 4 j
    unsigned char lab[kAreaRowsPerThread][4];
    const ushort4* sv = reinterpret_cast<const ushort4*>(s_seg) + lane;
    ushort4 hi4 = sv[(M - 1) * (kAreaTileW / 4)];
    int hi[4] = {hi4.x, hi4.y, hi4.z, hi4.w};
#pragma unroll
    for (int j = 0; j < kAreaRowsPerThread; ++j) {
        const int r = r0 + 4 * j;
#pragma unroll
        for (int c = 0; c < 4; ++c) lab[j][c] = r >= hi[c] ? (unsigned char)M : (unsigned char)0;
    }
    for (int k = M - 1; k >= 1; --k) {
        const ushort4 lo4 = sv[(k - 1) * (kAreaTileW / 4)];
        const int lo[4] = {lo4.x, lo4.y, lo4.z, lo4.w};
#pragma unroll
        for (int j = 0; j < kAreaRowsPerThread; ++j) {
            const int r = r0 + 4 * j;
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if (lab[j][c] == 0 && lo[c] <= r && r < hi[c]) lab[j][c] = (unsigned char)k;
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) hi[c] = lo[c];
    }
    unsigned char* out = labels + b * (size_t)H * W;
#pragma unroll
    for (int j = 0; j < kAreaRowsPerThread; ++j) {
        const int r = r0 + 4 * j;
        if (r >= H) break;
        unsigned char* q = out + (size_t)r * W + c0;
        if (c0 + 3 < W && ((uintptr_t)q & 3) == 0) {
            *reinterpret_cast<uchar4*>(q) = make_uchar4(lab[j][0], lab[j][1], lab[j][2], lab[j][3]);
        } else {
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if (c0 + c < W) q[c] = lab[j][c];
        }
    }
}

}  // namespace oct
