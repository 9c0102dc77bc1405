// Connected components of a class map on the device, and the filter that removes small or non-largest components.  The
// definitions are in include/oct_unet.h (oct_components, oct_component_filter) and restated in numpy by common/utils.py::
// components_reference / component_filter_reference; integers only, so the two agree bit for bit.
//
// Labelling is a union-find over "parent" words that hold a pixel index y*W + x of the SAME image and never exceed the
// index of the word itself.  The parent array is root_out.  Three launches label, a fourth forms the statistics:
//   cc_tile_k     one block per 64x64 tile: parents, labels and counts of the tile live in LDS (local index ly*64 + lx, whose
//                 order inside a tile is the order of y*W + x).  A wave holds one tile row per trip, so a pixel's first parent
//                 is the start of its horizontal run, read off a ballot; then one union per pair of touching runs of
//                 adjacent rows (at their leftmost common column; connectivity 8: also the diagonal pairs that no straight
//                 pair links); then every pixel finds its local root, counts itself there (lanes that share a root add
//                 once) and stores the root as an image index.  The size words get the count at a local root and 0
//                 elsewhere.
//   cc_border_k   one thread per pixel of a tile's first row or first column (not the image's): unions across the tile
//                 border, in global memory.  EVERY access to the parent array in this launch is a relaxed agent-scope atomic
//                 (a plain load may miss what a workgroup on another XCD stored earlier in the same launch).
//   cc_flatten_k  one thread per pixel: the final root replaces the parent; a local root that is not final adds its count
//                 to the final root's and clears its own.  No union runs in this launch, so a final root stays one: nobody
//                 adds to a word that its owner clears.
//   cc_stats_k    (stats wanted) blocks stride over an image, 8 pixels per thread: the roots count themselves and raise the
//                 maximum of their class, in LDS first, then one integer atomic per class and block.
// The filter: cc_best_k and cc_filter_k stride over an image in the same way, cc_column_fill_k is a thread per column.
// Termination.  cc_find follows parent words only while they are SMALLER than the index they were read at, so it ends after
// at most H*W steps whatever other threads store meanwhile.  cc_union repeats { a = find(a), b = find(b), a > b,
// old = atomicMin(parent[a], b) } and either ends (a == b, or old == a: a was a root and now hangs under b) or goes on with
// (old, b), old < a: a + b strictly decreases.  No thread waits for a value that another thread has yet to store.
// Determinism.  A union links the larger of two roots under the smaller, so a tree's root is its smallest index; when all
// unions of a component are done the root of every pixel is the component's smallest index, whatever the order.  Counts,
// statistics and the best-root keys are integer adds and maxima: order-independent.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace oct {

constexpr int kCcTile = 64;               // tile edge: 4096 pixels, 36 KB of LDS
constexpr int kCcThreads = 256;
constexpr int kCcMaxClasses = 32;         // classes with statistics / rules
constexpr int kCcMaxBatch = 65535;        // the image is a grid dimension
constexpr int kCcColThreads = 64;         // column fill: one wave per block, as the ordered decode
static_assert(kCcTile == 64 && kCcThreads % 64 == 0, "cc_tile_k: a wave holds one tile row");

struct CcArgs {
    const unsigned char* labels;   // (B, H, W)
    unsigned* root;                // (B, H, W): the parent array, final roots in the end
    unsigned* size;                // (B, H, W): size_out or the workspace
    unsigned* stats;               // (B, n_cls, 2) or nullptr
    int B, H, W, n_cls, conn8;
    int ntx;                       // tiles per image row: cc_tile_k's blockIdx.x is ty * ntx + tx (grid.y could not hold every ty)
};

struct CcFilterArgs {
    const unsigned char* labels;
    const unsigned* root;
    const unsigned* size;
    unsigned long long* best;      // workspace (B, 32): (size << 32) | (0xFFFFFFFF - root) of the best root, 0 = class absent
    unsigned char* flags;          // workspace (B, H, W): 1 = removed (fill mode 1)
    unsigned char* out;            // (B, H, W)
    unsigned* removed;             // (B, n_cls) or nullptr
    int B, H, W, n_cls, fill_mode, fill_label;
    unsigned keep_largest;
    unsigned min_pixels[kCcMaxClasses];
};

template <int SCOPE>
__device__ __forceinline__ unsigned cc_find(const unsigned* par, unsigned i) {
    for (;;) {
        const unsigned p = __hip_atomic_load(par + i, __ATOMIC_RELAXED, SCOPE);
        if (p >= i) return i;      // a root (p == i); `>=` keeps the walk strictly decreasing on any word
        i = p;
    }
}

template <int SCOPE>
__device__ __forceinline__ void cc_union(unsigned* par, unsigned a, unsigned b) {
    for (;;) {
        a = cc_find<SCOPE>(par, a);
        b = cc_find<SCOPE>(par, b);
        if (a == b) return;
        if (a < b) { const unsigned t = a; a = b; b = t; }
        const unsigned old = __hip_atomic_fetch_min(par + a, b, __ATOMIC_RELAXED, SCOPE);
        if (old == a) return;      // a was a root and now hangs under b
        a = old;                   // old < a: somebody linked a meanwhile; its tree still has to meet b's
    }
}

static __global__ void __launch_bounds__(kCcThreads) cc_tile_k(const CcArgs A) {
    constexpr int T = kCcTile, N = T * T;
    constexpr int WG = __HIP_MEMORY_SCOPE_WORKGROUP;
    __shared__ unsigned par[N];
    __shared__ unsigned cnt[N];
    __shared__ unsigned char lab[N];
    const int x0 = (int)(blockIdx.x % (unsigned)A.ntx) * T, y0 = (int)(blockIdx.x / (unsigned)A.ntx) * T;
    const int tw = A.W - x0 < T ? A.W - x0 : T, th = A.H - y0 < T ? A.H - y0 : T;
    const size_t img = (size_t)blockIdx.z * A.H * A.W;
    const unsigned char* __restrict__ src = A.labels + img;
    for (int l = threadIdx.x; l < N; l += kCcThreads) {
        const int ly = l / T, lx = l % T;
        lab[l] = (lx < tw && ly < th) ? src[(size_t)(y0 + ly) * A.W + x0 + lx] : (unsigned char)0;
        cnt[l] = 0u;
    }
    __syncthreads();
    // horizontal runs, without a union: a wave holds one tile row per trip (lane == lx), so the start of a pixel's run is the
    // highest set bit at or below its lane in the ballot of the run starts
    for (int l = threadIdx.x; l < N; l += kCcThreads) {
        const int ly = l / T, lx = l % T;
        const bool in = lx < tw && ly < th;
        const bool start = in && (lx == 0 || lab[l - 1] != lab[l]);
        const unsigned long long low = __ballot(start) & (~0ull >> (63 - lx));
        par[l] = in ? (unsigned)(ly * T + 63 - __clzll((long long)low)) : (unsigned)l;
    }
    __syncthreads();
    // vertical links, ONE union per pair of runs that touch: at the leftmost column where they overlap (connectivity 8: a
    // diagonal pair only where neither the pixel beside it nor the one above links the two runs anyway)
    for (int l = threadIdx.x; l < N; l += kCcThreads) {
        const int ly = l / T, lx = l % T;
        if (lx >= tw || ly >= th || ly == 0) continue;
        const unsigned char c = lab[l];
        if (lab[l - T] == c) {
            if (lx == 0 || lab[l - 1] != c || lab[l - T - 1] != c) cc_union<WG>(par, (unsigned)l, (unsigned)(l - T));
        } else if (A.conn8) {
            if (lx > 0 && lab[l - T - 1] == c && lab[l - 1] != c) cc_union<WG>(par, (unsigned)l, (unsigned)(l - T - 1));
            if (lx + 1 < tw && lab[l - T + 1] == c && lab[l + 1] != c) cc_union<WG>(par, (unsigned)l, (unsigned)(l - T + 1));
        }
    }
    __syncthreads();
    unsigned* __restrict__ root = A.root + img;
    for (int l = threadIdx.x; l < N; l += kCcThreads) {
        const int ly = l / T, lx = l % T;
        const bool in = lx < tw && ly < th;
        const unsigned r = in ? cc_find<WG>(par, (unsigned)l) : 0xFFFFFFFFu;
        // counts: the lanes of a row that share a root add once, for the first four roots of the row; the rest one by one
        unsigned long long todo = __ballot(in);
        for (int k = 0; k < 4 && todo; ++k) {
            const int lead = __ffsll((long long)todo) - 1;
            const unsigned rl = (unsigned)__shfl((int)r, lead);
            const unsigned long long same = __ballot(in && r == rl);
            if (lx == lead) atomicAdd(&cnt[rl], (unsigned)__popcll(same));
            todo &= ~same;
        }
        if (!in) continue;
        if ((todo >> lx) & 1ull) atomicAdd(&cnt[r], 1u);
        root[(size_t)(y0 + ly) * A.W + x0 + lx] = (unsigned)(y0 + (int)(r / T)) * (unsigned)A.W + (unsigned)(x0 + (int)(r % T));
    }
    __syncthreads();
    unsigned* __restrict__ size = A.size + img;
    for (int l = threadIdx.x; l < N; l += kCcThreads) {
        const int ly = l / T, lx = l % T;
        if (lx < tw && ly < th) size[(size_t)(y0 + ly) * A.W + x0 + lx] = cnt[l];
    }
}

// threads of an image: (nty - 1) * W pixels of the tiles' first rows, then (ntx - 1) * H pixels of their first columns
static __global__ void __launch_bounds__(kCcThreads) cc_border_k(const CcArgs A, int n_row, int n_all) {
    constexpr int T = kCcTile;
    constexpr int AG = __HIP_MEMORY_SCOPE_AGENT;
    int t = blockIdx.x * kCcThreads + threadIdx.x;
    if (t >= n_all) return;
    const int H = A.H, W = A.W;
    const size_t img = (size_t)blockIdx.z * H * W;
    const unsigned char* __restrict__ lab = A.labels + img;
    unsigned* par = A.root + img;
    if (t < n_row) {
        const int y = (t / W + 1) * T, x = t % W;
        const unsigned i = (unsigned)y * W + x;
        const unsigned char c = lab[i];
        if (lab[i - W] == c) {
            cc_union<AG>(par, i, i - W);
        } else if (A.conn8) {
            if (x > 0 && lab[i - W - 1] == c) cc_union<AG>(par, i, i - W - 1);
            if (x + 1 < W && lab[i - W + 1] == c) cc_union<AG>(par, i, i - W + 1);
        }
        // (N equal: NW and NE, where equal, hang on N by the western links of N's own row -- inside N's tile, or across a
        // column border that the other half of this launch unions)
    } else {
        t -= n_row;
        const int x = (t / H + 1) * T, y = t % H;
        const unsigned i = (unsigned)y * W + x;
        const unsigned char c = lab[i];
        if (lab[i - 1] == c) cc_union<AG>(par, i, i - 1);
        if (A.conn8) {
            if (y > 0 && lab[i - W - 1] == c) cc_union<AG>(par, i, i - W - 1);
            if (y + 1 < H && lab[i + W - 1] == c) cc_union<AG>(par, i, i + W - 1);
        }
    }
}

static __global__ void __launch_bounds__(kCcThreads) cc_flatten_k(const CcArgs A, unsigned hw, size_t npx) {
    constexpr int AG = __HIP_MEMORY_SCOPE_AGENT;
    const size_t g = (size_t)blockIdx.x * kCcThreads + threadIdx.x;
    if (g >= npx) return;
    const size_t img = g / hw * hw;
    const unsigned i = (unsigned)(g - img);
    unsigned* par = A.root + img;
    const unsigned r = cc_find<AG>(par, i);
    if (r == i) return;
    // (others may read this word on their way up: old parent or final root, either leads to the same root)
    __hip_atomic_store(par + i, r, __ATOMIC_RELAXED, AG);
    unsigned* size = A.size + img;
    const unsigned s = size[i];
    if (s) {
        atomicAdd(size + r, s);
        size[i] = 0u;
    }
}

// grid (blocks of an image, 1, B); a thread takes the pixels threadIdx + k * (threads of the image's blocks)
static __global__ void __launch_bounds__(kCcThreads) cc_stats_k(const CcArgs A) {
    __shared__ unsigned cnt[kCcMaxClasses], mx[kCcMaxClasses];
    if (threadIdx.x < kCcMaxClasses) { cnt[threadIdx.x] = 0u; mx[threadIdx.x] = 0u; }
    __syncthreads();
    const unsigned hw = (unsigned)A.H * A.W;
    const size_t img = (size_t)blockIdx.z * hw;
    const unsigned stride = gridDim.x * kCcThreads;
    for (unsigned i = blockIdx.x * kCcThreads + threadIdx.x; i < hw; i += stride) {
        const unsigned s = A.size[img + i];
        if (!s) continue;
        const unsigned c = A.labels[img + i];
        if (c < (unsigned)A.n_cls) { atomicAdd(&cnt[c], 1u); atomicMax(&mx[c], s); }
    }
    __syncthreads();
    if (threadIdx.x < (unsigned)A.n_cls && cnt[threadIdx.x]) {
        unsigned* st = A.stats + ((size_t)blockIdx.z * A.n_cls + threadIdx.x) * 2;
        atomicAdd(st, cnt[threadIdx.x]);
        atomicMax(st + 1, mx[threadIdx.x]);
    }
}

// ---- the filter ----
// best root of (image, class): the largest component, among equals the smallest root -- the maximum of
// (size << 32) | (0xFFFFFFFF - root) over the roots of the class.  Grid as cc_stats_k.
static __global__ void __launch_bounds__(kCcThreads) cc_best_k(const CcFilterArgs A) {
    __shared__ unsigned long long best[kCcMaxClasses];
    if (threadIdx.x < kCcMaxClasses) best[threadIdx.x] = 0ull;
    __syncthreads();
    const unsigned hw = (unsigned)A.H * A.W;
    const size_t img = (size_t)blockIdx.z * hw;
    const unsigned stride = gridDim.x * kCcThreads;
    for (unsigned i = blockIdx.x * kCcThreads + threadIdx.x; i < hw; i += stride) {
        const unsigned s = A.size[img + i];
        if (!s) continue;
        const unsigned c = A.labels[img + i];
        if (c < (unsigned)A.n_cls && ((A.keep_largest >> c) & 1u))
            atomicMax(&best[c], ((unsigned long long)s << 32) | (unsigned long long)(0xFFFFFFFFu - i));
    }
    __syncthreads();
    if (threadIdx.x < (unsigned)A.n_cls && best[threadIdx.x])
        atomicMax(A.best + (size_t)blockIdx.z * kCcMaxClasses + threadIdx.x, best[threadIdx.x]);
}

// per pixel (grid as cc_stats_k): removed or kept; a removed pixel gets fill_label (fill mode 1: for now, and its flag is set)
static __global__ void __launch_bounds__(kCcThreads) cc_filter_k(const CcFilterArgs A) {
    __shared__ unsigned rem[kCcMaxClasses];
    if (threadIdx.x < kCcMaxClasses) rem[threadIdx.x] = 0u;
    __syncthreads();
    const unsigned hw = (unsigned)A.H * A.W;
    const size_t img = (size_t)blockIdx.z * hw;
    const unsigned stride = gridDim.x * kCcThreads;
    for (unsigned i = blockIdx.x * kCcThreads + threadIdx.x; i < hw; i += stride) {
        const unsigned c = A.labels[img + i];
        bool gone = false;
        if (c < (unsigned)A.n_cls) {
            const unsigned r = A.root[img + i] < hw ? A.root[img + i] : i;      // (a root word that oct_components did not write)
            gone = A.size[img + r] < A.min_pixels[c];
            if ((A.keep_largest >> c) & 1u) {
                const unsigned long long k = A.best[(size_t)blockIdx.z * kCcMaxClasses + c];
                gone = gone || r != 0xFFFFFFFFu - (unsigned)(k & 0xFFFFFFFFull);
            }
            if (gone) atomicAdd(&rem[c], 1u);
        }
        A.out[img + i] = gone ? (unsigned char)A.fill_label : (unsigned char)c;
        if (A.fill_mode == 1) A.flags[img + i] = gone ? 1 : 0;
    }
    if (!A.removed) return;
    __syncthreads();
    if (threadIdx.x < (unsigned)A.n_cls && rem[threadIdx.x])
        atomicAdd(A.removed + (size_t)blockIdx.z * A.n_cls + threadIdx.x, rem[threadIdx.x]);
}

// fill mode 1, one thread per column, top to bottom: a removed pixel takes the label of the last SOURCE above it (a kept pixel
// with a label < n_cls).  Above the column's first source every pixel with a label < n_cls is removed (else it would be the
// first source): a second walk over those rows gives them the first source's label.  A column without a source keeps
// fill_label.  A thread rewrites only bytes of its own column.
static __global__ void __launch_bounds__(kCcColThreads) cc_column_fill_k(const CcFilterArgs A) {
    constexpr int D = 8;
    const size_t t = (size_t)blockIdx.x * kCcColThreads + threadIdx.x;
    if (t >= (size_t)A.B * A.W) return;
    const int b = (int)(t / A.W), x = (int)(t % A.W);
    const int H = A.H, W = A.W;
    const size_t col = (size_t)b * H * W + x;
    const unsigned char* __restrict__ lab = A.labels + col;
    const unsigned char* __restrict__ flg = A.flags + col;
    unsigned char* out = A.out + col;
    int above = -1, first = -1;
    for (int y0 = 0; y0 < H; y0 += D) {
        unsigned char l[D], f[D];
#pragma unroll
        for (int d = 0; d < D; ++d) {
            const bool in = y0 + d < H;
            l[d] = in ? lab[(size_t)(y0 + d) * W] : (unsigned char)0;
            f[d] = in ? flg[(size_t)(y0 + d) * W] : (unsigned char)0;
        }
#pragma unroll
        for (int d = 0; d < D; ++d) {
            if (y0 + d >= H) break;
            if (f[d]) {
                if (above >= 0) out[(size_t)(y0 + d) * W] = (unsigned char)above;
            } else if (l[d] < A.n_cls) {
                if (above < 0) first = y0 + d;
                above = l[d];
            }
        }
    }
    if (first <= 0) return;
    const unsigned char below = lab[(size_t)first * W];
    for (int y = 0; y < first; ++y)
        if (lab[(size_t)y * W] < A.n_cls) out[(size_t)y * W] = below;
}

}  // namespace oct
