// Contrast normalisation on the device: (B,H,W,ch) uint8 -> the same shape, by contrast-limited adaptive histogram
// equalisation ("clahe") or a per-tile percentile stretch ("stretch"), bilinearly blended between the tiles' look-up tables.
// The definition is include/oct_unet.h, oct_contrast_batch; common/utils.py contrast_luts_reference / contrast_reference
// restate it in numpy.  Integers only, so device and numpy agree byte for byte.
//
// Three launches behind one memset of the histograms:
//   contrast_hist_k   grid (tiles * split, ch, B).  `split` blocks share a tile (each takes a band of its rows), so that a
//                     (1,1) grid still fills the chip.  A wave keeps its own 256-bin uint32 histogram in LDS; a lane keeps
//                     the count of the byte value it last saw in a register and adds it to LDS when the value changes, so
//                     a dark tile costs a lane one LDS atomic, not one per pixel.  The four wave histograms are summed by
//                     bin and the non-zero sums added to the tile's histogram in the workspace with integer atomics:
//                     order-free, so the counts -- and every byte behind them -- do not depend on the schedule.
//   contrast_lut_k    grid (tiles, ch, B), thread i owns bin i: clip and redistribution (clahe) or the two percentile
//                     positions (stretch) by one block sum, one inclusive scan over the 256 bins (wave shuffles, then the
//                     four waves in order) and a coalesced 256-byte store.
//   contrast_apply_k  a thread owns V = 4 adjacent bytes of a row (one 4-byte load and store) where every row starts on a
//                     4-byte boundary, else V = 1.  The tile-centre tables of both axes are built in LDS per block; the row
//                     cell is found once per thread, the column cell once and then advanced (centres lie >= 8 pixels
//                     apart, so a step of one pixel crosses at most one).  Four byte gathers from the image's LUTs (L1 / L2:
//                     ty * tx * 256 bytes per channel) and one exact 32-bit division per byte.
// One thread owns each output byte and reads it before it writes, so the output may be the input.
#pragma once
#include <hip/hip_runtime.h>

namespace oct {

enum { CT_MAX_TILES = 16, CT_MIN_TILE = 8, CT_MAX_DIM = 4096, CT_MAX_SPLIT = 32, CT_THREADS = 256, CT_BINS = 256 };
enum { CT_CLAHE = 0, CT_STRETCH = 1 };

struct ContrastGeom {
    int H, W, ch, ty, tx;
    int method;
    unsigned clip_q8;
    int lo_bp, hi_bp;
    int split;          // blocks per tile of contrast_hist_k
};

// first row (column) of tile i of t over n pixels; i * n <= 16 * 4096
__device__ __forceinline__ int ct_edge(int i, int n, int t) { return (i * n) / t; }

__device__ __forceinline__ unsigned ct_div_ch(unsigned u, int ch) {
    return ch == 1 ? u : ch == 2 ? u >> 1 : ch == 4 ? u >> 2 : u / 3u;
}

// sum of v over the block's 256 threads, the four wave sums added in wave order; s: 4 words of LDS no one else uses
__device__ __forceinline__ unsigned ct_block_sum(unsigned v, unsigned* s) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = v;
    __syncthreads();
    return s[0] + s[1] + s[2] + s[3];
}

// inclusive prefix sum of v over the block's 256 threads in thread order; s as above
__device__ __forceinline__ unsigned ct_block_scan(unsigned v, unsigned* s) {
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned u = __shfl_up(v, o, 64);
        if (lane >= o) v += u;
    }
    if (lane == 63) s[wave] = v;
    __syncthreads();
    unsigned base = 0;
    for (int w = 0; w < 3; ++w) base += w < wave ? s[w] : 0u;
    return v + base;
}

__global__ __launch_bounds__(CT_THREADS) void contrast_hist_k(const unsigned char* __restrict__ x, const ContrastGeom g,
                                                              unsigned* __restrict__ hist) {
    __shared__ unsigned s_h[4][CT_BINS];
    const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
    for (int i = tid; i < 4 * CT_BINS; i += CT_THREADS) (&s_h[0][0])[i] = 0u;
    __syncthreads();
    const int tile = (int)blockIdx.x / g.split, sp = (int)blockIdx.x - tile * g.split;
    const int tr = tile / g.tx, tc = tile - tr * g.tx, c = (int)blockIdx.y, b = (int)blockIdx.z;
    const int y0 = ct_edge(tr, g.H, g.ty), y1 = ct_edge(tr + 1, g.H, g.ty);
    const int x0 = ct_edge(tc, g.W, g.tx), x1 = ct_edge(tc + 1, g.W, g.tx);
    const int th = y1 - y0, tw = x1 - x0;
    const int ys = y0 + sp * th / g.split, ye = y0 + (sp + 1) * th / g.split;      // this block's band of the tile's rows
    // a wave covers 64 / lpr rows of lpr lanes each, lpr the least power of two >= the tile's width, at most 64
    int lg = 3;
    while ((1 << lg) < tw && lg < 6) ++lg;
    const int lpr = 1 << lg, lr = lane >> lg, lc = lane & (lpr - 1), rpw = 64 >> lg;
    int cur = 0;
    unsigned cnt = 0;
    for (int y = ys + wave * rpw + lr; y < ye; y += 4 * rpw) {
        const unsigned char* row = x + (((size_t)b * g.H + y) * g.W) * g.ch + c;
        for (int xx = x0 + lc; xx < x1; xx += lpr) {
            const int v = row[(size_t)xx * g.ch];
            if (v != cur) {
                if (cnt) atomicAdd(&s_h[wave][cur], cnt);
                cur = v; cnt = 0;
            }
            ++cnt;
        }
    }
    if (cnt) atomicAdd(&s_h[wave][cur], cnt);
    __syncthreads();
    const unsigned s = s_h[0][tid] + s_h[1][tid] + s_h[2][tid] + s_h[3][tid];
    const size_t slot = ((size_t)b * g.ch + c) * (size_t)(g.ty * g.tx) + tile;
    if (s) atomicAdd(&hist[slot * CT_BINS + tid], s);
}

__global__ __launch_bounds__(CT_THREADS) void contrast_lut_k(const unsigned* __restrict__ hist, const ContrastGeom g,
                                                             unsigned char* __restrict__ lut) {
    __shared__ unsigned s_a[4], s_b[4];
    const int i = (int)threadIdx.x, tile = (int)blockIdx.x, c = (int)blockIdx.y, b = (int)blockIdx.z;
    const int tr = tile / g.tx, tc = tile - tr * g.tx;
    const unsigned A = (unsigned)((ct_edge(tr + 1, g.H, g.ty) - ct_edge(tr, g.H, g.ty)) *
                                  (ct_edge(tc + 1, g.W, g.tx) - ct_edge(tc, g.W, g.tx)));      // <= 2^24
    const size_t slot = ((size_t)b * g.ch + c) * (size_t)(g.ty * g.tx) + tile;
    unsigned h = hist[slot * CT_BINS + i];
    unsigned v;
    if (g.method == CT_CLAHE) {
        unsigned L = A;
        if (g.clip_q8) {
            const unsigned long long l = ((unsigned long long)g.clip_q8 * A) >> 16;
            L = l < 1 ? 1u : (unsigned)l;
        }
        const unsigned E = ct_block_sum(h > L ? h - L : 0u, s_a);
        const unsigned r = E & 255u;
        h = (h < L ? h : L) + (E >> 8) + ((((unsigned)(i + 1) * r) >> 8) > (((unsigned)i * r) >> 8) ? 1u : 0u);
        const unsigned cum = ct_block_scan(h, s_b);        // cum[255] = A; cum * 255 + A / 2 < 2^32
        v = (cum * 255u + A / 2u) / A;
    } else {
        const unsigned cum = ct_block_scan(h, s_b);
        const unsigned t_lo = (unsigned)(((unsigned long long)g.lo_bp * A) / 10000ull);
        const bool below_lo = cum <= t_lo;
        const bool below_hi = (unsigned long long)cum * 10000ull < (unsigned long long)g.hi_bp * A;
        // cum never decreases: the first bin past each threshold is the number of bins below it
        const unsigned both = ct_block_sum((below_lo ? 1u : 0u) | (below_hi ? 1u << 16 : 0u), s_a);
        const int v_lo = (int)(both & 0xffffu), v_hi = (int)(both >> 16);
        if (v_hi <= v_lo) v = (unsigned)i;
        else if (i <= v_lo) v = 0u;
        else if (i >= v_hi) v = 255u;
        else v = ((unsigned)(i - v_lo) * 255u + (unsigned)(v_hi - v_lo) / 2u) / (unsigned)(v_hi - v_lo);
    }
    lut[slot * CT_BINS + i] = (unsigned char)v;
}

// cell and weight of position p on an axis of t tiles with the doubled centres cen[0..t): the cell index, the next one,
// the weight a of the next one and the span D; cnt = the number of centres <= 2p
__device__ __forceinline__ void ct_cell(const int* cen, int t, int p, int cnt, int& r, int& r1, int& a, int& D) {
    r = 0; r1 = 0; a = 0; D = 1;
    if (t > 1) {
        r = cnt - 1;
        r = r < 0 ? 0 : r > t - 2 ? t - 2 : r;
        r1 = r + 1;
        D = cen[r1] - cen[r];
        a = 2 * p - cen[r];
        a = a < 0 ? 0 : a > D ? D : a;
    }
}

template <int V>
__global__ __launch_bounds__(CT_THREADS) void contrast_apply_k(const unsigned char* x, const unsigned char* __restrict__ lut,
                                                               const ContrastGeom g, unsigned upr, unsigned char* out) {
    __shared__ int s_cy[CT_MAX_TILES], s_cx[CT_MAX_TILES];
    const int tid = (int)threadIdx.x;
    if (tid < g.ty) s_cy[tid] = ct_edge(tid, g.H, g.ty) + ct_edge(tid + 1, g.H, g.ty) - 1;
    if (tid >= 64 && tid - 64 < g.tx) s_cx[tid - 64] = ct_edge(tid - 64, g.W, g.tx) + ct_edge(tid - 63, g.W, g.tx) - 1;
    __syncthreads();
    const unsigned idx = blockIdx.x * CT_THREADS + (unsigned)tid;       // < H * upr <= 2^26
    if (idx >= (unsigned)g.H * upr) return;
    const int y = (int)(idx / upr);
    const unsigned u0 = (idx - (unsigned)y * upr) * V;                  // first byte of this thread in its row
    const int b = (int)blockIdx.y, ch = g.ch, ty = g.ty, tx = g.tx;

    int cnt = 0;
    for (int i = 0; i < ty; ++i) cnt += s_cy[i] <= 2 * y ? 1 : 0;
    int r, r1, ay, Dy;
    ct_cell(s_cy, ty, y, cnt, r, r1, ay, Dy);

    int px = (int)ct_div_ch(u0, ch);
    int cntx = 0;
    for (int i = 0; i < tx; ++i) cntx += s_cx[i] <= 2 * px ? 1 : 0;

    const size_t off = (((size_t)b * g.H + y) * g.W) * ch + u0;
    const unsigned char* lb = lut + (size_t)b * ch * (size_t)(ty * tx) * CT_BINS;
    unsigned in;
    if (V == 4) in = *reinterpret_cast<const unsigned*>(x + off);
    else in = x[off];
    unsigned res = 0;
#pragma unroll
    for (int j = 0; j < V; ++j) {
        const unsigned u = u0 + j;
        const int p = (int)ct_div_ch(u, ch), cc = (int)(u - (unsigned)p * ch);
        if (p != px) {
            px = p;
            if (cntx < tx && s_cx[cntx] <= 2 * p) ++cntx;
        }
        int c, c1, ax, Dx;
        ct_cell(s_cx, tx, p, cntx, c, c1, ax, Dx);
        const unsigned v = (in >> (8 * j)) & 255u;
        const unsigned char* lc = lb + (size_t)cc * (size_t)(ty * tx) * CT_BINS + v;
        const unsigned v00 = lc[(r * tx + c) * CT_BINS], v01 = lc[(r * tx + c1) * CT_BINS];
        const unsigned v10 = lc[(r1 * tx + c) * CT_BINS], v11 = lc[(r1 * tx + c1) * CT_BINS];
        const unsigned D = (unsigned)(Dy * Dx);                         // <= 4096 * 4096: the numerator stays below 2^32
        const unsigned num = (unsigned)(Dy - ay) * ((unsigned)(Dx - ax) * v00 + (unsigned)ax * v01) +
                             (unsigned)ay * ((unsigned)(Dx - ax) * v10 + (unsigned)ax * v11) + D / 2u;
        res |= (num / D) << (8 * j);
    }
    if (V == 4) *reinterpret_cast<unsigned*>(out + off) = res;
    else out[off] = (unsigned char)res;
}

}  // namespace oct
