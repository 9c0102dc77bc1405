// Min-path boundary search on the device: the column recurrence of the grid graph of min_path_processing/graph_search.py
// (include/oct_unet.h, oct_minpath_device, states the arithmetic; min_path_processing/device_search.py restates it in numpy).
//
// One workgroup per boundary map, rows across threads (a thread loops over rows r, r + blockDim, ...).  The W column steps
// are sequential and separated by ONE barrier each: the distance column D and the probability column P live in LDS twice
// (read column j, write column j+1, swap).  The uint8 map is staged in tiles of kMpTile image columns with row-contiguous
// (coalesced) global loads -- a per-column read would be a stride-W byte gather -- into LDS rows of kMpTileStride bytes
// (17 dwords: the per-column byte reads of 64 consecutive rows fall on 64 different banks).  Every vertex stores one byte,
// predecessor offset + 16 in bits 0..5 and its tie bit in bit 6; the bytes stay in LDS when W*H of them fit beside the
// rest (256x512: 128 KiB of the CU's 160), else they go to the workspace.  The back-trace is a chain of W dependent
// reads by one thread; the end of the path is one block reduction.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace oct {

constexpr int kMpTile = 64;                 // image columns staged per tile
constexpr int kMpTileStride = kMpTile + 4;  // bytes per LDS tile row
constexpr int kMpMaxThreads = 256;
constexpr int kMpMaxGrad = 16;
constexpr size_t kMpLdsLimit = 160 * 1024;  // LDS of one gfx950 CU, all of it available to one workgroup

struct MinpathTable { double p[256]; };     // p[k] = k / 255 in fp64, divided on the host

struct MinpathArgs {
    const unsigned char* maps;   // (n_maps, H, W)
    unsigned char* choice;       // (n_maps, W, H) predecessor bytes, used when they do not fit LDS
    unsigned short* rows;        // (n_maps, W)
    double* cost;                // (n_maps)
    unsigned char* tied;         // (n_maps)
    int H, W, G;
    int vec4;                    // rows of the map are 4-byte aligned: stage with dword loads
};

// LDS bytes of one workgroup without / with the predecessor bytes
inline size_t minpath_lds_base(int H) {
    const size_t tile = ((size_t)H * kMpTileStride + 15) / 16 * 16;
    return 256 * sizeof(double) + 4 * (size_t)H * sizeof(double) + kMpMaxThreads * (sizeof(double) + 2 * sizeof(int)) + tile;
}
inline size_t minpath_lds_choice(int H, int W) { return ((size_t)H * W + 15) / 16 * 16; }

template <bool LDS_CHOICE>
__global__ __launch_bounds__(kMpMaxThreads) void minpath_k(const MinpathArgs A, const MinpathTable T) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) unsigned char mp_smem[];
    const int H = A.H, W = A.W, G = A.G, tid = threadIdx.x, nt = blockDim.x;
    double* tab = (double*)mp_smem;                  // 256
    double* Dbuf = tab + 256;                        // 2 x H
    double* Pbuf = Dbuf + 2 * (size_t)H;             // 2 x H
    double* red_v = Pbuf + 2 * (size_t)H;            // kMpMaxThreads
    int* red_i = (int*)(red_v + kMpMaxThreads);      // kMpMaxThreads
    int* red_t = red_i + kMpMaxThreads;              // kMpMaxThreads
    unsigned char* tile = (unsigned char*)(red_t + kMpMaxThreads);
    const size_t map = blockIdx.x;
    const unsigned char* src = A.maps + map * (size_t)H * W;
    unsigned char* choice = LDS_CHOICE ? tile + ((size_t)H * kMpTileStride + 15) / 16 * 16 : A.choice + map * (size_t)H * W;

    for (int i = tid; i < 256; i += nt) tab[i] = T.p[i];
    for (int r = tid; r < H; r += nt) { Dbuf[r] = 0.0; Pbuf[r] = 1.0; }      // graph column 0: distance 0, probability 1

    int cur = 0;
    for (int j = 0; j < W; ++j) {            // image column j = graph column j + 1
        const int c = j % kMpTile;
        if (c == 0) {
            // (every thread has passed the barrier behind column j - 1: nobody reads the old tile any more)
            if (A.vec4) {
                for (int i = tid; i < H * (kMpTile / 4); i += nt) {
                    const int r = i / (kMpTile / 4), q = i % (kMpTile / 4), col = j + 4 * q;
                    if (col < W) *(uint32_t*)(tile + (size_t)r * kMpTileStride + 4 * q) = *(const uint32_t*)(src + (size_t)r * W + col);
                }
            } else {
                for (int i = tid; i < H * kMpTile; i += nt) {
                    const int r = i / kMpTile, q = i % kMpTile, col = j + q;
                    if (col < W) tile[(size_t)r * kMpTileStride + q] = src[(size_t)r * W + col];
                }
            }
            __syncthreads();                 // (also orders the initial columns and the table before the first step)
        }
        const double* Dc = Dbuf + (size_t)cur * H;
        const double* Pc = Pbuf + (size_t)cur * H;
        double* Dn = Dbuf + (size_t)(cur ^ 1) * H;
        double* Pn = Pbuf + (size_t)(cur ^ 1) * H;
        for (int r = tid; r < H; r += nt) {
            const double pn = tab[tile[(size_t)r * kMpTileStride + c]];
            double best = Dc[r] + (2.0 - (Pc[r] + pn));          // right
            int off = 0, tie = 0;
            for (int g = 1; g <= G; ++g) {                       // from below, nearest first
                const int rr = r + g;
                if (rr >= H) break;
                const double v = Dc[rr] + (2.0 - (Pc[rr] + pn));
                if (v < best) { best = v; off = g; tie = 0; } else if (v == best) tie = 1;
            }
            for (int g = 1; g <= G; ++g) {                       // from above, nearest first
                const int rr = r - g;
                if (rr < 0) break;
                const double v = Dc[rr] + (2.0 - (Pc[rr] + pn));
                if (v < best) { best = v; off = -g; tie = 0; } else if (v == best) tie = 1;
            }
            Dn[r] = best;
            Pn[r] = pn;
            // ties among the predecessors in the appended column 0 (all distance 0, probability 1) change no delineation
            choice[(size_t)j * H + r] = (unsigned char)((off + 16) | ((tie && j >= 1) ? 64 : 0));
        }
        cur ^= 1;
        __syncthreads();
    }

    // end of the path: the zero-cost appended last column collapses to one reduction over the rows of image column W - 1
    {
        const double* Dc = Dbuf + (size_t)cur * H;
        const double* Pc = Pbuf + (size_t)cur * H;
        double best = __builtin_huge_val();
        int idx = 0x7fffffff, tie = 0;
        for (int r = tid; r < H; r += nt) {                      // ascending rows: the first minimum is the smallest row
            const double v = Dc[r] + (2.0 - (Pc[r] + 1.0));
            if (v < best) { best = v; idx = r; tie = 0; } else if (v == best) tie = 1;
        }
        red_v[tid] = best; red_i[tid] = idx; red_t[tid] = tie;
        __syncthreads();
        for (int s = nt >> 1; s > 0; s >>= 1) {                  // nt is a power of two
            if (tid < s) {
                const double a = red_v[tid], b = red_v[tid + s];
                if (b < a) { red_v[tid] = b; red_i[tid] = red_i[tid + s]; red_t[tid] = red_t[tid + s]; }
                else if (b == a) { red_i[tid] = min(red_i[tid], red_i[tid + s]); red_t[tid] = 1; }
            }
            __syncthreads();
        }
    }

    // back-trace: W dependent reads by one thread; the tie bits of the vertices ON the chosen path make the map's flag
    if (tid == 0) {
        int r = red_i[0], tied = red_t[0];
        unsigned short* rows = A.rows + map * (size_t)W;
        for (int j = W - 1; j >= 0; --j) {
            rows[j] = (unsigned short)r;
            const int e = choice[(size_t)j * H + r];
            tied |= e >> 6;
            r += (e & 63) - 16;
        }
        A.cost[map] = red_v[0];
        A.tied[map] = (unsigned char)(tied & 1);
    }
}

}  // namespace oct
