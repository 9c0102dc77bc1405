// Ordered layer decode on the device: for every column of the class probabilities the best labelling whose class index never
// decreases with depth, decoded jointly for all classes.  The definition is in include/oct_unet.h (oct_ordered_decode) and
// restated in numpy by common/utils.py::ordered_decode_reference; integers only behind the quantisation, so the two agree bit
// for bit.
//
//   ordered_decode_k<C, VEC>  probs (B,H,W,C) f32 -> labels (B,H,W) u8, rows (B,C-1,W) u16, score (B,W) u32.
//                   A column is sequential in its rows; the parallelism is the B*W columns.  A thread owns NC adjacent columns
//                   (1; VEC: 4, the 4 C consecutive floats of a row that are C float4 loads -- option "ordered_float4", under the
//                   conditions of mc_update_k: 16-byte aligned base, C <= 8, W*C % 4 == 0, so every row of every image starts
//                   on a float4.  Measured slower at every shape, DESIGN.md section 34: four times the serial work per wave, a
//                   quarter of the waves), adjacent lanes adjacent columns: the loads of a wave for one row cover one contiguous
//                   stretch.  Two sweeps in ONE launch, by the same thread:
//                   forward, r = 0..H-1: quantise, F = k + M, the running maximum over the classes; the C decision bits of
//                   (row, column) go to the workspace as one uint16 (bit c = s[r][c]; bit 0 is always set);
//                   back-trace, r = H-1..0: the class steps down to the highest set bit at or below it; the label is stored,
//                   and every step down notes the boundary rows it fixes, in registers -- the C-1 rows of a column are stored
//                   once, behind the walk.
//                   Neither sweep's addresses depend on the state, so both keep a ring of D rows of loads in flight (a
//                   register ring: the loop is unrolled D times so that every index is static).
//                   The workspace is (B, H, Wp) uint16 with Wp = W rounded up to 4, so that the four words of a VEC thread are
//                   one 8-byte store.  A thread reads back only what it wrote itself: no barrier, no atomics, and the bytes
//                   do not depend on the order in which threads run.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace oct {

constexpr int kOdThreads = 64;            // one wave per block: B*W columns are few (16 384 at B = 32, 256x512), so spread them
constexpr int kOdMinClasses = 2, kOdMaxClasses = 16;
constexpr int kOdMaxH = 4096;             // H * (2^20 - 1) < 2^32
constexpr int kOdMaxVec = 8;              // widest class count of the float4 path (kMcMaxVec)
constexpr unsigned kOdOne = 1u << 20;     // the quantisation scale

struct OdArgs {
    const float* probs;        // (B, H, W, C)
    unsigned short* bits;      // workspace (B, H, Wp)
    unsigned char* labels;     // (B, H, W)   or nullptr
    unsigned short* rows;      // (B, C-1, W) or nullptr
    unsigned int* score;       // (B, W)      or nullptr
    int B, H, W, Wp;
    int ipr;                   // threads per image row: W, or ceil(W / 4) with VEC
    int lab4;                  // VEC: the four labels of a thread are one aligned uchar4 store
};

__device__ __forceinline__ unsigned od_quant(float p) {
    const float q = p > 0.f ? (p < 1.f ? p : 1.f) : 0.f;       // NaN -> 0
    const unsigned k = (unsigned)(q * 1048576.f);               // exact product, truncation == floor
    return k < kOdOne - 1u ? k : kOdOne - 1u;
}

// one row of a thread's columns: column j, class c at v[j * C + c]
template <int C, bool VEC>
__device__ __forceinline__ void od_load(const float* __restrict__ p, int ncol, float (&v)[(VEC ? 4 : 1) * C]) {
    constexpr int NC = VEC ? 4 : 1;
    if constexpr (VEC) {
        if (ncol == 4) {
            const float4* p4 = reinterpret_cast<const float4*>(p);
#pragma unroll
            for (int q = 0; q < C; ++q) {
                const float4 a = p4[q];
                v[4 * q] = a.x; v[4 * q + 1] = a.y; v[4 * q + 2] = a.z; v[4 * q + 3] = a.w;
            }
            return;
        }
    }
#pragma unroll
    for (int j = 0; j < NC; ++j)        // (VEC: the columns behind the last whole item of a row)
#pragma unroll
        for (int c = 0; c < C; ++c) v[j * C + c] = j < ncol ? p[j * C + c] : 0.f;
}

template <int C, bool VEC>
__global__ void __launch_bounds__(kOdThreads) ordered_decode_k(const OdArgs A) {
    constexpr int NC = VEC ? 4 : 1;
    constexpr int D = NC * C <= 16 ? 8 : 4;          // rows in flight: D * NC * C floats of registers
    constexpr int DB = 8;                            // back-trace: words in flight
    const size_t t = (size_t)blockIdx.x * kOdThreads + threadIdx.x;
    if (t >= (size_t)A.B * A.ipr) return;
    const int b = (int)(t / A.ipr), x0 = (int)(t % A.ipr) * NC;
    const int ncol = A.W - x0 < NC ? A.W - x0 : NC;
    const int H = A.H;
    const size_t rs = (size_t)A.W * C;
    const float* __restrict__ p0 = A.probs + ((size_t)b * H * A.W + x0) * C;
    unsigned short* __restrict__ w0 = A.bits + (size_t)b * H * A.Wp + x0;
    const bool trace = A.labels || A.rows;

    // ---- forward sweep ----
    unsigned M[NC * C];
#pragma unroll
    for (int i = 0; i < NC * C; ++i) M[i] = 0u;
    float buf[D][NC * C];
#pragma unroll
    for (int d = 0; d < D; ++d)
        if (d < H) od_load<C, VEC>(p0 + (size_t)d * rs, ncol, buf[d]);
    for (int r0 = 0; r0 < H; r0 += D) {
#pragma unroll
        for (int d = 0; d < D; ++d) {
            const int r = r0 + d;
            if (r < H) {
                unsigned short bt[NC];
#pragma unroll
                for (int j = 0; j < NC; ++j) {
                    unsigned word = 1u, prev = 0u;
#pragma unroll
                    for (int c = 0; c < C; ++c) {
                        const unsigned F = od_quant(buf[d][j * C + c]) + M[j * C + c];
                        if (c == 0) {
                            prev = F;
                        } else {
                            const bool take = F > prev;      // strict: a tie stays with the lower class
                            word |= (take ? 1u : 0u) << c;
                            prev = take ? F : prev;
                        }
                        M[j * C + c] = prev;
                    }
                    bt[j] = (unsigned short)word;
                }
                if (trace) {
                    unsigned short* w = w0 + (size_t)r * A.Wp;
                    if constexpr (VEC) *reinterpret_cast<ushort4*>(w) = make_ushort4(bt[0], bt[1], bt[2], bt[3]);
                    else w[0] = bt[0];
                }
                if (r + D < H) od_load<C, VEC>(p0 + (size_t)(r + D) * rs, ncol, buf[d]);
            }
        }
    }
    if (A.score) {
#pragma unroll
        for (int j = 0; j < NC; ++j)
            if (j < ncol) A.score[(size_t)b * A.W + x0 + j] = M[j * C + C - 1];
    }
    if (!trace) return;

    // ---- back-trace ----
    int cur[NC];
    unsigned rowv[NC][C - 1];      // the boundary rows, in registers: 0 = the column starts below boundary i, unless a step sets it
#pragma unroll
    for (int j = 0; j < NC; ++j) {
        cur[j] = C - 1;
#pragma unroll
        for (int i = 0; i < C - 1; ++i) rowv[j][i] = 0u;
    }
    unsigned short* rows = A.rows ? A.rows + (size_t)b * (C - 1) * A.W + x0 : nullptr;
    unsigned char* lab0 = A.labels ? A.labels + (size_t)b * H * A.W + x0 : nullptr;
    unsigned short wb[DB][NC];
    auto load_bits = [&](int r, unsigned short (&o)[NC]) {
        const unsigned short* w = w0 + (size_t)r * A.Wp;
        if constexpr (VEC) {
            const ushort4 a = *reinterpret_cast<const ushort4*>(w);
            o[0] = a.x; o[1] = a.y; o[2] = a.z; o[3] = a.w;
        } else {
            o[0] = w[0];
        }
    };
#pragma unroll
    for (int d = 0; d < DB; ++d)
        if (d < H) load_bits(H - 1 - d, wb[d]);
    for (int q0 = 0; q0 < H; q0 += DB) {
#pragma unroll
        for (int d = 0; d < DB; ++d) {
            const int q = q0 + d;
            if (q < H) {
                const int r = H - 1 - q;
                unsigned char lb[NC];
#pragma unroll
                for (int j = 0; j < NC; ++j) {
                    const unsigned m = ((unsigned)wb[d][j] & ((2u << cur[j]) - 1u)) | 1u;
                    const int cn = 31 - __clz((int)m);      // the highest set bit at or below the class
                    // a step down fixes the boundaries cn..cur-1 at row r + 1 (no memory access in here: a store in a loop of
                    // unknown length would make every later load wait for all of them)
                    if (cn != cur[j]) {
#pragma unroll
                        for (int i = 0; i < C - 1; ++i)
                            if (i >= cn && i < cur[j]) rowv[j][i] = (unsigned)(r + 1);
                    }
                    cur[j] = cn;
                    lb[j] = (unsigned char)cn;
                }
                if (lab0) {
                    unsigned char* l = lab0 + (size_t)r * A.W;
                    if (VEC && A.lab4) {
                        *reinterpret_cast<uchar4*>(l) = make_uchar4(lb[0], lb[NC > 1 ? 1 : 0], lb[NC > 2 ? 2 : 0], lb[NC > 3 ? 3 : 0]);
                    } else {
#pragma unroll
                        for (int j = 0; j < NC; ++j)
                            if (j < ncol) l[j] = lb[j];
                    }
                }
                if (q + DB < H) load_bits(r - DB, wb[d]);
            }
        }
    }
    if (rows) {
#pragma unroll
        for (int j = 0; j < NC; ++j)
            if (j < ncol) {
#pragma unroll
                for (int i = 0; i < C - 1; ++i) rows[(size_t)i * A.W + j] = (unsigned short)rowv[j][i];
            }
    }
}

}  // namespace oct
