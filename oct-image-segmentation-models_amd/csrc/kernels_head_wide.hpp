// Channel-streaming head kernels: the head of kernels_head.hpp with the input channel count CIN (=
// start_neurons) as a RUNTIME argument, any multiple of 4 up to 64.  The register kernels keep a pixel's CIN activations and,
// in the backward pass, CIN*C + C + 2*CIN per-thread partial sums in VGPRs (264 accumulators at CIN 32, C 8); these keep
// nothing that grows with CIN:
//   * the logits are accumulated while z streams past in 16-byte steps (same fmaf chain per class, channel by channel, as
//     head_logits: the probabilities are bit-identical to the register kernels');
//   * the backward kernel reads z a second time (L2) in groups of 16 channels.  Per group every wave writes y, the masked
//     a = sum_c w dl and a * xhat of its 64 pixels to LDS tiles [pixel][16], dl once per chunk as [pixel][C padded to 16],
//     and forms the sums over pixels with v_mfma_f32_16x16x4_f32 (an exact fp32 fma chain), K = pixels:
//         dW[ch][c] = y^T dl,   sum a = a^T 1,   sum a xhat = (a xhat)^T 1,   db[c] = dl^T 1
//     Lane l reads tile[4t + (l >> 4)][l & 15] = word 64 t + l: 64 consecutive words, conflict-free, for both operands.
//     13 accumulators of 4 VGPRs (3 per channel group + the bias) are carried across the chunks a block walks.
// Summation order: MFMA k-steps in pixel order within a wave's 64 pixels, chunk after chunk, then (w0 + w1) + (w2 + w3)
// over the block's waves: fixed, so two runs give the same bits.  No atomics.  Invalid lanes of a ragged last chunk write
// dl = 0 and a = 0 (and a finite y of pixel 0), i.e. exact zeros into every sum; so do the pixels of the ignore label.
// Same buffers, same layouts as the register kernels: probs / argmax / Dice rows, g, part [B*nblk][2*CIN], wpart
// [B*nblk][CIN*C + C].  grid (nblk, B), a block walks chunks blockIdx.x, + nblk, ... of one image.
// Routing (host.hpp head_route): C = 2..8 with start_neurons > 32, or every width under option "head_wide".  C = 9..16 is
// kernels_head_cls.hpp at every width; it shares head_logits_stream below, so its probabilities are formed the same way.
#pragma once
#include "kernels_head.hpp"

namespace oct {

constexpr int kHeadWideMaxCin = 64;
typedef float hw_f32x4 __attribute__((ext_vector_type(4)));

// softmax probabilities of one pixel, z streamed from memory: head_logits without the y[] / zr[] arrays
template <int C, typename AT>
__device__ inline void head_logits_stream(const AT* __restrict__ zp, const float* __restrict__ ab, const float* __restrict__ w,
                                          const float* __restrict__ bias, const int CIN, float (&p)[C]) {
#pragma unroll
    for (int c = 0; c < C; ++c) p[c] = bias[c];
#pragma unroll 4
    for (int i = 0; i < CIN; i += 4) {
        const float4 v = lda4<AT>(zp + i);
        const float zz[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float y = fmaxf(fmaf(ab[i + k], zz[k], ab[CIN + i + k]), 0.f);
#pragma unroll
            for (int c = 0; c < C; ++c) p[c] = fmaf(y, w[(i + k) * C + c], p[c]);
        }
    }
    float mx = -3.4e38f;
#pragma unroll
    for (int c = 0; c < C; ++c) mx = fmaxf(mx, p[c]);
    head_softmax<C>(p, mx);
}

template <int C, typename AT>
__global__ __launch_bounds__(kBlock) void head_fwd_wide_k(const HeadFwdArgs A, const int CIN) {
    constexpr int N = DiceN<C>::value;
    __shared__ float red[256];
    const int b = blockIdx.y;
    float v[N];
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] = 0.f;
    for (int chunk = blockIdx.x; chunk * kBlock < A.HW; chunk += gridDim.x) {
        const int px = chunk * kBlock + threadIdx.x;
        const bool valid = px < A.HW;
        const size_t pix = (size_t)b * A.HW + (valid ? px : 0);
        float p[C];
        head_logits_stream<C, AT>(reinterpret_cast<const AT*>(A.z) + pix * CIN, A.ab, A.w, A.bias, CIN, p);
        if (valid) {
            if (A.probs) {
#pragma unroll
                for (int c = 0; c < C; ++c) A.probs[pix * C + c] = p[c];
            }
            if (A.argmax) {
                int am = 0; float best = p[0];
#pragma unroll
                for (int c = 1; c < C; ++c) if (p[c] > best) { best = p[c]; am = c; }  // first maximum, as np.argmax
                A.argmax[pix] = (unsigned char)am;
            }
        }
        const int lab = A.labels ? A.labels[pix] : 0;
        const float pw = A.pixw && A.labels ? A.pixw[pix] : 1.f;       // (uniform branch: see HeadQueue)
        if (valid && lab != A.ignore) {                     // the loss sums: counted pixels only (see head_fwd_k)
            if (A.labels) head_loss_sums<C, N>(A, lab, pw, p, v);
        }
    }
    if (A.labels) head_rows_store<N>(v, red, A.dice_part + ((size_t)b * gridDim.x + blockIdx.x) * N);
}

template <int C, typename AT>
__global__ __launch_bounds__(kBlock, 2) void head_bwd_wide_k(const HeadBwdArgs A, const int CIN) {
    constexpr int MAXG = kHeadWideMaxCin / 16, TILE = 64 * 16, NSLOT = 3 * MAXG + 1;
    static_assert(C <= 16, "dl rows are padded to 16 columns");
    static_assert(4 * NSLOT * 256 <= 4 * 4 * TILE, "the 4-wave sum reuses the tiles");
    __shared__ __attribute__((aligned(16))) float lds[4 * 4 * TILE];          // per wave: dl, y, a, a*xhat tiles of 64 pixels x 16
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float* const Tdl = lds + wave * 4 * TILE; float* const Ty = Tdl + TILE; float* const Ta = Ty + TILE; float* const Tx = Ta + TILE;
    const int b = blockIdx.y;
    hw_f32x4 accw[MAXG], acc1[MAXG], acc2[MAXG], accb = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int g = 0; g < MAXG; ++g) { accw[g] = hw_f32x4{0.f, 0.f, 0.f, 0.f}; acc1[g] = accw[g]; acc2[g] = accw[g]; }
    const float one = (lane & 15) == 0 ? 1.f : 0.f;      // B operand "column 0 = ones": D[row][0] = sum over pixels of A
    float num[C], den[C];
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const double* k = A.macro ? A.bc + 2 * (b * C + c) : A.bc + 2 * A.B * C;
        num[c] = (float)k[0]; den[c] = (float)k[1];
    }
    const float scale = (1.f - A.focal_w) * (A.macro ? A.loss_scale / (float)(A.B * C) : A.loss_scale);
    const HeadMeans hm = head_means<C>(A);
    const float fscale = A.focal_w * A.loss_scale * hm.inv_count;

    for (int chunk = blockIdx.x; chunk * kBlock < A.HW; chunk += gridDim.x) {
        const int px = chunk * kBlock + tid;
        const bool valid = px < A.HW;
        const size_t pix = (size_t)b * A.HW + (valid ? px : 0);
        const AT* const zp = reinterpret_cast<const AT*>(A.z) + pix * CIN;
        const int lab = A.labels[pix];
        const float pw = A.pixw ? A.pixw[pix] : 1.f;     // the pixel's loss weight: see head_bwd_k
        const bool counted = valid && lab != A.ignore;   // see head_bwd_k
        float p[C];
        head_logits_stream<C, AT>(zp, A.bn, A.w, A.bias, CIN, p);
        float dp[C], dot = 0.f;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const float yv = lab == c ? 1.f : 0.f;
            dp[c] = -scale * (2.f * yv * den[c] - num[c]) / (den[c] * den[c]);
            if (fscale != 0.f && lab == c) {        // focal term: see head_bwd_k
                const bool inr = p[c] >= kFocalEps && p[c] <= 1.f - kFocalEps;
                if (inr || !A.focal_clip_mod) {
                    const float pc = fminf(fmaxf(p[c], kFocalEps), 1.f - kFocalEps);
                    const float q = 1.f - p[c], cw = pw * (A.focal_cw ? A.focal_cw[c] : 1.f), qg1 = powf(q, A.focal_gamma - 1.f);
                    dp[c] += fscale * cw * (A.focal_gamma * qg1 * logf(pc) - (inr ? qg1 * q / pc : 0.f));
                }
            }
            dot = fmaf(p[c], dp[c], dot);
        }
        float dlb[C];
#pragma unroll
        for (int c = 0; c < C; ++c) dlb[c] = 0.f;
        if (A.bce_on) {                             // BCE term: see head_bwd_k
            float q[C], db[C];
            softmax_complement<C>(p, q);
            const float ws = pw * hm.bce_scale;
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const bool inr = counted && p[c] >= kFocalEps && q[c] >= kFocalEps;
                const float r = ws / ((lab == c ? p[c] : q[c]) + A.bce_inner);
                db[c] = inr ? (lab == c ? -r : r) : 0.f;
            }
#pragma unroll
            for (int c = 0; c < C; ++c) {
                float o = 0.f;
#pragma unroll
                for (int k = 0; k < C; ++k) if (k != c) o = fmaf(p[k], db[k], o);
                dlb[c] = p[c] * (q[c] * db[c] - o);
            }
        }
        float dl[16];
#pragma unroll
        for (int c = 0; c < 16; ++c) dl[c] = 0.f;
#pragma unroll
        for (int c = 0; c < C; ++c) dl[c] = (counted ? p[c] * (dp[c] - dot) : 0.f) + dlb[c];

        __syncthreads();                            // the previous chunk's operand reads are done
#pragma unroll
        for (int j = 0; j < 4; ++j) st4(Tdl + lane * 16 + 4 * j, make_float4(dl[4 * j], dl[4 * j + 1], dl[4 * j + 2], dl[4 * j + 3]));
#pragma unroll
        for (int g = 0; g < MAXG; ++g) {
            if (g * 16 < CIN) {                     // (uniform over the launch: the barriers below are reached by every thread)
                if (g > 0) __syncthreads();         // the previous group's operand reads are done
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int ch = g * 16 + 4 * j;
                    float yy[4] = {0.f, 0.f, 0.f, 0.f}, aa[4] = {0.f, 0.f, 0.f, 0.f}, xx[4] = {0.f, 0.f, 0.f, 0.f};
                    if (ch < CIN) {
                        const float4 zv = lda4<AT>(zp + ch);
                        const float zz[4] = {zv.x, zv.y, zv.z, zv.w};
#pragma unroll
                        for (int k = 0; k < 4; ++k) {
                            const int i = ch + k;
                            const float y = fmaxf(fmaf(A.bn[i], zz[k], A.bn[CIN + i]), 0.f);
                            float a = 0.f;
#pragma unroll
                            for (int c = 0; c < C; ++c) a = fmaf(A.w[i * C + c], dl[c], a);
                            a = (valid && y > 0.f) ? a : 0.f;
                            const float xh = (zz[k] - A.bn[BN_MEAN * CIN + i]) * A.bn[BN_RSTD * CIN + i];
                            yy[k] = y; aa[k] = a; xx[k] = a * xh;
                        }
                        if (valid) sta4<AT>(reinterpret_cast<AT*>(A.g) + pix * CIN + ch, make_float4(aa[0], aa[1], aa[2], aa[3]));
                    }
                    st4(Ty + lane * 16 + 4 * j, make_float4(yy[0], yy[1], yy[2], yy[3]));
                    st4(Ta + lane * 16 + 4 * j, make_float4(aa[0], aa[1], aa[2], aa[3]));
                    st4(Tx + lane * 16 + 4 * j, make_float4(xx[0], xx[1], xx[2], xx[3]));
                }
                __syncthreads();
#pragma unroll
                for (int t = 0; t < 16; ++t) {      // k-step t: pixels 4t .. 4t+3 of the wave
                    const float dv = Tdl[64 * t + lane], yv = Ty[64 * t + lane], av = Ta[64 * t + lane], xv = Tx[64 * t + lane];
                    accw[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(yv, dv, accw[g], 0, 0, 0);
                    acc1[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, one, acc1[g], 0, 0, 0);
                    acc2[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(xv, one, acc2[g], 0, 0, 0);
                    if (g == 0) accb = __builtin_amdgcn_mfma_f32_16x16x4f32(dv, one, accb, 0, 0, 0);
                }
            }
        }
    }
    // ---- 4-wave sum through LDS (fixed order), then the two partial rows.  Accumulator register r of lane l is
    // D[row 4 (l >> 4) + r][column l & 15]; slot 3g + {0, 1, 2} = dW / sum a / sum a xhat of group g, slot 3 MAXG = the bias ----
    __syncthreads();
    float* const red = lds + wave * NSLOT * 256;
#pragma unroll
    for (int g = 0; g < MAXG; ++g)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            red[(3 * g + 0) * 256 + r * 64 + lane] = accw[g][r];
            red[(3 * g + 1) * 256 + r * 64 + lane] = acc1[g][r];
            red[(3 * g + 2) * 256 + r * 64 + lane] = acc2[g][r];
        }
#pragma unroll
    for (int r = 0; r < 4; ++r) red[3 * MAXG * 256 + r * 64 + lane] = accb[r];
    __syncthreads();
    const size_t orow = (size_t)b * gridDim.x + blockIdx.x;
    float* const out = A.part + orow * (2 * CIN);
    float* const wout = A.wpart + orow * (size_t)(CIN * C + C);
    const int r = tid >> 6, row = 4 * (lane >> 4) + r, col = lane & 15;
    for (int slot = 0; slot < NSLOT; ++slot) {
        const float* q = lds + slot * 256 + tid;
        const float s = (q[0] + q[NSLOT * 256]) + (q[2 * NSLOT * 256] + q[3 * NSLOT * 256]);
        if (slot == 3 * MAXG) {
            if (col == 0 && row < C) wout[CIN * C + row] = s;
        } else {
            const int ch = (slot / 3) * 16 + row, kind = slot % 3;
            if (ch < CIN) {
                if (kind == 0) { if (col < C) wout[ch * C + col] = s; }
                else if (col == 0) out[(kind - 1) * CIN + ch] = s;
            }
        }
    }
}

}  // namespace oct
