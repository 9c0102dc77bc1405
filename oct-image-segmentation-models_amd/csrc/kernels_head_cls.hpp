// Class-streaming head kernels: the head for C = 9..16 classes, head_fwd_cls_k<C, AT> / head_bwd_cls_k<C, AT>.  The register
// kernels (kernels_head.hpp) and the channel-streaming ones (kernels_head_wide.hpp) stop at 8 classes; these
// take every class count above, at every start_neurons 4..64 (CIN is a RUNTIME argument, as in kernels_head_wide.hpp), and
// nothing below.  They are the channel-streaming kernels with what 16 classes change:
//   * probabilities: head_logits_stream, the same function in both kernels -- the backward pass recomputes the forward's
//     probabilities bit for bit.  Same max-subtract / expf / one reciprocal, same first-maximum arg-max.
//   * forward loss sums: a thread carries 5 C Dice sums and the focal / BCE sum at slot 5 C.  DiceN<C> = 64 holds them up to
//     C = 12 (61 slots); C = 13..16 (66..81 slots) take rows of 96 floats, reduced as 64 + 32 by two block_reduce_store
//     calls (fixed order).  dice_finalize_k takes C and the row width at run time.
//   * backward: the Dice derivative of class c takes one of two values per block, dp(y = 0) and dp(y = 1), formed once in
//     front of the chunk loop from the block-uniform (Num, Den) pair by the expression head_bwd_k evaluates per pixel (same
//     bits) and kept in SGPRs: 2 C scalar registers instead of 2 C VGPRs and C divisions per pixel.
//   * the BCE term is formed in a pass of its own over the classes, into the dl registers, after the Dice / focal term:
//     q, db and the O(C^2) Jacobian sum are live only inside it.
//   * dl goes to the [pixel][16] LDS tile, all 16 columns in use at C = 16; the sums over pixels are the fp32 MFMA chains of
//     head_bwd_wide_k (mfma_f32_16x16x4_f32, K = pixels, fixed order, no atomics).
// Same buffers and layouts as the other head kernels: probs / argmax / Dice rows [B][nblk][DiceN], g, part [B*nblk][2*CIN],
// wpart [B*nblk][CIN*C + C].  grid (nblk, B), a block walks chunks blockIdx.x, + nblk, ... of one image.  Invalid lanes of
// a ragged last chunk and pixels of the ignore label add exact zeros to every sum.
#pragma once
#include "kernels_head_wide.hpp"

namespace oct {

template <int C, typename AT>
__global__ __launch_bounds__(kBlock) void head_fwd_cls_k(const HeadFwdArgs A, const int CIN) {
    static_assert(C >= kHeadClsMin && C <= kHeadClsMax, "the class-streaming head carries 9..16 classes");
    constexpr int N = DiceN<C>::value;
    static_assert(N == 64 || N == 96, "rows of 64 floats, or 64 + 32");
    static_assert(C * kDiceVals < N, "slot 5 C is spare");
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
                float* const o = A.probs + pix * C;
                if constexpr (C % 4 == 0) {                 // rows of 16 C bytes: 16-byte aligned with the buffer
#pragma unroll
                    for (int c = 0; c < C; c += 4) st4(o + c, make_float4(p[c], p[c + 1], p[c + 2], p[c + 3]));
                } else {
#pragma unroll
                    for (int c = 0; c < C; ++c) o[c] = p[c];
                }
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

// a wave-uniform float held in a scalar register
__device__ __forceinline__ float head_uniform(float x) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(x))); }

template <int C, typename AT>
__global__ __launch_bounds__(kBlock, 2) void head_bwd_cls_k(const HeadBwdArgs A, const int CIN) {
    constexpr int MAXG = kHeadWideMaxCin / 16, TILE = 64 * 16, NSLOT = 3 * MAXG + 1;
    static_assert(C >= kHeadClsMin && C <= kHeadClsMax, "the class-streaming head carries 9..16 classes; dl rows have 16 columns");
    static_assert(4 * NSLOT * 256 <= 4 * 4 * TILE, "the 4-wave sum reuses the tiles");
    __shared__ __attribute__((aligned(16))) float lds[4 * 4 * TILE];          // per wave: dl, y, a, a*xhat tiles of 64 pixels x 16
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float* const Tdl = lds + wave * 4 * TILE; float* const Ty = Tdl + TILE; float* const Ta = Ty + TILE; float* const Tx = Ta + TILE;
    const int b = blockIdx.y;
    hw_f32x4 accw[MAXG], acc1[MAXG], acc2[MAXG], accb = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int g = 0; g < MAXG; ++g) { accw[g] = hw_f32x4{0.f, 0.f, 0.f, 0.f}; acc1[g] = accw[g]; acc2[g] = accw[g]; }
    const float one = (lane & 15) == 0 ? 1.f : 0.f;      // B operand "column 0 = ones": D[row][0] = sum over pixels of A
    const float scale = (1.f - A.focal_w) * (A.macro ? A.loss_scale / (float)(A.B * C) : A.loss_scale);
    // Dice derivative of class c at a pixel whose label is / is not c: head_bwd_k's expression at y = 0 and y = 1
    float dp0[C], dp1[C];
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const double* k = A.macro ? A.bc + 2 * (b * C + c) : A.bc + 2 * A.B * C;
        const float num = (float)k[0], den = (float)k[1];
        dp0[c] = head_uniform(-scale * (2.f * 0.f * den - num) / (den * den));
        dp1[c] = head_uniform(-scale * (2.f * 1.f * den - num) / (den * den));
    }
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
        float dl[16], dot = 0.f;                         // dl holds dp until the Jacobian below
#pragma unroll
        for (int c = 0; c < 16; ++c) dl[c] = 0.f;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            dl[c] = lab == c ? dp1[c] : dp0[c];
            if (fscale != 0.f && lab == c) {        // focal term: see head_bwd_k
                const bool inr = p[c] >= kFocalEps && p[c] <= 1.f - kFocalEps;
                if (inr || !A.focal_clip_mod) {
                    const float pc = fminf(fmaxf(p[c], kFocalEps), 1.f - kFocalEps);
                    const float q = 1.f - p[c], cw = pw * (A.focal_cw ? A.focal_cw[c] : 1.f), qg1 = powf(q, A.focal_gamma - 1.f);
                    dl[c] += fscale * cw * (A.focal_gamma * qg1 * logf(pc) - (inr ? qg1 * q / pc : 0.f));
                }
            }
            dot = fmaf(p[c], dl[c], dot);
        }
#pragma unroll
        for (int c = 0; c < C; ++c) dl[c] = counted ? p[c] * (dl[c] - dot) : 0.f;
        if (A.bce_on) {                             // BCE term, a second pass over the classes: see head_bwd_k
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
                dl[c] += p[c] * (q[c] * db[c] - o);
            }
        }

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
    // ---- 4-wave sum through LDS (fixed order), then the two partial rows: as head_bwd_wide_k.  Accumulator register r of
    // lane l is D[row 4 (l >> 4) + r][column l & 15]; slot 3g + {0, 1, 2} = dW / sum a / sum a xhat of group g, slot 3 MAXG = the bias ----
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
