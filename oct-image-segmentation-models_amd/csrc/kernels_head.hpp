// The head: BN+ReLU on load, 1x1 conv, softmax, optional probs / argmax / loss partial sums; and its backward: loss gradient
// -> softmax Jacobian -> 1x1 conv backward (data AND weights) -> mask + BN-backward statistics.
// Three kernel families run it (host.hpp head_route):
//   register           head_fwd_k / head_bwd_k<C, CIN, AT>, below: C 2..8, start_neurons <= 32 (the benched path)
//   channel-streaming  head_*_wide_k<C, AT>, kernels_head_wide.hpp: C 2..8, start_neurons > 32 or option "head_wide"
//   class-streaming    head_*_cls_k<C, AT>,  kernels_head_cls.hpp: C 9..16
// This file holds the argument blocks, what the forward kernels share -- the softmax tail (all three), the Dice / focal / BCE
// sums of a pixel (the two streaming kernels; head_fwd_k keeps them written out) and the row reduction (all three) -- and the
// register kernels.  The backward kernels' dlogits block, the two streaming backward kernels' tile code and the forward
// kernels' stores are still one copy per kernel: behind function calls they move the register allocation of most
// instantiations.
#pragma once
#include "common.hpp"
#include "kernels_fin.hpp"

namespace oct {

// ---- head: BN+ReLU on load, 1x1 conv, softmax, optional probs / argmax / Dice partial sums ---------------
constexpr int kDiceVals = 5;  // per class: I = sum y*p, T = sum y, P = sum p, Ih = sum y*[p>.5], Ph = sum [p>.5]
// floats of a Dice partial row: 5 C sums and slot 5 C.  Up to 12 classes a power of two (one block_reduce_store); 13..16
// classes need 66..81 and take 96 = 64 + 32 (head_rows_store).  oct_unet.hip::dice_n is the run-time twin.
constexpr int dice_row_floats(int C) { return 5 * C <= 16 ? 16 : (5 * C <= 32 ? 32 : (5 * C < 64 ? 64 : 96)); }
template <int C> struct DiceN { static constexpr int value = dice_row_floats(C); };

struct HeadFwdArgs {
    const void* z; const float* ab;    // last conv's raw output (activation storage type) + BN record
    const float* w; const float* bias; // (CIN, C), (C)
    float* probs; unsigned char* argmax; const unsigned char* labels;
    float* dice_part;                  // [B][nblk][DiceN]; slot 5*C (always spare: 5*C < DiceN) = focal-loss sum, or the BCE sum
    int HW, nblk, act_bf16;
    // focal half of focal_dice_loss (custom_losses.py:98-178): cw[y] * (1 - p_y)^gamma * (-log p_y), p clipped to [1e-7, 1-1e-7]
    int focal_on; float focal_gamma; const float* focal_cw;   // class weights (C) or nullptr
    int focal_clip_mod;                // 1: the (1 - p)^gamma modulation also sees the clipped p; 0: only the logarithm does
    // BCE half of bce_dice_loss (custom_losses.py:84-91; Keras 2.9 backend.binary_crossentropy restated, parity unpinned):
    //   sum_c -( y ln(pc + e) + (1 - y) ln(qc + e) ),  pc = clip(p, eps, 1-eps), qc = clip(1 - p, eps, 1-eps),  e = eps or 0
    // Never together with focal_on: the two share slot 5*C.
    int bce_on; float bce_inner;       // bce_inner = e (option bce_inner_eps)
    // ignore label (oct_unet_set_ignore_label): a pixel with this label byte adds nothing to the Dice sums or to slot 5*C;
    // its probs / argmax are written as ever.  -1 = off: a label byte never compares equal
    int ignore;
    // per-pixel weights of the focal / BCE term (oct_unet_set_pixel_weights): (B,H,W) f32, or nullptr = off.  One multiply per
    // term; the Dice sums never see it.  The mean still divides by B*H*W (or the counted pixels), NOT by the sum of the weights
    const float* pixw;
};
constexpr float kFocalEps = 1e-7f;
constexpr int kHeadClsMin = 9, kHeadClsMax = 16;     // the class-streaming family (kernels_head_cls.hpp); 16 = the columns of one dl tile

// q_c = 1 - p_c of a softmax row, taken as the sum of the other classes: `1.f - p` has an absolute error of one ulp of p,
// which is all of q where p saturates (and 1/q is what the BCE gradient multiplies by)
template <int C>
__device__ inline void softmax_complement(const float (&p)[C], float (&q)[C]) {
#pragma unroll
    for (int c = 0; c < C; ++c) {
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < C; ++k) if (k != c) s += p[k];
        q[c] = s;
    }
}

// ---- per-pixel functions shared by the forward kernels ----------------------------------------------------------------

// logits in p and their maximum -> probabilities: max-subtract, expf, one reciprocal
template <int C>
__device__ __forceinline__ void head_softmax(float (&p)[C], float mx) {
    float sum = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) { p[c] = expf(p[c] - mx); sum += p[c]; }
    const float inv = 1.f / sum;
#pragma unroll
    for (int c = 0; c < C; ++c) p[c] *= inv;
}

// what a COUNTED pixel (valid, labelled, not the ignore label) adds to its thread's row of loss sums: the five Dice sums
// per class and, at slot 5 C, the focal or the BCE sum
template <int C, int N>
__device__ __forceinline__ void head_loss_sums(const HeadFwdArgs& A, int lab, float pw, const float (&p)[C], float (&v)[N]) {
    static_assert(C * kDiceVals < N, "slot 5 C is spare");
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const float yv = lab == c ? 1.f : 0.f, ph = p[c] > 0.5f ? 1.f : 0.f;
        v[c * kDiceVals + 0] += yv * p[c]; v[c * kDiceVals + 1] += yv; v[c * kDiceVals + 2] += p[c];
        v[c * kDiceVals + 3] += yv * ph;   v[c * kDiceVals + 4] += ph;
    }
    if (A.focal_on) {
        float py = p[0];
#pragma unroll
        for (int c = 1; c < C; ++c) py = lab == c ? p[c] : py;
        const float pc = fminf(fmaxf(py, kFocalEps), 1.f - kFocalEps);
        const float cw = pw * (A.focal_cw ? A.focal_cw[lab < C ? lab : 0] : 1.f);     // the pixel's weight rides on the class weight
        v[C * kDiceVals] += cw * powf(1.f - (A.focal_clip_mod ? pc : py), A.focal_gamma) * -logf(pc);
    }
    if (A.bce_on) {
        float q[C], t = 0.f;
        softmax_complement<C>(p, q);
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const float u = lab == c ? p[c] : q[c];        // y picks one of the two logarithms
            t -= logf(fminf(fmaxf(u, kFocalEps), 1.f - kFocalEps) + A.bce_inner);
        }
        v[C * kDiceVals] = fmaf(pw, t, v[C * kDiceVals]);
    }
}

// block sum of the threads' rows -> one row of dice_part.  Rows of 96 floats go as 64 + 32 (fixed order).  `red`: 256 floats
// of LDS; every thread of the block must call it
template <int N>
__device__ __forceinline__ void head_rows_store(float (&v)[N], float* red, float* out) {
    static_assert(N == 16 || N == 32 || N == 64 || N == 96, "a power of two, or 64 + 32");
    if constexpr (N <= 64) {
        block_reduce_store<N>(v, red, out, N);
    } else {
        float lo[64], hi[32];
#pragma unroll
        for (int i = 0; i < 64; ++i) lo[i] = v[i];
#pragma unroll
        for (int i = 0; i < 32; ++i) hi[i] = v[64 + i];
        block_reduce_store<64>(lo, red, out, 64);
        block_reduce_store<32>(hi, red, out + 64, 32);
    }
}

// ---- the register family's forward kernel ------------------------------------------------------------------------

// raw z of one pixel (CIN values) -> registers; split from the arithmetic so that the head kernels can request later
// chunks' pixels before they work on the current one (HeadQueue)
template <int CIN, typename AT>
__device__ inline void head_load(const AT* __restrict__ zp, float (&zr)[CIN]) {
#pragma unroll
    for (int i = 0; i < CIN; i += 4) {
        const float4 v = lda4<AT>(zp + i);
        zr[i] = v.x; zr[i + 1] = v.y; zr[i + 2] = v.z; zr[i + 3] = v.w;
    }
}

// The head kernels' chunk walk keeps D chunks requested ahead of the one in work: a thread's pixel (CIN raw values) and its
// label byte sit in registers from D chunks before they are used, so a block has D x 256 x (CIN x 4 + 1) bytes in flight
// while it computes.  pop() hands out the oldest entry and requests chunk `next` into the freed slot (nothing once the
// walk runs past the image: the slot then keeps stale values that are never handed out).
constexpr int kHeadFwdAhead = 1, kHeadBwdAhead = 1;
template <int CIN, int D, typename AT>
struct HeadQueue {
    const AT* zb; const unsigned char* lb; const float* wb; int HW;
    float zq[D][CIN]; int lq[D]; float wq[D];       // wq: the pixel's loss weight, 1 unless a map is set (a uniform branch)
    __device__ HeadQueue(const AT* z, const unsigned char* l, const float* w, int hw) : zb(z), lb(l), wb(w), HW(hw) {}
    __device__ __forceinline__ void request(int d, int chunk) {
        if (chunk * kBlock < HW) {
            const int px = chunk * kBlock + (int)threadIdx.x, q = px < HW ? px : 0;
            head_load<CIN, AT>(zb + (size_t)q * CIN, zq[d]);
            if (lb) lq[d] = lb[q];
            if (wb) wq[d] = wb[q];
        }
    }
    __device__ __forceinline__ void fill(int first, int stride) {
#pragma unroll
        for (int d = 0; d < D; ++d) { lq[d] = 0; wq[d] = 1.f; request(d, first + d * stride); }
    }
    __device__ __forceinline__ int pop(float (&zr)[CIN], float& pw, int next) {
        const int lab = lq[0];
        pw = wq[0];
#pragma unroll
        for (int i = 0; i < CIN; ++i) zr[i] = zq[0][i];
#pragma unroll
        for (int d = 0; d + 1 < D; ++d) {
            lq[d] = lq[d + 1]; wq[d] = wq[d + 1];
#pragma unroll
            for (int i = 0; i < CIN; ++i) zq[d][i] = zq[d + 1][i];
        }
        request(D - 1, next);
        return lab;
    }
};

template <int C, int CIN>
__device__ inline void head_logits(const float* __restrict__ ab, const float* __restrict__ w, const float* __restrict__ bias,
                                   float (&y)[CIN], const float (&zr)[CIN], float (&p)[C]) {
#pragma unroll
    for (int i = 0; i < CIN; ++i) y[i] = fmaxf(fmaf(ldc(ab + i), zr[i], ldc(ab + CIN + i)), 0.f);
    float mx = -3.4e38f;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        float l = ldc(bias + c);
#pragma unroll
        for (int i = 0; i < CIN; ++i) l = fmaf(y[i], ldc(w + i * C + c), l);
        p[c] = l; mx = fmaxf(mx, l);
    }
    head_softmax<C>(p, mx);
}

// grid (nblk, B): each block walks the 256-pixel chunks  blockIdx.x, blockIdx.x + nblk, ...  of ONE image and emits
// one row of Dice partial sums
template <int C, int CIN, typename AT>
__global__ __launch_bounds__(kBlock) void head_fwd_k(const HeadFwdArgs A) {
    constexpr int N = DiceN<C>::value;
    __shared__ float red[256];
    const int b = blockIdx.y;
    float v[N];
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] = 0.f;
    HeadQueue<CIN, kHeadFwdAhead, AT> hq(reinterpret_cast<const AT*>(A.z) + (size_t)b * A.HW * CIN,
                                         A.labels ? A.labels + (size_t)b * A.HW : nullptr,
                                         A.pixw && A.labels ? A.pixw + (size_t)b * A.HW : nullptr, A.HW);
    hq.fill(blockIdx.x, gridDim.x);
    for (int chunk = blockIdx.x; chunk * kBlock < A.HW; chunk += gridDim.x) {
        const int px = chunk * kBlock + threadIdx.x;
        const bool valid = px < A.HW;
        const size_t pix = (size_t)b * A.HW + (valid ? px : 0);
        float y[CIN], zr[CIN], p[C], pw;
        const int lab = hq.pop(zr, pw, chunk + kHeadFwdAhead * (int)gridDim.x);     // this chunk's pixel; the one kHeadFwdAhead chunks on is requested
        head_logits<C, CIN>(A.ab, A.w, A.bias, y, zr, p);
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
        if (valid && lab != A.ignore) {                     // the loss sums: counted pixels only
            // head_loss_sums, written out.  Called as a function here it moves the register allocation of this kernel: 10 of
            // the 112 instantiations gain one or two VGPRs, head_fwd_k<7, 12, float> (87 -> 89) in every form of the call that
            // was tried.  Keep the two texts equal, statement for statement: tests/test_gpu_wide_head.py
            // holds the register and the channel-streaming kernels' results bit-equal
            if (A.labels) {
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    const float yv = lab == c ? 1.f : 0.f, ph = p[c] > 0.5f ? 1.f : 0.f;
                    v[c * kDiceVals + 0] += yv * p[c]; v[c * kDiceVals + 1] += yv; v[c * kDiceVals + 2] += p[c];
                    v[c * kDiceVals + 3] += yv * ph;   v[c * kDiceVals + 4] += ph;
                }
                if (A.focal_on) {
                    float py = p[0];
#pragma unroll
                    for (int c = 1; c < C; ++c) py = lab == c ? p[c] : py;
                    const float pc = fminf(fmaxf(py, kFocalEps), 1.f - kFocalEps);
                    const float cw = pw * (A.focal_cw ? A.focal_cw[lab < C ? lab : 0] : 1.f);     // the pixel's weight rides on the class weight
                    v[C * kDiceVals] += cw * powf(1.f - (A.focal_clip_mod ? pc : py), A.focal_gamma) * -logf(pc);
                }
                if (A.bce_on) {
                    float q[C], t = 0.f;
                    softmax_complement<C>(p, q);
#pragma unroll
                    for (int c = 0; c < C; ++c) {
                        const float u = lab == c ? p[c] : q[c];        // y picks one of the two logarithms
                        t -= logf(fminf(fmaxf(u, kFocalEps), 1.f - kFocalEps) + A.bce_inner);
                    }
                    v[C * kDiceVals] = fmaf(pw, t, v[C * kDiceVals]);
                }
            }
        }
    }
    if (A.labels) head_rows_store<N>(v, red, A.dice_part + ((size_t)b * gridDim.x + blockIdx.x) * N);
}

// ---- head backward: Dice gradient -> softmax Jacobian -> 1x1 conv backward (data AND weights) -> mask + stats ------
// Everything the head needs is in registers here (y, p, dlogits), so its dW/db are accumulated in the same pass:
// no dlogits tensor, no second read of z.  grid (nblk, B); a block walks chunks of one image and emits one row of
// BN-backward statistics and one row of head-weight partials.
struct HeadBwdArgs {
    const void* z; const float* bn;      // last conv block (z: activation storage type)
    const float* w; const float* bias;   // head (CIN,C),(C)
    const unsigned char* labels;
    const double* bc;                    // Dice constants from dice_finalize_k
    void* g;                             // (B,H,W,CIN) masked gradient of the last conv block (activation storage type)
    float* part;                         // [B*nblk][2*CIN]       BN-backward statistics
    float* wpart;                        // [B*nblk][CIN*C + C]   head kernel / bias gradient partials
    int HW, nblk, B, macro; float loss_scale; int act_bf16;
    // focal_dice_loss: L = w * focal + (1 - w) * dice  (focal_w = 0: plain Dice)
    float focal_w, focal_gamma; const float* focal_cw; float inv_count;   // inv_count = 1 / (B*H*W)
    int focal_clip_mod;                // see HeadFwdArgs
    // bce_dice_loss: L = bce + dice_micro (focal_w = 0, macro = 0); bce_scale = loss_scale / (B*H*W*C)
    int bce_on; float bce_inner, bce_scale;
    // ignore label (oct_unet_set_ignore_label; -1 = off): dl of such a pixel is exactly 0 for every class, so g is stored as 0
    // and the pixel adds nothing to the statistics or the head dW / db partials.  With it set, the means' 1 / (counted
    // pixels) comes from bc[2*B*C + 2] (dice_finalize_k) and stands in for inv_count, also inside bce_scale
    int ignore;
    // per-pixel weights (see HeadFwdArgs): multiply dp of the focal term and db of the BCE term; nullptr = off
    const float* pixw;
    FinDesc fin;                       // BN-backward sums of the last conv block finalized by the last block (kernels_fin.hpp)
};

// the two constants of the focal / BCE means: the host's with the mask off, else formed from the device's count by the same
// float expressions, read once in front of the chunk loop
struct HeadMeans { float inv_count, bce_scale; };
template <int C>
__device__ __forceinline__ HeadMeans head_means(const HeadBwdArgs& A) {
    HeadMeans m{A.inv_count, A.bce_scale};
    if (A.ignore >= 0) { m.inv_count = (float)A.bc[2 * A.B * C + 2]; m.bce_scale = A.loss_scale * m.inv_count / (float)C; }
    return m;
}

template <int C, int CIN, typename AT>
__global__ __launch_bounds__(kBlock) void head_bwd_k(const HeadBwdArgs A) {
    constexpr int NV = CIN * C + C, NG = (NV + 31) / 32;
    constexpr int CP = CIN <= 4 ? 4 : (CIN <= 8 ? 8 : (CIN <= 16 ? 16 : 32));     // the block reduction takes powers of two
    __shared__ float red[256];
    const int b = blockIdx.y;
    float s1[CP], s2[CP], wv[NG * 32];
#pragma unroll
    for (int i = 0; i < CP; ++i) { s1[i] = 0.f; s2[i] = 0.f; }
#pragma unroll
    for (int i = 0; i < NG * 32; ++i) wv[i] = 0.f;
    float num[C], den[C];
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const double* k = A.macro ? A.bc + 2 * (b * C + c) : A.bc + 2 * A.B * C;
        num[c] = (float)k[0]; den[c] = (float)k[1];
    }
    const float scale = (1.f - A.focal_w) * (A.macro ? A.loss_scale / (float)(A.B * C) : A.loss_scale);
    const HeadMeans hm = head_means<C>(A);
    const float fscale = A.focal_w * A.loss_scale * hm.inv_count;

    HeadQueue<CIN, kHeadBwdAhead, AT> hq(reinterpret_cast<const AT*>(A.z) + (size_t)b * A.HW * CIN, A.labels + (size_t)b * A.HW,
                                         A.pixw ? A.pixw + (size_t)b * A.HW : nullptr, A.HW);
    hq.fill(blockIdx.x, gridDim.x);
    for (int chunk = blockIdx.x; chunk * kBlock < A.HW; chunk += gridDim.x) {
        const int px = chunk * kBlock + threadIdx.x;
        const bool valid = px < A.HW;
        const size_t pix = (size_t)b * A.HW + (valid ? px : 0);
        float y[CIN], zr[CIN], p[C], pw;
        const int lab = hq.pop(zr, pw, chunk + kHeadBwdAhead * (int)gridDim.x);     // later chunks' pixels are requested before this one is used
        const bool counted = valid && lab != A.ignore;  // folded into the selects that `valid` already feeds: no new branch
        head_logits<C, CIN>(A.bn, A.w, A.bias, y, zr, p);
        float dp[C], dot = 0.f;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const float yv = lab == c ? 1.f : 0.f;
            dp[c] = -scale * (2.f * yv * den[c] - num[c]) / (den[c] * den[c]);
            if (fscale != 0.f && lab == c) {
                // d/dp [ cw (1-p)^g (-log pc) ],  pc = clip(p, eps, 1-eps):  cw ( g (1-p)^(g-1) log pc - (1-p)^g / pc * [p == pc] );
                // with the modulation clipped too (focal_clip_mod) both terms vanish where the clip is active
                const bool inr = p[c] >= kFocalEps && p[c] <= 1.f - kFocalEps;
                if (inr || !A.focal_clip_mod) {
                    const float pc = fminf(fmaxf(p[c], kFocalEps), 1.f - kFocalEps);
                    const float q = 1.f - p[c], cw = pw * (A.focal_cw ? ldc(A.focal_cw + c) : 1.f), qg1 = powf(q, A.focal_gamma - 1.f);
                    dp[c] += fscale * cw * (A.focal_gamma * qg1 * logf(pc) - (inr ? qg1 * q / pc : 0.f));
                }
            }
            dot = fmaf(p[c], dp[c], dot);
        }
        // BCE half of bce_dice_loss.  The branch sits HERE, at the join behind the focal branch of the last class, and its
        // result is added below unconditionally (x + 0 = x: the Dice and focal paths stay bit-identical): a branch between
        // dl and the 1x1 backward costs <3, 8, float> 8 VGPRs (126 -> 134) and with them the fourth wave per SIMD
        float dlb[C];
#pragma unroll
        for (int c = 0; c < C; ++c) dlb[c] = 0.f;
        if (A.bce_on) {
            // dBCE/dp_c = s ( -y/(pc + e) + (1 - y)/(qc + e) ) where neither clip is active.  With q = 1 - p and the usual
            // p (dp - dot) the result is lost where p saturates: 1/q blows up exactly where 1 - p and dp - dot cancel
            // (DESIGN.md section 11).  So q comes from the other classes' probabilities, and the Jacobian is applied as
            //   dl_c = p_c ( q_c dp_c - sum_{k != c} p_k dp_k )
            float q[C], db[C];
            softmax_complement<C>(p, q);
            const float ws = pw * hm.bce_scale;          // the pixel's weight, once for all classes
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const bool inr = counted && p[c] >= kFocalEps && q[c] >= kFocalEps;
                const float r = ws / ((lab == c ? p[c] : q[c]) + A.bce_inner);     // y picks the term
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
        float dl[C];
#pragma unroll
        for (int c = 0; c < C; ++c) { dl[c] = (counted ? p[c] * (dp[c] - dot) : 0.f) + dlb[c]; wv[CIN * C + c] += dl[c]; }
        float g[CIN];
#pragma unroll
        for (int i = 0; i < CIN; ++i) {
            float a = 0.f;
#pragma unroll
            for (int c = 0; c < C; ++c) { a = fmaf(ldc(A.w + i * C + c), dl[c], a); wv[i * C + c] = fmaf(y[i], dl[c], wv[i * C + c]); }
            a = (valid && y[i] > 0.f) ? a : 0.f;
            const float xh = (zr[i] - ldc(A.bn + BN_MEAN * CIN + i)) * ldc(A.bn + BN_RSTD * CIN + i);
            g[i] = a; s1[i] += a; s2[i] += a * xh;
        }
        if (valid) {
#pragma unroll
            for (int i = 0; i < CIN; i += 4) sta4<AT>(reinterpret_cast<AT*>(A.g) + pix * CIN + i, make_float4(g[i], g[i + 1], g[i + 2], g[i + 3]));
        }
    }
    const size_t row = (size_t)b * gridDim.x + blockIdx.x;
    float* out = A.part + row * (2 * CIN);
    block_reduce_store<CP, true>(s1, red, out, CIN);
    block_reduce_store<CP, true>(s2, red, out + CIN, CIN);
    float* wout = A.wpart + row * NV;
#pragma unroll
    for (int gi = 0; gi < NG; ++gi) {
        float t[32];
#pragma unroll
        for (int k = 0; k < 32; ++k) t[k] = wv[gi * 32 + k];
        block_reduce_store<32>(t, red, wout + gi * 32, NV - gi * 32 < 32 ? NV - gi * 32 : 32);
    }
    if (A.fin.counter) {
        __shared__ __attribute__((aligned(16))) char fin_lds[16 + kBlock * 16 + 2 * CP * 8];
        finalize_in_launch(A.fin, A.part, gridDim.x * gridDim.y, CIN, gridDim.x * gridDim.y, fin_lds);
    }
}

}  // namespace oct
