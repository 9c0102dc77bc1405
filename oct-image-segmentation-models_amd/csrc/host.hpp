// Host-side plumbing shared by the translation units of liboct_unet_hip.so: error channel, tuning options, the per-launch
// HIP-event profiler, the ONE shape rule that says which bf16-pipe kernel family can serve a conv launch (pipe_fit) and the
// signatures of the conv launchers.  The library is built from several .hip files compiled in parallel (build.sh):
// oct_unet.hip holds the plan (build_plan / carve at creation, plan_backward per backward call), the C ABI and the
// streaming kernels; tu_*.hip each instantiate one family of kernels (the MFMA convs, the head, ...) behind the launcher
// declared here.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "common.hpp"
#include "kernels_bwd.hpp"
#include "kernels_igemm.hpp"

struct oct_mc_out;                        // include/oct_unet.h

namespace octh {

// ---- tuning options.  oct_set_option edits the process-wide DEFAULTS (g_opt); a handle snapshots them when it is
// created and every launch of that handle reads the snapshot, so two handles with different settings can live in one
// process (train + eval engines) and a knob that shapes prepared weights or workspace rows (bt_m2, dw*_blocks) cannot
// change under a live handle. ----
struct Options {
    int thin_min_tiles = 2048;      // pixel tiles from which 8-channel layers use the VALU thin kernel
    int dw32_blocks = 512, dw16_blocks = 768;   // target resident blocks of a backward-weights launch (wide / thin fp32-pipe kernels)
    int igemm_p_blocks = 1280;      // persistent igemm grid
    int igemm_min_blocks = 512;     // a layer takes the taller pixel tile only if that still yields this many blocks
    int dwpair8 = 1;                // 3x3 layers with 8 output channels: pixel-pair backward-weights kernel (0 = padded 16-column kernel)
    int pair_geo = 221;             // pixel-pair kernel geometry NWY*100 + NWX*10 + RPW
    int pair_min_tiles = 2048;      // pixel tiles from which 3x3 layers with 8 output channels use the pixel-pair MFMA kernel
    int dw_side_stream = 1;         // backward-weights kernels on the handle's side stream beside the backward-data chain
    int bx_two_blocks = 1;          // wide bf16-pipe launches (3x3, 2x2-over-upsample) as 4-wave blocks with ONE input image, two per CU
                                    // (cfg-A +1.4 %, cfg-C bf16 +5.3 % over the 8-wave double-buffered blocks, which 0 selects)
    int bx_waves = 8;               // waves per block of conv_bx_k where the tile has >= 8 rows
    int fuse_first_apply = 1;       // the first conv's BN-backward transform is applied inside its backward-weights kernel
    int fuse_bn_apply = 1;          // every other block: the transform is applied by the dX / dW kernels while they stage g'
    int fuse_bn_apply16 = 1;        // ... also for the 16-K / 16-output thin backward-data launches (coefficients kept in LDS there)
    int fuse_dw_thin = 1;           // 3x3 layers with 8 output channels: backward-weights reduced inside the backward-data launches
    int timing_skip = 0;            // TIMING EXPERIMENTS ONLY (results become wrong): bit 0 / 1 = skip the forward / backward BN finalize launches after step 2
    int fuse_bn_finalize = 0;       // 1: the BN records of the thin layers are written by the last block of the launch that emits the
                                    // partial rows (kernels_fin.hpp) instead of by a bn_*_finalize launch.  Built, tested -- and measured
                                    // 0.5-1 % SLOWER per step than the 5 us finalize launches it removes: off
    int bt_m2 = 1;                  // conv_bt_k: 8-output-channel launches in the two-pixel form
    int dwbt_f32_all = 0;           // 1: fp32 mode also takes conv_dwbt_k for every thin shape
    int bt_blocks_per_cu = 0;       // thin bf16-pipe kernel: persistent blocks per CU (0 = what its LDS allows)
    int dwbx_enable = 1;            // wide backward-weights on the bf16 pipe (0: the fp32-pipe conv_dw32_k; experiments)
    int dwbx_blocks = 256;          // target grid of a bf16-pipe backward-weights launch
    int bx_min_blocks = 256;        // a bf16-pipe launch takes the taller pixel tile only if that still yields this many blocks
    int mfma_mode = 1;              // 1: bf16 MFMA pipe (split products in fp32 mode); 0: the fp32-pipe kernels everywhere
    int focal_clip_mod = 0;         // focal loss: 1 = the (1-p)^gamma modulation sees the clipped p too
    int bce_inner_eps = 1;          // bce_dice_loss: 1 = ln(clip(p) + 1e-7) (Keras backend restated from memory), 0 = ln(clip(p))
    int fork_on_launch = 1;         // the event a forked backward-weights kernel waits for is the completion signal of the preceding
                                    // launch itself (0: a recorded marker behind it -- ~6 us in front of every backward-data launch)
    int dw_fork_group = 1;          // blocks whose backward-weights launches share one fork to the side stream.  Measured: 2-4 halve the
                                    // caller stream's idle time (119 -> 71 us) and still lose 1.3-1.7 % per step -- the late kernels
                                    // pair with backward-data launches of the next level, which they slow down more
    int event_sysfence = 0;         // 1: the handle's fork/join events carry a system-scope fence (set before oct_unet_create)
    int persist_min_tiles = 2048;   // pixel tiles from which thin single-chunk convs use the persistent pipelined kernel
    int head_wide = 0;              // 1: every start_neurons takes the channel-streaming head kernels (kernels_head_wide.hpp), which
                                    // widths above 32 always take: holds them against the register kernels on equal inputs
    int pool_in_epilogue = 1;       // fp32 storage: the bf16-pipe forward convs in front of a max-pool write the pooled tensor from their
                                    // accumulators (raw window extrema; consumers apply BN + ReLU on load) -- no pool_fwd_k pass
    int bx_down2_ring = 1;          // conv_bx_k, stride-2 forms: a resident grid of blocks walks the (image, tile) items and stages the next
                                    // item's first tile under the current item's last tap row (0: one block per item)
    int ordered_float4 = 0;         // oct_ordered_decode: 1 = four adjacent columns per thread, float4 loads, wherever the alignment
                                    // conditions hold.  Built, tested -- and measured SLOWER than one column per thread at every shape
                                    // tried, 16 k to 1 M columns: a column is a serial chain, so the call wants
                                    // the most waves, not the widest loads: off
    int max_blocks = 0;             // FOR TESTS ("persistent_max_blocks"): > 0 caps the grid of every persistent launch, so that
                                    // small images make blocks walk several tiles (cap_grid below); 0 = the launches' own grids
};
extern Options g_opt;

int fail(int code, const std::string& msg);

#define HIP_OK(expr)                                                                                      \
    do {                                                                                                  \
        hipError_t e__ = (expr);                                                                          \
        if (e__ != hipSuccess) return ::octh::fail(-5, std::string(#expr) + ": " + hipGetErrorString(e__)); \
    } while (0)

// ---- per-launch HIP-event profiler (off by default; bench.py turns it on for a few untimed steps) ---------
struct ProfRec { std::string kernel, layer; double flops, bytes; hipEvent_t e0, e1; };
struct Profiler {
    bool on = false;
    std::vector<ProfRec> recs;
    std::vector<hipEvent_t> pool;
    hipEvent_t get() {
        if (!pool.empty()) { hipEvent_t e = pool.back(); pool.pop_back(); return e; }
        hipEvent_t e; (void)hipEventCreate(&e); return e;
    }
};
extern thread_local Profiler* t_prof;

// RAII: records an event pair around the launch(es) issued in its scope, on the launch stream itself
struct ProfScope {
    Profiler* p; hipStream_t s; size_t idx;
    ProfScope(hipStream_t st, const char* kernel, const char* layer, double flops, double bytes) : p(t_prof), s(st), idx(0) {
        if (!p || !p->on) { p = nullptr; return; }
        ProfRec r{kernel, layer, flops, bytes, p->get(), p->get()};
        (void)hipEventRecord(r.e0, s);
        idx = p->recs.size(); p->recs.push_back(r);
    }
    ~ProfScope() { if (p) (void)hipEventRecord(p->recs[idx].e1, s); }
};

// run a launch statement with `AT` bound to the activation storage type
#define AT_DISPATCH(bf, ...) do { if (bf) { using AT = ::oct::bf16_t; __VA_ARGS__; } else { using AT = float; __VA_ARGS__; } } while (0)
#define AT_NAME(bf) ((bf) ? "unsigned short" : "float")

inline int cdiv(int a, int b) { return (a + b - 1) / b; }
// the grid of a persistent launch (blocks that walk pixel tiles; one statistic row / dW slab per block) under the
// "persistent_max_blocks" test cap: every such launch sizes its grid, its rows and its slabs through here
inline int cap_grid(int grid, const Options& o) { return o.max_blocks > 0 ? std::min(grid, o.max_blocks) : grid; }
inline int bx_mb(int M) { return M % 64 == 0 ? 64 : 32; }
inline bool bt_k_ok(int k) { return k == 8 || k == 16 || k == 32; }

// what a conv launch needs besides its argument block
struct LaunchCtx {
    const Options* o; int B; hipStream_t s; const char* layer; double flops, bytes;
    bool* pooled = nullptr;     // out (optional): the launch wrote IgemmArgs::pool_out (the kernel form it picked can)
};

// kernel family a conv launch runs on
enum ConvRoute { ROUTE_BT = 0, ROUTE_BX = 1, ROUTE_F32 = 2 };

// THE shape rule: which bf16-pipe family can serve a conv launch of K channels into M output channels at channel offset
// m_off of the weights' output dimension -- the thin kernel (ROUTE_BT: conv_bt_k, and whether its two-pixel form applies),
// the wide one (ROUTE_BX: conv_bx_k) or neither (ROUTE_F32).  `two`: the input is a concat of two tensors, the first C0
// channels wide.  Everything that needs the answer asks here: carve() about a layer's forward and backward-data launches
// (which prepared weights exist), conv_route about an argument block (which kernel runs), launch_bt about the two-pixel form.
struct PipeFit { ConvRoute fam; bool m2; };
inline PipeFit pipe_fit(int K, int M, int m_off, bool two, int C0, int amode) {
    const bool down2 = amode == oct::A_DOWN2;
    if (two && C0 % 8) return {ROUTE_F32, false};          // staging moves 8-channel octets: one source tensor each
    // thin: <= 16 output channels per launch, K exactly 8, 16 or 32 (the 2x-strided input tile only fits LDS at 8);
    // two-pixel form: exactly 8 output channels, 8 or 16 K channels, not the stride-2 gather
    if (M <= 16 && M % 4 == 0 && bt_k_ok(K) && (!down2 || K == 8)) return {ROUTE_BT, M == 8 && !down2 && K <= 16};
    // wide: 32-channel output blocks, K in octets up to the affine rows the kernel caches in LDS
    if (M % 32 == 0 && K % 8 == 0 && K <= (down2 ? 256 : 512) && m_off % bx_mb(M) == 0) return {ROUTE_BX, false};
    return {ROUTE_F32, false};
}

// The route of one launch: the family pipe_fit names, if mfma_mode is on, its prepared weights exist and the input carries
// no dropout the family cannot apply; else the fp32 pipe.  Asked ONCE per launch -- by conv_forward, and by plan_backward
// for each backward-data launch of a block (DxLaunch::route) -- because only the bf16-pipe kernels can apply the
// BN-backward transform on load and finalize statistics in the launch; launch_igemm is handed the answer.
ConvRoute conv_route(const oct::IgemmArgs& a, int amode, const Options& o);

// MFMA conv launchers (forward and backward-data); *rows = statistic partial rows the launch writes.
// Defined in launch_conv.hpp, instantiated one per tu_conv_*.hip.
template <int KH, int AMODE, int EPI>
int launch_igemm(const oct::IgemmArgs& a, ConvRoute r, const LaunchCtx& c, int* rows);

// Backward-weights plan of a layer (oct_unet.hip::dw_plan): the kernel family, its channel chunking, pixel-tile height,
// pixel-block count.  MFMA launchers: launch_dw.hpp, instantiated in tu_dw_*.hip.
enum DwKind {
    DW_VALU,      // VALU kernels of oct_unet.hip (image input / head)
    DW_F32_16,    // fp32 pipe, thin (conv_dw16_k, conv_dwpair8_k)
    DW_F32_32,    // fp32 pipe, wide (conv_dw32_k)
    DW_BX,        // bf16 pipe, wide (conv_dwbx_k)
    DW_BT,        // bf16 pipe, thin (conv_dwbt_k)
};
struct DwPlan { DwKind kind; int cic, coc, th, chunks, npb, tiles; };
int launch_dw_bf16pipe(const oct::ConvBwdWArgs& a, const DwPlan& p, int kh, bool up, const LaunchCtx& c);
int launch_dw_f32pipe(const oct::ConvBwdWArgs& a, const DwPlan& p, int kh, bool up, const LaunchCtx& c);

// The head's kernel family (kernels_head.hpp, kernels_head_wide.hpp, kernels_head_cls.hpp).  THE routing rule of the head: forward_head, head_backward and the gate of the
// in-launch statistics finalize (register kernels only) ask here.  The register kernels are instantiated for every
// start_neurons (= the head's input channels) up to 32; wider heads, and every head under option "head_wide", take the
// channel-streaming kernels, whose register use does not grow with cin.  More than 8 classes: the class-streaming kernels at
// every width, whatever "head_wide" says -- neither of the other two families is built there.
enum HeadRoute { HEAD_REG = 0, HEAD_WIDE = 1, HEAD_CLS = 2 };
inline HeadRoute head_route(const Options& o, int n_cls, int cin) {
    return n_cls >= oct::kHeadClsMin ? HEAD_CLS : (cin > 32 || o.head_wide ? HEAD_WIDE : HEAD_REG);
}
// The two head launchers (tu_head.hip): C classes, cin input channels, on the family r.  Same argument blocks, output buffers
// and layouts on every family; a.fin is for HEAD_REG alone.  Neither allocates or waits.
int launch_head_fwd(const oct::HeadFwdArgs& a, HeadRoute r, int C, int cin, int B, hipStream_t s);
int launch_head_bwd(const oct::HeadBwdArgs& a, HeadRoute r, int C, int cin, int B, hipStream_t s);
// The kernels are instantiated a class range to a translation unit (launch_head.hpp; tu_head_<family>_<direction>_<first C>.hip),
// sized so that build.sh compiles them side by side and none is the slowest unit of the build.  X(family, direction: 0 forward |
// 1 backward, first C, last C); unit X's entry point is head_unit_<family>_<direction>_<first C>.  A unit whose four defines are
// not a row of this list does not compile (launch_head.hpp).
#define OCT_HEAD_UNITS(X)                                             \
    X(0, 0, 2, 5) X(0, 0, 6, 8)                                       \
    X(0, 1, 2, 4) X(0, 1, 5, 6) X(0, 1, 7, 7) X(0, 1, 8, 8)           \
    X(1, 0, 2, 8) X(1, 1, 2, 8)                                       \
    X(2, 0, 9, 12) X(2, 0, 13, 16) X(2, 1, 9, 12) X(2, 1, 13, 16)
#define OCT_HEAD_UNIT_ARGS_0 ::oct::HeadFwdArgs
#define OCT_HEAD_UNIT_ARGS_1 ::oct::HeadBwdArgs
#define OCT_HEAD_UNIT_DECL(fam, bwd, c0, c1) \
    int head_unit_##fam##_##bwd##_##c0(const OCT_HEAD_UNIT_ARGS_##bwd& a, int C, int cin, dim3 grid, hipStream_t s);
OCT_HEAD_UNITS(OCT_HEAD_UNIT_DECL)
#undef OCT_HEAD_UNIT_DECL

// Monte-Carlo dropout reduction (tu_mc.hip): every argument error of oct_mc_update(probs, ..., t, T, ws, ws_bytes, out), with
// nothing launched -- oct_unet_infer (kind MC) asks about its last sample before its first launch
int mc_validate(const float* probs, int B, int H, int W, int n_cls, int t, int T, const void* ws, size_t ws_bytes,
                const oct_mc_out* out);

// Test-time augmentation (tu_tta.hip): every argument error of oct_flip_batch / oct_tta_update, with nothing launched --
// oct_unet_infer (kind TTA) asks about all of its views before its first launch.  *bytes (optional): the size of either buffer
int flip_validate(const void* src, int B, int H, int W, int pixel_bytes, int view, const void* dst, size_t* bytes);
int tta_validate(const float* probs, int B, int H, int W, int n_cls, int view, int t, int T, const void* ws, size_t ws_bytes,
                 const oct_mc_out* out);

}  // namespace octh
