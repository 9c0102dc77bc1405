// liboct_unet_hip.so -- host plan + C ABI of the MI355X-native OCT U-Net engine.  See include/oct_unet.h.
// Graph definition follows /root/reference/oct_image_segmentation_models/models/unet.py:106-153.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/oct_unet.h"
#include "host.hpp"
#include "kernels_bwd.hpp"
#include "kernels_fwd.hpp"
#include "kernels_igemm.hpp"
#include "kernels_bx.hpp"

using namespace oct;
using namespace octh;

#ifndef OCT_SRC_HASH
#define OCT_SRC_HASH "unstamped"     // build.sh passes the SHA-256 (12 hex digits) of csrc/*.hip, csrc/*.hpp, include/*.h
#endif

namespace octh {
Options g_opt;
thread_local Profiler* t_prof = nullptr;
namespace { thread_local std::string g_err; }
int fail(int code, const std::string& msg) { g_err = msg; return code; }

// the conv launchers live in their own translation units (tu_conv_*.hip): one explicit instantiation each
extern template int launch_igemm<3, A_NORMAL, EPI_FWD>(const IgemmArgs&, ConvRoute, const LaunchCtx&, int*);
extern template int launch_igemm<2, A_UPF, EPI_FWD>(const IgemmArgs&, ConvRoute, const LaunchCtx&, int*);
extern template int launch_igemm<3, A_NORMAL, EPI_MASK>(const IgemmArgs&, ConvRoute, const LaunchCtx&, int*);
extern template int launch_igemm<3, A_NORMAL, EPI_RAW>(const IgemmArgs&, ConvRoute, const LaunchCtx&, int*);
extern template int launch_igemm<3, A_DOWN2, EPI_MASK>(const IgemmArgs&, ConvRoute, const LaunchCtx&, int*);

// which kernel family runs a launch (host.hpp)
ConvRoute conv_route(const IgemmArgs& a, int amode, const Options& o) {
    const ConvRoute f = pipe_fit(a.Cin, a.Mout, a.m_off, a.flags & F_TWO, a.C0, amode).fam;
    if (o.mfma_mode && f == ROUTE_BT && a.wbt && !(a.flags & F_DROP)) return ROUTE_BT;    // (conv_bt_k applies no dropout)
    if (o.mfma_mode && f == ROUTE_BX && a.wbx) return ROUTE_BX;
    return ROUTE_F32;
}
}  // namespace octh

namespace {

enum Src { SRC_INPUT, SRC_PREV, SRC_POOL, SRC_UP, SRC_CONCAT, SRC_HEAD };

struct Layer {
    char name[32];
    int kh, kw, cin, cout, level, H, W, has_bn, src, skip_from, drop_in;
    size_t w_off, b_off, gamma_off, beta_off, mm_off, mv_off;
    // workspace (device) pointers
    void* z = nullptr; void* g = nullptr;   // activation storage type (f32 or bf16)
    float* bn = nullptr;
    float* dwp = nullptr;  // this layer's dW slabs [npb][kh*kw*cin*cout + cout]
    int dw_rows = 0;       // slabs allocated at creation: a launch never uses more (tuning options may change later)
    float* wt = nullptr;   // backward-data weights: transposed+flipped 3x3, or effective 3x3 of an up-conv (9*cin*cout)
    bf16_t* wbx_f = nullptr; bf16_t* wbx_b = nullptr;   // split weights for the bf16-pipe kernels (forward / backward-data)
    bool bt_m2_f = false, bt_m2_b = false;                // thin kernel: this layer's forward / backward-data launches use the two-pixel form
    bf16_t* wbt_f = nullptr; bf16_t* wbt_b = nullptr;   // ... for the thin bf16-pipe kernel (16-row slices; backward: cin / Cg slices)
};

struct Plan {
    std::vector<Layer> L;
    size_t n_params = 0, n_state = 0;
    int P = 0;
    std::vector<int> enc_last;  // per level: conv index whose output is pooled + skip-concatenated
};

int check_cfg(const oct_unet_cfg* c) {
    if (!c) return fail(-1, "null cfg");
    if (c->in_ch < 1) return fail(-1, "in_ch must be >= 1");
    if (c->n_cls < 2 || c->n_cls > 16) return fail(-1, "n_cls must be in 2..16");
    if (c->pool_layers < 1 || c->pool_layers > 6) return fail(-1, "pool_layers must be in 1..6");
    if (c->conv_layers < 1) return fail(-1, "conv_layers must be >= 1");
    if (c->start_neurons < 4 || c->start_neurons > 64 || c->start_neurons % 4)
        return fail(-1, "start_neurons must be a multiple of 4 in 4..64");
    if (c->enc_k != 3 || c->dec_k != 2) return fail(-1, "only enc_kernel (3,3) / dec_kernel (2,2) are implemented");
    const int m = 1 << c->pool_layers;
    if (c->H < m || c->W < m || c->H % m || c->W % m) return fail(-1, "H and W must be multiples of 2^pool_layers");
    if (c->max_batch < 1) return fail(-1, "max_batch must be >= 1");
    if (c->dtype != 0 && c->dtype != 1) return fail(-2, "dtype must be 0 (f32) or 1 (bf16 activation storage, f32 arithmetic)");
    if (!(c->dropout_rate >= 0.f && c->dropout_rate < 1.f)) return fail(-1, "dropout_rate must be in [0,1)");
    if (c->pool_layers * (2 * c->conv_layers + 1) + c->conv_layers + 1 > ReduceAllArgs::MAXL)
        return fail(-1, "too many conv layers (pool_layers*(2*conv_layers+1)+conv_layers+1 must be <= 40)");
    // the dropped tensor is the bottleneck output: (H/2^P, W/2^P, start_neurons*2^P)
    if ((size_t)c->max_batch * (c->H >> c->pool_layers) * (c->W >> c->pool_layers) *
            (size_t)(c->start_neurons << c->pool_layers) >= (1ull << 32))
        return fail(-1, "bottleneck tensor too large for 32-bit dropout indexing");
    if ((size_t)c->max_batch * c->H * c->W * (size_t)(2 * c->start_neurons) >= (1ull << 31))
        return fail(-1, "max_batch * H * W too large for the 32-bit element indexing used inside a layer");
    // (B,H,W,n_cls) probabilities: only at start_neurons 4 with more than 8 classes is this the tighter bound of the two
    if ((size_t)c->max_batch * c->H * c->W * (size_t)c->n_cls >= (1ull << 31))
        return fail(-1, "max_batch * H * W * n_cls must stay below 2^31 (32-bit element indexing of the probability maps)");
    return 0;
}

Plan build_plan(const oct_unet_cfg& c) {
    Plan pl; pl.P = c.pool_layers;
    const int sn = c.start_neurons, P = c.pool_layers, Lc = c.conv_layers;
    int cin = c.in_ch;
    auto add = [&](const std::string& nm, int k, int ci, int co, int lvl, int bn, int src, int skip) {
        Layer l{}; snprintf(l.name, sizeof l.name, "%s", nm.c_str());
        l.kh = l.kw = k; l.cin = ci; l.cout = co; l.level = lvl; l.H = c.H >> lvl; l.W = c.W >> lvl;
        l.has_bn = bn; l.src = src; l.skip_from = skip; l.drop_in = 0;
        l.w_off = pl.n_params; pl.n_params += (size_t)k * k * ci * co;
        l.b_off = pl.n_params; pl.n_params += co;
        if (bn) {
            l.gamma_off = pl.n_params; pl.n_params += co;
            l.beta_off = pl.n_params; pl.n_params += co;
            l.mm_off = pl.n_state; pl.n_state += co;
            l.mv_off = pl.n_state; pl.n_state += co;
        }
        pl.L.push_back(l);
    };
    for (int i = 0; i < P; ++i) {
        const int size = sn << i;
        for (int j = 0; j < Lc; ++j) {
            const int src = (i == 0 && j == 0) ? SRC_INPUT : (j == 0 ? SRC_POOL : SRC_PREV);
            add("enc" + std::to_string(i) + ".conv" + std::to_string(j), c.enc_k, cin, size, i, 1, src, -1);
            cin = size;
        }
        pl.enc_last.push_back((int)pl.L.size() - 1);
    }
    for (int j = 0; j < Lc; ++j) {
        add("mid.conv" + std::to_string(j), c.enc_k, cin, sn << P, P, 1, j == 0 ? SRC_POOL : SRC_PREV, -1);
        cin = sn << P;
    }
    for (int i = 0; i < P; ++i) {
        const int lvl = P - 1 - i, size = sn << lvl;
        add("dec" + std::to_string(i) + ".up", c.dec_k, cin, size, lvl, 1, SRC_UP, -1);
        if (i == 0 && c.dropout_rate > 0.f) pl.L.back().drop_in = 1;  // Dropout(0.5) sits on the bottleneck output
        cin = 2 * size;
        for (int j = 0; j < Lc; ++j) {
            add("dec" + std::to_string(i) + ".conv" + std::to_string(j), c.enc_k, cin, size, lvl, 1,
                j == 0 ? SRC_CONCAT : SRC_PREV, j == 0 ? pl.enc_last[lvl] : -1);
            cin = size;
        }
    }
    add("head", 1, cin, c.n_cls, 0, 0, SRC_HEAD, -1);
    return pl;
}

inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }
inline int tiles_of(int H, int W) { return cdiv(H, kTileY) * cdiv(W, kTileX); }
inline int chunk_of(int c) { return c % 16 == 0 ? 16 : (c % 8 == 0 ? 8 : 4); }   // channel chunk per thread

// ---- the shape rule (host.hpp: pipe_fit) asked about a layer's own conv launches: which prepared bf16 weights can be read.
// Forward: one launch of cin -> cout channels.  Backward-data: cout -> Cg channels at a time -- a concat's dX is two
// launches of cin / 2 channels each (the skip half at offset cin / 2, the up-path half at 0), an up-conv's the stride-2 gather ----
inline bool mfma_conv(const Layer& l) { return l.src != SRC_INPUT && l.has_bn; }   // not the image layer, not the head
inline int bwd_cg(const Layer& l) { return l.src == SRC_CONCAT ? l.cin / 2 : l.cin; }
inline PipeFit fit_fwd(const Layer& l) {
    if (!mfma_conv(l)) return {ROUTE_F32, false};
    return pipe_fit(l.cin, l.cout, 0, l.src == SRC_CONCAT, l.cin / 2, l.src == SRC_UP ? A_UPF : A_NORMAL);
}
inline PipeFit fit_bwd(const Layer& l) {
    PipeFit f{ROUTE_F32, false};
    if (!mfma_conv(l)) return f;
    for (int off = 0; off < l.cin && f.fam == ROUTE_F32; off += bwd_cg(l))      // (prepared if any of the launches can read them)
        f = pipe_fit(l.cout, bwd_cg(l), off, false, 0, l.src == SRC_UP ? A_DOWN2 : A_NORMAL);
    return f;
}

// thin backward-weights on the bf16 pipe (conv_dwbt_k): the instantiated (cin, cout) pairs
inline bool dwbt_ok(const Layer& l) {
    if (l.src == SRC_INPUT || l.kh == 1 || !l.has_bn) return false;
    const int ci = l.cin, co = l.cout;
    if (l.src == SRC_UP) return (ci == 16 && co == 8) || (ci == 32 && co == 16);
    if (l.src == SRC_CONCAT && (l.cin / 2) % 8) return false;         // staging moves 8-channel octets: one source tensor each
    return (ci == 8 && co == 8) || (ci == 8 && co == 16) || (ci == 16 && co == 8) || (ci == 16 && co == 16) ||
           (ci == 16 && co == 32) || (ci == 32 && co == 16);
}

// dW plan: which kernel handles a layer, its channel chunking, pixel-tile height and pixel-block count
DwPlan dw_plan(const Layer& l, int B, int mfma_mode, int bf16, const Options& o) {
    DwPlan p{};
    if (mfma_mode && o.dwbx_enable && l.src != SRC_INPUT && l.kh != 1 && l.cin % 32 == 0 && l.cout % 32 == 0) {
        // wide layers on the bf16 pipe: one block per (32 ci, 32 co) pair and pixel slice, ~1 block per CU in total
        p.kind = DW_BX; p.cic = 32; p.coc = 32; p.th = 4;
        p.chunks = (l.cin / 32) * (l.cout / 32);
        p.tiles = cdiv(l.H, p.th) * cdiv(l.W, kTileX);
        p.npb = std::max(1, std::min(B * p.tiles, cdiv(o.dwbx_blocks, p.chunks)));
        return p;
    }
    // fp32 mode: the three-term split of both operands makes conv_dwbt_k VALU-bound; measured per shape (B=32 256x512,
    // us, fp32-pipe kernel vs this one): 8->8 89 / 100, up-convs 98 / 113 and 55 / 66 stay on the fp32 pipe; 16->8 149 /
    // 143, 32->16 103 / 92, 8->16 39 / 35, 16->16 59 / 48, 16->32 come here.  bf16 mode (one rounding, one product): all.
    if (mfma_mode && dwbt_ok(l) && (bf16 || o.dwbt_f32_all || (l.src != SRC_UP && !(l.cin == 8 && l.cout == 8)))) {
        // thin layers on the bf16 pipe (conv_dwbt_k): one block holds all channels; 1 or 2 blocks per CU (LDS images)
        p.kind = DW_BT; p.cic = l.cin; p.coc = l.cout; p.th = 4; p.chunks = 1;
        p.tiles = cdiv(l.H, p.th) * cdiv(l.W, kTileX);
        p.npb = std::max(1, std::min(B * p.tiles, 256 * (l.cin + l.cout >= 48 ? 1 : 2)));
        return p;
    }
    if (l.src == SRC_INPUT || l.cin % 4 || l.cout % 4 || l.kh == 1) {
        // first layer (ANY in_ch: its source is the caller's image, uint8 or f32 -- only the VALU kernel's fetch_x reads
        // that; the MFMA stagers assume an activation-typed tensor) and the 1x1 n_cls-wide head
        p.kind = DW_VALU; p.cic = (l.src == SRC_INPUT || l.cin % 4) ? 1 : chunk_of(l.cin); p.coc = l.cout % 4 ? (l.cout <= 4 ? 4 : 8) : chunk_of(l.cout); p.th = kTileY;
    } else if (l.cin >= 32 && l.cout >= 32) {
        p.kind = DW_F32_32; p.cic = l.cin % 64 == 0 ? 64 : 32; p.coc = 32; p.th = p.cic == 64 ? 2 : 4;
    } else {
        p.kind = DW_F32_16; p.cic = l.cin >= 16 ? 16 : 8; p.coc = 16; p.th = 8;
    }
    p.chunks = cdiv(l.cin, p.cic) * cdiv(l.cout, p.coc);
    p.tiles = cdiv(l.H, p.th) * cdiv(l.W, kTileX);
    const int total = B * p.tiles;
    // one full round of resident blocks (no half-empty tail round): the wide kernel fits 2 blocks per CU (registers),
    // for the thin one 768 blocks measured best
    int target = p.kind == DW_F32_32 ? o.dw32_blocks : o.dw16_blocks;
    if (p.kind == DW_F32_16 && l.src == SRC_UP && p.cic == 16 && l.cout == 8) target = target * 4 / 3;   // (dz staged 8 wide: 4 blocks per CU)
    p.npb = std::max(1, std::min(total, cdiv(target, p.chunks)));
    return p;
}

// ---- what one block's backward launches (plan_backward decides, backward_impl walks) ----
// One backward-data launch: dz of the block x its transposed / effective weights.  `a` is the argument block the route
// was asked about and the one that is launched: a.out / a.Mout / a.m_off are the output buffer, its channel count Cg and
// the offset ci_off of those channels in the conv's input.
struct DxLaunch {
    IgemmArgs a;
    const Layer* prod;     // the block whose mask the launch applies and whose statistics it emits (nullptr: raw gradient)
    bool up;               // up-conv: stride-2 gather of dz
    const Layer* dw_x;     // with fdw: the block whose output is this launch's slice of the conv input ...
    bool dw_bias;          // ... and whether this launch also sums the bias gradient (one launch per block does)
    ConvRoute route;
};
struct BwdRoute {
    DwPlan dw;             // backward-weights plan, npb clipped to the slabs the layer owns
    bool fuse = false;     // dz = BN-backward transform of the masked gradient g', applied on load by every consumer of dz
                           // (the g buffer keeps g'); false: the stand-alone pass turns g into dz in place
    bool fdw = false;      // the backward-data launches reduce the backward-weights too (conv_bt_k FDW): no dW launch
    int n_dx = 0;
    DxLaunch dx[2];        // a concat: the skip half, then the up-path half
};

}  // namespace

struct oct_unet {
    oct_unet_cfg cfg;
    Options opt;                           // snapshot of the process-wide defaults at creation (host.hpp)
    Plan plan;
    float* params; float* grads; float* state;
    std::vector<void*> pooled, gpooled;    // per encoder level (activation storage type)
    std::vector<char> pool_raw;            // per encoder level, set by every forward: pooled[level] holds the window extrema of the
                                           // producer's RAW z (written by its conv launch; consumers apply its BN record on load)
                                           // instead of pool_fwd_k's activated maxima
    std::vector<BwdRoute> route;           // per layer: refilled at the top of every backward (options and B may change between calls)
    float* stat_part = nullptr;            // BN statistic partials (fwd and bwd share it: stream-ordered)
    unsigned* fin_counters = nullptr;      // [2 * layers] arrival counters of the in-launch finalizes (kernels_fin.hpp): zero between launches
    ReduceAllArgs red{};                   // filled while backward runs; one reduce launch at the end
    float* dice_part = nullptr; double* dice_bc = nullptr; float* loss4 = nullptr;   // loss4: 8 floats (dice_finalize_k)
    float focal_w = 0.f, focal_gamma = 2.f; const float* focal_cw = nullptr;           // focal_dice_loss (0 = plain Dice)
    int bce_on = 0;                                                                    // bce_dice_loss (never with focal_w > 0)
    int ignore = -1;                                                                   // ignore label of the loss (-1 = none)
    const float* pixw = nullptr;                                                       // per-pixel weights of the focal / BCE term (nullptr = off)
    // oct_unet_set_dice_shape (shape_on = 0: plain Dice, dice_finalize_k).  The folded macro and micro tables, each laid out as
    // dice_bc, and the sums table live in one device buffer the handle allocates at the first shape and frees in destroy: the
    // workspace keeps its size (tests/test_many_classes.py pins it)
    int shape_on = 0, shape_wmode = 0; float shape_alpha = .5f, shape_beta = .5f, shape_gamma = 1.f; const float* shape_cw = nullptr;
    double* shape_bcm = nullptr; double* shape_bcu = nullptr; double* shape_tab = nullptr;
    WtDesc* wt_descs = nullptr; int n_wt = 0; unsigned wt_total = 0;
    WbxDesc* wbx_descs = nullptr; int n_wbx_f = 0, n_wbx_b = 0; unsigned wbx_f_total = 0, wbx_b_total = 0;   // [fwd..., bwd...]
    WbtDesc* wbt_descs = nullptr; int n_wbt_f = 0, n_wbt_b = 0; unsigned wbt_f_total = 0, wbt_b_total = 0;   // [fwd..., bwd...]
    unsigned long long drop_step = 0; int drop_advance = 0;
    int last_B = 0; int last_training = 0; int have_dice = 0; int dice_final = 0;
    const void* last_x = nullptr; int last_u8 = 0;   // input of the last forward (first layer's dW re-reads it)
    hipGraph_t graph = nullptr; hipGraphExec_t graph_exec = nullptr;
    hipEvent_t tail_event = nullptr;       // recorded in backward once the decoder + bottleneck gradients are final
    // backward-weights kernels run on an internal low-priority side stream beside the backward-data chain (they are off
    // the critical path: dz_L -> dW_L feeds nothing until the slab reduce): fork / join with events, created with the handle
    hipStream_t side = nullptr; std::vector<hipEvent_t> fork_ev; hipEvent_t join_ev = nullptr, prep_ev = nullptr;
    Profiler prof;
};

namespace {

// Carve the workspace; with base == nullptr only sizes are computed.  Returns total bytes.
size_t carve(const oct_unet_cfg& c, Plan& pl, oct_unet* h, char* base, const Options& o) {
    size_t off = 0;
    auto take = [&](size_t bytes) -> char* { char* p = base ? base + off : nullptr; off += align256(bytes); return p; };
    const size_t B = (size_t)c.max_batch, esz = c.dtype ? 2 : 4;   // bytes per stored activation element
    size_t stat_max = 0;
    for (auto& l : pl.L) {
        const size_t n = B * l.H * l.W * l.cout;
        void* z = l.has_bn ? (void*)take(n * esz) : nullptr;   // the head writes straight to the caller's buffers
        void* g = c.training && l.has_bn ? (void*)take(n * esz) : nullptr;
        float* bn = l.has_bn ? (float*)take((size_t)BN_ARRAYS * l.cout * 4) : nullptr;
        float* wt = (c.training && l.has_bn && l.src != SRC_INPUT) ? (float*)take((size_t)9 * l.cin * l.cout * 4) : nullptr;
        const int ns = c.dtype ? 1 : 3;
        // prepared bf16 weights: exactly those a launch of this layer can be routed to
        const PipeFit ff = fit_fwd(l), fb = c.training ? fit_bwd(l) : PipeFit{ROUTE_F32, false};
        const bool m2f = o.bt_m2 && ff.m2, m2b = o.bt_m2 && fb.m2;
        bf16_t* wf = ff.fam == ROUTE_BX ? (bf16_t*)take(wbx_bytes(l.kh, l.cin, l.cout, bx_mb(l.cout), ns)) : nullptr;
        bf16_t* wb = fb.fam == ROUTE_BX ? (bf16_t*)take(wbx_bytes(3, l.cout, l.cin, bx_mb(bwd_cg(l)), ns)) : nullptr;
        bf16_t* tf = ff.fam == ROUTE_BT ? (bf16_t*)take(wbt_bytes(l.kh, l.cin, ns, m2f)) : nullptr;
        bf16_t* tb = fb.fam == ROUTE_BT ? (bf16_t*)take(wbt_bytes(3, l.cout, ns, m2b) * (l.cin / bwd_cg(l))) : nullptr;
        if (base) { l.bt_m2_f = m2f; l.bt_m2_b = m2b; }
        if (base) { l.z = z; l.g = g; l.bn = bn; l.wt = wt; l.wbx_f = wf; l.wbx_b = wb; l.wbt_f = tf; l.wbt_b = tb; }
        // statistic partial rows: one per pixel tile; the MFMA kernels may use tiles as small as 2 x 32 pixels
        stat_max = std::max(stat_max, B * cdiv(l.H, 2) * cdiv(l.W, kTileX) * 2 * (size_t)std::max(l.cout, l.cin));
        if (c.training) {
            const size_t wsz = (size_t)l.kh * l.kw * l.cin * l.cout + l.cout;
            const size_t rows = l.src == SRC_HEAD ? (size_t)(2048 + c.max_batch)
                                                  : (size_t)std::max(dw_plan(l, c.max_batch, 0, 0, o).npb, std::max(dw_plan(l, c.max_batch, 1, 1, o).npb, dw_plan(l, c.max_batch, 1, 0, o).npb));
            float* dwp = (float*)take(rows * wsz * 4);
            if (base) { l.dwp = dwp; l.dw_rows = (int)rows; }
        }
    }
    for (int i = 0; i < pl.P; ++i) {
        const size_t n = B * (c.H >> (i + 1)) * (c.W >> (i + 1)) * ((size_t)c.start_neurons << i);
        void* p = (void*)take(n * esz);
        void* gp = c.training ? (void*)take(n * esz) : nullptr;
        if (h) { h->pooled.push_back(p); h->gpooled.push_back(gp); h->pool_raw.push_back(0); }
    }
    const int nblk_head = cdiv(c.H * c.W, kBlock);
    stat_max = std::max(stat_max, B * nblk_head * 2 * (size_t)c.start_neurons);
    float* sp = (float*)take(stat_max * 4);
    // (rows of 64 floats and 8 pairs per image up to 8 classes, whatever n_cls: those workspaces keep their size)
    float* dp = (float*)take(B * nblk_head * (size_t)std::max(64, dice_row_floats(c.n_cls)) * 4);
    double* bc = (double*)take((B * std::max(8, c.n_cls) * 2 + 3) * 8);       // per (b, c) pairs, the micro pair, 1 / (counted pixels)
    float* l4 = (float*)take(8 * 4);
    unsigned* fc = (unsigned*)take(2 * pl.L.size() * sizeof(unsigned));
    if (h) h->fin_counters = fc;
    WtDesc* wd = c.training ? (WtDesc*)take(pl.L.size() * sizeof(WtDesc)) : nullptr;
    WbxDesc* xd = (WbxDesc*)take(2 * pl.L.size() * sizeof(WbxDesc));
    WbtDesc* td = (WbtDesc*)take(3 * pl.L.size() * sizeof(WbtDesc));
    if (h) { h->wt_descs = wd; h->wbx_descs = xd; h->wbt_descs = td; }
    if (h) { h->stat_part = sp; h->dice_part = dp; h->dice_bc = bc; h->loss4 = l4; }
    return off;
}

DropCfg make_drop(const oct_unet* h) {
    DropCfg d;
    d.seed = h->cfg.seed; d.step = h->drop_step;
    const double r = h->cfg.dropout_rate;
    d.thresh = (unsigned)std::min(4294967295.0, std::floor(r * 4294967296.0));
    d.scale = (float)(1.0 / (1.0 - r));
    return d;
}

// statistics of block li finalized by the last block of the launch that emits them (kernels_fin.hpp): thin channel counts
// only -- the reduction is done by ONE block
inline bool fin_ok(const oct_unet* h, const Layer& l) { return h->opt.fuse_bn_finalize && l.has_bn && l.cout <= 32 && l.cout % 2 == 0; }
FinDesc fin_desc(const oct_unet* h, int li, int bwd, int B) {
    const Layer& l = h->plan.L[li];
    FinDesc f{};
    f.counter = h->fin_counters + 2 * li + (bwd ? 1 : 0); f.bwd = bwd; f.count = (double)B * l.H * l.W;
    f.bn = l.bn; f.gamma = h->params + l.gamma_off; f.beta = h->params + l.beta_off;
    f.mm = h->state + l.mm_off; f.mv = h->state + l.mv_off;
    f.eps = h->cfg.bn_eps; f.momentum = h->cfg.bn_momentum; f.unbiased = h->cfg.bn_unbiased_moving_var;
    if (bwd) { f.dgamma = h->grads + l.gamma_off; f.dbeta = h->grads + l.beta_off; }
    return f;
}

// ---------------------------------------------------------------------------------------------------------------
// forward launches
// ---------------------------------------------------------------------------------------------------------------
template <int KH, int FLAGS>
int launch_conv_fwd_co(const ConvFwdArgs& a, int B, hipStream_t s, const char* layer, double flops, double bytes) {
    const int co_t = chunk_of(a.Cout);
    dim3 grid(a.tiles, a.Cout / co_t, B), block(kBlock);
    char nm[64]; snprintf(nm, sizeof nm, "conv_fwd_k<%d,%d,%d,%s>", KH, co_t, FLAGS, AT_NAME(a.act_bf16));
    ProfScope ps(s, nm, layer, flops, bytes);
    switch (co_t) {
        case 16: AT_DISPATCH(a.act_bf16, conv_fwd_k<KH, 16, FLAGS, AT><<<grid, block, 0, s>>>(a)); break;
        case 8: AT_DISPATCH(a.act_bf16, conv_fwd_k<KH, 8, FLAGS, AT><<<grid, block, 0, s>>>(a)); break;
        default: AT_DISPATCH(a.act_bf16, conv_fwd_k<KH, 4, FLAGS, AT><<<grid, block, 0, s>>>(a)); break;
    }
    HIP_OK(hipGetLastError());
    return 0;
}

// source description of layer li's input (shared by forward conv and dW)
struct SrcDesc { const void* x0; const float* ab0; int C0; const void* x1; const float* ab1; int C1; int flags; };

SrcDesc src_of(const oct_unet* h, int li, const void* x_in, int x_is_u8) {
    const Layer& l = h->plan.L[li];
    SrcDesc d{}; d.x1 = nullptr; d.ab1 = nullptr; d.C1 = 0;
    switch (l.src) {
        case SRC_INPUT: d.x0 = x_in; d.ab0 = nullptr; d.C0 = l.cin; d.flags = x_is_u8 ? F_U8 : 0; break;
        case SRC_PREV: case SRC_HEAD: { const Layer& p = h->plan.L[li - 1]; d.x0 = p.z; d.ab0 = p.bn; d.C0 = p.cout; d.flags = F_AFF; break; }
        case SRC_POOL: {       // a raw level (pool_raw): extrema of the producer's z, activated on load like a SRC_PREV input
            const bool raw = h->pool_raw[l.level - 1] != 0;
            d.x0 = h->pooled[l.level - 1]; d.ab0 = raw ? h->plan.L[li - 1].bn : nullptr; d.C0 = l.cin; d.flags = raw ? F_AFF : 0; break;
        }
        case SRC_UP: { const Layer& p = h->plan.L[li - 1]; d.x0 = p.z; d.ab0 = p.bn; d.C0 = p.cout; d.flags = F_AFF | F_UP; break; }
        case SRC_CONCAT: {
            const Layer& p = h->plan.L[li - 1]; const Layer& k = h->plan.L[l.skip_from];
            d.x0 = p.z; d.ab0 = p.bn; d.C0 = p.cout; d.x1 = k.z; d.ab1 = k.bn; d.C1 = k.cout; d.flags = F_AFF | F_TWO; break;
        }
    }
    return d;
}

// algorithmic bytes of a conv's logical input, read once: low-res tensor for an up-conv, both
// halves of a concat, the pooled tensor after a pool, 1 B/px for a u8 image
double in_bytes(const Layer& l, int B, int x_is_u8, int es = 4) {
    const double px = (double)B * l.H * l.W;
    if (l.src == SRC_INPUT) return px * l.cin * (x_is_u8 ? 1 : 4);
    if (l.src == SRC_UP) return px / 4 * l.cin * es;
    return px * l.cin * es;
}

// `dropout`: the layer's input passes through the dropout stream of the handle's current step, if the layer sits behind the
// dropout at all -- a training forward, or a Monte-Carlo sample of an inference forward (training == 0: BN from the moving
// statistics, no statistic rows)
int conv_forward(oct_unet* h, int li, const void* x_in, int x_is_u8, int B, int training, bool dropout, hipStream_t s) {
    Layer& l = h->plan.L[li];
    const SrcDesc sd = src_of(h, li, x_in, x_is_u8);
    ConvFwdArgs a{};
    a.x0 = sd.x0; a.ab0 = sd.ab0; a.C0 = sd.C0; a.x1 = nullptr; a.ab1 = nullptr; a.C1 = 0;   // VALU kernel: first layer only
    a.w = h->params + l.w_off; a.bias = h->params + l.b_off; a.z = l.z;
    a.part = (training && l.has_bn) ? h->stat_part : nullptr;
    a.H = l.H; a.W = l.W; a.Cin = l.cin; a.Cout = l.cout;
    a.tiles_x = cdiv(l.W, kTileX); a.tiles = tiles_of(l.H, l.W);
    a.drop = make_drop(h); a.act_bf16 = h->cfg.dtype;
    const bool drop = dropout && l.drop_in;
    const double px = (double)B * l.H * l.W, fl = 2.0 * l.kh * l.kw * l.cin * l.cout * px;
    const int es = h->cfg.dtype ? 2 : 4;
    const double by = in_bytes(l, B, x_is_u8, es) + px * l.cout * es;   // logical input once + output once
    int rc;
    int stat_rows = B * a.tiles;
    bool fin_in_launch = false;
    if (l.src != SRC_INPUT && l.cin % 4 == 0) {   // MFMA path (every conv except the 1-channel first layer)
        IgemmArgs g{};
        g.x0 = sd.x0; g.ab0 = sd.ab0; g.C0 = sd.C0; g.x1 = sd.x1; g.ab1 = sd.ab1; g.C1 = sd.C1;
        g.flags = sd.flags | (drop ? F_DROP : 0);
        g.Cin = l.cin; g.w = a.w; g.w_ld = l.cout; g.m_off = 0; g.bias = a.bias; g.out = l.z; g.Mout = l.cout;
        g.Ho = l.H; g.Wo = l.W; g.Hi = l.src == SRC_UP ? l.H / 2 : l.H; g.Wi = l.src == SRC_UP ? l.W / 2 : l.W;
        g.part = a.part; g.drop = a.drop; g.act_bf16 = h->cfg.dtype;
        g.wbx = l.wbx_f; g.wbx_M = l.cout; g.wbt = l.wbt_f; g.bt_m2 = l.bt_m2_f;
        // the block in front of a max-pool: the launch writes the pooled tensor too where its kernel form can (fp32 storage)
        const bool feeds_pool = li + 1 < (int)h->plan.L.size() && h->plan.L[li + 1].src == SRC_POOL;
        bool pooled = false;
        if (feeds_pool && h->opt.pool_in_epilogue && !h->cfg.dtype && l.has_bn) {
            g.pool_out = h->pooled[h->plan.L[li + 1].level - 1]; g.pool_gamma = h->params + l.gamma_off;
        }
        const LaunchCtx lc{&h->opt, B, s, l.name, fl, by, &pooled};
        const ConvRoute rt = conv_route(g, l.src == SRC_UP ? A_UPF : A_NORMAL, h->opt);
        if (training && fin_ok(h, l) && rt == ROUTE_BT) { g.fin = fin_desc(h, li, 0, B); fin_in_launch = true; }
        rc = l.src == SRC_UP ? launch_igemm<2, A_UPF, EPI_FWD>(g, rt, lc, &stat_rows)
                             : launch_igemm<3, A_NORMAL, EPI_FWD>(g, rt, lc, &stat_rows);
        if (feeds_pool) h->pool_raw[h->plan.L[li + 1].level - 1] = pooled ? 1 : 0;
    } else if (l.src == SRC_INPUT && l.cin == 1 && l.cout == 8 && l.kh == 3) {   // the real first layer: persistent streaming kernel
        const int tx = cdiv(l.W, 128), tiles = tx * cdiv(l.H, 8), total = B * tiles;
        const int grid = cap_grid(std::min(total, 2048), h->opt);      // <= B*ceil(H/2)*ceil(W/32) statistic rows guaranteed by carve()
        const int bf = h->cfg.dtype;
        if (training && fin_ok(h, l)) { a.fin = fin_desc(h, li, 0, B); fin_in_launch = true; }
        ProfScope ps(s, bf ? "conv_first_fwd_k<unsigned short>" : "conv_first_fwd_k<float>", l.name, fl, by);
        AT_DISPATCH(bf, conv_first_fwd_k<AT><<<grid, kBlock, 0, s>>>(a, x_is_u8, tx, tiles, total, a.w, a.bias));
        HIP_OK(hipGetLastError());
        stat_rows = grid; rc = 0;
    } else if (l.src == SRC_INPUT) {   // other first layers (odd channel counts): uint8 /255 table on load -> VALU direct conv
        rc = x_is_u8 ? launch_conv_fwd_co<3, F_U8>(a, B, s, l.name, fl, by) : launch_conv_fwd_co<3, 0>(a, B, s, l.name, fl, by);
    } else {
        return fail(-3, "conv_forward: channel count not a multiple of 4");
    }
    if (rc) return rc;
    if (l.has_bn && training && !fin_in_launch && !(h->opt.timing_skip & 1 && h->drop_step > 2)) {
        ProfScope ps(s, "bn_fwd_finalize_k", l.name, 0, (double)stat_rows * 2 * l.cout * 4);
        BnFinArgs f{};
        f.part = h->stat_part; f.nblk = stat_rows; f.C = l.cout; f.count = (double)B * l.H * l.W;
        f.gamma = h->params + l.gamma_off; f.beta = h->params + l.beta_off; f.bn = l.bn;
        f.mm = h->state + l.mm_off; f.mv = h->state + l.mv_off;
        f.eps = h->cfg.bn_eps; f.momentum = h->cfg.bn_momentum; f.unbiased = h->cfg.bn_unbiased_moving_var;
        bn_fwd_finalize_k<<<l.cout, kBlock, 0, s>>>(f);
        HIP_OK(hipGetLastError());
    }
    return 0;
}

// blocks per image of the head kernels: ~2048 blocks in total, each walking several 256-pixel chunks
int head_nblk(int HW, int B) { return std::max(1, std::min(cdiv(HW, kBlock), cdiv(2048, B))); }

int dice_n(int C) { return dice_row_floats(C); }

// this step's weights in the operand layouts of the bf16-pipe conv kernels (split in fp32 mode, rounded in bf16 mode):
// one launch per kernel family, over the forward descriptors or the backward-data ones (which read the prep_wt_k output)
int prep_split_weights(oct_unet* h, bool bwd, hipStream_t s) {
    if (!h->opt.mfma_mode) return 0;
    const int item_bytes = 8 * (4 + 2 * (h->cfg.dtype ? 1 : 3));
    auto grid = [](unsigned total) { return std::min<unsigned>((total + kBlock - 1) / kBlock, 2048u); };
    if (const int n = bwd ? h->n_wbx_b : h->n_wbx_f) {
        const unsigned total = bwd ? h->wbx_b_total : h->wbx_f_total;
        ProfScope ps(s, "prep_wbx_k", "all", 0, (double)total * item_bytes);
        prep_wbx_k<<<grid(total), kBlock, 0, s>>>(h->wbx_descs + (bwd ? h->n_wbx_f : 0), n, total);
        HIP_OK(hipGetLastError());
    }
    if (const int n = bwd ? h->n_wbt_b : h->n_wbt_f) {
        const unsigned total = bwd ? h->wbt_b_total : h->wbt_f_total;
        ProfScope ps(s, "prep_wbt_k", "all", 0, (double)total * item_bytes);
        prep_wbt_k<<<grid(total), kBlock, 0, s>>>(h->wbt_descs + (bwd ? h->n_wbt_f : 0), n, total);
        HIP_OK(hipGetLastError());
    }
    return 0;
}

// The forward in three parts, so that a Monte-Carlo forward can run the first once and the other two per sample:
// forward_prepare (this step's weights; the BN records from the moving statistics), forward_stages (the conv blocks
// [li0, li1) with their pools) and forward_head.  fside: the weight preparation runs on the side stream under the first layer.
int forward_prepare(oct_unet* h, int training, bool fside, hipStream_t s) {
    Plan& pl = h->plan;
    // this step's weights, split / rounded into bf16 MFMA operand order (one launch per kernel family).  In a training
    // step they run on the side stream under the first layer (which does not use them).
    hipStream_t ps_ = fside ? h->side : s;
    if (fside) { HIP_OK(hipEventRecord(h->fork_ev[0], s)); HIP_OK(hipStreamWaitEvent(h->side, h->fork_ev[0], 0)); }
    if (int rc = prep_split_weights(h, false, ps_)) return rc;
    if (fside) HIP_OK(hipEventRecord(h->prep_ev, h->side));
    if (!training) {  // (a, b) of every block from the moving statistics: one launch
        ProfScope ps(s, "bn_infer_all_k", "all", 0, (double)pl.n_state * 4 * 3);
        BnInferAll ia{};
        for (auto& l : pl.L)
            if (l.has_bn) {
                auto& e = ia.L[ia.n++];
                e.gamma = h->params + l.gamma_off; e.beta = h->params + l.beta_off;
                e.mm = h->state + l.mm_off; e.mv = h->state + l.mv_off; e.bn = l.bn; e.C = l.cout;
            }
        bn_infer_all_k<<<ia.n, 128, 0, s>>>(ia, h->cfg.bn_eps);
        HIP_OK(hipGetLastError());
    }
    return 0;
}

int forward_stages(oct_unet* h, const void* x, int x_is_u8, int B, int training, bool dropout, bool fside, int li0, int li1,
                   hipStream_t s) {
    Plan& pl = h->plan;
    for (int li = li0; li < li1; ++li) {
        Layer& l = pl.L[li];
        // pool the previous block's output (BN+ReLU applied on load) -- unless its conv launch has written the raw window
        // extrema already (pool_raw: set by conv_forward of block li - 1 just before)
        if (l.src == SRC_POOL && !h->pool_raw[l.level - 1]) {
            const Layer& p = pl.L[li - 1];
            const size_t n = (size_t)B * (p.H / 2) * (p.W / 2) * (p.cout / 4);
            const int grid = (int)std::min<size_t>((n + kBlock - 1) / kBlock, 8192);
            const int bf = h->cfg.dtype;
            ProfScope ps(s, bf ? "pool_fwd_k<unsigned short>" : "pool_fwd_k<float>", p.name, 0, (double)n * (bf ? 8 : 16) * 5);   // read 4 px, write 1
            AT_DISPATCH(bf, pool_fwd_k<AT><<<grid, kBlock, 0, s>>>((const AT*)p.z, p.bn, (AT*)h->pooled[l.level - 1], B, p.H, p.W, p.cout));
            HIP_OK(hipGetLastError());
        }
        if (fside && li == 1) HIP_OK(hipStreamWaitEvent(s, h->prep_ev, 0));     // first layer that reads the split weights
        const int rc = conv_forward(h, li, x, x_is_u8, B, training, dropout, s);
        if (rc) return rc;
    }
    return 0;
}

int forward_head(oct_unet* h, int B, const oct_unet_io* io, hipStream_t s) {
    Plan& pl = h->plan;
    const int nl = (int)pl.L.size();
    const Layer& hd = pl.L[nl - 1]; const Layer& last = pl.L[nl - 2];
    HeadFwdArgs a{};
    a.z = last.z; a.ab = last.bn; a.w = h->params + hd.w_off; a.bias = h->params + hd.b_off;
    a.probs = io ? io->probs : nullptr; a.argmax = io ? io->argmax : nullptr; a.labels = io ? io->labels : nullptr;
    a.dice_part = h->dice_part; a.HW = hd.H * hd.W; a.nblk = head_nblk(a.HW, B); a.act_bf16 = h->cfg.dtype;
    a.focal_on = h->focal_w > 0.f; a.focal_gamma = h->focal_gamma; a.focal_cw = h->focal_cw; a.focal_clip_mod = h->opt.focal_clip_mod;
    a.bce_on = h->bce_on; a.bce_inner = h->opt.bce_inner_eps ? kFocalEps : 0.f; a.ignore = h->ignore;
    a.pixw = h->pixw;
    if (int rc = launch_head_fwd(a, head_route(h->opt, h->cfg.n_cls, hd.cin), h->cfg.n_cls, hd.cin, B, s)) return rc;
    h->have_dice = a.labels != nullptr;
    return 0;
}

int forward_impl(oct_unet* h, const void* x, int x_is_u8, int B, int training, const oct_unet_io* io, hipStream_t s) {
    const int nl = (int)h->plan.L.size();
    const bool fside = training && h->opt.dw_side_stream && h->side && !(t_prof && t_prof->on);
    if (int rc = forward_prepare(h, training, fside, s)) return rc;
    if (int rc = forward_stages(h, x, x_is_u8, B, training, training != 0, fside, 0, nl - 1, s)) return rc;
    if (fside && nl - 1 <= 1) HIP_OK(hipStreamWaitEvent(s, h->prep_ev, 0));
    if (int rc = forward_head(h, B, io, s)) return rc;
    h->last_B = B; h->last_training = training;
    return 0;
}

// index of the first decoder layer (the up-convolution behind the bottleneck, whose input the dropout sits on)
int first_dec_layer(const Plan& pl) {
    for (int li = 0; li < (int)pl.L.size(); ++li) if (pl.L[li].src == SRC_UP) return li;
    return (int)pl.L.size() - 1;
}

// ---------------------------------------------------------------------------------------------------------------
// backward launches
// ---------------------------------------------------------------------------------------------------------------
template <int KH>
int launch_dw(const ConvBwdWArgs& a, int ci_t, int co_t, hipStream_t s, const char* layer, double flops, double bytes) {
    dim3 grid(a.npb, cdiv(a.Cin, ci_t), cdiv(a.Cout, co_t)), block(kBlock);
    char nm[64]; snprintf(nm, sizeof nm, "conv_bwd_w_k<%d,%d,%d,%s>", KH, ci_t, co_t, AT_NAME(a.act_bf16));
    ProfScope ps(s, nm, layer, flops, bytes);
#define DW_CASE(CI, CO) if (ci_t == CI && co_t == CO) { AT_DISPATCH(a.act_bf16, conv_bwd_w_k<KH, CI, CO, AT><<<grid, block, 0, s>>>(a)); HIP_OK(hipGetLastError()); return 0; }
    DW_CASE(1, 4) DW_CASE(1, 8) DW_CASE(1, 16)
#undef DW_CASE
    return fail(-3, "dW: unsupported channel chunking");
}

// index of the first bottleneck conv: layers [0, idx) are the encoder
int first_mid_layer(const Plan& pl) { return pl.enc_last.empty() ? 0 : pl.enc_last.back() + 1; }

// register a layer's slabs for the single end-of-backward reduce launch
void queue_reduce(oct_unet* h, const Layer& l, int npb) {
    ReduceAllArgs& R = h->red;
    ReduceAllArgs::Entry& e = R.L[R.n];
    e.part = l.dwp; e.dw = h->grads + l.w_off; e.db = h->grads + l.b_off; e.npb = npb;
    e.wsize = (unsigned)((size_t)l.kh * l.kw * l.cin * l.cout); e.stride = e.wsize + l.cout;
    e.jw = e.stride < 16384 ? 16 : 64;
    e.blk_start = R.n ? R.L[R.n - 1].blk_start + cdiv((int)R.L[R.n - 1].stride, R.L[R.n - 1].jw) : 0;
    ++R.n;
}

int flush_reduce(oct_unet* h, hipStream_t s) {
    ReduceAllArgs& R = h->red;
    if (!R.n) return 0;
    const ReduceAllArgs::Entry& last = R.L[R.n - 1];
    const unsigned blocks = last.blk_start + cdiv((int)last.stride, last.jw);
    double bytes = 0;
    for (int i = 0; i < R.n; ++i) bytes += (double)R.L[i].npb * R.L[i].stride * 4;
    ProfScope ps(s, "reduce_all_k", "all", 0, bytes);
    reduce_all_k<<<blocks, kBlock, 0, s>>>(R);
    HIP_OK(hipGetLastError());
    R.n = 0;
    return 0;
}

// the real first layer (1 -> 8 channels, 3x3, image input): streaming backward-weights kernel; it can apply the layer's
// BN-backward transform itself (nothing else reads that dz).  The one predicate of the plan and of the launch: the image
// layer is always DW_VALU, carries BN, is never behind the dropout, and its source flags are F_U8 or none.
inline bool first_dw_streams(const Layer& l) { return l.src == SRC_INPUT && l.cin == 1 && l.cout == 8 && l.kh == 3; }

// Decide what every block's backward launches for this call's B and the handle's current options: h->route.  Host
// arithmetic only -- nothing is launched here, and everything below that launches reads the record instead of deciding again.
int plan_backward(oct_unet* h, int B) {
    const Plan& pl = h->plan;
    const Options& o = h->opt;
    for (int li = 0; li + 1 < (int)pl.L.size(); ++li) {
        const Layer& l = pl.L[li];
        BwdRoute& r = h->route[li];
        r = BwdRoute{};
        r.dw = dw_plan(l, B, o.mfma_mode, h->cfg.dtype, o);
        r.dw.npb = cap_grid(std::min(r.dw.npb, l.dw_rows), o);
        // The block's BN-backward transform dz = ga g' + gb z + gd is applied by the consumers of dz while they stage it --
        // the backward-weights kernel and the backward-data launches -- whenever all of them can (the bf16-pipe conv kernels
        // and every MFMA backward-weights kernel); otherwise by the stand-alone pass, in place.
        if (l.src == SRC_INPUT) {      // its dz has ONE consumer, the streaming backward-weights kernel
            r.fuse = o.fuse_first_apply && first_dw_streams(l);
            continue;
        }
        // a backward-data launch: dz x transposed / effective weights through the MFMA implicit-GEMM kernels, into the Cg
        // channels at ci_off of the conv's input
        auto add = [&](void* gout, int Cg, int ci_off, const Layer* prod, bool up, const Layer* dw_x, bool dw_bias) {
            DxLaunch& d = r.dx[r.n_dx++];
            d.prod = prod; d.up = up; d.dw_x = dw_x; d.dw_bias = dw_bias;
            IgemmArgs& g = d.a;
            g.x0 = l.g; g.C0 = l.cout; g.flags = 0; g.Cin = l.cout;
            g.w = l.wt; g.w_ld = l.cin; g.m_off = ci_off; g.out = gout; g.Mout = Cg;
            g.Hi = l.H; g.Wi = l.W; g.Ho = up ? l.H / 2 : l.H; g.Wo = up ? l.W / 2 : l.W;
            g.part = prod ? h->stat_part : nullptr; g.zin = prod ? prod->z : nullptr; g.bnin = prod ? prod->bn : nullptr;
            g.drop_out = (up && l.drop_in) ? 1 : 0; g.drop = make_drop(h); g.act_bf16 = h->cfg.dtype;
            g.wbx = l.wbx_b; g.wbx_M = l.cin;
            g.wbt = l.wbt_b ? l.wbt_b + (size_t)(ci_off / Cg) * (wbt_bytes(3, l.cout, h->cfg.dtype ? 1 : 3, l.bt_m2_b) / 2) : nullptr;
            g.bt_m2 = l.bt_m2_b;
            d.route = conv_route(d.a, up ? A_DOWN2 : A_NORMAL, o);
        };
        const Layer& p = pl.L[li - 1];
        switch (l.src) {
            case SRC_PREV: add(p.g, p.cout, 0, &p, false, &p, true); break;
            case SRC_POOL: add(h->gpooled[l.level - 1], l.cin, 0, nullptr, false, nullptr, false); break;   // raw: the pool backward routes it into block li-1
            case SRC_UP: add(p.g, p.cout, 0, &p, true, nullptr, false); break;
            case SRC_CONCAT: {
                const Layer& k = pl.L[l.skip_from];
                add(k.g, k.cout, p.cout, nullptr, false, &k, false);   // skip half first (raw, merged later by the pool backward of that encoder level) ...
                add(p.g, p.cout, 0, &p, false, &p, true);              // ... then the up-path half, whose statistics must be the ones pending for block li-1
                break;
            }
            default: return fail(-3, "backward: bad src");
        }
        bool all_bf16 = true, all_bt = true;
        for (int i = 0; i < r.n_dx; ++i) { all_bf16 = all_bf16 && r.dx[i].route != ROUTE_F32; all_bt = all_bt && r.dx[i].route == ROUTE_BT; }
        const ConvRoute r0 = r.dx[r.n_dx - 1].route;      // the launch at channel offset 0 (a concat's halves have the same K and Cg)
        const bool up = l.src == SRC_UP;
        const int cg = bwd_cg(l);
        // (three bf16-pipe instantiations stay out: the stride-2 gather beyond the coefficient rows its LDS holds; the
        //  thin kernel at 32 K channels, whose staging registers for g' AND z no longer fit; and the thin kernel at 16 K
        //  channels with 16 output channels, where the second raw register set spills under the 256-register budget of two
        //  blocks per CU: 87 us against 45 + 33 for the separate pass at B = 32, 128 x 256)
        r.fuse = o.fuse_bn_apply && r.dw.kind != DW_VALU && all_bf16 && !(up && r0 == ROUTE_BX && l.cout > kBxGbDown2MaxC) &&
                 !(r0 == ROUTE_BT && l.cout == 32) && !(r0 == ROUTE_BT && l.cout == 16 && cg == 16 && !o.fuse_bn_apply16);
        // 3x3 layers with 8 output channels on the thin kernel (the full-resolution convs): their backward-data launches
        // reduce the backward-weights too (conv_bt_k FDW) -- g', z and the producer's z are read once for both
        r.fdw = r.fuse && o.fuse_dw_thin && l.kh == 3 && l.cout == 8 && !l.drop_in && (l.src == SRC_PREV || l.src == SRC_CONCAT) &&
                cg == 8 && l.dw_rows >= cap_grid(std::min(B * cdiv(l.W, 32) * cdiv(l.H, 8), 512), o) &&      // (one slab per block of that launch)
                all_bt;
    }
    return 0;
}

// backward-weights of block li, as routed by r.  With r.fuse its g buffer is the masked gradient g' and the kernel applies
// the BN-backward transform of the block on load (every kernel but the generic VALU one of odd first layers can)
int conv_backward_w(oct_unet* h, int li, const BwdRoute& r, const void* x_in, int x_is_u8, int B, hipStream_t s) {
    const Layer& l = h->plan.L[li];
    const SrcDesc sd = src_of(h, li, x_in, x_is_u8);
    const DwPlan& p = r.dw;
    ConvBwdWArgs a{};
    a.x0 = sd.x0; a.ab0 = sd.ab0; a.C0 = sd.C0; a.x1 = sd.x1; a.ab1 = sd.ab1; a.C1 = sd.C1;
    a.flags = sd.flags | (l.drop_in ? F_DROP : 0);
    a.dz = l.g; a.part = l.dwp;
    a.B = B; a.H = l.H; a.W = l.W; a.Cin = l.cin; a.Cout = l.cout;
    a.tiles_x = cdiv(l.W, kTileX); a.tiles = p.tiles; a.total_tiles = B * a.tiles; a.npb = p.npb;
    a.drop = make_drop(h); a.act_bf16 = h->cfg.dtype;
    if (r.fuse) { a.zf = l.z; a.bnf = l.bn; }
    const double px = (double)B * l.H * l.W, fl = 2.0 * l.kh * l.kw * l.cin * l.cout * px;
    const int es = h->cfg.dtype ? 2 : 4;
    const double by = in_bytes(l, B, x_is_u8, es) + px * l.cout * es * (r.fuse ? 2 : 1);   // conv input once + dz once (fused: g' and z)
    const bool up = l.src == SRC_UP;
    const LaunchCtx lc{&h->opt, B, s, l.name, fl, by};
    int rc = 0;
    if (p.kind == DW_VALU && first_dw_streams(l)) {
        // streaming reduction kernel (kernels_bwd.hpp)
        const int tx = cdiv(l.W, 128), tiles = tx * cdiv(l.H, 8), total = B * tiles;
        const int grid = std::min(total, a.npb);
        a.npb = grid;
        const int bf = a.act_bf16;
        ProfScope ps(s, bf ? "conv_dw_first_k<unsigned short>" : "conv_dw_first_k<float>", l.name, fl, by);
        if (r.fuse) AT_DISPATCH(bf, (conv_dw_first_k<AT, true><<<grid, kBlock, 0, s>>>(a, tx, tiles, total)));
        else AT_DISPATCH(bf, (conv_dw_first_k<AT, false><<<grid, kBlock, 0, s>>>(a, tx, tiles, total)));
        HIP_OK(hipGetLastError());
    } else if (p.kind == DW_VALU) {
        if (r.fuse) return fail(-3, "conv_backward_w: the generic first-layer kernel does not apply the BN-backward transform");
        rc = launch_dw<3>(a, p.cic, p.coc, s, l.name, fl, by);   // other 1-channel / odd-channel first layers
    } else if (p.kind == DW_BX || p.kind == DW_BT) {
        rc = launch_dw_bf16pipe(a, p, l.kh, up, lc);
    } else {
        rc = launch_dw_f32pipe(a, p, l.kh, up, lc);
    }
    if (rc) return rc;
    queue_reduce(h, l, a.npb);
    return 0;
}

// Launch a kernel; `done`, when given, is bound to the dispatch as its own completion signal (hipExtLaunchKernelGGL's
// stopEvent).  Without one this is the plain launch.
template <typename... KA, typename... A>
void launch_signalling(void (*kernel)(KA...), dim3 grid, hipStream_t s, hipEvent_t done, A... args) {
    if (done) hipExtLaunchKernelGGL(kernel, grid, dim3(kBlock), 0, s, nullptr, done, 0, static_cast<KA>(args)...);
    else kernel<<<grid, kBlock, 0, s>>>(static_cast<KA>(args)...);
}

// finalize (and, unless the consumers apply it on load, apply) BN backward for block li: its g buffer holds masked
// gradients, stat_part the partials
// `done` (optional): an event that must complete when the block's dz inputs are final.  It is bound to the LAST kernel
// launched here as that dispatch's own completion signal instead of being recorded behind it: a recorded event is a marker
// packet of its own in the stream, and the next backward-data launch waits ~6 us for the command processor to retire it --
// on every block that forks a backward-weights kernel.  *bound = false when nothing was launched (the caller then records
// the event the ordinary way).
int bn_backward(oct_unet* h, int li, int nblk, int B, hipStream_t s, bool finalize_only, bool finalized_in_launch,
                hipEvent_t done = nullptr, bool* bound = nullptr) {
    const Layer& l = h->plan.L[li];
    if (bound) *bound = false;
    if (!finalized_in_launch && !(h->opt.timing_skip & 2 && h->drop_step > 2)) {
        BnBwdFinArgs f{};
        f.part = h->stat_part; f.nblk = nblk; f.C = l.cout; f.count = (double)B * l.H * l.W;
        f.bn = l.bn; f.gamma = h->params + l.gamma_off; f.dgamma = h->grads + l.gamma_off; f.dbeta = h->grads + l.beta_off;
        ProfScope ps(s, "bn_bwd_finalize_k", l.name, 0, (double)nblk * 2 * l.cout * 4);
        launch_signalling(bn_bwd_finalize_k, dim3(l.cout), s, finalize_only ? done : nullptr, f);
        if (bound && done && finalize_only) *bound = true;
        HIP_OK(hipGetLastError());
    }
    if (finalize_only) return 0;      // the consumers apply the transform themselves
    const size_t n4 = (size_t)B * l.H * l.W * l.cout / 4;
    const int bf = h->cfg.dtype;
    if (bf && l.cout % 8 == 0) {           // 16-byte accesses in bf16 mode
        const size_t n8 = n4 / 2;
        const int grid8 = (int)std::min<size_t>((n8 + kBlock - 1) / kBlock, 8192);
        ProfScope ps(s, "bn_bwd_apply8_bf16_k", l.name, 0, (double)n4 * 8 * 3);
        launch_signalling(bn_bwd_apply8_bf16_k, dim3(grid8), s, done, l.g, l.z, l.bn, n8, l.cout);
    } else {
        const int grid = (int)std::min<size_t>((n4 + kBlock - 1) / kBlock, 8192);
        ProfScope ps(s, bf ? "bn_bwd_apply_k<unsigned short>" : "bn_bwd_apply_k<float>", l.name, 0, (double)n4 * (bf ? 8 : 16) * 3);
        AT_DISPATCH(bf, launch_signalling(bn_bwd_apply_k<AT>, dim3(grid), s, done, l.g, l.z, l.bn, n4, l.cout));
    }
    if (bound && done) *bound = true;
    HIP_OK(hipGetLastError());
    return 0;
}

// head backward: dlogits, the head's kernel / bias gradient rows, the masked gradient of the last block and its
// statistics.  *rows = statistic partial rows it wrote; *fin = true if it finalized those statistics itself
int head_backward(oct_unet* h, const unsigned char* labels, int macro, float loss_scale, int B, hipStream_t s, int* rows, bool* fin) {
    const int nl = (int)h->plan.L.size();
    const Layer& hd = h->plan.L[nl - 1]; const Layer& last = h->plan.L[nl - 2];
    HeadBwdArgs hb{};
    hb.z = last.z; hb.bn = last.bn; hb.w = h->params + hd.w_off; hb.bias = h->params + hd.b_off;
    hb.labels = labels; hb.bc = h->dice_bc; hb.g = last.g; hb.part = h->stat_part; hb.wpart = hd.dwp;
    hb.HW = hd.H * hd.W; hb.nblk = head_nblk(hb.HW, B); hb.B = B; hb.macro = macro; hb.loss_scale = loss_scale; hb.act_bf16 = h->cfg.dtype;
    hb.focal_w = h->focal_w; hb.focal_gamma = h->focal_gamma; hb.focal_cw = h->focal_cw; hb.focal_clip_mod = h->opt.focal_clip_mod; hb.inv_count = 1.f / ((float)B * hb.HW);
    hb.bce_on = h->bce_on; hb.bce_inner = h->opt.bce_inner_eps ? kFocalEps : 0.f; hb.bce_scale = loss_scale * hb.inv_count / (float)h->cfg.n_cls;
    hb.pixw = h->pixw;
    hb.ignore = h->ignore;       // >= 0: the kernels take 1 / (counted pixels) from dice_bc instead of inv_count
    // shaped Dice: the folded per-(b, c) table of this combination, read with the macro indexing (its 1 / (B C) is folded in)
    if (h->shape_on) { hb.bc = macro ? h->shape_bcm : h->shape_bcu; hb.macro = 1; }
    const HeadRoute r = head_route(h->opt, h->cfg.n_cls, hd.cin);
    if (r == HEAD_REG && fin_ok(h, last)) { hb.fin = fin_desc(h, nl - 2, 1, B); *fin = true; }   // (only the register kernels finalize the statistics in the launch)
    *rows = B * hb.nblk;
    return launch_head_bwd(hb, r, h->cfg.n_cls, hd.cin, B, s);
}

// one backward-data launch of block li.  *rows = statistic partial rows it wrote; *fin = true if it finalized the
// producer's statistics itself
int launch_dx(oct_unet* h, int li, const DxLaunch& d, int B, hipStream_t s, int* rows, bool* fin) {
    const Layer& l = h->plan.L[li];
    const BwdRoute& r = h->route[li];
    IgemmArgs g = d.a;
    if (r.fuse) { g.gb_z = l.z; g.gb_bn = l.bn; }
    const int Cg = g.Mout;
    const double px = (double)B * l.H * l.W, pxg = (double)B * g.Ho * g.Wo;
    double fl = 2.0 * l.kh * l.kw * Cg * l.cout * px;                // algorithmic flops of the original conv's dX
    const int es = h->cfg.dtype ? 2 : 4;
    double by = px * l.cout * es * (r.fuse ? 2 : 1) + pxg * Cg * es * (d.prod ? 2 : 1);
    if (r.fdw) {
        g.dw_x = d.dw_x->z; g.dw_ab = d.dw_x->bn; g.dw_part = l.dwp; g.dw_Cin = l.cin; g.dw_ci_off = g.m_off; g.dw_bias = d.dw_bias ? 1 : 0;
        fl *= 2; if (!d.prod) by += pxg * Cg * es;                    // + the dW flops; + the X read where no mask reads it
    }
    const LaunchCtx lc{&h->opt, B, s, l.name, fl, by};
    if (d.prod && fin_ok(h, *d.prod) && d.route == ROUTE_BT) {
        g.fin = fin_desc(h, (int)(d.prod - h->plan.L.data()), 1, B); *fin = true;
    }
    if (d.up) return launch_igemm<3, A_DOWN2, EPI_MASK>(g, d.route, lc, rows);
    return d.prod ? launch_igemm<3, A_NORMAL, EPI_MASK>(g, d.route, lc, rows)
                  : launch_igemm<3, A_NORMAL, EPI_RAW>(g, d.route, lc, rows);
}

// max-pool backward in front of block li: routes the raw gradient wrt the pooled tensor into block li-1, masked, and emits
// that block's statistics.  *rows / *fin as launch_dx
int pool_backward(oct_unet* h, int li, int B, hipStream_t s, int* rows, bool* fin) {
    const Layer& l = h->plan.L[li]; const Layer& p = h->plan.L[li - 1];
    PoolBwdArgs pb{};
    pb.gp = h->gpooled[l.level - 1]; pb.z = p.z; pb.bn = p.bn; pb.g = p.g; pb.part = h->stat_part;
    pb.act_bf16 = h->cfg.dtype; pb.H = p.H; pb.W = p.W; pb.C = p.cout; pb.tiles_x = cdiv(p.W / 2, kTileX); pb.tiles = tiles_of(p.H / 2, p.W / 2);
    const int bf = h->cfg.dtype, c4 = p.cout / 4;
    const double pbytes = (double)B * p.H * p.W * p.cout * (bf ? 2 : 4) * 3.25;
    if (c4 >= 1 && c4 <= 64 && (c4 & (c4 - 1)) == 0) {     // flat, channel-contiguous mapping
        const bool v8 = bf && p.cout % 8 == 0;                               // bf16 storage: 8 channels (16 bytes) per thread
        const size_t items = (size_t)B * (p.H / 2) * (p.W / 2) * (v8 ? c4 / 2 : c4);
        const size_t cap = (size_t)B * cdiv(p.H, 2) * cdiv(p.W, kTileX);     // statistic rows carve() guarantees
        const int grid = (int)std::max<size_t>(1, std::min<size_t>(std::min<size_t>(cdiv((int)items, kBlock), 2048), cap));
        if (fin_ok(h, p)) { pb.fin = fin_desc(h, li - 1, 1, B); *fin = true; }
        ProfScope ps(s, bf ? (v8 ? "pool_bwd_flat_k<unsigned short,8>" : "pool_bwd_flat_k<unsigned short>") : "pool_bwd_flat_k<float>", p.name, 0, pbytes);
        if (v8) pool_bwd_flat_k<bf16_t, 8><<<grid, kBlock, 0, s>>>(pb, B);
        else AT_DISPATCH(bf, pool_bwd_flat_k<AT><<<grid, kBlock, 0, s>>>(pb, B));
        *rows = grid;
    } else {
        dim3 grid(pb.tiles, p.cout / 4, B);
        ProfScope ps(s, bf ? "pool_bwd_k<4,unsigned short>" : "pool_bwd_k<4,float>", p.name, 0, pbytes);
        AT_DISPATCH(bf, pool_bwd_k<4, AT><<<grid, kBlock, 0, s>>>(pb));
        *rows = B * pb.tiles;
    }
    HIP_OK(hipGetLastError());
    return 0;
}

// Fork the backward-weights launches of the blocks in `pend` to the side stream: it waits for `fe` -- dz of every pending
// block is final there; recorded on s here unless a launch already carries it -- and takes the launches.
int fork_pending_dw(oct_unet* h, std::vector<int>& pend, hipEvent_t fe, bool fe_bound, const void* x_in, int x_is_u8, int B, hipStream_t s) {
    if (!fe_bound) HIP_OK(hipEventRecord(fe, s));
    HIP_OK(hipStreamWaitEvent(h->side, fe, 0));
    for (int li : pend)
        if (int rc = conv_backward_w(h, li, h->route[li], x_in, x_is_u8, B, h->side)) return rc;
    pend.clear();
    return 0;
}

int backward_impl(oct_unet* h, const void* x_in, int x_is_u8, const unsigned char* labels, int macro, float loss_scale, hipStream_t s) {
    const Plan& pl = h->plan;
    const Options& o = h->opt;
    const int nl = (int)pl.L.size(), B = h->last_B;
    int rc = plan_backward(h, B);
    if (rc) return rc;
    // backward-data weights of every block for this step's parameters: transposed / effective fp32 kernels, then their
    // bf16 operand layouts.  Nothing needs them before the first backward-data launch, so they run on the side stream
    // under the head backward and the last block's BN backward.
    // (the per-launch profiler wants serial launches)
    const bool side_ok = o.dw_side_stream && h->side && !(t_prof && t_prof->on);
    hipStream_t ps_ = side_ok ? h->side : s;
    if (side_ok) { HIP_OK(hipEventRecord(h->fork_ev[0], s)); HIP_OK(hipStreamWaitEvent(h->side, h->fork_ev[0], 0)); }
    {
        ProfScope ps(ps_, "prep_wt_k", "all", 0, (double)h->wt_total * 8);
        prep_wt_k<<<std::min<unsigned>((h->wt_total + kBlock - 1) / kBlock, 2048u), kBlock, 0, ps_>>>(h->wt_descs, h->n_wt, h->wt_total);
        HIP_OK(hipGetLastError());
    }
    if ((rc = prep_split_weights(h, true, ps_))) return rc;
    if (side_ok) HIP_OK(hipEventRecord(h->prep_ev, h->side));
    bool prep_pending = side_ok;
    int pending_nblk = 0;                     // number of stat partial rows waiting for block (li-1)
    bool pending_fin = false;                 // the pending statistics were finalized by the launch that emitted them
    if ((rc = head_backward(h, labels, macro, loss_scale, B, s, &pending_nblk, &pending_fin))) return rc;
    std::vector<int> pend;                    // blocks whose forked backward-weights launch is not yet issued
    unsigned n_forks = 0;                     // forks so far: they rotate through the handle's events
    h->red.n = 0;
    queue_reduce(h, pl.L[nl - 1], pending_nblk);   // head kernel/bias gradient rows written by head_bwd_k

    for (int li = nl - 2; li >= 0; --li) {
        const Layer& l = pl.L[li];
        const BwdRoute& r = h->route[li];
        // g buffer of block li is complete (+ partials in stat_part).  Its backward-weights launch goes to the side stream
        // unless the backward-data launches carry it; the input layer has no backward-data launch to run beside, so its
        // kernel stays on the caller's stream: no fork, no join wait in front of the slab reduce
        const bool fork = side_ok && !r.fdw && l.src != SRC_INPUT;
        const bool tail_here = li == first_mid_layer(pl);      // every gradient from the first bottleneck conv on is queued here
        // Forked launches go to the side stream in GROUPS (dw_fork_group blocks per fork): every event the side stream waits
        // for costs the caller's stream ~6 us in front of its next launch (the dispatch that carries the completion signal
        // has to be retired by the command processor first), and a block's dz, z and record stay valid until the end of
        // the backward pass, so its backward-weights kernel may start a block or two late.
        if (fork) pend.push_back(li);
        const bool flush = !pend.empty() && (!fork || (int)pend.size() >= o.dw_fork_group || tail_here);
        hipEvent_t fe = flush ? h->fork_ev[1 + n_forks++ % (h->fork_ev.size() - 1)] : nullptr;
        bool fe_bound = false;
        rc = bn_backward(h, li, pending_nblk, B, s, r.fuse, pending_fin, (flush && o.fork_on_launch) ? fe : nullptr, &fe_bound);
        if (rc) return rc;
        pending_fin = false;
        if (flush && (rc = fork_pending_dw(h, pend, fe, fe_bound, x_in, x_is_u8, B, s))) return rc;
        if (!r.fdw && !fork && (rc = conv_backward_w(h, li, r, x_in, x_is_u8, B, s))) return rc;
        if (tail_here && (n_forks || h->tail_event)) {
            // every parameter gradient at offsets >= L[li].w_off (bottleneck, decoder, head: Keras creation order) is
            // final once the queued slabs are summed: the DP launcher all-reduces that segment on a side stream while
            // the encoder backward runs.  The sum runs on the handle's side stream, behind the backward-weights
            // kernels that write those slabs (the slabs written by launches of the caller's stream -- head, fused dX+dW --
            // are older than the fork event that stream last waited for): the caller's stream neither waits for the side
            // stream here nor carries the reduce, and the end-of-backward reduce is left with the encoder's slabs.
            hipStream_t rs = n_forks ? h->side : s;
            if ((rc = flush_reduce(h, rs))) return rc;
            if (h->tail_event) HIP_OK(hipEventRecord(h->tail_event, rs));
        }
        if (l.src == SRC_INPUT) break;
        if (prep_pending) { HIP_OK(hipStreamWaitEvent(s, h->prep_ev, 0)); prep_pending = false; }   // first backward-data launch
        int rows = 0, rows_before = 0;
        for (int i = 0; i < r.n_dx; ++i) {
            rows_before = rows;
            if ((rc = launch_dx(h, li, r.dx[i], B, s, &rows, &pending_fin))) return rc;
        }
        pending_nblk = rows;                  // of the last launch: the one that emits block li-1's statistics, if any does
        if (r.fdw) {
            if (r.n_dx == 2 && rows != rows_before) return fail(-3, "fused backward-weights: the two halves ran different grids");
            queue_reduce(h, l, rows);
        }
        if (l.src == SRC_POOL && (rc = pool_backward(h, li, B, s, &pending_nblk, &pending_fin))) return rc;
    }
    if (n_forks) { HIP_OK(hipEventRecord(h->join_ev, h->side)); HIP_OK(hipStreamWaitEvent(s, h->join_ev, 0)); }
    return flush_reduce(h, s);
}

// ---------------------------------------------------------------------------------------------------------------
// creation: the descriptor lists of the weight-preparation kernels, one entry per prepared buffer carve() handed out
// ---------------------------------------------------------------------------------------------------------------
template <typename T>
int upload(T* dst, const std::vector<T>& v, const char* what) {
    if (v.empty()) return 0;
    const hipError_t e = hipMemcpy(dst, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
    return e == hipSuccess ? 0 : fail(-5, std::string("hipMemcpy(") + what + "): " + hipGetErrorString(e));
}

// transposed / effective fp32 backward-data weights (prep_wt_k)
int build_wt_descs(oct_unet* h) {
    std::vector<WtDesc> d;
    unsigned off = 0;
    for (auto& l : h->plan.L) {
        if (!l.wt) continue;
        WtDesc w{}; w.w = h->params + l.w_off; w.wt = l.wt; w.kh = l.kh; w.cin = l.cin; w.cout = l.cout;
        w.mode = l.kh == 3 ? 0 : 1; w.start = off; w.count = 9u * l.cin * l.cout;
        off += w.count; d.push_back(w);
    }
    h->n_wt = (int)d.size(); h->wt_total = off;
    return upload(h->wt_descs, d, "wt_descs");
}

// split weights of the wide bf16-pipe kernel (prep_wbx_k): forward entries first, then backward-data entries
int build_wbx_descs(oct_unet* h) {
    std::vector<WbxDesc> d;
    const int ns = h->cfg.dtype ? 1 : 3;
    auto add = [&](const float* src, bf16_t* dst, int KH, int Kc, int M, int MB, unsigned* off) {
        WbxDesc w{}; w.src = src; w.dst = dst; w.KH = KH; w.Kc = Kc; w.M = M; w.ld = M; w.MB = MB; w.NS = ns; w.start = *off;
        w.count = (unsigned)(((Kc + 15) / 16) * ((M + MB - 1) / MB) * KH * KH * MB * 2);
        *off += w.count; d.push_back(w);
    };
    for (auto& l : h->plan.L) if (l.wbx_f) add(h->params + l.w_off, l.wbx_f, l.kh, l.cin, l.cout, bx_mb(l.cout), &h->wbx_f_total);
    h->n_wbx_f = (int)d.size();
    for (auto& l : h->plan.L) if (l.wbx_b) add(l.wt, l.wbx_b, 3, l.cout, l.cin, bx_mb(bwd_cg(l)), &h->wbx_b_total);
    h->n_wbx_b = (int)d.size() - h->n_wbx_f;
    return upload(h->wbx_descs, d, "wbx_descs");
}

// weight slices of the thin bf16-pipe kernel (prep_wbt_k): forward entries first, then backward-data entries (one per
// launch: Cg output channels at offset m_off)
int build_wbt_descs(oct_unet* h) {
    std::vector<WbtDesc> d;
    const int ns = h->cfg.dtype ? 1 : 3;
    auto add = [&](const float* src, bf16_t* dst, int KH, int Kc, int M, int m_off, bool m2, unsigned* off) {
        WbtDesc w{}; w.src = src; w.dst = dst; w.KH = KH; w.Kc = Kc; w.M = M; w.ld = M; w.m_off = m_off; w.CT = Kc; w.NS = ns; w.m2 = m2;
        w.start = *off; w.count = (unsigned)wbt_groups(KH, Kc, m2) * 64;
        *off += w.count; d.push_back(w);
    };
    for (auto& l : h->plan.L) if (l.wbt_f) add(h->params + l.w_off, l.wbt_f, l.kh, l.cin, l.cout, 0, l.bt_m2_f, &h->wbt_f_total);
    h->n_wbt_f = (int)d.size();
    for (auto& l : h->plan.L) {
        if (!l.wbt_b) continue;
        const int cg = bwd_cg(l);
        for (int sl = 0; sl < l.cin / cg; ++sl)
            add(l.wt, l.wbt_b + (size_t)sl * (wbt_bytes(3, l.cout, ns, l.bt_m2_b) / 2), 3, l.cout, l.cin, sl * cg, l.bt_m2_b, &h->wbt_b_total);
    }
    h->n_wbt_b = (int)d.size() - h->n_wbt_f;
    return upload(h->wbt_descs, d, "wbt_descs");
}

}  // namespace

// =================================================================================================================
// C ABI
// =================================================================================================================
extern "C" {

const char* oct_last_error(void) { return g_err.c_str(); }
const char* oct_version(void) { return "oct_unet_hip 0.3 (gfx950) src:" OCT_SRC_HASH; }

void oct_unet_cfg_default(oct_unet_cfg* c) {
    if (!c) return;
    memset(c, 0, sizeof *c);
    c->in_ch = 1; c->n_cls = 3; c->H = 256; c->W = 512; c->max_batch = 1;
    c->start_neurons = 8; c->pool_layers = 4; c->conv_layers = 2; c->enc_k = 3; c->dec_k = 2;
    c->dtype = 0; c->training = 0; c->bn_eps = 1e-3f; c->bn_momentum = 0.99f; c->dropout_rate = 0.5f;
    c->bn_unbiased_moving_var = 1; c->seed = 0x0C7ull;
}

int oct_unet_cfg_check(const oct_unet_cfg* c) { return check_cfg(c); }

size_t oct_unet_param_count(const oct_unet_cfg* c) { return check_cfg(c) ? 0 : build_plan(*c).n_params; }
size_t oct_unet_state_count(const oct_unet_cfg* c) { return check_cfg(c) ? 0 : build_plan(*c).n_state; }
int oct_unet_layer_count(const oct_unet_cfg* c) { return check_cfg(c) ? -1 : (int)build_plan(*c).L.size(); }

size_t oct_unet_workspace_bytes(const oct_unet_cfg* c) {
    if (check_cfg(c)) return 0;
    Plan pl = build_plan(*c);
    return carve(*c, pl, nullptr, nullptr, g_opt);
}

int oct_unet_layer_info(const oct_unet_cfg* c, int index, oct_layer_info* out) {
    if (int rc = check_cfg(c)) return rc;
    if (!out) return fail(-1, "null out");
    Plan pl = build_plan(*c);
    if (index < 0 || index >= (int)pl.L.size()) return fail(-1, "layer index out of range");
    const Layer& l = pl.L[index];
    memset(out, 0, sizeof *out);
    snprintf(out->name, sizeof out->name, "%s", l.name);
    out->kh = l.kh; out->kw = l.kw; out->cin = l.cin; out->cout = l.cout; out->has_bn = l.has_bn;
    out->out_h = l.H; out->out_w = l.W;
    out->kernel_off = l.w_off; out->bias_off = l.b_off; out->gamma_off = l.gamma_off; out->beta_off = l.beta_off;
    out->moving_mean_off = l.mm_off; out->moving_var_off = l.mv_off;
    return 0;
}

int oct_unet_create(const oct_unet_cfg* c, float* params, float* grads, float* state, void* ws, size_t ws_bytes,
                    oct_unet** out) {
    if (int rc = check_cfg(c)) return rc;
    if (!out || !params || !state || !ws) return fail(-1, "null pointer argument");
    if (c->training && !grads) return fail(-1, "training handle needs a grads buffer");
    std::unique_ptr<oct_unet, void (*)(oct_unet*)> own(new oct_unet(), oct_unet_destroy);   // every error path below frees it
    oct_unet* h = own.get();
    h->cfg = *c; h->plan = build_plan(*c); h->opt = g_opt;
    h->params = params; h->grads = grads; h->state = state;
    const size_t need = carve(*c, h->plan, nullptr, nullptr, h->opt);
    if (ws_bytes < need) return fail(-4, "workspace too small: need " + std::to_string(need) + " bytes");
    if (((uintptr_t)ws & 255) || ((uintptr_t)params & 15) || ((uintptr_t)state & 15) || (grads && ((uintptr_t)grads & 15)))
        return fail(-1, "buffers must be aligned (workspace 256 B, params/grads/state 16 B)");
    carve(*c, h->plan, h, (char*)ws, h->opt);
    h->route.resize(h->plan.L.size());
    if (c->training) if (int rc = build_wt_descs(h)) return rc;
    if (int rc = build_wbx_descs(h)) return rc;
    if (int rc = build_wbt_descs(h)) return rc;
    hipError_t e = hipMemset(h->fin_counters, 0, 2 * h->plan.L.size() * sizeof(unsigned));
    if (e != hipSuccess) return fail(-5, std::string("hipMemset(fin_counters): ") + hipGetErrorString(e));
    float lut[256];
    for (int i = 0; i < 256; ++i) lut[i] = (float)((double)i / 255.0);
    e = hipMemcpyToSymbol(HIP_SYMBOL(c_u8_lut), lut, sizeof lut);
    if (e != hipSuccess) return fail(-5, std::string("hipMemcpyToSymbol: ") + hipGetErrorString(e));
    if (c->training) {
        int lo = 0, hi = 0;
        (void)hipDeviceGetStreamPriorityRange(&lo, &hi);         // lo = numerically largest = least urgent
        if (hipStreamCreateWithPriority(&h->side, hipStreamNonBlocking, lo) != hipSuccess) h->side = nullptr;
        if (h->side) {
            h->fork_ev.resize(9);
            // the events order work between two streams of ONE device: no system-scope fence (an L2 write-back in front of
            // the next launch, which reads these layers' tensors from L2) unless asked for
            const unsigned evf = hipEventDisableTiming | (h->opt.event_sysfence ? 0u : (unsigned)hipEventDisableSystemFence);
            bool ok = hipEventCreateWithFlags(&h->join_ev, evf) == hipSuccess &&
                      hipEventCreateWithFlags(&h->prep_ev, evf) == hipSuccess;
            for (auto& e : h->fork_ev) ok = ok && hipEventCreateWithFlags(&e, evf) == hipSuccess;
            if (!ok) { (void)hipStreamDestroy(h->side); h->side = nullptr; }
        }
    }
    *out = own.release();
    return 0;
}

void oct_unet_destroy(oct_unet* h) {
    if (!h) return;
    if (t_prof == &h->prof) t_prof = nullptr;     // the handle-less entry points (oct_augment_batch, ...) consult t_prof too
    if (h->side) {
        (void)hipStreamSynchronize(h->side);
        for (auto e : h->fork_ev) if (e) (void)hipEventDestroy(e);
        if (h->join_ev) (void)hipEventDestroy(h->join_ev);
        if (h->prep_ev) (void)hipEventDestroy(h->prep_ev);
        (void)hipStreamDestroy(h->side);
    }
    if (h->shape_bcm) (void)hipFree(h->shape_bcm);
    if (h->graph_exec) (void)hipGraphExecDestroy(h->graph_exec);
    if (h->graph) (void)hipGraphDestroy(h->graph);
    delete h;
}

int oct_unet_forward(oct_unet* h, const void* x, int x_is_u8, int B, int training, const oct_unet_io* io, oct_stream_t stream) {
    if (!h || !x) return fail(-1, "null handle or input");
    if (B < 1 || B > h->cfg.max_batch) return fail(-1, "B out of range (1..max_batch)");
    if (training && !h->cfg.training) return fail(-1, "handle was created without training workspaces");
    if (training) {  // every training forward draws a fresh dropout mask; backward replays the same one
        if (h->drop_advance) ++h->drop_step;
        h->drop_advance = 1;
    }
    t_prof = &h->prof;
    const int rc = forward_impl(h, x, x_is_u8, B, training, io, (hipStream_t)stream);
    if (rc) return rc;
    h->last_x = x; h->last_u8 = x_is_u8; h->dice_final = 0;
    return 0;
}

// ---- inference: ONE chain described by oct_infer, run eagerly (oct_unet_infer) or recorded (oct_unet_graph_capture_infer) ----
// the four maps of an oct_mc_out with the bytes of a pixel of each
struct MapSet { void* p[4]; int pb[4]; };
static MapSet map_set(const oct_mc_out& o, int n_cls) {
    return {{o.mean_probs, o.argmax, o.entropy, o.mutual_info}, {n_cls * (int)sizeof(float), 1, (int)sizeof(float), (int)sizeof(float)}};
}

// What the chain's launches would refuse, with nothing launched.  (oct_pad_batch raises its own errors: it is the first launch.)
static int infer_check(oct_unet* h, const oct_infer* d) {
    if (!h || !d) return fail(-1, "infer: null handle or descriptor");
    if (d->kind != OCT_INFER_PLAIN && d->kind != OCT_INFER_MC && d->kind != OCT_INFER_TTA)
        return fail(-1, "infer: unknown kind " + std::to_string(d->kind));
    const oct_unet_cfg& c = h->cfg;
    const oct_mc_out& o = d->out;
    const bool plain = d->kind == OCT_INFER_PLAIN, padded = d->x_pad_dev != nullptr;
    if (!d->x_dev || (!plain && (!d->probs_scratch_dev || !d->ws_dev || !(o.mean_probs || o.argmax || o.entropy || o.mutual_info))))
        return fail(-1, "infer: null input, scratch, workspace or out (no map asked for)");
    if (d->B < 1 || d->B > c.max_batch) return fail(-1, "B out of range (1..max_batch)");
    if (!padded && (d->H != c.H || d->W != c.W)) return fail(-1, "infer: a size other than the handle's needs x_pad_dev");
    if (plain && (o.entropy || o.mutual_info)) return fail(-1, "infer: a plain forward has no entropy or mutual_info");
    const int T = d->T;
    if (d->kind == OCT_INFER_MC) {      // what the T reductions would refuse: the last one reads `out`
        if (T < 1 || T > 64) return fail(-1, "infer: T out of range (1..64)");
        if (int rc = mc_validate(d->probs_scratch_dev, d->B, c.H, c.W, c.n_cls, T - 1, T, d->ws_dev, d->ws_bytes, &o)) return rc;
    } else if (d->kind == OCT_INFER_TTA) {
        if (T < 1 || T > 4) return fail(-1, "infer: T out of range (1..4)");
        const void* x = padded ? d->x_pad_dev : d->x_dev;      // THE input of the views: the padded batch where there is one
        const int64_t pb = (int64_t)c.in_ch * (d->x_is_u8 ? 1 : 4);
        for (int t = 0; t < T; ++t) {
            const int v = d->views[t];
            if (v < 0 || v > 3) return fail(-1, "infer: view " + std::to_string(v) + " outside 0..3");
            if (!v) continue;
            if (!d->x_view_dev) return fail(-1, "infer: a flipped view needs x_view_dev");
            if (pb > 32) return fail(-1, "infer: a pixel of the input has more than 32 bytes");
            if (int rc = flip_validate(x, d->B, c.H, c.W, (int)pb, v, d->x_view_dev, nullptr)) return rc;
        }
        if (int rc = tta_validate(d->probs_scratch_dev, d->B, c.H, c.W, c.n_cls, d->views[T - 1], T - 1, T, d->ws_dev, d->ws_bytes, &o))
            return rc;
    }
    if (!padded) return 0;
    const MapSet from = map_set(o, c.n_cls), to = map_set(d->out_crop, c.n_cls);
    for (int i = 0; i < 4; ++i) {
        if (!to.p[i]) continue;
        if (!from.p[i]) return fail(-1, "infer: out_crop asks for a map that out does not hold");
        // the one error of oct_crop_batch that the pad in front does not raise first (a size that does not fit is the pad's)
        const uintptr_t a = (uintptr_t)from.p[i], b = (uintptr_t)to.p[i];
        const size_t px = (size_t)d->B * from.pb[i], na = px * c.H * c.W, nb = px * std::max(d->H, 0) * std::max(d->W, 0);
        if (a < b + nb && b < a + na) return fail(-1, "infer: a map of out_crop overlaps its source in out");
    }
    return 0;
}

// The chain on stream s: the pad; one weight preparation; per sample or view the flip (unless identity), the conv blocks -- for
// MC only those behind the dropout, the encoder and the bottleneck having run once --, the head and the fold; the crops.
static int infer_chain(oct_unet* h, const oct_infer& d, hipStream_t s) {
    const oct_unet_cfg& c = h->cfg;
    const bool plain = d.kind == OCT_INFER_PLAIN, mc = d.kind == OCT_INFER_MC;
    const int nl = (int)h->plan.L.size(), B = d.B, u8 = d.x_is_u8, T = plain ? 1 : d.T;
    const int k = mc ? first_dec_layer(h->plan) : 0;           // the up-convolution behind the bottleneck: the dropout sits on its input
    const void* x = d.x_dev;
    int rc = 0;
    if (d.x_pad_dev) {
        rc = oct_pad_batch(x, u8, B, d.H, d.W, c.in_ch, c.H, c.W, d.top, d.left, d.pad_mode, d.pad_value, d.x_pad_dev, s);
        x = d.x_pad_dev;
    }
    oct_unet_io io{};                                           // PLAIN: the head writes the caller's maps itself
    io.probs = plain ? d.out.mean_probs : d.probs_scratch_dev; io.argmax = plain ? d.out.argmax : nullptr;
    const unsigned long long step_saved = h->drop_step;
    if (!rc) rc = forward_prepare(h, 0, false, s);
    if (!rc) rc = forward_stages(h, x, u8, B, 0, false, false, 0, k, s);
    for (int t = 0; t < T && !rc; ++t) {
        const int v = plain || mc ? 0 : d.views[t];
        const void* xt = x;
        if (v) { rc = oct_flip_batch(x, B, c.H, c.W, c.in_ch * (u8 ? 1 : 4), v, d.x_view_dev, s); xt = d.x_view_dev; }
        if (mc) h->drop_step = d.step0 + (unsigned long long)t;                     // by value into layer k's kernel arguments
        if (!rc) rc = forward_stages(h, xt, u8, B, 0, mc, false, k, nl - 1, s);
        if (!rc) rc = forward_head(h, B, &io, s);
        if (!rc && mc) rc = oct_mc_update(io.probs, B, c.H, c.W, c.n_cls, t, T, d.ws_dev, d.ws_bytes, &d.out, s);
        if (!rc && !mc && !plain) rc = oct_tta_update(io.probs, B, c.H, c.W, c.n_cls, v, t, T, d.ws_dev, d.ws_bytes, &d.out, s);
    }
    h->drop_step = step_saved;
    if (!plain) { h->have_dice = 0; h->dice_final = 0; }       // a pending Dice sum is dropped
    else if (!rc) { h->last_B = B; h->last_training = 0; }     // as forward_impl leaves the handle
    if (d.x_pad_dev) {
        const MapSet from = map_set(d.out, c.n_cls), to = map_set(d.out_crop, c.n_cls);
        for (int i = 0; i < 4 && !rc; ++i)
            if (to.p[i]) {
                // oct_crop_batch takes pixels of up to 32 bytes: the probabilities of more than 8 classes go as n_cls 4-byte
                // pixels each (the kernel moves a row's bytes; a pixel is only what `left` and the widths count in)
                const int k = to.pb[i] > 32 ? to.pb[i] / 4 : 1;
                rc = oct_crop_batch(from.p[i], B, c.H, c.W * k, to.pb[i] / k, d.H, d.W * k, d.top, d.left * k, to.p[i], s);
            }
    }
    return rc;
}

int oct_unet_infer(oct_unet* h, const oct_infer* d, oct_stream_t stream) {
    if (int rc = infer_check(h, d)) return rc;
    t_prof = &h->prof;
    return infer_chain(h, *d, (hipStream_t)stream);
}

// Dice (and focal) loss of the last forward: out holds n_user floats
static int loss_finalize(oct_unet* h, const char* what, float smooth, float* out, int n_user, oct_stream_t stream) {
    if (!h) return fail(-1, "null handle");
    if (!h->have_dice) return fail(-1, std::string(what) + " needs a preceding forward with io.labels");
    DiceFinArgs a{};
    a.part = h->dice_part; a.B = h->last_B; a.C = h->cfg.n_cls; a.nblk = head_nblk(h->cfg.H * h->cfg.W, h->last_B);
    a.N = dice_n(a.C); a.smooth = smooth; a.out4 = h->loss4; a.out4_user = out; a.bc = h->dice_bc;
    a.n_user = n_user; a.inv_count = 1.0 / ((double)h->last_B * h->cfg.H * h->cfg.W); a.focal_w = h->focal_w; a.bce_on = h->bce_on;
    a.masked = h->ignore >= 0;
    t_prof = &h->prof;
    if (h->shape_on) {
        DiceShapeArgs sa{};
        sa.f = a; sa.alpha = h->shape_alpha; sa.beta = h->shape_beta; sa.gamma = h->shape_gamma; sa.wmode = h->shape_wmode;
        sa.cw = h->shape_cw; sa.bcm = h->shape_bcm; sa.bcu = h->shape_bcu; sa.tab = h->shape_tab;
        ProfScope ps((hipStream_t)stream, "dice_shape_finalize_k", "loss", 0, (double)a.B * a.nblk * a.N * 4);
        dice_shape_finalize_k<<<1, kBlock, 0, (hipStream_t)stream>>>(sa);
    } else {
        ProfScope ps((hipStream_t)stream, "dice_finalize_k", "loss", 0, (double)a.B * a.nblk * a.N * 4);
        dice_finalize_k<<<1, kBlock, 0, (hipStream_t)stream>>>(a);
    }
    HIP_OK(hipGetLastError());
    h->dice_final = 1;
    return 0;
}

int oct_unet_loss_dice(oct_unet* h, float smooth, float* out4, oct_stream_t stream) { return loss_finalize(h, "loss_dice", smooth, out4, 4, stream); }
int oct_unet_loss_focal_dice(oct_unet* h, float smooth, float* out8, oct_stream_t stream) { return loss_finalize(h, "loss_focal_dice", smooth, out8, 8, stream); }
int oct_unet_loss_bce_dice(oct_unet* h, float smooth, float* out8, oct_stream_t stream) { return loss_finalize(h, "loss_bce_dice", smooth, out8, 8, stream); }

int oct_unet_set_focal_dice(oct_unet* h, float focal_loss_weight, float gamma, const float* class_weight_dev) {
    if (!h) return fail(-1, "null handle");
    if (!(focal_loss_weight >= 0.f && focal_loss_weight <= 1.f) || !(gamma >= 0.f)) return fail(-1, "focal_dice: weight must be in [0,1], gamma >= 0");
    h->focal_w = focal_loss_weight; h->focal_gamma = gamma; h->focal_cw = class_weight_dev;
    if (focal_loss_weight > 0.f) h->bce_on = 0;     // the two share one slot of the Dice partial rows
    return 0;
}

int oct_unet_set_bce_dice(oct_unet* h, int on) {
    if (!h) return fail(-1, "null handle");
    h->bce_on = on != 0;
    if (h->bce_on) h->focal_w = 0.f;
    return 0;
}

int oct_unet_set_ignore_label(oct_unet* h, int label) {
    if (!h) return fail(-1, "null handle");
    if (label != -1 && (label < h->cfg.n_cls || label > 255))
        return fail(-1, "ignore label must be -1 (none) or in n_classes..255: got " + std::to_string(label));
    if (label != h->ignore) { h->have_dice = 0; h->dice_final = 0; }    // sums of a forward under the other setting are not this loss's
    h->ignore = label;
    return 0;
}

int oct_unet_set_pixel_weights(oct_unet* h, const float* weights_dev) {
    if (!h) return fail(-1, "null handle");
    if ((uintptr_t)weights_dev % 4) return fail(-1, "pixel weights must be 4-byte aligned");
    if (weights_dev != h->pixw) { h->have_dice = 0; h->dice_final = 0; }    // sums of a forward under the other setting are not this loss's
    h->pixw = weights_dev;
    return 0;
}

int oct_unet_set_dice_shape(oct_unet* h, const oct_dice_shape* s) {
    if (!h) return fail(-1, "null handle");
    oct_dice_shape d{0.5f, 0.5f, 1.f, 0, nullptr};
    if (s) d = *s;
    if (!(d.alpha >= 0.f) || !(d.beta >= 0.f) || !(d.alpha + d.beta > 0.f) || !std::isfinite(d.alpha) || !std::isfinite(d.beta))
        return fail(-1, "dice_shape: alpha, beta must be finite and >= 0 with alpha + beta > 0");
    if (!(d.gamma > 0.f && d.gamma <= 8.f)) return fail(-1, "dice_shape: gamma must be in (0, 8]");
    if (d.weight_mode < 0 || d.weight_mode > 2) return fail(-1, "dice_shape: weight_mode must be 0 (none), 1 (class_weight_dev) or 2 (volume)");
    if (d.weight_mode == 1) {
        if (!d.class_weight_dev) return fail(-1, "dice_shape: weight_mode 1 needs class_weight_dev");
        float w[16]; bool any = false;                 // the setter is no hot path: read the weights back once
        HIP_OK(hipMemcpy(w, d.class_weight_dev, sizeof(float) * h->cfg.n_cls, hipMemcpyDeviceToHost));
        for (int c = 0; c < h->cfg.n_cls; ++c) {
            if (!(w[c] >= 0.f) || !std::isfinite(w[c])) return fail(-1, "dice_shape: class weights must be finite and >= 0");
            any = any || w[c] > 0.f;
        }
        if (!any) return fail(-1, "dice_shape: class weights must not all be zero");
    }
    const bool on = !(d.alpha == 0.5f && d.beta == 0.5f && d.gamma == 1.f && d.weight_mode == 0);
    if (on && !h->shape_bcm) {
        const size_t pairs = (size_t)h->cfg.max_batch * h->cfg.n_cls, bc_n = 2 * pairs + 3;
        void* p = nullptr;
        HIP_OK(hipMalloc(&p, (2 * bc_n + 3 * pairs) * sizeof(double)));
        h->shape_bcm = (double*)p; h->shape_bcu = h->shape_bcm + bc_n; h->shape_tab = h->shape_bcm + 2 * bc_n;
    }
    h->have_dice = 0; h->dice_final = 0;               // sums finalized under the other setting are not this loss's
    h->shape_alpha = d.alpha; h->shape_beta = d.beta; h->shape_gamma = d.gamma; h->shape_wmode = d.weight_mode;
    h->shape_cw = d.weight_mode == 1 ? d.class_weight_dev : nullptr;
    h->shape_on = on;
    return 0;
}

int oct_unet_backward(oct_unet* h, const unsigned char* labels, int macro, float loss_scale, oct_stream_t stream) {
    if (!h || !labels) return fail(-1, "null handle or labels");
    if (!h->last_training || !h->have_dice || !h->dice_final)
        return fail(-1, "backward needs a training forward with io.labels followed by oct_unet_loss_dice");
    if (h->bce_on && macro) return fail(-1, "bce_dice_loss is defined with dice_loss_micro only: macro must be 0");
    t_prof = &h->prof;
    const int rc = backward_impl(h, h->last_x, h->last_u8, labels, macro, loss_scale, (hipStream_t)stream);
    if (rc && h->side && h->join_ev) {
        // an error part-way: work may have been forked to the internal side stream -- join it to the caller's stream before
        // returning, so that the caller's stream order covers everything this call launched
        const std::string msg = oct_last_error();
        if (hipEventRecord(h->join_ev, h->side) == hipSuccess) (void)hipStreamWaitEvent((hipStream_t)stream, h->join_ev, 0);
        fail(rc, msg);
    }
    return rc;
}

int oct_adam_step(float* p, const float* g, float* m, float* v, size_t n, float lr, float b1, float b2, float eps,
                  long step, oct_stream_t stream) {
    if (!p || !g || !m || !v || step < 1) return fail(-1, "adam: bad arguments");
    const double lr_t = (double)lr * std::sqrt(1.0 - std::pow((double)b2, (double)step)) / (1.0 - std::pow((double)b1, (double)step));
    const int grid = (int)std::min<size_t>((n + kBlock - 1) / kBlock, 4096);
    adam_k<<<grid, kBlock, 0, (hipStream_t)stream>>>(p, g, m, v, n, (float)lr_t, b1, b2, eps);
    HIP_OK(hipGetLastError());
    return 0;
}

int oct_sgd_step(float* p, const float* g, float* mom, size_t n, float lr, float momentum, oct_stream_t stream) {
    if (!p || !g) return fail(-1, "sgd: bad arguments");
    const int grid = (int)std::min<size_t>((n + kBlock - 1) / kBlock, 4096);
    sgd_k<<<grid, kBlock, 0, (hipStream_t)stream>>>(p, g, mom, n, lr, momentum);
    HIP_OK(hipGetLastError());
    return 0;
}

int oct_unet_set_dropout_step(oct_unet* h, unsigned long long step) {
    if (!h) return fail(-1, "null handle");
    h->drop_step = step; h->drop_advance = 0;
    return 0;
}

int oct_unet_dropout_mask(oct_unet* h, int B, unsigned char* mask, oct_stream_t stream) {
    if (!h || !mask) return fail(-1, "null argument");
    const int P = h->cfg.pool_layers;
    const size_t n = (size_t)B * (h->cfg.H >> P) * (h->cfg.W >> P) * ((size_t)h->cfg.start_neurons << P);
    dropout_mask_k<<<(int)std::min<size_t>((n + 255) / 256, 4096), 256, 0, (hipStream_t)stream>>>(mask, n, make_drop(h));
    HIP_OK(hipGetLastError());
    return 0;
}

int oct_unet_graph_capture_infer(oct_unet* h, const oct_infer* d, oct_stream_t stream) {
    if (int rc = infer_check(h, d)) return rc;
    if (d->kind == OCT_INFER_MC)
        return fail(-1, "graph_capture_infer: a Monte-Carlo chain cannot be captured: the dropout step travels by value in the "
                        "kernel arguments, so a replay would repeat the captured steps");
    hipStream_t s = (hipStream_t)stream;
    if (!s) return fail(-1, "graph capture needs a non-default stream");
    if (h->graph_exec) { (void)hipGraphExecDestroy(h->graph_exec); h->graph_exec = nullptr; }
    if (h->graph) { (void)hipGraphDestroy(h->graph); h->graph = nullptr; }
    t_prof = nullptr;  // no event records inside a capture
    HIP_OK(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
    const int rc = infer_chain(h, *d, s);
    const std::string msg = rc ? oct_last_error() : "";        // the body's message, not that of the capture's end
    hipError_t e = hipStreamEndCapture(s, &h->graph);
    if (rc) return fail(rc, msg);
    if (e != hipSuccess) return fail(-5, std::string("hipStreamEndCapture: ") + hipGetErrorString(e));
    HIP_OK(hipGraphInstantiate(&h->graph_exec, h->graph, nullptr, nullptr, 0));
    return 0;
}

int oct_unet_graph_launch(oct_unet* h, oct_stream_t stream) {
    if (!h || !h->graph_exec) return fail(-1, "no captured graph");
    HIP_OK(hipGraphLaunch(h->graph_exec, (hipStream_t)stream));
    return 0;
}

int oct_unet_set_tail_event(oct_unet* h, void* hip_event) {
    if (!h) return fail(-1, "null handle");
    h->tail_event = (hipEvent_t)hip_event;
    return 0;
}

size_t oct_unet_grad_tail_offset(const oct_unet_cfg* c) {
    if (check_cfg(c)) return 0;
    const Plan pl = build_plan(*c);
    return pl.L[first_mid_layer(pl)].w_off;
}

int oct_unet_profile_begin(oct_unet* h) {
    if (!h) return fail(-1, "null handle");
    for (auto& r : h->prof.recs) { h->prof.pool.push_back(r.e0); h->prof.pool.push_back(r.e1); }
    h->prof.recs.clear();
    h->prof.on = true;
    return 0;
}

int oct_unet_profile_end(oct_unet* h, oct_profile_entry* out, int max_entries, int* n_out) {
    if (!h || !n_out) return fail(-1, "null argument");
    h->prof.on = false;
    HIP_OK(hipDeviceSynchronize());
    std::vector<oct_profile_entry> agg;
    for (auto& r : h->prof.recs) {
        float ms = 0.f;
        HIP_OK(hipEventElapsedTime(&ms, r.e0, r.e1));
        oct_profile_entry* e = nullptr;
        for (auto& a : agg) if (r.kernel == a.kernel && r.layer == a.layer) { e = &a; break; }
        if (!e) {
            oct_profile_entry n{}; snprintf(n.kernel, sizeof n.kernel, "%s", r.kernel.c_str());
            snprintf(n.layer, sizeof n.layer, "%s", r.layer.c_str());
            agg.push_back(n); e = &agg.back();
        }
        e->launches += 1; e->total_ms += ms; e->flops += r.flops; e->bytes += r.bytes;
    }
    *n_out = (int)agg.size();
    for (int i = 0; i < (int)agg.size() && i < max_entries && out; ++i) out[i] = agg[i];
    return 0;
}

int oct_boundary_maps(const unsigned char* labels, int B, int H, int W, int n_cls, int bg_ilm, int bg_csi,
                      unsigned char* maps, oct_stream_t stream) {
    if (!labels || !maps || B < 1 || H < 1 || W < 1 || n_cls < 2) return fail(-1, "boundary_maps: bad arguments");
    const size_t n = (size_t)B * H * W;
    boundary_maps_k<<<(int)std::min<size_t>((n + kBlock - 1) / kBlock, 8192), kBlock, 0, (hipStream_t)stream>>>(
        labels, maps, B, H, W, n_cls, bg_ilm, bg_csi);
    HIP_OK(hipGetLastError());
    return 0;
}

namespace {
struct Opt { const char* name; int Options::*var; int lo, hi; };     // values are clamped to [lo, hi]
const Opt k_opts[] = {
    {"igemm_persistent_min_tiles", &Options::persist_min_tiles, 1, 1 << 30}, {"dw32_blocks", &Options::dw32_blocks, 64, 1 << 20},
    {"dw16_blocks", &Options::dw16_blocks, 64, 1 << 20}, {"igemm_persistent_blocks", &Options::igemm_p_blocks, 8, 1 << 20},
    {"igemm_min_blocks", &Options::igemm_min_blocks, 1, 1 << 30}, {"dwpair8_enable", &Options::dwpair8, 0, 1},
    {"pair8_geometry", &Options::pair_geo, 111, 221}, {"pair8_min_tiles", &Options::pair_min_tiles, 1, 1 << 30},
    {"thin8_min_tiles", &Options::thin_min_tiles, 1, 1 << 30}, {"focal_clip_modulation", &Options::focal_clip_mod, 0, 1},
    {"bce_inner_eps", &Options::bce_inner_eps, 0, 1}, {"head_wide", &Options::head_wide, 0, 1},
    {"mfma_mode", &Options::mfma_mode, 0, 1}, {"bx_min_blocks", &Options::bx_min_blocks, 1, 1 << 30},
    {"dwbx_blocks", &Options::dwbx_blocks, 8, 1 << 20}, {"bt_blocks_per_cu", &Options::bt_blocks_per_cu, 0, 8},
    {"dwbt_f32_all", &Options::dwbt_f32_all, 0, 1}, {"bt_m2", &Options::bt_m2, 0, 1},
    {"fuse_first_apply", &Options::fuse_first_apply, 0, 1}, {"fuse_bn_apply", &Options::fuse_bn_apply, 0, 1},
    {"fuse_bn_finalize", &Options::fuse_bn_finalize, 0, 1}, {"bx_waves", &Options::bx_waves, 4, 8},
    {"dw_side_stream", &Options::dw_side_stream, 0, 1}, {"timing_skip", &Options::timing_skip, 0, 255}, {"fuse_dw_thin", &Options::fuse_dw_thin, 0, 1},
    {"dwbx_enable", &Options::dwbx_enable, 0, 1}, {"persistent_max_blocks", &Options::max_blocks, 0, 1 << 20},
    {"bx_two_blocks", &Options::bx_two_blocks, 0, 1}, {"fork_on_launch", &Options::fork_on_launch, 0, 1},
    {"event_sysfence", &Options::event_sysfence, 0, 1}, {"dw_fork_group", &Options::dw_fork_group, 1, 8}, {"fuse_bn_apply16", &Options::fuse_bn_apply16, 0, 1},
    {"pool_in_epilogue", &Options::pool_in_epilogue, 0, 1}, {"bx_down2_ring", &Options::bx_down2_ring, 0, 1},
    {"ordered_float4", &Options::ordered_float4, 0, 1},
};
const Opt* find_opt(const char* name) {
    for (const Opt& o : k_opts) if (!strcmp(name, o.name)) return &o;
    fail(-1, std::string("unknown option: ") + name);
    return nullptr;
}
int check_opt(const char* name, int value) {     // the options whose valid values are not a clamped range
    if (!strcmp(name, "pair8_geometry") && value != 221 && value != 111) return fail(-1, "pair8_geometry must be 221 or 111");
    if (!strcmp(name, "bx_waves") && value != 4 && value != 8) return fail(-1, "bx_waves must be 4 or 8");
    if (!strcmp(name, "persistent_max_blocks") && (value < 0 || value > (1 << 20))) return fail(-1, "persistent_max_blocks must be 0 (no cap) .. 1048576");
    return 0;
}
int get_opt(const Options& from, const char* name, int* value) {
    const Opt* o = find_opt(name);
    if (o) *value = from.*o->var;
    return o ? 0 : -1;
}
int set_opt(Options& to, const char* name, int value) {
    if (int rc = check_opt(name, value)) return rc;
    const Opt* o = find_opt(name);
    if (o) to.*o->var = value < o->lo ? o->lo : (value > o->hi ? o->hi : value);
    return o ? 0 : -1;
}
}  // namespace

int oct_get_option(const char* name, int* value) {
    if (!name || !value) return fail(-1, "null argument");
    return get_opt(g_opt, name, value);
}

int oct_set_option(const char* name, int value) {
    if (!name) return fail(-1, "null option name");
    return set_opt(g_opt, name, value);
}

int oct_unet_get_option(const oct_unet* h, const char* name, int* value) {
    if (!h || !name || !value) return fail(-1, "null argument");
    return get_opt(h->opt, name, value);
}

int oct_unet_set_option(oct_unet* h, const char* name, int value) {
    if (!h || !name) return fail(-1, "null argument");
    if (!strcmp(name, "bt_m2")) return fail(-1, "bt_m2 shapes the prepared weights: set the default before oct_unet_create");
    return set_opt(h->opt, name, value);
}

int oct_unet_debug_layer_fused(const oct_unet* h, int layer) {
    if (!h || layer < 0 || layer >= (int)h->plan.L.size()) return -1;
    return h->route[layer].fuse ? 1 : 0;
}

const void* oct_unet_debug_activation(oct_unet* h, int layer, int which) {
    if (!h || layer < 0 || layer >= (int)h->plan.L.size()) return nullptr;
    const Layer& l = h->plan.L[layer];
    return which == 0 ? (const void*)l.z : which == 1 ? (const void*)l.g : which == 2 ? (const void*)l.bn : nullptr;
}

}  // extern "C"
