"""Shared by tests/test_tile_walk.py (CPU) and tests/test_gpu_tile_walk.py (GPU): not a test module.

(a) ``walk`` / ``next_org`` restate ``TileWalk`` of csrc/kernels_igemm.hpp in plain Python and ``regime`` classifies a
    launch by it (blocks without a tile, unequal tile counts, banded or strided).  They exist to CLASSIFY the GPU cases, not
    to prove the kernel: the kernels are judged on the GPU, per element, by tests/layer_local.py.
(b) ``launch_model`` restates the host's routing rules (which kernel family, pixel tile and grid every launch of a step
    has); the GPU module asserts it against the step's profile, the CPU module checks its option defaults against the
    library and classifies every GPU case with it.
(c) The GPU module's inputs and cases: SCANS, ROUTES, PURPOSE / CASES_A, CASES_WIDE."""
import collections

from oracle import unet_numpy as on

NX = 8          # XCDs: the bands of the walk
CAPS = (8, 12, 16, 256, 512, 768, 1024, 1280, 1536)     # the test caps and every built-in grid cap


def _block(total, grid, blk, banded=True):
    """(tl0, tlend, step) of block ``blk``: TileWalk::init, both branches.  ``banded=False``: the kernels that stride by
    their grid whatever it is (conv_first_fwd_k, conv_dw_first_k, the conv_dw*_k family)."""
    if banded and grid % NX == 0:
        xcd, chunk = blk % NX, (total + NX - 1) // NX
        return xcd * chunk + blk // NX, min((xcd + 1) * chunk, total), grid // NX
    return blk, total, grid


def walk(total, grid, banded=True):
    """The tiles each of ``grid`` blocks visits, in order, out of ``total``: a list of tile lists per block.

    Restates TileWalk::init of csrc/kernels_igemm.hpp (grid % 8 == 0: the sequence is cut into 8 bands of
    ceil(total / 8) tiles, block i serves band i % 8 from tile i / 8 of it in steps of grid / 8; otherwise blocks stride the
    whole sequence by the grid) and the loop ``for (tl = tl0; tl < tlend; tl += step)`` every walker runs.  It exists to
    classify the GPU cases, not to prove the kernel."""
    out = []
    for blk in range(grid):
        tl0, tlend, step = _block(total, grid, blk, banded)
        out.append(list(range(tl0, tlend, step)))
    return out


Regime = collections.namedtuple("Regime", "idle tmin tmax banded")


def regime(total, grid, banded=True):
    """Blocks without a tile, and the fewest and most tiles of the blocks that have one; ``banded``: the walk cut the
    sequence into bands (else every block strides the whole sequence)."""
    n = [len(t) for t in walk(total, grid, banded)]
    busy = [k for k in n if k]
    return Regime(n.count(0), min(busy), max(busy), bool(banded and grid % NX == 0))


def uneven_band(total, grid):
    """A banded walk in which the blocks of ONE band that have a tile have unequal counts (the band's tile count is no
    multiple of its block count: next() runs a different number of times per block)."""
    if grid % NX:
        return False
    w = walk(total, grid)
    for xcd in range(NX):
        n = {len(w[blk]) for blk in range(xcd, grid, NX) if w[blk]}
        if len(n) > 1:
            return True
    return False


def crosses_image(total, grid, tiles, banded=True):
    """Some block visits tiles of more than one image (``tiles`` per image)."""
    return any(len({t // tiles for t in blk}) > 1 for blk in walk(total, grid, banded))


def next_org(o, step, tiles, tiles_x):
    """TileWalk::next on (b, ty, tx): the decomposed stride with two carries."""
    tiles_y = tiles // tiles_x
    sb, sy, sx = step // tiles, (step % tiles) // tiles_x, step % tiles_x
    b, ty, tx = o
    tx += sx; carry = 0
    if tx >= tiles_x:
        tx -= tiles_x; carry = 1
    ty += sy + carry; carry = 0
    if ty >= tiles_y:
        ty -= tiles_y; carry = 1
    return b + sb + carry, ty, tx



C = 3
ENGINE_SEED, DROP_STEP, ROLL = 5, 3, 5
# key: (B, H, W, start_neurons, pool_layers, scan seed).  Seeds: the first of 31, 32, ... for which the reference alone
# (tests/test_tile_walk.py: the layer-local model on a defect-free engine's tensors, fp32 and bf16) reports no failure and
# excludes nothing at the two small shapes, 0 of 8.7e6 elements at 344x192 and 4 of 3.9e7 at 688x384 (cap 1e-5 of them).
SCANS = {"small": (3, 40, 96, 8, 2, 31), "wide32": (3, 32, 64, 32, 1, 32),
         "344x192": (1, 344, 192, 8, 2, 31), "688x384": (1, 688, 384, 8, 3, 31)}

# ---- the host's routing rules, restated (csrc/host.hpp pipe_fit, oct_unet.hip conv_route / dw_plan / plan_backward,
# launch_conv.hpp launch_igemm) so that a case knows which kernel family, pixel tile and grid each launch must have had ----

DEFAULTS = dict(mfma_mode=1, persistent=0, thin8=0, pair8=0, pair8_geometry=221, dwpair8_enable=1, dwbx_enable=1,
                dwbx_blocks=256, dw32_blocks=512, dw16_blocks=768, igemm_persistent_blocks=1280, igemm_min_blocks=512,
                bt_blocks_per_cu=0, fuse_bn_finalize=0)
# the library's own defaults of the options the model reads or takes for granted (tests/test_tile_walk.py holds them to it)
LIBRARY_DEFAULTS = dict(mfma_mode=1, igemm_persistent_min_tiles=2048, thin8_min_tiles=2048, pair8_min_tiles=2048, pair8_geometry=221,
                        dwpair8_enable=1, dwbx_enable=1, dwbx_blocks=256, dw32_blocks=512, dw16_blocks=768, igemm_persistent_blocks=1280,
                        igemm_min_blocks=512, bt_blocks_per_cu=0, fuse_bn_finalize=0, fuse_dw_thin=1, fuse_bn_apply=1,
                        dwbt_f32_all=0, persistent_max_blocks=0)
# routes of case A: option name -> value as oct_set_option takes them
ROUTES = {
    "default": {},
    "persistent": dict(mfma_mode=0, igemm_persistent_min_tiles=1),
    "thin8": dict(mfma_mode=0, thin8_min_tiles=1),
    "pair8_221": dict(mfma_mode=0, pair8_min_tiles=1, thin8_min_tiles=1, pair8_geometry=221),
    "pair8_111": dict(mfma_mode=0, pair8_min_tiles=1, thin8_min_tiles=1, pair8_geometry=111),
    "dw16_padded": dict(mfma_mode=0, dwpair8_enable=0),
}
WALKERS = ("conv_bt_k", "conv_igemm_p_k", "conv_thin8_k", "conv_pair8_k")        # TileWalk: banded when grid % 8 == 0
STRIDERS = ("conv_first_fwd_k", "conv_dw_first_k", "conv_bwd_w_k", "conv_dw16_k", "conv_dwpair8_k", "conv_dw32_k", "conv_dwbt_k",
            "conv_dwbx_k")


def _cdiv(a, b):
    return (a + b - 1) // b


def _model_opts(opts):
    o = dict(DEFAULTS)
    for k, v in opts.items():
        if k.endswith("_min_tiles"):
            o[{"igemm_persistent_min_tiles": "persistent", "thin8_min_tiles": "thin8", "pair8_min_tiles": "pair8"}[k]] = int(v == 1)
        elif k in o:
            o[k] = v
    return o


def _pipe_fit(K, M, two, C0, down2):
    if two and C0 % 8:
        return None
    if M <= 16 and M % 4 == 0 and K in (8, 16, 32) and (not down2 or K == 8):
        return "conv_bt_k"
    if M % 32 == 0 and K % 8 == 0 and K <= (256 if down2 else 512):
        return "conv_bx_k"
    return None


def _conv_family(K, M, kh, amode, two, C0, drop, o):
    f = _pipe_fit(K, M, two, C0, amode == "down2")
    if o["mfma_mode"] and f == "conv_bt_k" and not drop:
        return f
    if o["mfma_mode"] and f == "conv_bx_k":
        return f
    if amode == "normal" and kh == 3 and M == 8 and K <= 16 and o["pair8"]:
        return "conv_pair8_k"
    if amode != "down2" and M == 8 and K <= 16 and o["thin8"]:
        return "conv_thin8_k"
    if amode != "down2" and K <= 16 and M <= 16 and o["persistent"]:
        return "conv_igemm_p_k"
    return "conv_igemm_k"


def _tile(fam, o):
    if fam == "conv_thin8_k":
        return 8, 64
    if fam == "conv_pair8_k":
        g = o["pair8_geometry"]
        return 4 * (g % 10) * (g // 100), 32 * (g // 10 % 10)
    if fam in ("conv_first_fwd_k", "conv_dw_first_k"):
        return 8, 128
    return 8, 32


def _igemm_th(B, ho, wo, M, o):
    """Pixel-tile height of the tile-per-block fp32-pipe kernel (launch_igemm): the taller tile only if that still yields
    igemm_min_blocks blocks."""
    blocks = lambda th, mb: B * _cdiv(ho, th) * _cdiv(wo, 32) * _cdiv(M, mb)
    if M <= 16:
        return 8 if blocks(8, 16) >= o["igemm_min_blocks"] else 4
    if M <= 32:
        return 8 if blocks(8, 32) >= o["igemm_min_blocks"] else 4
    return 4 if blocks(4, 64) >= o["igemm_min_blocks"] else 2


def _builtin_cap(fam, K, fdw, o):
    if fam == "conv_bt_k":
        per_cu = 2 if fdw else {32: 1, 16: 2, 8: 3}[K]
        return 256 * (min(o["bt_blocks_per_cu"], per_cu) if o["bt_blocks_per_cu"] else per_cu)
    return {"conv_igemm_p_k": o["igemm_persistent_blocks"], "conv_thin8_k": 1536, "conv_first_fwd_k": 2048}.get(fam, 1 << 30)


class Launch:
    """One modelled launch: kernel family, layer (as the profile names it), what it is ("fwd", "dx", "dx+dw", "dw"), its
    pixel-tile count and grid, and the BN layer whose statistic rows it emits (None: none, or a non-walking kernel)."""

    def __init__(self, fam, layer, kind, B, H, W, th, tw, grid_cap, stats_for=None):
        self.fam, self.layer, self.kind, self.stats_for, self.th = fam, layer, kind, stats_for, th
        self.tiles = _cdiv(H, th) * _cdiv(W, tw)
        self.total = B * self.tiles
        self.walks = fam in WALKERS or fam in STRIDERS
        self.banded = fam in WALKERS
        self.grid = min(self.total, grid_cap) if self.walks else self.total

    def flags(self):
        if not self.walks:
            return set()
        r = regime(self.total, self.grid, self.banded)
        f = set()
        if r.idle:
            f.add("idle")
        if self.banded and uneven_band(self.total, self.grid):
            f.add("uneven")
        if self.banded and not r.banded and r.tmax >= 3:
            f.add("unbanded3")
        if r.tmax > 1:
            f.add("multi")
        if r.tmax != r.tmin:
            f.add("unequal")
        if crosses_image(self.total, self.grid, self.tiles, self.banded):
            f.add("crossing")
        return f

    def __repr__(self):
        return f"{self.fam}@{self.layer}[{self.kind}] {self.total} tiles on {self.grid} blocks {sorted(self.flags())}"


def _dwbt_ok(sp, two_c0):
    if sp.src in ("input", "head") or sp.kh == 1 or not sp.has_bn:
        return False
    if sp.src == "up":
        return (sp.cin, sp.cout) in ((16, 8), (32, 16))
    if sp.src == "concat" and two_c0 % 8:
        return False
    return (sp.cin, sp.cout) in ((8, 8), (8, 16), (16, 8), (16, 16), (16, 32), (32, 16))


def launch_model(cfg, B, H, W, bf16, opts, cap, training=True):
    """The conv and backward-weights launches of one step under ``opts`` (oct_set_option names) and the grid cap
    ``cap`` (0 = none): (launches, set of layers whose backward-weights ride in their conv_bt_k backward-data launches,
    expected bytes of the slab reduce)."""
    o = _model_opts(opts)
    big = cap if cap else 1 << 30
    plan = on.build_plan(cfg)
    nb = len(plan) - 1
    drop_li = [sp.name for sp in plan].index(f"mid.conv{cfg.conv_layers - 1}") + 1       # the layer that reads the dropped tensor
    dims = lambda sp: (H >> sp.level, W >> sp.level)
    out = []
    for li, sp in enumerate(plan[:nb]):
        h, w = dims(sp)
        if sp.src == "input":
            fam = "conv_first_fwd_k" if (sp.cin, sp.cout) == (1, 8) else "conv_fwd_k"      # (other first layers: tile per block)
        else:
            fam = _conv_family(sp.cin, sp.cout, sp.kh, "upf" if sp.src == "up" else "normal", sp.src == "concat", sp.cin // 2,
                               training and li == drop_li, o)
        th, tw = _tile(fam, o)
        if fam == "conv_igemm_k":
            th = _igemm_th(B, h, w, sp.cout, o)
        out.append(Launch(fam, sp.name, "fwd", B, h, w, th, tw, min(big, _builtin_cap(fam, sp.cin, False, o)), stats_for=sp.name))
    if not training:
        return out, set(), 0
    fdw_layers, reduce_bytes = set(), 0
    hd = plan[nb]
    reduce_bytes += B * max(1, min(_cdiv(H * W, 256), _cdiv(2048, B))) * (hd.cin * hd.cout + hd.cout) * 4
    for li in range(nb - 1, -1, -1):
        sp = plan[li]
        h, w = dims(sp)
        stride = sp.kh * sp.kw * sp.cin * sp.cout + sp.cout
        # backward-data launches (K = the layer's output channels, M = the channels of the input slice)
        dx = []
        if sp.src != "input":
            p = plan[li - 1]
            if sp.src == "prev":
                dx = [(p.cout, "normal", h, w, p.name)]
            elif sp.src == "pool":
                dx = [(sp.cin, "normal", h, w, None)]
            elif sp.src == "up":
                dx = [(p.cout, "down2", h // 2, w // 2, p.name)]
            else:
                dx = [(plan[sp.skip_from].cout, "normal", h, w, None), (p.cout, "normal", h, w, p.name)]
        fams = [_conv_family(sp.cout, M, 3, am, False, 0, False, o) for (M, am, _, _, _) in dx]
        # backward-weights plan
        if o["mfma_mode"] and o["dwbx_enable"] and sp.src != "input" and sp.cin % 32 == 0 and sp.cout % 32 == 0:
            kind, th, chunks, target = "conv_dwbx_k", 4, (sp.cin // 32) * (sp.cout // 32), o["dwbx_blocks"]
        elif o["mfma_mode"] and _dwbt_ok(sp, sp.cin // 2) and (bf16 or (sp.src != "up" and (sp.cin, sp.cout) != (8, 8))):
            kind, th, chunks, target = "conv_dwbt_k", 4, 1, 256 * (1 if sp.cin + sp.cout >= 48 else 2)
        elif sp.src == "input":
            first = (sp.cin, sp.cout) == (1, 8)
            kind, th, chunks, target = ("conv_dw_first_k" if first else "conv_bwd_w_k"), 8, (1 if first else _cdiv(sp.cout, 16)), o["dw16_blocks"]
        elif sp.cin >= 32 and sp.cout >= 32:
            cic = 64 if sp.cin % 64 == 0 else 32
            kind, th, chunks, target = "conv_dw32_k", (2 if cic == 64 else 4), _cdiv(sp.cin, cic) * _cdiv(sp.cout, 32), o["dw32_blocks"]
        else:
            cic = 16 if sp.cin >= 16 else 8
            pair = sp.src != "up" and sp.cout == 8 and sp.kh == 3 and o["dwpair8_enable"]
            kind, th, chunks, target = ("conv_dwpair8_k" if pair else "conv_dw16_k"), 8, _cdiv(sp.cin, cic) * _cdiv(sp.cout, 16), o["dw16_blocks"]
            if sp.src == "up" and cic == 16 and sp.cout == 8:
                target = target * 4 // 3
        fdw = (o["mfma_mode"] and sp.src != "input" and sp.kh == 3 and sp.cout == 8 and li != drop_li and sp.src in ("prev", "concat")
               and (sp.cin // 2 if sp.src == "concat" else sp.cin) == 8 and all(f == "conv_bt_k" for f in fams))
        if fdw:
            fdw_layers.add(sp.name)
        else:
            total32 = B * _cdiv(h, th) * _cdiv(w, 32)
            npb = max(1, min(total32, _cdiv(target, chunks)))
            if kind == "conv_dw_first_k":
                L = Launch(kind, sp.name, "dw", B, h, w, 8, 128, min(big, npb))
            else:
                L = Launch(kind, sp.name, "dw", B, h, w, th, 32, min(big, npb))
            out.append(L)
            reduce_bytes += L.grid * stride * 4
        for (M, am, ho, wo, stats), fam in zip(dx, fams):
            th, tw = _tile(fam, o)
            if fam == "conv_igemm_k":
                th = _igemm_th(B, ho, wo, M, o)
            L = Launch(fam, sp.name, "dx+dw" if fdw else "dx", B, ho, wo, th, tw, min(big, _builtin_cap(fam, sp.cout, fdw, o)), stats_for=stats)
            out.append(L)
        if fdw:
            reduce_bytes += out[-1].grid * stride * 4
    return out, fdw_layers, reduce_bytes


def flags_of(launches, fam, kind=None):
    """Union of the walk regimes of the modelled launches of one kernel family (and kind)."""
    f = set()
    for L in launches:
        if L.fam == fam and (kind is None or L.kind == kind):
            f |= L.flags()
    return f


# ---- A. capped grids at a small shape -------------------------------------------------------------------------------------

# What each (route, cap) is there for: the regimes its forced kernel families must show (launch kind -> regimes), by the
# geometry of the small shape.  Levels 40x96, 20x48, 10x24: 45, 18 and 6 tiles of 8x32; 30 and 9 of 8x64; 90 and 30 of 4x32.
#   5: unbanded; the backward-data launches that do not also reduce dW are at half resolution: 18 tiles, 3 to 4 per block.
#   8: banded, step 1: 18 tiles leave the last two bands idle (9 tiles of 8x64 the last three); 45 tiles give blocks six
#      consecutive tiles across both image boundaries.
#  12: unbanded, 3 to 4 tiles per block (8x64: 2 to 3).
#  16: banded, step 2: the last band of 45 tiles is uneven; 18 tiles leave four blocks idle.  The 8x64 and 4x32 kernels walk
#      2 and 6 (last band: 1 and 3) tiles per block, evenly, across image boundaries: that is all 16 shows on them.
#  24: banded, step 3, for the 8x64 kernels, whose 30-tile launches are even under 16: bands of 4 tiles on three blocks
#      (2, 1, 1) and a last band of 2 tiles that leaves a block idle.
#  56: banded, step 7, for the 4x32 kernel: bands of 12 of its 90 tiles on seven blocks (2, 2, 2, 2, 2, 1, 1), a last band
#      of 6 tiles that leaves a block idle.
PURPOSE = {
    ("default", 8): {"conv_bt_k": {"fwd": {"idle", "crossing", "multi"}, "dx": {"idle", "multi"}, "dx+dw": {"crossing", "multi"}},
                     "conv_first_fwd_k": {"fwd": {"multi", "unequal"}}, "conv_dw_first_k": {"dw": {"multi", "unequal"}},
                     "conv_dwbt_k": {"dw": {"multi", "unequal"}}},
    ("default", 5): {"conv_bt_k": {"dx": {"unbanded3", "crossing"}}},
    ("default", 12): {"conv_bt_k": {"fwd": {"unbanded3"}, "dx": {"multi", "unequal"}, "dx+dw": {"unbanded3"}}},
    ("default", 16): {"conv_bt_k": {"fwd": {"uneven", "idle"}, "dx": {"uneven", "idle"}, "dx+dw": {"uneven"}}},
    ("persistent", 8): {"conv_igemm_p_k": {"fwd": {"idle", "crossing"}, "dx": {"idle", "crossing"}}},
    ("persistent", 12): {"conv_igemm_p_k": {"fwd": {"unbanded3"}, "dx": {"unbanded3"}}},
    ("persistent", 16): {"conv_igemm_p_k": {"fwd": {"uneven", "idle"}, "dx": {"uneven", "idle"}}},
    ("thin8", 8): {"conv_thin8_k": {"fwd": {"crossing", "multi"}, "dx": {"idle", "crossing"}}},
    ("thin8", 12): {"conv_thin8_k": {"fwd": {"unbanded3"}, "dx": {"unbanded3"}}},
    ("thin8", 24): {"conv_thin8_k": {"fwd": {"uneven", "idle"}, "dx": {"uneven", "idle"}}},
    ("pair8_221", 8): {"conv_pair8_k": {"fwd": {"crossing", "multi"}, "dx": {"idle", "crossing"}}},
    ("pair8_221", 12): {"conv_pair8_k": {"fwd": {"unbanded3"}, "dx": {"unbanded3"}}},
    ("pair8_221", 16): {"conv_pair8_k": {"fwd": {"multi", "crossing"}, "dx": {"multi", "crossing"}}},
    ("pair8_221", 24): {"conv_pair8_k": {"fwd": {"uneven", "idle"}, "dx": {"uneven", "idle"}}},
    ("pair8_111", 8): {"conv_pair8_k": {"fwd": {"crossing", "multi"}, "dx": {"crossing", "multi"}}},
    ("pair8_111", 12): {"conv_pair8_k": {"fwd": {"unbanded3"}, "dx": {"unbanded3"}}},
    ("pair8_111", 16): {"conv_pair8_k": {"fwd": {"multi", "crossing"}, "dx": {"multi", "crossing"}}},
    ("pair8_111", 56): {"conv_pair8_k": {"fwd": {"uneven", "idle"}, "dx": {"uneven", "idle"}}},
    ("dw16_padded", 8): {"conv_dw16_k": {"dw": {"multi", "unequal", "crossing"}}, "conv_first_fwd_k": {"fwd": {"multi", "unequal"}},
                         "conv_dw_first_k": {"dw": {"multi", "unequal"}}},
    ("dw16_padded", 12): {"conv_dw16_k": {"dw": {"multi", "unequal"}}},
    ("dw16_padded", 16): {"conv_dw16_k": {"dw": {"multi", "unequal", "crossing"}}},
    ("thin8", 16): {"conv_thin8_k": {"fwd": {"multi", "crossing"}, "dx": {"multi", "crossing"}}, "conv_dwpair8_k": {"dw": {"multi", "unequal"}}, "conv_dw16_k": {"dw": {"multi", "unequal"}}},
}
CASES_A = [(r, c, m) for (r, c) in PURPOSE for m in (("f32", "bf16") if r == "default" else ("f32",))]


def check_purpose(launches, purpose):
    for fam, kinds in purpose.items():
        for kind, want in kinds.items():
            got = flags_of(launches, fam, kind)
            assert want <= got, (fam, kind, "wanted", sorted(want), "got", sorted(got), [L for L in launches if L.fam == fam])


CASES_WIDE = [
    (dict(), 8, {"conv_dwbx_k": {"multi", "unequal", "crossing"}, "conv_bwd_w_k": {"multi"}}),
    (dict(dwbx_enable=0), 8, {"conv_dw32_k": {"multi", "unequal", "crossing"}}),
    (dict(mfma_mode=0), 10, {"conv_dw32_k": {"multi", "unequal"}}),
]


def reduce_loop(npb, stride):
    """(the 8-way unrolled slab loop of reduce_all_k runs, its remainder loop runs) for some thread of a column: nq =
    256 / jw slab phases, jw = 16 columns per block below a stride of 16384 floats and 64 from there."""
    nq = 256 // (16 if stride < 16384 else 64)
    unrolled = rest = False
    for q in range(nq):
        p = q
        while p + 7 * nq < npb:
            unrolled = True; p += 8 * nq
        rest = rest or p < npb
    return unrolled, rest


# ---- C. the grid options: (id, SCANS key, route options, the knob under test, kernel families whose grid or tile it must move) ----
# Each runs where the knob CHANGES a launch (asserted from the model, ``moved_by``): dw16_blocks / dw32_blocks have a
# minimum of 64 and igemm_min_blocks = 1 << 30 differs from the default 512 only from 512 tiles on, so those run on the
# 688x384 image; bt_blocks_per_cu = 8 is clamped to what the kernel's LDS allows, i.e. to the default, everywhere.
F32 = dict(mfma_mode=0)
CASES_C = [
    ("igemm_persistent_blocks12", "small", ROUTES["persistent"], dict(igemm_persistent_blocks=12), {"conv_igemm_p_k"}),
    ("dwbx_blocks8", "wide32", {}, dict(dwbx_blocks=8), {"conv_dwbx_k"}),
    ("dwbx_blocks20", "wide32", {}, dict(dwbx_blocks=20), {"conv_dwbx_k"}),
    ("dw16_dw32_blocks64", "688x384", F32, dict(dw16_blocks=64, dw32_blocks=64), {"conv_dw16_k", "conv_dwpair8_k", "conv_dw32_k", "conv_dw_first_k"}),
    ("igemm_min_blocks1", "small", {}, dict(igemm_min_blocks=1), {"conv_igemm_k"}),
    ("f32pipe_igemm_min_blocks1", "small", F32, dict(igemm_min_blocks=1), {"conv_igemm_k"}),
    ("f32pipe_igemm_min_blocks_max", "688x384", F32, dict(igemm_min_blocks=1 << 30), {"conv_igemm_k"}),
    ("bt_blocks_per_cu1", "344x192", {}, dict(bt_blocks_per_cu=1), {"conv_bt_k"}),
    ("bt_blocks_per_cu8", "344x192", {}, dict(bt_blocks_per_cu=8), set()),
]


def moved_by(key, route, knob):
    """Kernel families of which some launch has another grid or pixel-tile height under ``knob`` than without it."""
    B, H, W, sn, P, _ = SCANS[key]
    cfg = on.UNetConfig(num_classes=C, start_neurons=sn, pool_layers=P)
    base = launch_model(cfg, B, H, W, False, route, 0)[0]
    with_knob = launch_model(cfg, B, H, W, False, dict(route, **knob), 0)[0]
    assert [(L.fam, L.layer, L.kind) for L in base] == [(L.fam, L.layer, L.kind) for L in with_knob]
    return {a.fam for a, b in zip(base, with_knob) if (a.grid, a.th) != (b.grid, b.th)}
