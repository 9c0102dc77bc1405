"""The persistent kernels' tile walk on the GPU: idle, uneven and strided blocks.

Every hot conv kernel but the wide forward kernel is persistent: a capped grid of blocks walks the pixel tiles
(``TileWalk`` of csrc/kernels_igemm.hpp, or a plain stride by the grid) and every block writes one row of BN-statistic
partials and, for backward-weights, one dW slab.  The option "persistent_max_blocks" caps those grids, so that a SMALL
image runs what only ordinary but large shapes reach otherwise: blocks without a tile (they must still write a zero row and
a zero slab and arrive at the in-launch finalize), unequal tile counts inside one band, the unbanded stride with several
tiles per block, blocks that cross an image boundary -- on every kernel family, including the fp32-pipe kernels the
default route never takes.

Every case runs one training step and one inference forward through tests/layer_local.py exactly as
tests/test_gpu_layer_local.py does (every stored tensor per element against fp64 recomputed from the engine's own stored
inputs; gates and EXCLUDE_MAX unchanged), so a missed, repeated or misplaced tile fails in the layer where it happens.
Besides the numbers each case asserts, from the step's own profile and a restatement of the host's routing rules
(``tests/tile_walk.launch_model``): WHAT RAN (the kernel family of every conv and backward-weights launch, per layer), THE GRID THAT RAN
(a bn_*_finalize entry carries bytes = rows * 2 * cout * 4 and the slab reduce carries the bytes of every slab: rows and
slabs must be min(tiles, cap)) and THE WALK REGIME of its launches (tests/tile_walk.regime).
The inputs, routes and cases are tables of tests/tile_walk.py, which tests/test_tile_walk.py checks on the CPU.

Kernels that stride by their grid (conv_first_fwd_k, conv_dw_first_k, conv_dw16_k / conv_dwpair8_k, conv_dw32_k,
conv_dwbt_k, conv_dwbx_k) are launched with grid <= tiles and visit tl = blockIdx, blockIdx + grid, ...: no block of
theirs can be without a tile; what is asserted for them is several tiles per block and unequal counts."""
import contextlib
import time

import numpy as np
import pytest
import torch

from oracle import unet_numpy as on
from tests import layer_local as ll
from tests.tile_walk import (C, CASES_A, CASES_C, CASES_WIDE, DROP_STEP, ENGINE_SEED, PURPOSE, ROLL, ROUTES, SCANS, check_purpose,
                             flags_of, launch_model, moved_by, reduce_loop, regime)

pytestmark = pytest.mark.gpu


# ---- running a case --------------------------------------------------------------------------------------------------------

@contextlib.contextmanager
def options(opts):
    """Set process-wide option defaults (a handle snapshots them at creation) and put back what was there."""
    from oct_image_segmentation_models_amd import _hip
    before = {k: _hip.get_option(k) for k in opts}
    try:
        for k, v in opts.items():
            _hip.set_option(k, v)
        yield
    finally:
        for k, v in before.items():
            _hip.set_option(k, v)


def _epi(kernel):
    """The epilogue template argument of a conv kernel name: 0 forward, 1 raw gradient, 2 masked gradient (+ statistics)."""
    fam, args = kernel.split("<", 1)
    a = args.rstrip(">").split(",")
    return int(a[{"conv_bt_k": 2, "conv_thin8_k": 2, "conv_bx_k": 2, "conv_igemm_p_k": 3, "conv_igemm_k": 3, "conv_pair8_k": 0}[fam]])


def check_profile(ents, launches, fdw_layers, reduce_bytes, cfg, training):
    """What ran and the grid that ran, from the profile entries of the step."""
    for e in ents:
        print(f"    {e['kernel']:60s} {e['layer']:12s} x{e['launches']} bytes {e['bytes']:.0f}")
    conv = {(e["kernel"].split("<")[0], e["layer"], "fwd" if e["kernel"].startswith("conv_first_fwd_k") or _epi(e["kernel"]) == 0 else "dx")
            for e in ents if e["kernel"].startswith(("conv_bt_k", "conv_bx_k", "conv_igemm", "conv_thin8_k", "conv_pair8_k", "conv_first_fwd_k"))}
    want = {(L.fam, L.layer, "fwd" if L.kind == "fwd" else "dx") for L in launches if L.kind != "dw" and L.fam != "conv_fwd_k"}
    assert conv == want, ("missing", sorted(want - conv), "unexpected", sorted(conv - want))
    # pixel-tile height of the tile-per-block fp32-pipe kernel: conv_igemm_k<SHAPE,KH,AMODE,EPI,TH,...>
    th = {(e["layer"], _epi(e["kernel"]), int(e["kernel"].split(",")[4])) for e in ents if e["kernel"].startswith("conv_igemm_k<")}
    th_want = {(L.layer, "fwd" if L.kind == "fwd" else "dx", L.th) for L in launches if L.fam == "conv_igemm_k"}
    assert {(l, "fwd" if k == 0 else "dx", t) for l, k, t in th} == th_want, (sorted(th), sorted(th_want))
    if not training:
        return
    dw = {(e["kernel"].split("<")[0], e["layer"]) for e in ents if e["kernel"].startswith(("conv_dw", "conv_bwd_w_k"))}
    want = {(L.fam, L.layer) for L in launches if L.kind == "dw"}
    assert dw == want, ("missing", sorted(want - dw), "unexpected", sorted(dw - want))
    assert {e["layer"] for e in ents if e["kernel"].startswith("conv_bt_k<") and e["kernel"].endswith(",dw>")} == fdw_layers
    # statistic rows: bytes = rows * 2 * cout * 4 per finalize launch
    cout = {sp.name: sp.cout for sp in on.build_plan(cfg)}
    checked = {}              # (layer, "fwd" | "dx") -> rows, of the entries whose emitting launch is modelled
    for e in ents:
        if e["kernel"] not in ("bn_fwd_finalize_k", "bn_bwd_finalize_k"):
            continue
        assert e["launches"] == 1
        rows = e["bytes"] / (2 * cout[e["layer"]] * 4)
        kind = "fwd" if e["kernel"] == "bn_fwd_finalize_k" else "dx"
        src = [L for L in launches if L.stats_for == e["layer"] and (L.kind == "fwd") == (kind == "fwd")]
        if not src or src[0].fam in ("conv_bx_k", "conv_fwd_k"):
            continue              # rows of the wide kernel (its tile is not modelled), the pool backward or the head backward
        assert len(src) == 1 and rows == src[0].grid, (e, src)       # (a tile-per-block kernel: grid = its tiles)
        checked[e["layer"], kind] = int(rows)
    red = [e for e in ents if e["kernel"] == "reduce_all_k"]
    assert sum(e["bytes"] for e in red) == reduce_bytes, (red, reduce_bytes)
    return checked


def params_from_engine(eng):
    from tests.test_gpu_layer_local import _params_from_engine
    return _params_from_engine(eng)


def run_case(key, mode, opts, cap, title, live_cap=False):
    """One training step and one inference forward at SCANS[key] under ``opts`` with the grid cap ``cap``, both through
    the layer-local model; returns the modelled launches of the training step (their kernels and grids asserted against
    the profile).  ``live_cap``: the cap is set on the live handle (oct_unet_set_option), not on the defaults."""
    from oct_image_segmentation_models_amd import _hip
    from oct_image_segmentation_models_amd.engine import UNetEngine
    from tests.test_gpu_layer_local import _finish, ragged_scans
    t0 = time.time()
    B, H, W, sn, P, seed = SCANS[key]
    cfg = on.UNetConfig(num_classes=C, start_neurons=sn, pool_layers=P)
    params, state = on.init_params(cfg, seed=7, dtype=np.float32, randomize_bn=True)
    img, lab = ragged_scans(B, H, W, seed, ROLL)
    x = torch.from_numpy(img).cuda(); l = torch.from_numpy(lab[..., 0].copy()).cuda()
    all_opts = dict(opts)
    if cap and not live_cap:
        all_opts["persistent_max_blocks"] = cap
    with options(all_opts):
        mm = _hip.get_option("mfma_mode")
        kw = dict(device="cuda:0", input_channels=1, num_classes=C, image_height=H, image_width=W, max_batch=B,
                  start_neurons=sn, pool_layers=P, seed=ENGINE_SEED, init_seed=1, dtype="bfloat16" if mode == "bf16" else "float32")
        eng = UNetEngine(training=True, **kw)
        inf = UNetEngine(training=False, **kw)
    if cap and live_cap:
        eng.set_option("persistent_max_blocks", cap); inf.set_option("persistent_max_blocks", cap)
    assert eng.handle_option("persistent_max_blocks") == cap and _hip.get_option("persistent_max_blocks") == 0
    eng.set_weights(on.keras_weight_list(params, state))
    eng.set_dropout_step(DROP_STEP)
    mask = eng.dropout_mask(B).double()
    eng.profile_begin()
    probs, _ = eng.forward(x, training=True, labels=l)
    eng.loss_dice()
    eng.backward(l, macro=True, loss_scale=1.0)
    ents = eng.profile_end()
    launches, fdw_layers, reduce_bytes = launch_model(cfg, B, H, W, mode == "bf16", opts, cap)
    print(f"\n{title}: modelled launches")
    for L in launches:
        print("   ", L)
    n_rows = check_profile(ents, launches, fdw_layers, reduce_bytes, cfg, True)
    p64, _ = params_from_engine(eng)
    S = ll.engine_stored(eng, B, probs)
    rep = ll.LayerLocal(cfg, p64, S, img, labels=lab[..., 0], dropout_mask=mask, mode=mode, mfma_mode=mm, device="cuda:0").run()
    _finish(rep, t0, title + " (training step)")
    # inference forward on its own handle (moving statistics of the parameters)
    inf.set_weights(on.keras_weight_list(params, state))
    inf.profile_begin()
    probs_i, am = inf.forward(x, training=False, want_argmax=True)
    ents_i = inf.profile_end()
    check_profile(ents_i, launch_model(cfg, B, H, W, mode == "bf16", opts, cap, training=False)[0], set(), 0, cfg, False)
    p64i, s64i = params_from_engine(inf)
    Si = ll.engine_stored(inf, B, probs_i, training=False, argmax=am)
    repi = ll.LayerLocal(cfg, p64i, Si, img, training=False, state=s64i, mode=mode, mfma_mode=mm, device="cuda:0").run()
    _finish(repi, t0, title + " (inference forward)")
    return launches, n_rows, ents


@pytest.mark.parametrize("route,cap,mode", CASES_A, ids=[f"{r}-cap{c}-{m}" for r, c, m in CASES_A])
def test_capped_grid_small_shape(route, cap, mode):
    """B = 3, 40x96, start_neurons 8, pool_layers 2, u8 input, dropout on: every persistent launch on min(tiles, cap) blocks."""
    launches, n_rows, _ = run_case("small", mode, ROUTES[route], cap, f"{route} cap {cap} {mode} 3x40x96")
    # the finalize entries whose rows were held to min(tiles, cap): every launch of a walking kernel that emits statistics
    want = {(L.stats_for, "fwd" if L.kind == "fwd" else "dx") for L in launches if L.stats_for and L.walks}
    assert want <= set(n_rows) and len(want) >= (1 if route == "dw16_padded" else 4), sorted(want - set(n_rows))
    assert all(n_rows[k] <= cap for k in want)
    check_purpose(launches, PURPOSE[route, cap])


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_capped_grid_in_launch_finalize_with_idle_blocks(mode):
    """fuse_bn_finalize = 1 under cap 8: the arrival counter of the in-launch finalize is met by blocks without a tile
    (18 tiles on 8 blocks: two idle), and their zero rows are part of what the last block sums.  The cap is set on the
    live handles here."""
    launches, _, ents = run_case("small", mode, dict(fuse_bn_finalize=1), 8, f"in-launch finalize cap 8 {mode} 3x40x96", live_cap=True)
    # the launches that emit the rows finalized them: no finalize launch is left for their layers
    own = {(L.stats_for, L.kind == "fwd") for L in launches if L.fam in ("conv_bt_k", "conv_first_fwd_k") and L.stats_for}
    left = {(e["layer"], e["kernel"] == "bn_fwd_finalize_k") for e in ents if e["kernel"] in ("bn_fwd_finalize_k", "bn_bwd_finalize_k")}
    assert len(own) >= 12 and not (own & left), sorted(own & left)
    assert {"idle", "crossing"} <= flags_of(launches, "conv_bt_k", "fwd") and "idle" in flags_of(launches, "conv_bt_k", "dx")


@pytest.mark.parametrize("opts,cap,fams", CASES_WIDE, ids=["dwbx-cap8", "dw32-cap8", "f32pipe-dw32-cap10"])
def test_capped_grid_wide_backward_weights(opts, cap, fams):
    """B = 3, 32x64, start_neurons 32, pool_layers 1: the wide backward-weights kernels (conv_dwbx_k with 1, 2 and 4
    channel chunks; conv_dw32_k with dwbx_enable = 0 or on the fp32 pipe) walk several tiles per block, unequally many."""
    launches, _, _ = run_case("wide32", "f32", opts, cap, f"wide {opts} cap {cap} 3x32x64")
    for fam, want in fams.items():
        assert want <= flags_of(launches, fam, "dw"), (fam, [L for L in launches if L.fam == fam])
    if not opts:
        assert {L.layer for L in launches if L.fam == "conv_dwbx_k"} >= {"enc0.conv1", "mid.conv0", "mid.conv1", "dec0.conv0"}


# ---- B. idle blocks on the default route without the cap ---------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_idle_blocks_at_688x384_default_route(mode):
    """One 688x384 image, pool_layers 3, bt_blocks_per_cu = 1: level 0 is 1032 tiles on 256 blocks (4 or 5 per block),
    level 1 (344x192) 258 tiles on 256 blocks -- 5 idle -- on the 16-channel conv_bt_k forward and backward-data launches
    and the up-conv; level 2 runs one tile per block."""
    launches, n_rows, _ = run_case("688x384", mode, dict(bt_blocks_per_cu=1), 0, f"688x384 {mode} bt_blocks_per_cu 1")
    bt = [L for L in launches if L.fam == "conv_bt_k"]
    lvl1 = [L for L in bt if L.total == 258]
    assert {L.layer for L in lvl1 if L.kind == "fwd"} >= {"enc1.conv0", "enc1.conv1", "dec1.conv0", "dec1.conv1"}
    assert any(L.kind == "dx" for L in lvl1)
    assert all(L.grid == 256 and regime(L.total, L.grid).idle == 5 for L in lvl1)
    assert all(regime(L.total, L.grid) == (0, 4, 5, True) for L in bt if L.total == 1032) and any(L.total == 1032 for L in bt)
    # rows = 256 from the finalize entries of every launch at levels 0 and 1 that emits statistics
    want = {(L.stats_for, "fwd" if L.kind == "fwd" else "dx") for L in bt if L.stats_for and L.total in (258, 1032)}
    assert len(want) >= 14 and {("enc1.conv0", "fwd"), ("enc1.conv1", "fwd"), ("dec1.up", "fwd"), ("dec1.conv0", "fwd"),
                                ("dec1.conv1", "fwd"), ("enc1.conv0", "dx"), ("dec1.conv0", "dx")} <= want
    assert {k: n_rows.get(k) for k in want} == {k: 256 for k in want}


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_idle_blocks_at_344x192_fused_backward_weights(mode):
    """One 344x192 image, pool_layers 2, bt_blocks_per_cu = 1: the 5 idle blocks are on the full-resolution 8 -> 8 layers,
    whose backward-data launches also reduce dW, one slab per block: an idle block's slab must be zero.  The slab counts
    of this step also run both loops of the slab reduce."""
    launches, n_rows, _ = run_case("344x192", mode, dict(bt_blocks_per_cu=1), 0, f"344x192 {mode} bt_blocks_per_cu 1")
    fdw = [L for L in launches if L.kind == "dx+dw"]
    assert {L.layer for L in fdw} == {"enc0.conv1", "dec1.conv0", "dec1.conv1"}
    assert all(L.fam == "conv_bt_k" and L.total == 258 and L.grid == 256 and regime(258, 256).idle == 5 for L in fdw)
    assert all(L.grid == 256 for L in launches if L.fam == "conv_bt_k" and L.total == 258)
    # reduce_all_k: the head's 258 rows (stride 27) and the 129 slabs of a half-resolution conv_dwbt_k launch enter the
    # unrolled loop and leave a remainder; the fused layers' 256 slabs run the unrolled loop alone
    assert reduce_loop(258, 27) == (True, True) and reduce_loop(256, 584) == (True, False)
    half = [L for L in launches if L.kind == "dw" and L.grid == 129]
    assert half and reduce_loop(129, 9 * 16 * 16 + 16) == (True, True)
    want = {(L.stats_for, "fwd" if L.kind == "fwd" else "dx") for L in launches if L.fam == "conv_bt_k" and L.stats_for and L.total == 258}
    assert {("enc0.conv1", "fwd"), ("dec1.up", "fwd"), ("dec1.conv0", "fwd"), ("dec1.conv1", "fwd"), ("enc0.conv0", "dx"),
            ("dec1.up", "dx"), ("dec1.conv0", "dx")} == want
    assert {k: n_rows.get(k) for k in want} == {k: 256 for k in want}


# ---- C. the grid options do not change results beyond rounding ---------------------------------------------------------------

@pytest.mark.parametrize("name,key,route,knob,moves", CASES_C, ids=[c[0] for c in CASES_C])
def test_grid_options_do_not_change_results(name, key, route, knob, moves):
    """The header's promise for the grid knobs -- "results do not depend on them beyond fp32 rounding" -- through the same
    layer-local gates, no cap, each at a shape where the knob moves a grid or a pixel tile (tests/tile_walk.CASES_C); the
    profile check of run_case holds the moved grids (rows, slab bytes) and tile heights to what ran."""
    assert moved_by(key, route, knob) == moves
    launches, _, _ = run_case(key, "f32", dict(route, **knob), 0, f"{name} {key}")
    if name == "igemm_persistent_blocks12":       # 45 tiles on 12 blocks: the unbanded stride through the option itself
        assert "unbanded3" in flags_of(launches, "conv_igemm_p_k")
    if "dwbx_blocks" in knob:                     # ceil(target / chunks) blocks per chunk: 8 -> 8, 4, 2; 20 -> 20, 10, 5
        grids = {L.grid for L in launches if L.fam == "conv_dwbx_k"}
        assert grids == ({8, 4, 2} if knob["dwbx_blocks"] == 8 else {20, 10, 5}), grids
        assert "multi" in flags_of(launches, "conv_dwbx_k")
    if "dw16_blocks" in knob:                     # 64 blocks over a launch's channel chunks (85 where the target is 4/3 of it)
        big = [L for L in launches if L.kind == "dw" and L.total > 85]
        assert len(big) >= 6 and all(L.grid <= 85 and "multi" in L.flags() for L in big), big
    if "igemm_min_blocks" in knob:                # the taller tile wherever there is one (1) / nowhere (1 << 30)
        ths = {L.th for L in launches if L.fam == "conv_igemm_k"}
        assert (ths <= {8, 4} and 8 in ths) if knob["igemm_min_blocks"] == 1 else (ths <= {4, 2} and 4 in ths), ths
