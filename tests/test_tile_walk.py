"""CPU tests of the persistent kernels' tile walk and of the inputs of tests/test_gpu_tile_walk.py, no GPU.

(a) ``walk`` / ``next_org`` (tests/tile_walk.py) restate ``TileWalk`` of csrc/kernels_igemm.hpp in plain Python.  They exist to CLASSIFY the
    GPU cases -- which launches leave blocks without a tile, give blocks of one band unequal tile counts, stride the
    whole sequence, cross an image boundary (``regime``) -- not to prove the kernel: the kernels are judged on the GPU,
    per element, by tests/layer_local.py.  What is checked here is that the restatement is a walk at all (every tile once)
    and that its carry logic agrees with ``divmod`` of the linear tile index, so that it cannot drift from what it describes.
(b) For every (shape, scan seed) the GPU module uses, the layer-local fp64 model on the tensors of a defect-free engine
    (tests/test_layer_local.perfect_engine) reports no failure and stays inside EXCLUDE_MAX: what a device run excludes or
    fails beyond that is the device's."""
import collections

import numpy as np
import pytest

from oracle import unet_numpy as on
from tests import layer_local as ll

from tests.tile_walk import CAPS, NX, Regime, _block, _cdiv, crosses_image, next_org, regime, uneven_band, walk  # noqa: F401


@pytest.mark.parametrize("cap", CAPS)
def test_every_tile_is_visited_exactly_once(cap):
    for total in range(1, 3001):
        grid = min(total, cap)
        for banded in (True, False):
            seen = sorted(t for blk in walk(total, grid, banded) for t in blk)
            assert seen == list(range(total)), (total, grid, banded)


def test_idle_blocks_at_a_full_cap():
    """grid = cap, total = cap + r: the remainders that leave blocks of the last band(s) without a tile; one 344x192 image
    is 258 tiles of 8x32 on the thin kernel's 256 blocks (r = 2).  A strided walk never idles a block of a grid <= total."""
    idle = [r for r in range(1, 64) if regime(256 + r, 256).idle]
    assert idle == [1, 2, 3, 4, 5, 6, 9, 10, 11, 12, 13, 17, 18, 19, 20, 25, 26, 27, 33, 34, 41]
    assert regime(258, 256) == Regime(5, 1, 2, True) and regime(1032, 256) == Regime(0, 4, 5, True)
    assert all(regime(256 + r, 256, banded=False).idle == 0 for r in range(64))
    # the small shape of the GPU module (levels of 45, 18 and 6 tiles of 8x32) under its three caps
    assert regime(18, 8) == Regime(2, 3, 3, True) and regime(45, 8) == Regime(0, 3, 6, True)
    assert regime(45, 12) == Regime(0, 3, 4, False) and regime(18, 12) == Regime(0, 1, 2, False)
    assert regime(45, 16) == Regime(0, 1, 3, True) and uneven_band(45, 16) and regime(18, 16).idle == 4
    assert not uneven_band(45, 8) and not uneven_band(45, 12)


# every (B, H, W) x (tile height, tile width) of the GPU module's levels, under every grid its cases run
WALK_GEOMETRIES = [(B, H >> lv, W >> lv, th, tw)
                   for (B, H, W, P) in ((3, 40, 96, 2), (3, 32, 64, 1), (1, 688, 384, 3), (1, 344, 192, 2))
                   for lv in range(P + 1) for (th, tw) in ((8, 32), (8, 64), (4, 32), (8, 128), (2, 32))]


def test_the_carry_restatement_agrees_with_divmod():
    checked = carried_row = carried_image = 0
    for B, H, W, th, tw in WALK_GEOMETRIES:
        tiles_x = _cdiv(W, tw); tiles = tiles_x * _cdiv(H, th); total = B * tiles
        for cap in (8, 12, 16, 20, 64, 256, 512):
            grid = min(total, cap)
            for blk in range(grid):
                tl0, tlend, step = _block(total, grid, blk)
                if tl0 >= tlend:
                    continue
                o = (tl0 // tiles, (tl0 % tiles) // tiles_x, tl0 % tiles_x)          # TileWalk::first
                for tl in range(tl0, tlend, step):
                    assert o == (tl // tiles, (tl % tiles) // tiles_x, tl % tiles_x), (B, H, W, th, tw, grid, blk, tl)
                    n = next_org(o, step, tiles, tiles_x)
                    carried_row += n[1] != o[1] and n[2] < o[2]
                    carried_image += n[0] != o[0]
                    o = n; checked += 1
    assert checked > 10000 and carried_row > 100 and carried_image > 100


# ---- the GPU module's cases, by geometry alone (its routing model; the GPU run asserts the model against the profile) ---------

def _model(key, mode, opts, cap):
    from tests import tile_walk as g
    B, H, W, sn, P, _ = g.SCANS[key]
    cfg = on.UNetConfig(num_classes=3, start_neurons=sn, pool_layers=P)
    return g.launch_model(cfg, B, H, W, mode == "bf16", opts, cap)[0]


def test_every_capped_case_shows_the_regimes_it_is_there_for():
    from tests import tile_walk as g
    for route, cap, mode in g.CASES_A:
        g.check_purpose(_model("small", mode, g.ROUTES[route], cap), g.PURPOSE[route, cap])
    for opts, cap, fams in g.CASES_WIDE:
        launches = _model("wide32", "f32", opts, cap)
        for fam, want in fams.items():
            assert want <= g.flags_of(launches, fam, "dw"), (opts, cap, fam)


def test_model_defaults_are_the_librarys():
    """The routing model's option defaults (tile_walk.DEFAULTS; grid targets 256, 512, 768, 1280, ...) are what the library
    ships: read from the built library, no GPU."""
    import __graft_entry__ as ge
    from tests import tile_walk as g
    ge.build()
    from oct_image_segmentation_models_amd import _hip
    assert {k: _hip.get_option(k) for k in g.LIBRARY_DEFAULTS} == g.LIBRARY_DEFAULTS
    for k, v in g.DEFAULTS.items():
        if k in g.LIBRARY_DEFAULTS:
            assert g.LIBRARY_DEFAULTS[k] == v, k
        else:              # the model's on/off form of a *_min_tiles threshold: off at 2048 tiles for every test shape
            assert v == 0 and g.LIBRARY_DEFAULTS[{"persistent": "igemm_persistent_min_tiles"}.get(k, k + "_min_tiles")] == 2048, k


def test_every_grid_option_case_moves_a_grid():
    from tests import tile_walk as g
    for name, key, route, knob, moves in g.CASES_C:
        assert g.moved_by(key, route, knob) == moves, name


def test_every_kernel_family_meets_every_regime_somewhere():
    """Across the GPU module: idle blocks, an uneven band, the unbanded stride at >= 3 tiles per block and an image crossing
    for every TileWalk kernel (conv_bt_k as forward, backward-data and fused backward-weights launch; conv_pair8_k in both
    geometries); several and unequally many tiles per block for the kernels that stride by their grid, which cannot idle."""
    from tests import tile_walk as g
    seen = collections.defaultdict(set)
    for route, cap, mode in g.CASES_A:
        for L in _model("small", mode, g.ROUTES[route], cap):
            fam = L.fam + ("_111" if L.fam == "conv_pair8_k" and route == "pair8_111" else "")
            seen[fam, L.kind if L.fam == "conv_bt_k" else ""] |= L.flags()
    for opts, cap, _ in g.CASES_WIDE:
        for L in _model("wide32", "f32", opts, cap):
            seen[L.fam, ""] |= L.flags()
    for key in ("344x192", "688x384"):
        for mode in ("f32", "bf16"):
            for L in _model(key, mode, dict(bt_blocks_per_cu=1), 0):
                seen[L.fam, L.kind if L.fam == "conv_bt_k" else ""] |= L.flags()
    four = {"idle", "uneven", "unbanded3", "crossing"}
    for k in (("conv_bt_k", "fwd"), ("conv_bt_k", "dx"), ("conv_bt_k", "dx+dw"), ("conv_igemm_p_k", ""), ("conv_thin8_k", ""),
              ("conv_pair8_k", ""), ("conv_pair8_k_111", "")):
        assert four <= seen[k], (k, sorted(four - seen[k]))
    for fam in ("conv_first_fwd_k", "conv_dw_first_k", "conv_dw16_k", "conv_dwpair8_k", "conv_dw32_k", "conv_dwbt_k", "conv_dwbx_k"):
        assert {"multi", "unequal"} <= seen[fam, ""] and "idle" not in seen[fam, ""], (fam, sorted(seen[fam, ""]))


# ---- (b) the GPU module's inputs on a defect-free engine ---------------------------------------------------------------------

# keys of tests/tile_walk.SCANS (the largest, one 688x384 image, takes the fp64 reference about 10 s per mode here)
REFERENCE_CASES = ["small", "wide32", "344x192", "688x384"]


def test_every_gpu_input_is_listed():
    from tests.tile_walk import SCANS
    assert sorted(SCANS) == sorted(REFERENCE_CASES)


@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("key", REFERENCE_CASES)
def test_reference_alone_passes_its_gates_on_the_gpu_inputs(key, mode):
    from tests.helpers import dropout_keep_mask
    from tests.test_gpu_layer_local import ragged_scans
    from tests.tile_walk import DROP_STEP, ENGINE_SEED, ROLL, SCANS
    from tests.test_layer_local import perfect_engine
    B, H, W, sn, P, seed = SCANS[key]
    cfg = on.UNetConfig(num_classes=3, start_neurons=sn, pool_layers=P)
    params, _ = on.init_params(cfg, seed=7, dtype=np.float32, randomize_bn=True)
    p64 = [{k: v.astype(np.float64) for k, v in p.items()} for p in params]
    img, lab = ragged_scans(B, H, W, seed, ROLL)
    mask = dropout_keep_mask(ENGINE_SEED, DROP_STEP, (B, H >> P, W >> P, sn << P)).astype(np.float64)
    fused = [True] * (len(on.build_plan(cfg)) - 1)
    S, _, _, _ = perfect_engine(cfg, p64, img, lab[..., 0], mask, mode, fused)
    rep = ll.LayerLocal(cfg, p64, S, img, labels=lab[..., 0], dropout_mask=mask, mode=mode, chunk=1).run()
    print(f"{key} {mode}: excluded {rep.excluded} of {rep.elements}")
    assert not rep.failures, rep.failures[:10]
    assert rep.excluded <= ll.EXCLUDE_MAX * rep.elements
    if key in ("small", "wide32"):
        assert rep.excluded == 0
