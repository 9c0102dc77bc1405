"""The wide backward-weights kernel's tile pipeline (conv_dwbx_k): the staged low-res footprint of the up-conv form, the
next tile's staging items among the MFMA steps, the unguarded slab store.

A block of conv_dwbx_k owns one (32 input, 32 output channel) chunk and walks 4 x 32 pixel tiles blockIdx.x, + grid, ...:
tile t is multiplied out of one LDS buffer while tile t + 1 is converted, split and written into the other and tile t + 2
is requested into the same registers; one slab per block.  The up-conv form stages the 3 x 17 low-res footprint of the
virtual 5 x 33 tile -- one (pixel, channel octet) per thread, converted once and written to every slot it covers, the last
footprint row and column to one slot row / column only.  A slot the copy misses or doubles, a footprint pixel taken from
the wrong image of a tile that crosses images, a staging register reloaded before it was converted, or a dropout
multiplier indexed by the slot instead of the low-res element would each change a weight gradient.  Every case

  * runs its first training step through the layer-local fp64 model (tests/layer_local.py; gates unchanged) -- every stored
    tensor, and the kernel and bias gradient of every layer, the wide ones asserted to be among them;
  * runs three training steps (forward, Dice loss, backward, Adam) twice on fresh handles with the same seeds and asks
    for torch.equal on the loss, every gradient and every updated parameter after every step;
  * asserts from the step's profile which conv_dwbx_k forms ran on which layers, and from the launch model
    (tests/tile_walk.py) how their blocks walked.

Shapes (B, H, W, start_neurons, pool_layers), fp32 and bf16 storage each:
  deep    3 x 36x72, 32, 2   levels 36x72, 18x36, 9x18: 27, 10 and 3 tiles of 4x32 per image, ragged in x and y at levels 0
                             and 1 (and in y at level 2); dec0.up (128 -> 64) is the up-conv form with dropout on its input,
                             dec1.up (64 -> 32) the one without; 1, 2, 4, 8 and 16 channel chunks; dec0.conv0 and dec1.conv0
                             read a two-source concat
  wide32  3 x 32x64, 32, 1   the shape of tests/tile_walk.py (CASES_C)
under "dwbx_blocks" 8 and 20 (several unequal tiles per block, blocks crossing images) and 256, the default, at which every
launch of both shapes has one tile per block (asserted).

test_up_layers_one_slab_per_tile compares the up-conv layers' gradients between grids: dwbx_blocks = 2^20 (one slab per
tile), the default and 8.  The sum over tiles is then taken in another order (inside a block's accumulators or over
slabs): fp32 rounding of that sum, PARAM_RTOL of the tensor's scale -- what tests/layer_local.py allows a dW against fp64
on any grid.  At this shape the default grid is one slab per tile already; the pair that differs is (2^20, 8)."""
import time

import numpy as np
import pytest
import torch

from oracle import unet_numpy as on
from tests import layer_local as ll
from tests.tile_walk import C, DROP_STEP, ENGINE_SEED, ROLL, SCANS, launch_model

pytestmark = pytest.mark.gpu

SHAPES = {"deep": (3, 36, 72, 32, 2, 42), "wide32": SCANS["wide32"]}
BLOCKS = (8, 20, 256)
STEPS = 3
CASES = [(k, b, m) for k in SHAPES for b in BLOCKS for m in ("f32", "bf16")]
IDS = [f"{k}-blocks{b}-{m}" for k, b, m in CASES]
_first = {}          # (key, blocks, mode) -> (snapshots, profile entries, layer-local report) of the checked run


def _cfg(key):
    B, H, W, sn, P, seed = SHAPES[key]
    return on.UNetConfig(num_classes=C, start_neurons=sn, pool_layers=P)


def _wide(cfg):
    """The layers whose backward-weights run on conv_dwbx_k: name -> (channel chunks, up-conv form, concat input)."""
    return {sp.name: ((sp.cin // 32) * (sp.cout // 32), sp.src == "up", sp.src == "concat")
            for sp in on.build_plan(cfg) if sp.src not in ("input", "head") and sp.kh != 1 and sp.cin % 32 == 0 and sp.cout % 32 == 0}


def _run(key, mode, blocks, check):
    from oct_image_segmentation_models_amd import _hip
    from oct_image_segmentation_models_amd.engine import UNetEngine
    from tests.test_gpu_layer_local import _finish, _params_from_engine, ragged_scans
    from tests.test_gpu_tile_walk import options
    t0 = time.time()
    B, H, W, sn, P, seed = SHAPES[key]
    cfg = _cfg(key)
    params, state = on.init_params(cfg, seed=7, dtype=np.float32, randomize_bn=True)
    img, lab = ragged_scans(B, H, W, seed, ROLL)
    x = torch.from_numpy(img).cuda(); l = torch.from_numpy(lab[..., 0].copy()).cuda()
    with options(dict(dwbx_blocks=blocks)):
        mm = _hip.get_option("mfma_mode")
        eng = UNetEngine(training=True, device="cuda:0", input_channels=1, num_classes=C, image_height=H, image_width=W, max_batch=B,
                         start_neurons=sn, pool_layers=P, seed=ENGINE_SEED, init_seed=1, dtype="bfloat16" if mode == "bf16" else "float32")
    assert eng.handle_option("dwbx_blocks") == blocks and _hip.get_option("dwbx_blocks") == 256
    eng.set_weights(on.keras_weight_list(params, state))
    snaps, ents, rep, model = [], None, None, None
    for step in range(STEPS):
        eng.set_dropout_step(DROP_STEP + step)
        if step == 0:
            eng.profile_begin()
        probs, _ = eng.forward(x, training=True, labels=l)
        loss4 = eng.loss_dice()
        eng.backward(l, macro=True, loss_scale=1.0)
        if step == 0:
            ents = eng.profile_end()
        torch.cuda.synchronize()
        snap = {"loss4": loss4.clone(), "grads": eng.grads.clone()}
        if step == 0 and check:
            mask = eng.dropout_mask(B).double()
            p64, _ = _params_from_engine(eng)
            S = ll.engine_stored(eng, B, probs)
            model = ll.LayerLocal(cfg, p64, S, img, labels=lab[..., 0], dropout_mask=mask, mode=mode, mfma_mode=mm, device="cuda:0")
            rep = model.run()
            _finish(rep, t0, f"{key} {mode} dwbx_blocks {blocks} (training step 1)")
        eng.adam_step()
        torch.cuda.synchronize()
        snap["params"] = eng.params.clone()
        snaps.append(snap)
    return snaps, ents, rep, eng.layers, model


def _checked(key, blocks, mode):
    k = (key, blocks, mode)
    if k not in _first:
        _first[k] = _run(key, mode, blocks, True)
    return _first[k]


def _layer_grads(snap, L):
    """(kernel gradient, bias gradient) of one layer out of a step's flat gradient buffer."""
    g = snap["grads"]
    n = L["kh"] * L["kw"] * L["cin"] * L["cout"]
    return g[L["kernel_off"]:L["kernel_off"] + n], g[L["bias_off"]:L["bias_off"] + L["cout"]]


@pytest.mark.parametrize("key,blocks,mode", CASES, ids=IDS)
def test_first_step_against_the_layer_local_model(key, blocks, mode):
    B, H, W, sn, P, _ = SHAPES[key]
    cfg = _cfg(key)
    wide = _wide(cfg)
    snaps, ents, rep, _, _ = _checked(key, blocks, mode)
    # the forms that ran, and where
    at = "unsigned short" if mode == "bf16" else "float"
    ns = 1 if mode == "bf16" else 3
    ran = {e["layer"]: e["kernel"] for e in ents if e["kernel"].startswith("conv_dwbx_k<")}
    print(f"\n{key} {mode} dwbx_blocks {blocks}: conv_dwbx_k launches")
    for layer, kern in ran.items():
        print(f"    {kern:44s} {layer:12s} chunks {wide[layer][0]}")
    assert ran == {name: f"conv_dwbx_k<{'2,true' if up else '3,false'},{ns},{at},gb>" for name, (_, up, _) in wide.items()}, ran
    if key == "deep":
        assert {n for n, (_, up, _) in wide.items() if up} == {"dec0.up", "dec1.up"}
        assert {c for c, _, _ in wide.values()} >= {1, 2, 4, 8} and any(two for _, _, two in wide.values())
    # how the blocks walked
    launches = [L for L in launch_model(cfg, B, H, W, mode == "bf16", dict(dwbx_blocks=blocks), 0)[0] if L.fam == "conv_dwbx_k"]
    assert {L.layer for L in launches} == set(wide)
    for L in launches:
        print("   ", L)
    if blocks == 256:
        assert all(L.grid == L.total for L in launches), launches
    else:
        flags = set().union(*(L.flags() for L in launches))      # (wide32 under 8: 48 and 12 tiles divide evenly)
        assert ({"multi", "crossing"} if (key, blocks) == ("wide32", 8) else {"multi", "unequal", "crossing"}) <= flags, flags
        if key == "deep":       # both up-conv launches walk several tiles per block
            assert all("multi" in L.flags() for L in launches if L.layer in ("dec0.up", "dec1.up")), launches
    # kernel and bias gradients of every wide layer were judged (a failure anywhere is raised by the run itself)
    for name in wide:
        assert {"dW", "bias"} <= set(rep.rows[name]), (name, sorted(rep.rows[name]))
    for s in snaps:
        assert all(torch.isfinite(s[k].float()).all() for k in s)


@pytest.mark.parametrize("key,blocks,mode", CASES, ids=IDS)
def test_three_steps_repeat_bit_for_bit(key, blocks, mode):
    first, _, _, layers, _ = _checked(key, blocks, mode)
    again = _run(key, mode, blocks, False)[0]
    for step, (a, b) in enumerate(zip(first, again)):
        for k in ("loss4", "grads", "params"):
            assert torch.equal(a[k], b[k]), (key, blocks, mode, step, k, float((a[k].double() - b[k].double()).abs().max()))
        for L in layers:
            for u, v in zip(_layer_grads(a, L), _layer_grads(b, L)):
                assert torch.equal(u, v), (key, blocks, mode, step, L["name"])


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_up_layers_one_slab_per_tile(mode):
    B, H, W, sn, P, _ = SHAPES["deep"]
    cfg = _cfg("deep")
    grids = {}
    for blocks in (1 << 20, 256, 8):
        snaps, _, _, layers, model = _checked("deep", blocks, mode) if blocks in BLOCKS else _run("deep", mode, blocks, False)
        grids[blocks] = snaps[0]
        up = {L.layer: L for L in launch_model(cfg, B, H, W, mode == "bf16", dict(dwbx_blocks=blocks), 0)[0]
              if L.fam == "conv_dwbx_k" and L.layer in ("dec0.up", "dec1.up")}
        assert len(up) == 2 and all((L.grid == L.total) == (blocks != 8) for L in up.values()), (blocks, up)
    names = [sp.name for sp in on.build_plan(cfg)]
    checked = 0
    for L in layers:
        if L["name"] not in ("dec0.up", "dec1.up"):
            continue
        ref_k, ref_b = (t.double() for t in _layer_grads(grids[1 << 20], L))
        # the scale of the bias accumulation, sum |dz| per channel, from the layer-local model of the last checked run (the
        # forward pass, and with it dz, does not depend on the grid): layer_local's own bias rule
        li = names.index(L["name"])
        dabs = float(sum(model._dz(li, lo, hi)[0].abs().sum((0, 1, 2)) for lo, hi in model._chunks()).max())
        tk = ll.PARAM_RTOL * float(ref_k.abs().max())
        tb = (1e-5 if mode == "bf16" else ll.PARAM_RTOL) * dabs + (1e-7 if mode == "bf16" else 0.0)
        for blocks in (256, 8):
            k, b = (t.double() for t in _layer_grads(grids[blocks], L))
            ek, eb = float((k - ref_k).abs().max()), float((b - ref_b).abs().max())
            print(f"{L['name']} {mode} dwbx_blocks {blocks} vs one slab per tile: dW {ek:.3e} (allowed {tk:.3e}), bias {eb:.3e} (allowed {tb:.3e})")
            assert ek <= tk and eb <= tb, (L["name"], blocks, ek, tk, eb, tb)
            checked += 1
    assert checked == 4
