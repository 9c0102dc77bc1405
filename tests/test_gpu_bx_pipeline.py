"""The wide bf16-pipe conv kernel's pipeline: unconditional staging loads, the one-trip prologue and the stride-2 tile ring
("bx_down2_ring").

conv_bx_k requests its input tiles by unconditional loads (an item outside the image reads a clamped address and is
discarded) and its prologue requests the first slab, the first tile and the affine rows before its first wait; the
barriers of its (K chunk, tap row) pipeline are raw barriers behind explicit waits.  A fragment read before its slab
landed, a tile converted before it arrived, or a staging load that took a clamped address for a real one would change
stored numbers.  The stride-2 forms (backward-data of the up-convolutions) run a resident grid
of blocks that walk (image, tile) items: the next item's first K chunk is requested, converted into the free input image and
its first slab copied while the current item's last tap row is multiplied, and the epilogue scratch moves to the slab slot
that row just freed.  "persistent_max_blocks" caps that grid, so small images make a block walk several items and cross
image boundaries.  Every case

  * runs its first training step through the layer-local fp64 model (tests/layer_local.py, as tests/test_gpu_tile_walk.py
    runs a case): every stored tensor element by element, gates unchanged;
  * runs three training steps (forward, Dice loss, backward, Adam) with the ring on and off (one block per item) on fresh
    handles with the same seeds, inputs and cap, and asks for torch.equal after EVERY step on every layer's z, gradient buffer and BN record, the probabilities, the loss, the gradients and the updated
    parameters -- a stale read in step n shows in step n + 1 at the latest;
  * asserts from the step's profile that the kernel forms it is meant for ran.

Shapes (B, H, W, start_neurons, pool_layers), fp32 and bf16 storage each:
  single   3 x 36x72, 16, 1   dec0.up's backward-data is the stride-2 form with ONE K chunk (K = 16, M = 32); its low-res
                              grid 18x36 is 5 x 2 tiles of 4x32, ragged in both directions: 30 items.  Cap 4: 8/8/7/7 items
                              per block, items crossing images; cap 64: one item per block
  two      3 x 36x72, 32, 1   the stride-2 form with two chunks and the 64-row M block; 3x3 forward and backward-data forms
                              with 2 and 4 chunks, one of them over a concat input; the up-conv forward
  deep     2 x 48x96, 8, 4    up to 16 chunks, tile rows of 3 < TH, both stride-2 M blocks (4, 6 and 24 items)
"two" and "deep" run under cap 4 as well: without it their grids hold one block per item."""
import time

import numpy as np
import pytest
import torch

from oracle import unet_numpy as on
from tests import layer_local as ll
from tests.tile_walk import C, DROP_STEP, ENGINE_SEED, ROLL

pytestmark = pytest.mark.gpu

SHAPES = {"single": (3, 36, 72, 16, 1, 41), "two": (3, 36, 72, 32, 1, 42), "deep": (2, 48, 96, 8, 4, 43)}
BWD3 = ("conv_bx_k<3,0,1,", "conv_bx_k<3,0,2,")          # 3x3 backward-data: raw or masked epilogue
# kernel-name prefixes (conv_bx_k<KH,AMODE,EPI,TH,MB,...) of which each must have run; a tuple = any of its members
WANT = {"single": ["conv_bx_k<3,2,2,4,32,"],
        "two": ["conv_bx_k<3,2,2,4,64,", "conv_bx_k<3,0,0,", "conv_bx_k<2,1,0,", BWD3],
        "deep": ["conv_bx_k<3,2,2,4,32,", "conv_bx_k<3,2,2,4,64,", "conv_bx_k<3,0,0,", "conv_bx_k<2,1,0,", BWD3]}
STEPS = 3
CASES = [("single", 4), ("single", 64), ("two", 4), ("deep", 4)]


def _snapshot(eng, B, probs, loss4):
    nb = len(eng.layers) - 1
    torch.cuda.synchronize()
    return {"z": [eng.debug_activation(li, 0)[:B].clone() for li in range(nb)],
            "gbuf": [eng.debug_activation(li, 1)[:B].clone() for li in range(nb)],
            "rec": [eng.debug_bn_record(li).clone() for li in range(nb)],
            "probs": probs.clone(), "loss4": loss4.clone(), "grads": eng.grads.clone()}


def _run(key, mode, cap, on_, check_layers):
    from oct_image_segmentation_models_amd import _hip
    from oct_image_segmentation_models_amd.engine import UNetEngine
    from tests.test_gpu_layer_local import _finish, _params_from_engine, ragged_scans
    from tests.test_gpu_tile_walk import options
    t0 = time.time()
    B, H, W, sn, P, seed = SHAPES[key]
    cfg = on.UNetConfig(num_classes=C, start_neurons=sn, pool_layers=P)
    params, state = on.init_params(cfg, seed=7, dtype=np.float32, randomize_bn=True)
    img, lab = ragged_scans(B, H, W, seed, ROLL)
    x = torch.from_numpy(img).cuda(); l = torch.from_numpy(lab[..., 0].copy()).cuda()
    with options(dict(bx_down2_ring=on_, persistent_max_blocks=cap)):
        mm = _hip.get_option("mfma_mode")
        eng = UNetEngine(training=True, device="cuda:0", input_channels=1, num_classes=C, image_height=H, image_width=W, max_batch=B,
                         start_neurons=sn, pool_layers=P, seed=ENGINE_SEED, init_seed=1, dtype="bfloat16" if mode == "bf16" else "float32")
    assert eng.handle_option("bx_down2_ring") == on_
    assert eng.handle_option("persistent_max_blocks") == cap and _hip.get_option("bx_down2_ring") == 1
    eng.set_weights(on.keras_weight_list(params, state))
    snaps, ents = [], None
    for step in range(STEPS):
        eng.set_dropout_step(DROP_STEP + step)
        if step == 0:
            eng.profile_begin()
        probs, _ = eng.forward(x, training=True, labels=l)
        loss4 = eng.loss_dice()
        eng.backward(l, macro=True, loss_scale=1.0)
        if step == 0:
            ents = eng.profile_end()
        snaps.append(_snapshot(eng, B, probs, loss4))
        if step == 0 and check_layers:
            mask = eng.dropout_mask(B).double()
            p64, _ = _params_from_engine(eng)
            S = ll.engine_stored(eng, B, probs)
            rep = ll.LayerLocal(cfg, p64, S, img, labels=lab[..., 0], dropout_mask=mask, mode=mode, mfma_mode=mm, device="cuda:0").run()
            _finish(rep, t0, f"{key} {mode} cap {cap} ring {on_} (training step 1)")
        eng.adam_step()
        torch.cuda.synchronize()
        snaps[-1]["params"] = eng.params.clone()
    return snaps, ents


@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("key,cap", CASES, ids=[f"{k}-cap{c}" for k, c in CASES])
def test_tile_ring_changes_nothing(key, cap, mode):
    new, ents = _run(key, mode, cap, 1, True)
    old, ents_old = _run(key, mode, cap, 0, False)
    ran = sorted({e["kernel"] for e in ents if e["kernel"].startswith("conv_bx_k<")})
    print(f"\n{key} {mode}: conv_bx_k forms of the step")
    for e in ents:
        if e["kernel"].startswith("conv_bx_k<"):
            print(f"    {e['kernel']:56s} {e['layer']:12s} x{e['launches']}")
    assert ran == sorted({e["kernel"] for e in ents_old if e["kernel"].startswith("conv_bx_k<")})
    for want in WANT[key]:
        assert any(k.startswith(want) for k in ran), (want, ran)
    # the stride-2 forms keep two input images and four waves, with the transform on load
    assert all(k.endswith(",gb>") and ",1img" not in k and k.split(",")[6] == "4" for k in ran if k.startswith("conv_bx_k<3,2,")), ran
    for step, (a, b) in enumerate(zip(new, old)):
        for k in ("loss4", "probs", "grads", "params"):
            assert torch.isfinite(a[k].float()).all(), (step, k)
            assert torch.equal(a[k], b[k]), (key, mode, step, k, float((a[k].double() - b[k].double()).abs().max()))
        for k in ("z", "gbuf", "rec"):
            for li, (u, v) in enumerate(zip(a[k], b[k])):
                assert torch.equal(u, v), (key, mode, step, k, li, float((u.double() - v.double()).abs().max()))
