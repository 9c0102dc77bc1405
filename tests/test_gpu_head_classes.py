"""GPU parity at the class counts and widths the other GPU tests never reach: num_classes 5 .. 8 and start_neurons 20 / 24 / 28.

num_classes >= 5 changes real code in the head: the per-block Dice partial row is 32 floats wide for C = 4 .. 6 and 64 for
C = 7, 8 (DiceN<C>, kernels_head.hpp; the focal sum sits at slot 5 C), head_bwd_k keeps CIN * C + C partial sums in
registers and reduces them in groups of 32 with a ragged last group (264 values at CIN 32, C 8), dice_finalize_k indexes
its per-(image, class) sums by B * C.  start_neurons 20 / 24 / 28 give the wide MFMA kernel K = 80 / 48 / 112 input
channels (multiples of 8 but not of 16 or 32) and send the backward-weights of those layers to conv_dw32_k with a ragged
last 32-channel chunk.

Tolerances are those of tests/test_gpu_parity.py (fp64 oracle, margin seeds) and tests/layer_local.py (layer-local gates);
nothing here is tuned."""
import time

import numpy as np
import pytest
import torch

from oracle import unet_numpy as on
from tests import layer_local as ll
from tests.helpers import relu_margin
from tests.test_gpu_parity import (DICE_TOL, DROP_STEP, GRAD_RTOL, PROB_TOL, bf16_step_layer_local,  # noqa: F401
                                   check_grads_vs_oracle, data, make, make_bf16, training_step_vs_oracle)

pytestmark = pytest.mark.gpu

# B, H, W, C, sn, P, L, in_ch -> data seed with a ReLU margin > 2e-5 (tools/find_margin_seed.py, oracle only; re-asserted
# by the tests)
HEAD_CASES = {
    (1, 32, 64, 5, 8, 2, 2, 1): 63,       # 3.25e-5
    (1, 32, 64, 5, 28, 1, 1, 1): 55,      # 3.94e-5; 28-channel head
    (1, 32, 64, 6, 16, 1, 2, 1): 36,      # 2.59e-5
    (2, 32, 64, 7, 8, 2, 2, 1): 238,      # 4.36e-5; 64-wide Dice partial rows, two images
    (2, 32, 64, 8, 8, 2, 2, 1): 194,      # 2.61e-5
    (1, 32, 64, 8, 12, 2, 2, 1): 328,     # 3.30e-5; 12-channel head
    (1, 32, 64, 8, 32, 1, 1, 1): 141,     # 2.54e-5; CIN 32, C 8: the 264-value head_bwd_k
}
CASES = list(HEAD_CASES)


@pytest.mark.parametrize("macro", [True, False])
@pytest.mark.parametrize("case", CASES)
def test_training_step_matches_oracle_for_5_to_8_classes(case, macro):
    B, H, W, C, sn, P, L, ic = case
    cfg, eng, p64, s64 = make(B, H, W, C, sn, P, L, ic, training=True)
    images, labels = data(B, H, W, C, ic, seed=HEAD_CASES[case])
    assert set(np.unique(labels)) == set(range(C))            # every class occurs (the absent-class test edits this)
    eng.profile_begin()
    training_step_vs_oracle(cfg, eng, p64, s64, case, images, labels, macro, "default")
    kernels = {e["kernel"] for e in eng.profile_end()}
    assert {f"head_fwd_k<{C},{sn},float>", f"head_bwd_k<{C},{sn},float>"} <= kernels, sorted(kernels)


@pytest.mark.parametrize("case", CASES)
def test_inference_forward_matches_oracle_for_5_to_8_classes(case):
    B, H, W, C, sn, P, L, ic = case
    cfg, eng, p64, s64 = make(B, H, W, C, sn, P, L, ic, training=False)
    images, labels = data(B, H, W, C, ic, seed=HEAD_CASES[case])
    x = torch.from_numpy(images).cuda()
    probs, am = eng.forward(x, training=False, want_argmax=True)
    ref, cache = on.forward(cfg, p64, s64, on.preprocess_u8(images, np.float64), training=False)
    for li, spec in enumerate(on.build_plan(cfg)[:-1]):
        z = eng.debug_activation(li, 0)[:B].cpu().numpy()
        scale = max(1.0, np.abs(cache[li]["z"]).max())
        assert np.abs(z - cache[li]["z"]).max() / scale < 1e-4, f"layer {li} {spec.name} pre-BN output differs"
    assert np.abs(probs.cpu().numpy() - ref).max() < PROB_TOL
    # identical argmax except at numerical ties
    diff = am.cpu().numpy() != ref.argmax(-1)
    if diff.any():
        srt = np.sort(ref, -1)
        assert (srt[..., -1] - srt[..., -2])[diff].max() < 1e-4
    assert int(am.max()) < C


def _step(case, labels, macro, focal=None):
    """One training step on the case's margin-seed images with the given label maps: (engine, probs, oracle probs,
    oracle gradients)."""
    B, H, W, C, sn, P, L, ic = case
    cfg, eng, p64, s64 = make(B, H, W, C, sn, P, L, ic, training=True)
    images, _ = data(B, H, W, C, ic, seed=HEAD_CASES[case])
    x = torch.from_numpy(images).cuda(); lab = torch.from_numpy(labels[..., 0].copy()).cuda()
    eng.set_dropout_step(DROP_STEP)
    mask = eng.dropout_mask(B).cpu().numpy().astype(np.float64)
    if focal is not None:
        eng.set_focal_dice(*focal)
    probs, _ = eng.forward(x, training=True, labels=lab)
    v = (eng.loss_focal_dice() if focal is not None else eng.loss_dice()).cpu().numpy()
    eng.backward(lab, macro=macro, loss_scale=0.5)
    torch.cuda.synchronize()
    ref, cache = on.forward(cfg, p64, s64, on.preprocess_u8(images, np.float64), training=True, dropout_mask=mask)
    assert relu_margin(cfg, p64, cache) > 2e-5
    assert np.abs(probs.cpu().numpy() - ref).max() < PROB_TOL
    kw = {} if focal is None else dict(focal=focal)
    _, grads = on.backward(cfg, p64, cache, labels, macro=macro, loss_scale=0.5, **kw)
    return eng, v, ref, grads


@pytest.mark.parametrize("macro", [True, False])
def test_focal_dice_loss_with_eight_class_weights(macro):
    """focal_dice_loss at C = 8 with eight distinct class weights: the focal sum sits behind the 5 C Dice sums of the
    64-wide partial row.  The seven loss values and every gradient, as test_focal_dice_loss_and_gradients_match_oracle."""
    case = (2, 32, 64, 8, 8, 2, 2, 1)
    C = case[3]
    fw, gamma, cw = 0.35, 2.0, (0.5, 2.0, 1.25, 0.75, 3.0, 1.5, 0.25, 1.75)
    _, labels = data(case[0], case[1], case[2], C, 1, seed=HEAD_CASES[case])
    eng, v, ref, grads = _step(case, labels, macro, focal=(fw, gamma, cw))
    y = on.one_hot(labels, C, np.float64)
    focal = on.focal_loss_mean(labels, ref, gamma, cw)
    assert abs(v[0] - on.dice_loss_macro(y, ref)) < 1e-5 and abs(v[1] - on.dice_loss_micro(y, ref)) < 1e-5
    assert abs(v[2] - on.dice_coef_macro(y, ref)) < DICE_TOL and abs(v[3] - on.dice_coef_micro(y, ref)) < DICE_TOL
    assert abs(v[4] - focal) < 1e-5 * max(1.0, focal)
    assert abs(v[5] - on.focal_dice_loss(labels, ref, C, gamma, cw, fw, True)) < 1e-5
    assert abs(v[6] - on.focal_dice_loss(labels, ref, C, gamma, cw, fw, False)) < 1e-5
    check_grads_vs_oracle(eng, grads)


def _absent_everywhere(labels, C):
    lab = labels.copy(); lab[lab == C - 1] = C - 2            # class C - 1 merged into C - 2: T = 0 for every image
    return lab


def _absent_in_one_image(labels, C):
    lab = labels.copy(); lab[0][lab[0] == C - 1] = C - 2      # ... for image 0 only
    return lab


def _one_image_single_class(labels, C):
    lab = labels.copy(); lab[1] = 3                            # every pixel of image 1 one class: T = 0 for all others
    return lab


@pytest.mark.parametrize("macro", [True, False])
@pytest.mark.parametrize("edit", [_absent_everywhere, _absent_in_one_image, _one_image_single_class])
@pytest.mark.parametrize("C", [7, 8])
def test_absent_classes(C, edit, macro):
    """Label maps in which a class does not occur (per-(image, class) T = 0: the Dice term is s / (P + s)): the ReLU
    margin depends on the images only, so the labels of the margin-seed cases may be edited freely.  Losses, Dice
    coefficients and every gradient against the oracle."""
    case = (2, 32, 64, C, 8, 2, 2, 1)
    _, labels = data(2, 32, 64, C, 1, seed=HEAD_CASES[case])
    labels = edit(labels, C)
    counts = np.stack([np.bincount(labels[b].ravel(), minlength=C) for b in range(2)])
    assert (counts == 0).any()
    eng, v, ref, grads = _step(case, labels, macro)
    y = on.one_hot(labels, C, np.float64)
    assert abs(v[0] - on.dice_loss_macro(y, ref)) < 1e-5 and abs(v[1] - on.dice_loss_micro(y, ref)) < 1e-5
    assert abs(v[2] - on.dice_coef_macro(y, ref)) < DICE_TOL
    assert np.allclose(v[3], on.dice_coef_micro(y, ref), rtol=0, atol=DICE_TOL, equal_nan=True)
    assert np.isfinite(eng.grads.cpu().numpy()).all()
    check_grads_vs_oracle(eng, grads)


@pytest.mark.parametrize("C", [5, 6, 7, 8])
def test_boundary_maps_for_5_to_8_classes(C):
    """Arg-max -> boundary maps on the device for n_cls 5 .. 8, bit-exact against the numpy restatement of the reference's
    definition, the three background settings, including a class that never occurs."""
    cfg, eng, _, _ = make(2, 32, 64, C, 8, 2, training=False)
    rng = np.random.default_rng(C)
    _, smooth = on.synth_scans(3, 32, 64, C, seed=6)
    missing = smooth[..., 0].copy(); missing[missing == 2] = 1                  # class 2 never occurs
    edge = np.zeros((2, 32, 64), np.uint8); edge[0, 1:, :] = 1; edge[1, :-1, :] = C - 2; edge[1, -1, :] = C - 1
    for lab in (smooth[..., 0], missing, rng.integers(0, C, (3, 32, 64)).astype(np.uint8), edge):
        cat = np.transpose(np.eye(C, dtype=np.float32)[lab], (0, 3, 1, 2))
        for kw in (dict(bg_ilm=True, bg_csi=False), dict(bg_ilm=False, bg_csi=True), dict(bg_ilm=True, bg_csi=True)):
            with np.errstate(invalid="ignore"):
                ref = on.convert_predictions_to_maps_semantic(cat, **kw)
            got = eng.boundary_maps(torch.from_numpy(np.ascontiguousarray(lab)).cuda(), **kw).cpu().numpy()
            assert got.shape == ref.shape and np.array_equal(got, ref), (C, kw)


def test_bf16_storage_with_eight_classes():
    """The C = 8, start_neurons 8 case in bf16 storage through the layer-local one-rounding checks (head arithmetic is
    fp32: probabilities within 2e-4 of the softmax of the recomputed logits)."""
    from oct_image_segmentation_models_amd import _hip
    case = (2, 32, 64, 8, 8, 2, 2, 1)
    B, H, W, C, sn, P, L, ic = case
    try:
        _hip.set_option("fuse_first_apply", 0); _hip.set_option("fuse_bn_apply", 0)     # (every block's dz is stored)
        cfg, eng, p64, s64 = make_bf16(B, H, W, C, sn, P, L, ic)
    finally:
        _hip.set_option("fuse_first_apply", 1); _hip.set_option("fuse_bn_apply", 1)
    images, labels = data(B, H, W, C, ic, seed=HEAD_CASES[case])
    eng.profile_begin()
    bf16_step_layer_local(cfg, eng, p64, case, images, labels)
    kernels = {e["kernel"] for e in eng.profile_end()}
    assert {"head_fwd_k<8,8,unsigned short>", "head_bwd_k<8,8,unsigned short>"} <= kernels, sorted(kernels)


# ---- start_neurons 20 / 24 / 28 -------------------------------------------------------------------------------------
# No data seed in 1 .. 399 keeps these nets 2e-5 away from every ReLU kink (oracle search), so the backward pass is held
# to the layer-local harness (every layer recomputed in fp64 from the engine's own stored inputs, mask / route decisions
# within fp32 rounding excluded and counted) and only the forward to the oracle itself.
# (sn, P) -> the layers whose forward must run on conv_bx_k with K = 2 sn .. input channels that no other test reaches
WIDE = {(24, 2): {"mid.conv0": (48, 96), "mid.conv1": (96, 96)},
        (20, 3): {"mid.conv0": (80, 160), "mid.conv1": (160, 160)},
        (28, 3): {"mid.conv0": (112, 224), "mid.conv1": (224, 224)}}


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("sn,P", list(WIDE))
def test_start_neurons_20_24_28(sn, P, B, dtype):
    from oct_image_segmentation_models_amd import _hip
    t0 = time.time()
    H, W, C = 32, 64, 3
    bf = dtype == "bf16"
    cfg, eng, p64, s64 = (make_bf16 if bf else make)(B, H, W, C, sn, P)
    images, labels = data(B, H, W, C, 1, seed=17 + B)
    x = torch.from_numpy(images).cuda(); lab = torch.from_numpy(labels[..., 0].copy()).cuda()
    eng.set_dropout_step(DROP_STEP)
    mask = eng.dropout_mask(B).double()
    eng.profile_begin()
    probs, _ = eng.forward(x, training=True, labels=lab)
    eng.loss_dice()
    eng.backward(lab, macro=True, loss_scale=1.0)
    ents = eng.profile_end()
    by_layer = {}
    for e in ents:
        by_layer.setdefault(e["layer"], []).append(e["kernel"])
    for name, (cin, cout) in WIDE[(sn, P)].items():
        L_ = next(l for l in eng.layers if l["name"] == name)
        assert (L_["cin"], L_["cout"]) == (cin, cout)
        ks = by_layer[name]
        fwd = [k for k in ks if k.startswith("conv_bx_k<3,") and k.split(",")[2] == "0"]
        print(f"sn={sn} P={P} B={B} {dtype} {name} {cin}->{cout}: {sorted(ks)}")
        assert len(fwd) == 1, (name, ks)                          # the wide kernel ran this layer's forward
        dw = [k for k in ks if k.startswith(("conv_dw", "conv_bwd_w"))]
        assert len(dw) == 1, (name, ks)
        if cin % 32:     # dw_plan: conv_dwbx_k wants 32-divisible channels; these go to the fp32-pipe kernel, last chunk ragged
            assert dw[0].startswith("conv_dw32_k"), (name, dw)
    assert f"head_fwd_k<{C},{sn},{'unsigned short' if bf else 'float'}>" in by_layer["head"], by_layer["head"]

    if not bf:           # forward against the oracle itself (needs no margin)
        ref, cache = on.forward(cfg, p64, s64, on.preprocess_u8(images, np.float64), training=True,
                                dropout_mask=mask.cpu().numpy())
        for li, spec in enumerate(on.build_plan(cfg)[:-1]):
            z = eng.debug_activation(li, 0)[:B].cpu().numpy()
            scale = max(1.0, np.abs(cache[li]["z"]).max())
            assert np.abs(z - cache[li]["z"]).max() / scale < 1e-4, f"layer {li} {spec.name} pre-BN output differs"
        assert np.abs(probs.cpu().numpy() - ref).max() < PROB_TOL
    S = ll.engine_stored(eng, B, probs)
    rep = ll.LayerLocal(cfg, p64, S, images, labels=labels[..., 0], dropout_mask=mask, mode=dtype,
                        mfma_mode=_hip.get_option("mfma_mode"), device="cuda:0", wide_rel_l2=True).run()
    title = f"start_neurons {sn} P={P} B={B} {dtype}"
    K = max(sp.kh * sp.kw * sp.cin for sp in on.build_plan(cfg))
    print(f"\n{title}: per-layer worst err / bound, relative L2 ('.L2'; gate {ll.rel_l2_gate(K):.3g} at the widest layer, K = {K}: "
          f"estimate {ll.rel_l2_gate(K) / ll.REL_L2_RATIO:.3g})")
    print(rep.table())
    print(f"{title}: wall time {time.time() - t0:.1f} s")
    assert not rep.failures, "\n".join(rep.failures[:20])
