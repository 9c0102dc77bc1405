"""GPU parity of start_neurons 36 .. 64 and of the channel-streaming head kernels that carry them
(head_fwd_wide_k / head_bwd_wide_k<C, AT>, csrc/kernels_head_wide.hpp: the head's input channel count is a run-time
argument, the sums over pixels are formed on the fp32 matrix pipe).

Tolerances are those of tests/test_gpu_parity.py (fp64 oracle, margin seeds) and tests/layer_local.py (layer-local gates);
nothing here is tuned.  Under option "head_wide" the same kernels also run the verified narrow cases of
tests/test_gpu_head_classes.py, where the register kernels are the default."""
import time

import numpy as np
import pytest
import torch

from oracle import unet_numpy as on
from tests import layer_local as ll
from tests.helpers import relu_margin
from tests.test_gpu_bce_dice_loss import autograd_oracle, bce_step, check_values
from tests.test_gpu_head_classes import HEAD_CASES
from tests.test_gpu_parity import (DICE_TOL, DROP_STEP, GRAD_RTOL, PROB_TOL, bf16_step_layer_local,  # noqa: F401
                                   check_grads_vs_oracle, data, make, make_bf16, training_step_vs_oracle)

pytestmark = pytest.mark.gpu

# B, H, W, C, sn, P, L, in_ch -> data seed with a ReLU margin > 2e-5 (tools/find_margin_seed.py ... 2e-5, oracle only;
# re-asserted by the tests)
WIDE_CASES = {
    (1, 16, 32, 3, 64, 1, 1, 1): 1,       # 2.95e-5; the widest head; 512 pixels = 2 chunks
    (1, 16, 32, 8, 40, 1, 1, 1): 6,       # 4.06e-5; all 8 classes occur: 64-wide Dice row; CIN 40 = 2 1/2 groups of 16
    (2, 18, 34, 5, 48, 1, 1, 1): 19,      # 2.34e-5; 612 pixels per image: two full chunks and a ragged one of 100; two images
    (1, 16, 32, 4, 44, 1, 2, 1): 16,      # 2.98e-5; 44 is not a multiple of 8
    (1, 16, 32, 3, 64, 2, 2, 1): 56,      # 4.24e-5; two levels, 256-channel bottleneck
}
CASES = list(WIDE_CASES)
SN64, SN40_C8, SN48, SN64_P2 = CASES[0], CASES[1], CASES[2], CASES[4]
# the verified narrow cases the wide kernels are held to under "head_wide" = 1
NARROW = [(2, 32, 64, 8, 8, 2, 2, 1), (1, 32, 64, 8, 32, 1, 1, 1), (1, 32, 64, 5, 28, 1, 1, 1)]
assert [HEAD_CASES[c] for c in NARROW] == [194, 141, 55]


def wide_names(C, sn, at="float"):
    return {f"head_fwd_wide_k<{C},{sn},{at}>", f"head_bwd_wide_k<{C},{sn},{at}>"}


def assert_wide_route(kernels, C, sn, at="float", training=True):
    want = wide_names(C, sn, at) if training else {f"head_fwd_wide_k<{C},{sn},{at}>"}
    assert want <= kernels, sorted(kernels)
    assert not [k for k in kernels if k.startswith(("head_fwd_k<", "head_bwd_k<"))], sorted(kernels)


def case_data(case):
    B, H, W, C, sn, P, L, ic = case
    images, labels = data(B, H, W, C, ic, seed=WIDE_CASES[case])
    assert set(np.unique(labels)) == set(range(C))            # every class occurs
    return images, labels


@pytest.mark.parametrize("macro", [True, False])
@pytest.mark.parametrize("case", CASES)
def test_training_step_matches_oracle(case, macro):
    B, H, W, C, sn, P, L, ic = case
    cfg, eng, p64, s64 = make(B, H, W, C, sn, P, L, ic, training=True)
    images, labels = case_data(case)
    eng.profile_begin()
    training_step_vs_oracle(cfg, eng, p64, s64, case, images, labels, macro, "default")
    assert_wide_route({e["kernel"] for e in eng.profile_end()}, C, sn)


@pytest.mark.parametrize("case", CASES)
def test_inference_forward_matches_oracle(case):
    B, H, W, C, sn, P, L, ic = case
    cfg, eng, p64, s64 = make(B, H, W, C, sn, P, L, ic, training=False)
    images, labels = case_data(case)
    x = torch.from_numpy(images).cuda()
    eng.profile_begin()
    probs, am = eng.forward(x, training=False, want_argmax=True)
    assert_wide_route({e["kernel"] for e in eng.profile_end()}, C, sn, training=False)
    ref, cache = on.forward(cfg, p64, s64, on.preprocess_u8(images, np.float64), training=False)
    for li, spec in enumerate(on.build_plan(cfg)[:-1]):
        z = eng.debug_activation(li, 0)[:B].cpu().numpy()
        scale = max(1.0, np.abs(cache[li]["z"]).max())
        assert np.abs(z - cache[li]["z"]).max() / scale < 1e-4, f"layer {li} {spec.name} pre-BN output differs"
    assert np.abs(probs.cpu().numpy() - ref).max() < PROB_TOL
    diff = am.cpu().numpy() != ref.argmax(-1)                 # identical argmax except at numerical ties
    if diff.any():
        srt = np.sort(ref, -1)
        assert (srt[..., -1] - srt[..., -2])[diff].max() < 1e-4
    assert int(am.max()) < C
    if case == SN64:                                          # the wide forward records into a graph: replay = eager, bit for bit
        eager_am = am.clone()
        xb = x.clone()
        gp, gam = eng.graph_capture(xb, want_probs=True, want_argmax=True)
        eng.graph_launch(); torch.cuda.synchronize()
        assert torch.equal(gp, probs) and torch.equal(gam, eager_am)
        gp.zero_(); eng.graph_launch(); torch.cuda.synchronize()
        assert torch.equal(gp, probs)


def _step(case, labels, macro, focal=None):
    """One training step on the case's margin-seed images with the given label maps: (engine, loss vector, oracle
    probabilities, oracle gradients)."""
    B, H, W, C, sn, P, L, ic = case
    cfg, eng, p64, s64 = make(B, H, W, C, sn, P, L, ic, training=True)
    images, _ = data(B, H, W, C, ic, seed=WIDE_CASES[case])
    x = torch.from_numpy(images).cuda(); lab = torch.from_numpy(labels[..., 0].copy()).cuda()
    eng.set_dropout_step(DROP_STEP)
    mask = eng.dropout_mask(B).cpu().numpy().astype(np.float64)
    if focal is not None:
        eng.set_focal_dice(*focal)
    eng.profile_begin()
    probs, _ = eng.forward(x, training=True, labels=lab)
    v = (eng.loss_focal_dice() if focal is not None else eng.loss_dice()).cpu().numpy()
    eng.backward(lab, macro=macro, loss_scale=0.5)
    torch.cuda.synchronize()
    assert_wide_route({e["kernel"] for e in eng.profile_end()}, C, sn)
    ref, cache = on.forward(cfg, p64, s64, on.preprocess_u8(images, np.float64), training=True, dropout_mask=mask)
    assert relu_margin(cfg, p64, cache) > 2e-5
    assert np.abs(probs.cpu().numpy() - ref).max() < PROB_TOL
    kw = {} if focal is None else dict(focal=focal)
    _, grads = on.backward(cfg, p64, cache, labels, macro=macro, loss_scale=0.5, **kw)
    return eng, v, ref, grads


@pytest.mark.parametrize("macro", [True, False])
def test_focal_dice_loss_with_eight_class_weights(macro):
    """focal_dice_loss at C = 8, start_neurons 40, eight distinct class weights: the seven loss values and every gradient."""
    case = SN40_C8
    C = case[3]
    fw, gamma, cw = 0.35, 2.0, (0.5, 2.0, 1.25, 0.75, 3.0, 1.5, 0.25, 1.75)
    _, labels = case_data(case)
    eng, v, ref, grads = _step(case, labels, macro, focal=(fw, gamma, cw))
    y = on.one_hot(labels, C, np.float64)
    focal = on.focal_loss_mean(labels, ref, gamma, cw)
    assert abs(v[0] - on.dice_loss_macro(y, ref)) < 1e-5 and abs(v[1] - on.dice_loss_micro(y, ref)) < 1e-5
    assert abs(v[2] - on.dice_coef_macro(y, ref)) < DICE_TOL and abs(v[3] - on.dice_coef_micro(y, ref)) < DICE_TOL
    assert abs(v[4] - focal) < 1e-5 * max(1.0, focal)
    assert abs(v[5] - on.focal_dice_loss(labels, ref, C, gamma, cw, fw, True)) < 1e-5
    assert abs(v[6] - on.focal_dice_loss(labels, ref, C, gamma, cw, fw, False)) < 1e-5
    check_grads_vs_oracle(eng, grads)


@pytest.mark.parametrize("inner_eps", [1, 0])
def test_bce_dice_loss_at_64_channels(inner_eps):
    """bce_dice_loss on the widest head, both settings of "bce_inner_eps", against torch-fp64 autograd with the same setting
    (tests/test_gpu_bce_dice_loss.py)."""
    case = SN64
    B, H, W, C, sn, P, L, ic = case
    cfg, eng, p64, s64 = make(B, H, W, C, sn, P, L, ic, training=True)
    images, labels = case_data(case)
    eng.set_option("bce_inner_eps", inner_eps)
    eng.set_bce_dice(True)
    eng.profile_begin()
    probs, v, mask = bce_step(eng, images, labels, 0.5)
    assert_wide_route({e["kernel"] for e in eng.profile_end()}, C, sn)
    _, cache = on.forward(cfg, p64, s64, on.preprocess_u8(images, np.float64), training=True, dropout_mask=mask)
    assert relu_margin(cfg, p64, cache) > 2e-5
    bce, dice, ref, grads = autograd_oracle(cfg, p64, s64, images, labels, mask, 0.5, inner_eps=bool(inner_eps))
    assert np.abs(probs.cpu().numpy() - ref).max() < PROB_TOL
    check_values(v, labels, ref, bce, dice, C)
    worst = check_grads_vs_oracle(eng, grads)
    print(f"{case} bce_inner_eps={inner_eps}: worst gradient piece error {worst:.3g} (GRAD_RTOL {GRAD_RTOL})")


def _absent_everywhere(labels, C):
    lab = labels.copy(); lab[lab == C - 1] = C - 2            # class C - 1 merged into C - 2: T = 0 for every image
    return lab


def _absent_in_one_image(labels, C):
    lab = labels.copy(); lab[0][lab[0] == C - 1] = C - 2      # ... for image 0 only
    return lab


def _one_image_single_class(labels, C):
    lab = labels.copy(); lab[1] = C - 2                        # every pixel of image 1 one class: T = 0 for all others
    return lab


@pytest.mark.parametrize("macro", [True, False])
@pytest.mark.parametrize("edit", [_absent_everywhere, _absent_in_one_image, _one_image_single_class])
def test_absent_classes(edit, macro):
    """Label maps in which a class does not occur, on the start_neurons 48 case (C = 5, two images, ragged last chunk): the
    ReLU margin depends on the images only, so the labels may be edited freely."""
    case = SN48
    B, H, W, C = case[:4]
    _, labels = case_data(case)
    labels = edit(labels, C)
    counts = np.stack([np.bincount(labels[b].ravel(), minlength=C) for b in range(B)])
    assert (counts == 0).any()
    eng, v, ref, grads = _step(case, labels, macro)
    y = on.one_hot(labels, C, np.float64)
    assert abs(v[0] - on.dice_loss_macro(y, ref)) < 1e-5 and abs(v[1] - on.dice_loss_micro(y, ref)) < 1e-5
    assert abs(v[2] - on.dice_coef_macro(y, ref)) < DICE_TOL
    assert np.allclose(v[3], on.dice_coef_micro(y, ref), rtol=0, atol=DICE_TOL, equal_nan=True)
    assert np.isfinite(eng.grads.cpu().numpy()).all()
    check_grads_vs_oracle(eng, grads)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_blocks_walk_chunks_unevenly(dtype):
    """B = 64, 64 x 160, start_neurons 40: 40 chunks of 256 pixels per image on 32 blocks per image (2048 / B), so blocks
    0 .. 7 take two chunks and the rest one -- the accumulators are carried across chunks in some blocks only.  No margin
    seed exists at this size: the backward pass is held to the layer-local harness (as test_start_neurons_20_24_28), the
    forward to the oracle itself in f32."""
    from oct_image_segmentation_models_amd import _hip
    t0 = time.time()
    B, H, W, C, sn, P, L = 64, 64, 160, 3, 40, 1, 1
    assert -(-H * W // 256) == 40 and min(40, -(-2048 // B)) == 32
    bf = dtype == "bf16"
    cfg, eng, p64, s64 = (make_bf16 if bf else make)(B, H, W, C, sn, P, L)
    images, labels = data(B, H, W, C, 1, seed=18)
    x = torch.from_numpy(images).cuda(); lab = torch.from_numpy(labels[..., 0].copy()).cuda()
    eng.set_dropout_step(DROP_STEP)
    mask = eng.dropout_mask(B).double()
    eng.profile_begin()
    probs, _ = eng.forward(x, training=True, labels=lab)
    eng.loss_dice()
    eng.backward(lab, macro=True, loss_scale=1.0)
    assert_wide_route({e["kernel"] for e in eng.profile_end()}, C, sn, "unsigned short" if bf else "float")
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
    title = f"start_neurons {sn} P={P} B={B} {H}x{W} {dtype}"
    print(f"\n{title}: per-layer worst err / bound")
    print(rep.table())
    print(f"{title}: wall time {time.time() - t0:.1f} s")
    assert not rep.failures, "\n".join(rep.failures[:20])


def _make_head_wide(case, **options):
    """An engine created under "head_wide" = 1 (+ other process defaults), which are restored before it is used."""
    from oct_image_segmentation_models_amd import _hip
    B, H, W, C, sn, P, L, ic = case
    options = dict(options, head_wide=1)
    old = {k: _hip.get_option(k) for k in options}
    try:
        for k, v in options.items():
            _hip.set_option(k, v)
        made = make(B, H, W, C, sn, P, L, ic, training=True)
    finally:
        for k, v in old.items():
            _hip.set_option(k, v)
    assert made[1].handle_option("head_wide") == 1 and _hip.get_option("head_wide") == 0
    return made


@pytest.mark.parametrize("macro", [True, False])
@pytest.mark.parametrize("case", NARROW)
def test_head_wide_option_on_verified_narrow_cases(case, macro):
    B, H, W, C, sn, P, L, ic = case
    cfg, eng, p64, s64 = _make_head_wide(case)
    images, labels = data(B, H, W, C, ic, seed=HEAD_CASES[case])
    assert set(np.unique(labels)) == set(range(C))
    eng.profile_begin()
    training_step_vs_oracle(cfg, eng, p64, s64, case, images, labels, macro, "default")
    assert_wide_route({e["kernel"] for e in eng.profile_end()}, C, sn)


def test_head_wide_leaves_the_finalize_to_its_own_launch():
    """ "fuse_bn_finalize" = 1 lets the register head kernel finalize the last block's BN-backward statistics; the wide
    kernels never do, so the stand-alone launch must have run for that block -- and the step still matches the oracle."""
    case = NARROW[0]
    B, H, W, C, sn, P, L, ic = case
    cfg, eng, p64, s64 = _make_head_wide(case, fuse_bn_finalize=1)
    assert eng.handle_option("fuse_bn_finalize") == 1
    images, labels = data(B, H, W, C, ic, seed=HEAD_CASES[case])
    eng.profile_begin()
    training_step_vs_oracle(cfg, eng, p64, s64, case, images, labels, True, "bn_finalize_in_launch")
    ents = eng.profile_end()
    assert_wide_route({e["kernel"] for e in ents}, C, sn)
    last = eng.layers[-2]["name"]
    fin = {e["layer"] for e in ents if e["kernel"] == "bn_bwd_finalize_k"}
    assert last in fin, (last, sorted(fin))
    assert len(fin) < len(eng.layers) - 1, sorted(fin)        # ... while other blocks were finalized inside their launches


def test_bf16_storage_at_64_channels():
    """The start_neurons 64 one-level case in bf16 storage through the layer-local one-rounding checks."""
    from oct_image_segmentation_models_amd import _hip
    case = SN64
    B, H, W, C, sn, P, L, ic = case
    try:
        _hip.set_option("fuse_first_apply", 0); _hip.set_option("fuse_bn_apply", 0)     # (every block's dz is stored)
        cfg, eng, p64, s64 = make_bf16(B, H, W, C, sn, P, L, ic)
    finally:
        _hip.set_option("fuse_first_apply", 1); _hip.set_option("fuse_bn_apply", 1)
    images, labels = case_data(case)
    eng.profile_begin()
    bf16_step_layer_local(cfg, eng, p64, case, images, labels)
    assert_wide_route({e["kernel"] for e in eng.profile_end()}, 3, sn, "unsigned short")


def test_two_runs_give_the_same_bits():
    """Every sum of the wide kernels is taken in a fixed order (no atomics): two fresh engines, same step, equal bits."""
    case = SN48
    B, H, W, C, sn, P, L, ic = case
    images, labels = case_data(case)
    x = torch.from_numpy(images).cuda(); lab = torch.from_numpy(labels[..., 0].copy()).cuda()
    out = []
    for _ in range(2):
        eng = make(B, H, W, C, sn, P, L, ic, training=True)[1]
        eng.set_dropout_step(DROP_STEP)
        probs, _ = eng.forward(x, training=True, labels=lab)
        v = eng.loss_dice().clone()
        eng.backward(lab, macro=True, loss_scale=0.5)
        torch.cuda.synchronize()
        out.append((probs.clone(), v, eng.grads.clone()))
    assert float(out[0][2].abs().max()) > 0
    for a, b in zip(*out):
        assert torch.equal(a, b)


def test_host_mirror_trains_saves_and_reloads_at_40_channels(tmp_path):
    from oct_image_segmentation_models_amd import optimizers
    from oct_image_segmentation_models_amd.common import custom_losses, custom_metrics
    from oct_image_segmentation_models_amd.common.data_generator import DataGenerator
    from oct_image_segmentation_models_amd.models import get_model_class
    from oct_image_segmentation_models_amd.models.engine_model import load_model
    cfg = dict(input_channels=1, num_classes=3, image_height=32, image_width=64, start_neurons=40, pool_layers=2)
    model = get_model_class("unet")(**cfg).build_model()
    model.config["seed"] = 3
    loss = custom_losses.custom_loss_objects["dice_loss_macro"]["function"](num_classes=3, is_y_true_sparse=True)
    metric = custom_metrics.training_monitor_metric_objects["dice_coef_macro"](True, 3)
    model.compile(optimizer=optimizers.Adam(learning_rate=1e-3), loss=loss, metrics=[metric])
    images, labels = on.synth_scans(8, 32, 64, 3, seed=5)
    hist = model.fit(x=DataGenerator(images, labels, 4, [], "none", (), True, None, seed=8), epochs=1, verbose=0)
    assert np.isfinite(hist.history["loss"]).all() and len(hist.history["loss"]) == 1
    x = images[:4].astype(np.float32) / 255.0
    live = model.predict(x, batch_size=4)
    assert np.isfinite(live).all() and live.shape == (4, 32, 64, 3)
    back = load_model(model.save(tmp_path / "model.hdf5"))
    assert back.config["start_neurons"] == 40
    assert np.array_equal(back.predict(x, batch_size=4), live)
