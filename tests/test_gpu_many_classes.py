"""GPU parity of num_classes 9 .. 16 and of the class-streaming head kernels that carry them (head_fwd_cls_k /
head_bwd_cls_k<C, AT>, csrc/kernels_head_cls.hpp: 5 C + 1 loss sums per thread in rows of 64 or 96 floats, the Dice
derivative as two block-uniform values per class, dl in a full 16-column tile for the fp32 matrix pipe).

Tolerances are those of tests/test_gpu_parity.py (fp64 oracle, margin seeds) and tests/layer_local.py; nothing here is tuned.
The helpers of the suites for 2..8 classes are reused by import; only the engine makers are restated, because an engine for
more than 8 classes is asked for with ``max_classes=16``."""
from pathlib import Path

import numpy as np
import pytest
import torch

from oracle import unet_numpy as on
from tests.helpers import relu_margin, stored_activation_view, tree_equal
from tests.test_gpu_bce_dice_loss import autograd_oracle, bce_step, check_values
from tests.test_gpu_masked_loss import IGN, _cw, check_against_oracle, frame_labels, select, step
from tests.test_gpu_parity import (DICE_TOL, DROP_STEP, GRAD_RTOL, PROB_TOL, assert_same_as_fresh_engine,  # noqa: F401
                                   bf16_step_layer_local, check_grads_vs_oracle, data, training_step_vs_oracle)

pytestmark = pytest.mark.gpu

ENTROPY_TOL = 2e-5          # include/oct_unet.h: entropy / mutual information against fp64, n_cls <= 32, T <= 64

# B, H, W, C, sn, P, L, in_ch -> data seed with a ReLU margin > 2e-5 in which every class occurs in every image
# (tools/find_margin_seed.py ... 2e-5, oracle only; both re-asserted by the tests)
CLS_CASES = {
    (2, 32, 64, 9, 8, 2, 2, 1): 219,      # 2.27e-5; the first class count past the register kernels, two images
    (1, 32, 64, 10, 8, 2, 2, 1): 17,      # 2.73e-5
    (2, 32, 64, 12, 8, 2, 2, 1): 12,      # 2.08e-5; 61 of the 64 row slots in use
    (2, 32, 64, 13, 8, 2, 2, 1): 256,     # 2.75e-5; the first 96-float Dice row
    (2, 32, 64, 16, 8, 2, 2, 1): 23,      # 2.04e-5; a full dl tile, 81 sums
    (1, 32, 64, 16, 32, 1, 1, 1): 116,    # 2.04e-5; the widest former register width
    (1, 16, 32, 16, 64, 1, 1, 1): 2,      # 4.18e-5; the widest head with the most classes; 512 pixels = 2 chunks
    (2, 18, 34, 11, 48, 1, 1, 1): 3,      # 3.83e-5; 612 pixels: two chunks and a ragged one, two images
    (1, 18, 34, 16, 40, 1, 1, 1): 5,      # 5.19e-5; ragged chunk, CIN 2 1/2 groups, 16 classes
}
CASES = list(CLS_CASES)
C9, C10, C12, C13, C16, C16_SN32, C16_SN64, C11_SN48, C16_SN40 = CASES


def make(B, H, W, C, sn, P, L=2, in_ch=1, seed=0, training=True, max_batch=None, dtype="float32"):
    """tests/test_gpu_parity.py::make / make_bf16 with ``max_classes=16``."""
    from oct_image_segmentation_models_amd.engine import UNetEngine
    cfg = on.UNetConfig(input_channels=in_ch, num_classes=C, start_neurons=sn, pool_layers=P, conv_layers=L)
    params, state = on.init_params(cfg, seed=seed, dtype=np.float32, randomize_bn=True)
    eng = UNetEngine(device="cuda:0", input_channels=in_ch, num_classes=C, image_height=H, image_width=W,
                     start_neurons=sn, pool_layers=P, conv_layers=L, max_batch=max_batch or B, training=training,
                     seed=seed + 100, dtype=dtype, max_classes=16)
    eng.set_weights(on.keras_weight_list(params, state))
    p64 = [{k: v.astype(np.float64) for k, v in p.items()} for p in params]
    s64 = [{k: v.astype(np.float64) for k, v in s.items()} for s in state]
    return cfg, eng, p64, s64


def cls_names(C, sn, at="float", training=True):
    return {f"head_fwd_cls_k<{C},{sn},{at}>"} | ({f"head_bwd_cls_k<{C},{sn},{at}>"} if training else set())


def assert_cls_route(kernels, C, sn, at="float", training=True):
    assert cls_names(C, sn, at, training) <= kernels, sorted(kernels)
    other = ("head_fwd_k<", "head_bwd_k<", "head_fwd_wide_k<", "head_bwd_wide_k<")
    assert not [k for k in kernels if k.startswith(other)], sorted(kernels)


def case_data(case):
    B, H, W, C, sn, P, L, ic = case
    images, labels = data(B, H, W, C, ic, seed=CLS_CASES[case])
    for b in range(B):
        assert set(np.unique(labels[b])) == set(range(C))     # every class occurs in every image
    return images, labels


@pytest.mark.parametrize("macro", [True, False])
@pytest.mark.parametrize("case", CASES)
def test_training_step_matches_oracle(case, macro):
    B, H, W, C, sn, P, L, ic = case
    cfg, eng, p64, s64 = make(B, H, W, C, sn, P, L, ic, training=True)
    images, labels = case_data(case)
    eng.profile_begin()
    training_step_vs_oracle(cfg, eng, p64, s64, case, images, labels, macro, "default")
    assert_cls_route({e["kernel"] for e in eng.profile_end()}, C, sn)


@pytest.mark.parametrize("case", CASES)
def test_inference_forward_matches_oracle(case):
    B, H, W, C, sn, P, L, ic = case
    cfg, eng, p64, s64 = make(B, H, W, C, sn, P, L, ic, training=False)
    images, labels = case_data(case)
    x = torch.from_numpy(images).cuda()
    eng.profile_begin()
    probs, am = eng.forward(x, training=False, want_argmax=True)
    assert_cls_route({e["kernel"] for e in eng.profile_end()}, C, sn, training=False)
    ref, _ = on.forward(cfg, p64, s64, on.preprocess_u8(images, np.float64), training=False)
    assert np.abs(probs.cpu().numpy() - ref).max() < PROB_TOL
    diff = am.cpu().numpy() != ref.argmax(-1)                 # identical argmax except at numerical ties
    if diff.any():
        srt = np.sort(ref, -1)
        assert (srt[..., -1] - srt[..., -2])[diff].max() < 1e-4
    assert int(am.max()) < C
    if case == C16_SN64:                                      # the forward records into a graph: replay = eager, bit for bit
        eager_am = am.clone()
        gp, gam = eng.graph_capture(x.clone(), want_probs=True, want_argmax=True)
        eng.graph_launch(); torch.cuda.synchronize()
        assert torch.equal(gp, probs) and torch.equal(gam, eager_am)
        gp.zero_(); eng.graph_launch(); torch.cuda.synchronize()
        assert torch.equal(gp, probs)


def _step(case, labels, macro, focal=None):
    """One training step on the case's margin-seed images with the given label maps: (engine, loss vector, oracle
    probabilities, oracle gradients)."""
    B, H, W, C, sn, P, L, ic = case
    cfg, eng, p64, s64 = make(B, H, W, C, sn, P, L, ic, training=True)
    images, _ = data(B, H, W, C, ic, seed=CLS_CASES[case])
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
    assert_cls_route({e["kernel"] for e in eng.profile_end()}, C, sn)
    ref, cache = on.forward(cfg, p64, s64, on.preprocess_u8(images, np.float64), training=True, dropout_mask=mask)
    assert relu_margin(cfg, p64, cache) > 2e-5
    assert np.abs(probs.cpu().numpy() - ref).max() < PROB_TOL
    kw = {} if focal is None else dict(focal=focal)
    _, grads = on.backward(cfg, p64, cache, labels, macro=macro, loss_scale=0.5, **kw)
    return eng, v, ref, grads


@pytest.mark.parametrize("macro", [True, False])
@pytest.mark.parametrize("case", [C16, C13])
def test_focal_dice_loss_with_a_weight_per_class(case, macro):
    """focal_dice_loss with C distinct class weights: the seven loss values and every gradient."""
    C = case[3]
    fw, gamma = 0.35, 2.0
    cw = tuple(0.25 + 0.125 * ((7 * c) % 16) for c in range(C))
    assert len(set(cw)) == C
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


@pytest.mark.parametrize("clip_mod", [0, 1])
def test_focal_clip_modulation_switch_at_12_classes(clip_mod):
    """tests/test_gpu_parity.py::test_focal_clip_modulation_switch on a saturated 12-class head (bias +12 on class 0, -12 on
    class 11: p_11 ~ e^-24 is clipped on its own pixels), with that test's bounds."""
    case = C12
    B, H, W, C, sn, P, L, ic = case
    fw, gamma = 0.6, 2.0
    cw = tuple(0.5 + 0.25 * (c % 5) for c in range(C))
    cfg, eng, p64, s64 = make(B, H, W, C, sn, P, L, ic, training=True)
    wl = eng.get_weights()
    wl[-1] = np.array([12.0] + [0.0] * (C - 2) + [-12.0], np.float32)
    eng.set_weights(wl)
    p64[-1]["bias"] = wl[-1].astype(np.float64)
    images, labels = case_data(case)
    x = torch.from_numpy(images).cuda(); lab = torch.from_numpy(labels[..., 0].copy()).cuda()
    eng.set_dropout_step(DROP_STEP)
    mask = eng.dropout_mask(B).cpu().numpy().astype(np.float64)
    ref, cache = on.forward(cfg, p64, s64, on.preprocess_u8(images, np.float64), training=True, dropout_mask=mask)
    py = np.take_along_axis(ref, labels.astype(np.int64), axis=-1)
    assert (py < 1e-7).any()                                                    # the clip really is active
    eng.set_option("focal_clip_modulation", clip_mod)
    eng.set_focal_dice(fw, gamma, cw)
    eng.forward(x, training=True, labels=lab, want_probs=False)
    v = eng.loss_focal_dice().cpu().numpy()
    eng.backward(lab, macro=True, loss_scale=1.0)
    g = eng.grads.cpu().numpy().astype(np.float64)
    focal = on.focal_loss_mean(labels, ref, gamma, cw, clip_modulation=bool(clip_mod))
    assert abs(v[4] - focal) < 2e-5 * max(1.0, focal), (v[4], focal)
    both = [on.backward(cfg, p64, cache, labels, macro=True, loss_scale=1.0, focal=(fw, gamma, cw),
                        focal_clip_modulation=m)[1] for m in (False, True)]
    gref = on.flatten_grads(both[clip_mod]); gother = on.flatten_grads(both[1 - clip_mod])
    scale = np.abs(gref).max()
    assert np.abs(g - gref).max() / scale < 2e-3       # saturated softmax: f32 cancellation in p*(dp - dot) limits this case
    assert np.abs(gref - gother).max() / scale < 1e-6


@pytest.mark.parametrize("inner_eps", [1, 0])
@pytest.mark.parametrize("case", [C12, C16])
def test_bce_dice_loss(case, inner_eps):
    """bce_dice_loss, both settings of "bce_inner_eps", against torch-fp64 autograd with the same setting
    (tests/test_gpu_bce_dice_loss.py): the O(C^2) complement and Jacobian loops at 12 and 16 classes."""
    B, H, W, C, sn, P, L, ic = case
    cfg, eng, p64, s64 = make(B, H, W, C, sn, P, L, ic, training=True)
    images, labels = case_data(case)
    eng.set_option("bce_inner_eps", inner_eps)
    eng.set_bce_dice(True)
    eng.profile_begin()
    probs, v, mask = bce_step(eng, images, labels, 0.5)
    assert_cls_route({e["kernel"] for e in eng.profile_end()}, C, sn)
    _, cache = on.forward(cfg, p64, s64, on.preprocess_u8(images, np.float64), training=True, dropout_mask=mask)
    assert relu_margin(cfg, p64, cache) > 2e-5
    bce, dice, ref, grads = autograd_oracle(cfg, p64, s64, images, labels, mask, 0.5, inner_eps=bool(inner_eps))
    assert np.abs(probs.cpu().numpy() - ref).max() < PROB_TOL
    check_values(v, labels, ref, bce, dice, C)
    worst = check_grads_vs_oracle(eng, grads)
    print(f"{case} bce_inner_eps={inner_eps}: worst gradient piece error {worst:.3g} (GRAD_RTOL {GRAD_RTOL})")


def _labels_ignored(labels):
    """A 255 frame, a rectangle in image 0, and image 1 without a counted pixel."""
    return frame_labels(labels, (3, 2, 4, 5), rects=((0, 8, 15, 20, 41),), whole=(1,))


@pytest.mark.parametrize("kind, macro", [("dice", True), ("dice", False), ("focal", True), ("bce", False)])
def test_ignore_label_at_13_classes(kind, macro):
    """Ignore label 255 against the masked fp64 oracle of tests/test_gpu_masked_loss.py; then the same step with the label C
    (= 13, the lowest value that is no class) standing for 255: the same pixels are left out, so every bit is the same."""
    case = C13
    B, H, W, C, sn, P, L, ic = case
    made = make(B, H, W, C, sn, P, L, ic, training=True)
    w0 = made[1].get_weights()
    eng, kernels, labels = check_against_oracle(case, CLS_CASES[case], _labels_ignored, kind, macro, eng_made=made)
    assert_cls_route(kernels, C, sn)
    assert (labels[1] == IGN).all() and (labels[0] != IGN).sum() > 1000
    # ignored pixels carry an exactly zero gradient into the last block
    g = stored_activation_view(eng, len(eng.layers) - 2, 1)[:B]
    ign = torch.from_numpy(labels[..., 0] == IGN).cuda()
    assert int(torch.count_nonzero(g[ign])) == 0 and float(g[~ign].abs().max()) > 0
    grads_255, state_255 = eng.grads.clone(), eng.state.clone()
    images, _ = data(B, H, W, C, ic, seed=CLS_CASES[case])
    lab_c = labels.copy(); lab_c[lab_c == IGN] = C
    eng.set_weights(w0)
    eng.set_ignore_label(C)
    select(eng, kind, _cw(C) if kind == "focal" else None)
    step(eng, images, lab_c, kind, macro)
    assert torch.equal(eng.grads, grads_255) and torch.equal(eng.state, state_255)


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
@pytest.mark.parametrize("case", [C13, C16])
def test_absent_classes(case, edit, macro):
    """Label maps in which a class does not occur: the ReLU margin depends on the images only, so the labels may be edited."""
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


def test_bf16_storage_at_16_classes():
    """The 16-class case in bf16 storage through the layer-local one-rounding checks."""
    from oct_image_segmentation_models_amd import _hip
    case = C16
    B, H, W, C, sn, P, L, ic = case
    try:
        _hip.set_option("fuse_first_apply", 0); _hip.set_option("fuse_bn_apply", 0)     # (every block's dz is stored)
        cfg, eng, p64, s64 = make(B, H, W, C, sn, P, L, ic, dtype="bfloat16")
    finally:
        _hip.set_option("fuse_first_apply", 1); _hip.set_option("fuse_bn_apply", 1)
    images, labels = case_data(case)
    eng.profile_begin()
    bf16_step_layer_local(cfg, eng, p64, case, images, labels)
    assert_cls_route({e["kernel"] for e in eng.profile_end()}, C, sn, "unsigned short")


def _plain_step(eng, x, lab, macro=True):
    eng.set_dropout_step(DROP_STEP)
    probs, _ = eng.forward(x, training=True, labels=lab)
    v = eng.loss_dice().clone()
    eng.backward(lab, macro=macro, loss_scale=0.5)
    torch.cuda.synchronize()
    return probs.clone(), v


def test_partial_batch_on_a_used_engine_at_13_classes():
    """max_batch 3 stepped with B = 2 after a step with B = 3: the Dice rows, the per-(b, c) constants and the partial rows
    are carved for 3 images and still hold the larger step.  Equal to a fresh max_batch 2 engine, bit for bit."""
    case = C13
    B, H, W, C, sn, P, L, ic = case
    assert B == 2
    cfg, eng, _, _ = make(B, H, W, C, sn, P, L, ic, training=True, max_batch=3)
    w0 = eng.get_weights()
    big_i, big_l = data(3, H, W, C, ic, seed=CLS_CASES[case] + 1000)
    _plain_step(eng, torch.from_numpy(big_i).cuda(), torch.from_numpy(big_l[..., 0].copy()).cuda())
    eng.set_weights(w0)
    images, labels = case_data(case)
    x = torch.from_numpy(images).cuda(); lab = torch.from_numpy(labels[..., 0].copy()).cuda()
    probs, v = _plain_step(eng, x, lab)
    _, fresh, _, _ = make(B, H, W, C, sn, P, L, ic, training=True)
    probs_f, v_f = _plain_step(fresh, x, lab)
    assert_same_as_fresh_engine(eng, fresh, B, probs, probs_f, v, v_f)


def test_two_runs_give_the_same_bits():
    """Every sum of the class-streaming kernels is taken in a fixed order (no atomics): two fresh engines, equal bits."""
    case = C16
    B, H, W, C, sn, P, L, ic = case
    images, labels = case_data(case)
    x = torch.from_numpy(images).cuda(); lab = torch.from_numpy(labels[..., 0].copy()).cuda()
    out = []
    for _ in range(2):
        eng = make(B, H, W, C, sn, P, L, ic, training=True)[1]
        probs, v = _plain_step(eng, x, lab)
        out.append((probs, v, eng.grads.clone()))
    assert float(out[0][2].abs().max()) > 0
    for a, b in zip(*out):
        assert torch.equal(a, b)


# ---- downstream of the head at 10 and 16 classes --------------------------------------------------------------------------
@pytest.fixture(scope="module", params=[10, 16])
def infer_engine(request):
    C = request.param
    B, H, W = 2, 32, 64
    _, eng, _, _ = make(B, H, W, C, 8, 2, training=False)
    images, labels = on.synth_scans(B, H, W, C, seed=5)
    return C, eng, torch.from_numpy(images).cuda(), labels


def test_boundary_maps_equal_their_restatements(infer_engine):
    from oct_image_segmentation_models_amd.common import utils as cu
    C, eng, x, labels = infer_engine
    lab = np.ascontiguousarray(labels[..., 0]).astype(np.uint8)
    lab[lab == 4] = 3                                           # a class that never occurs
    assert 4 not in np.unique(lab)
    probs, _ = eng.forward(x, training=False)
    p = probs.cpu().numpy()
    for bg_ilm, bg_csi in ((True, False), (False, True), (False, False)):
        got = eng.boundary_maps(torch.from_numpy(lab).cuda(), bg_ilm=bg_ilm, bg_csi=bg_csi).cpu().numpy()
        cat = cu.labels_to_categorical(lab.astype(np.int64), C)
        want = on.convert_predictions_to_maps_semantic(cat, bg_ilm=bg_ilm, bg_csi=bg_csi)
        assert got.shape == (2, C - 1, 32, 64) and np.array_equal(got, want)
        soft = eng.boundary_maps_soft(probs, bg_ilm=bg_ilm, bg_csi=bg_csi).cpu().numpy()
        assert np.array_equal(soft, cu.soft_boundary_maps_reference(p, bg_ilm, bg_csi))


def test_forward_mc_and_tta_equal_their_restatements(infer_engine):
    from oct_image_segmentation_models_amd.common import utils as cu
    C, eng, x, _ = infer_engine
    host = lambda out: {k: v.cpu().numpy().copy() for k, v in out.items()}
    # Monte-Carlo dropout, T = 3: the three single samples reduced
    s = 7
    singles = np.stack([host(eng.forward_mc(x, 1, step0=s + t, want_mean_probs=True))["mean_probs"] for t in range(3)])
    assert not np.array_equal(singles[0], singles[1])
    got = host(eng.forward_mc(x, 3, step0=s, want_mean_probs=True))
    m32, a32, _, _ = cu.mc_reduce_reference(singles, np.float32)
    _, _, e64, i64 = cu.mc_reduce_reference(singles, np.float64)
    assert np.array_equal(got["mean_probs"].view(np.uint32), m32.view(np.uint32)) and np.array_equal(got["argmax"], a32)
    assert np.abs(got["entropy"] - e64).max() <= ENTROPY_TOL and np.abs(got["mutual_info"] - i64).max() <= ENTROPY_TOL
    # test-time augmentation, two views
    views = ("identity", "flip_lr")
    codes = [cu.TTA_VIEWS[v] for v in views]
    stack = np.stack([eng.forward(eng.flip(x, v) if v != "identity" else x, training=False)[0].cpu().numpy() for v in views])
    got = host(eng.forward_tta(x, views, want_mean_probs=True))
    m32, a32, _, _ = cu.tta_reduce_reference(stack, codes, np.float32)
    _, _, e64, i64 = cu.tta_reduce_reference(stack, codes, np.float64)
    assert np.array_equal(got["mean_probs"].view(np.uint32), m32.view(np.uint32)) and np.array_equal(got["argmax"], a32)
    assert np.abs(got["entropy"] - e64).max() <= ENTROPY_TOL and np.abs(got["mutual_info"] - i64).max() <= ENTROPY_TOL


@pytest.mark.parametrize("C", [9, 10, 16])
def test_padded_inference_crops_pixels_of_more_than_32_bytes(C):
    """A pixel of the probability maps has 36 .. 64 bytes here and ``oct_crop_batch`` takes 32 at the most: the padded chain
    and ``UNetEngine.crop`` hand it rows of 4-byte pixels.  30 x 61 scans on a 32 x 64 engine, plain, MC and TTA, eager and
    captured: equal to the same call on the padded batch, cropped on the host."""
    from oct_image_segmentation_models_amd.common import utils as cu
    B, H, W = 2, 30, 61
    Hp, Wp, top, left = cu.padded_geometry(H, W, 2)
    assert (Hp, Wp) == (32, 64) and top == 1 and left == 1
    _, eng, _, _ = make(B, Hp, Wp, C, 8, 2, training=False)
    images = on.synth_scans(B, Hp, Wp, C, seed=9)[0][:, :H, :W]
    x = torch.from_numpy(np.ascontiguousarray(images)).cuda()
    xp = torch.from_numpy(cu.pad_reference(images, Hp, Wp, top, left, "reflect")).cuda()
    host = lambda out: {k: v.cpu().numpy().copy() for k, v in out.items()}
    pad = (top, left, "reflect", 0)
    for kw in (dict(), dict(mc=(2, 5)), dict(tta=("identity", "flip_both"))):
        want = host(eng.infer(xp, want_probs=True, want_argmax=True, **kw))
        got = host(eng.infer(x, pad=pad, want_probs=True, want_argmax=True, **kw))
        assert set(got) == set(want) and ("probs" in got or "mean_probs" in got)
        for k in want:
            assert got[k].shape[:3] == (B, H, W)
            assert got[k].tobytes() == cu.crop_reference(want[k], H, W, top, left).tobytes(), (kw, k)
    probs = eng.infer(xp, want_probs=True, want_argmax=False)["probs"]
    assert probs.shape[-1] * 4 > 32
    assert np.array_equal(eng.crop(probs, H, W, top, left).cpu().numpy(), cu.crop_reference(probs.cpu().numpy(), H, W, top, left))
    # the captured padded chain replays the eager bits
    eager = host(eng.infer(x, pad=pad, want_probs=True, want_argmax=True))
    xb = x.clone()
    outs = eng.infer(xb, pad=pad, want_probs=True, want_argmax=True, capture=True)
    for _ in range(2):
        for t in outs.values():
            t.zero_()
        eng.graph_launch(); torch.cuda.synchronize()
        assert all(np.array_equal(outs[k].cpu().numpy(), eager[k]) for k in eager)


# ---- the workflow at 10 classes ---------------------------------------------------------------------------------------------
def test_workflow_at_10_classes(tmp_path):
    """train_model (2 epochs) -> evaluate_model (host path, then metrics_device + gs_device) -> predict (host path, then
    gs_labels_device + gs_device) on a 10-class synthetic HDF5 of 32 x 64 scans.  The device-path files equal the host-path
    files, and the Dice in them equals dice_from_counts of the saved label maps."""
    from oct_image_segmentation_models_amd import optimizers
    from oct_image_segmentation_models_amd.common import h5io
    from oct_image_segmentation_models_amd.common.dataset import Dataset
    from oct_image_segmentation_models_amd.evaluation import dice_device, eval_model
    from oct_image_segmentation_models_amd.evaluation.evaluation_parameters import EvaluationParameters, EvaluationSaveParams
    from oct_image_segmentation_models_amd.prediction import predict
    from oct_image_segmentation_models_amd.prediction.prediction_parameters import PredictionParams, PredictionSaveParams
    from oct_image_segmentation_models_amd.training.training import train_model
    from oct_image_segmentation_models_amd.training.training_parameters import TrainingParams
    H, W, C, N = 32, 64, 10, 5
    metrics = ["dice_coef_classes", "dice_coef_macro", "dice_coef_micro"]
    tr_i, tr_l = on.synth_scans(8, H, W, C, seed=1)
    va_i, va_l = on.synth_scans(4, H, W, C, seed=2)
    te_i, te_l = on.synth_scans(N, H, W, C, seed=3)
    assert len(np.unique(tr_l)) == C
    dpath = tmp_path / "data.hdf5"
    h5io.save(dpath, {"train_images": tr_i, "train_labels": tr_l, "val_images": va_i, "val_labels": va_l,
                      "test_images": te_i, "test_labels": te_l})
    tp = TrainingParams(model_architecture="unet", training_dataset_path=dpath, initial_model=None,
                        results_location=tmp_path / "results", opt_con=optimizers.Adam, opt_params={"learning_rate": 4e-3},
                        loss="dice_loss_macro", metric="dice_coef_macro", epochs=2, batch_size=4,
                        model_hyperparameters={"pool_layers": 2}, patience=3, seed=7)
    res = train_model(tp, None)
    assert len(res.history["loss"]) == 2 and np.isfinite(res.history["loss"]).all() and np.isfinite(res.history["val_loss"]).all()
    ckpt = Path(res.checkpoints[-1])

    def evaluate(name, **kw):
        ep = EvaluationParameters(model_path=ckpt, mlflow_tracking_uri=None, mlflow_run_uuid=None, test_dataset_path=dpath,
                                  save_foldername=tmp_path / name, save_params=EvaluationSaveParams(), graph_search=True,
                                  metrics=metrics, batch_size=2, **kw)
        assert ep.num_classes == C
        ep.gs_workers = 1
        return eval_model(ep)

    def run_predict(name, **kw):
        ds = Dataset(te_i, [Path(f"scan_{i}.tiff") for i in range(N)], [tmp_path / name / f"image_{i}" for i in range(N)])
        pp = PredictionParams(model_path=ckpt, mlflow_tracking_uri=None, mlflow_run_uuid=None, dataset=ds,
                              config_output_dir=tmp_path / name, save_params=PredictionSaveParams(), graph_search=True,
                              batch_size=2, **kw)
        pp.gs_workers = 1
        return predict(pp)

    host = evaluate("eval_host")
    dev = evaluate("eval_dev", metrics_device=True, gs_device=True, gs_device_ties="host")
    p_host = run_predict("pred_host")
    p_dev = run_predict("pred_dev", gs_labels_device=True, gs_device=True, gs_device_ties="host")
    tree_equal(tmp_path / "eval_host", tmp_path / "eval_dev",
               ["evaluation_results.hdf5", "gs_evaluation_results.hdf5", "overall_evaluation_results.hdf5"])
    tree_equal(tmp_path / "pred_host", tmp_path / "pred_dev", ["prediction_info.hdf5", "graph_search_prediction_info.hdf5"])
    assert len(host) == len(dev) == len(p_host) == len(p_dev) == N
    gt = te_l[..., 0].astype(np.uint8)
    for i, (h, d, p) in enumerate(zip(host, dev, p_dev)):
        assert h.predicted_labels.shape == (H, W) and int(h.predicted_labels.max()) < C
        assert np.array_equal(h.predicted_labels, d.predicted_labels) and np.array_equal(h.predicted_labels, p.predicted_labels)
        assert h.boundary_maps.shape == (C - 1, H, W) and np.array_equal(h.gs_pred_segs, d.gs_pred_segs)
        f = h5io.load(d.image_output_dir / "evaluation_results.hdf5")
        saved, truth = (np.asarray(f[k]).reshape(1, H, W) for k in ("predicted_segmentation_map", "eval_labels"))
        assert saved.dtype == np.uint8 and np.array_equal(truth[0], gt[i])
        counts = dice_device.confusion_counts_reference(saved, truth, C)[0, :C * C].reshape(C, C)
        for key, want in zip(metrics, dice_device.dice_from_counts(counts, metrics)):
            assert np.array_equal(np.asarray(f[key]).reshape(-1), np.asarray(want, np.float64).reshape(-1)), (i, key)
