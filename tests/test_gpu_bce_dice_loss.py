"""bce_dice_loss on the device (reference common/custom_losses.py:84-91): keras binary_crossentropy + dice_loss_micro with
the BCE arithmetic inside head_fwd_k / dice_finalize_k / head_bwd_k.

The oracle is torch-fp64 autograd over ``oracle/unet_torch.forward`` with the loss written out from its definition
(Keras parity itself is unpinned: TensorFlow is not available).  Shapes and seeds are the margin-seed
tables of tests/test_gpu_parity.py and tests/test_gpu_head_classes.py (every BN pre-activation > 2e-5 from the ReLU kink,
re-asserted), tolerances are the project's: 1e-5 for losses, DICE_TOL for the coefficients, GRAD_RTOL for every
gradient piece; the saturated head uses the bounds of test_focal_clip_modulation_switch for the same head."""
import numpy as np
import pytest
import torch

from oracle import unet_numpy as on
from oracle import unet_torch as ot
from tests.helpers import relu_margin
from tests.layer_local import bf16_round, bf16_ulp
from tests.test_gpu_head_classes import HEAD_CASES
from tests.test_gpu_parity import (CASES, DICE_TOL, DROP_STEP, GRAD_RTOL, MARGIN_SEED, PROB_TOL, check_grads_vs_oracle, data,
                                   make, make_bf16)

pytestmark = pytest.mark.gpu

EPS = 1e-7


def bce_terms(y, p, inner_eps=True):
    """Per-(pixel, class) binary cross-entropy of the definition, torch (differentiable)."""
    e = EPS if inner_eps else 0.0
    pc = torch.clamp(p, EPS, 1.0 - EPS); qc = torch.clamp(1.0 - p, EPS, 1.0 - EPS)
    return -(y * torch.log(pc + e) + (1.0 - y) * torch.log(qc + e))


def autograd_oracle(cfg, p64, s64, images, labels, mask, loss_scale, inner_eps=True):
    """(bce mean, dice_loss_micro, probabilities, gradients in the numpy oracle's structure) of loss_scale * (bce + dice_micro)."""
    tp, ts = ot.to_torch(p64, s64, requires_grad=True)
    x = torch.tensor(on.preprocess_u8(images, np.float64))
    probs = ot.forward(cfg, tp, ts, x, training=True, dropout_mask=torch.tensor(mask))
    lab = torch.tensor(labels[..., 0].astype(np.int64))
    y = torch.nn.functional.one_hot(lab, cfg.num_classes).to(torch.float64)
    bce = bce_terms(y, probs, inner_eps).mean(dim=-1).mean()          # class axis, then SUM_OVER_BATCH_SIZE
    dice = ot.dice_loss(y, probs, macro=False)
    ((bce + dice) * loss_scale).backward()
    grads = [{k: v.grad.numpy() for k, v in p.items()} for p in tp]
    return float(bce.detach()), float(dice.detach()), probs.detach().numpy(), grads


def bce_step(eng, images, labels, loss_scale):
    """forward + loss_bce_dice + backward on ``eng`` (BCE already selected) with the replayed dropout mask."""
    B = images.shape[0]
    x = torch.from_numpy(images).cuda(); lab = torch.from_numpy(labels[..., 0].copy()).cuda()
    eng.set_dropout_step(DROP_STEP)
    mask = eng.dropout_mask(B).cpu().numpy().astype(np.float64)
    probs, _ = eng.forward(x, training=True, labels=lab)
    v = eng.loss_bce_dice().cpu().numpy()
    eng.backward(lab, macro=False, loss_scale=loss_scale)
    torch.cuda.synchronize()
    return probs, v, mask


def check_values(v, labels, ref, bce, dice, C):
    y = on.one_hot(labels, C, np.float64)
    print(f"out8 {v.tolist()}  bce {bce} dice_micro {dice}")
    assert abs(v[0] - on.dice_loss_macro(y, ref)) < 1e-5 and abs(v[1] - on.dice_loss_micro(y, ref)) < 1e-5
    assert abs(v[2] - on.dice_coef_macro(y, ref)) < DICE_TOL and abs(v[3] - on.dice_coef_micro(y, ref)) < DICE_TOL
    assert abs(v[4] - bce) < 1e-5 * max(1.0, bce), (v[4], bce)
    assert abs(v[6] - (bce + dice)) < 1e-5 * max(1.0, bce + dice), (v[6], bce + dice)
    assert v[5] == 0.0 and v[7] == 0.0


SEEDS = {**{c: MARGIN_SEED[c] for c in CASES[:2]}, **HEAD_CASES}


@pytest.mark.parametrize("case", [(2, 32, 64, 3, 8, 2, 2, 1), (1, 32, 64, 6, 16, 1, 2, 1), (2, 32, 64, 8, 8, 2, 2, 1)])
def test_loss_values_and_gradients_match_autograd(case):
    """C = 3 and C = 6 put the slot BCE shares with the focal sum at the last column of the 16- and 32-wide Dice partial
    rows; C = 8 uses the 64-wide row, two images."""
    B, H, W, C, sn, P, L, ic = case
    cfg, eng, p64, s64 = make(B, H, W, C, sn, P, L, ic, training=True)
    images, labels = data(B, H, W, C, ic, seed=SEEDS[case])
    eng.set_bce_dice(True)
    eng.profile_begin()
    probs, v, mask = bce_step(eng, images, labels, 0.5)
    kernels = {e["kernel"] for e in eng.profile_end()}
    assert {f"head_fwd_k<{C},{sn},float>", f"head_bwd_k<{C},{sn},float>"} <= kernels, sorted(kernels)
    _, cache = on.forward(cfg, p64, s64, on.preprocess_u8(images, np.float64), training=True, dropout_mask=mask)
    assert relu_margin(cfg, p64, cache) > 2e-5
    bce, dice, ref, grads = autograd_oracle(cfg, p64, s64, images, labels, mask, 0.5)
    assert np.abs(probs.cpu().numpy() - ref).max() < PROB_TOL
    check_values(v, labels, ref, bce, dice, C)
    worst = check_grads_vs_oracle(eng, grads)
    print(f"{case}: worst gradient piece error {worst:.3g} (GRAD_RTOL {GRAD_RTOL})")


@pytest.mark.parametrize("inner_eps", [1, 0])
def test_saturated_head(inner_eps):
    """Head bias +12 / 0 / -12 (the head of test_focal_clip_modulation_switch): p_0 ~ 1 - 6e-6, a third of the (pixel,
    class) probabilities outside [eps, 1 - eps].  This is where dBCE/dp = 1/q meets the cancelling 1 - p and dp - dot of the
    obvious softmax Jacobian; head_bwd_k takes q from the other classes and applies p_c (q_c dp_c - sum_{k != c} p_k dp_k).
    Both settings of the unverifiable inner epsilon (option "bce_inner_eps"), each against autograd with the same setting.
    Measured on MI355X: see DESIGN.md section 11."""
    from oct_image_segmentation_models_amd import _hip
    case = CASES[0]
    B, H, W, C, sn, P, L, ic = case
    cfg, eng, p64, s64 = make(B, H, W, C, sn, P, L, ic, training=True)
    wl = eng.get_weights()
    wl[-1] = np.array([12.0, 0.0, -12.0], np.float32)
    eng.set_weights(wl)
    p64[-1]["bias"] = wl[-1].astype(np.float64)
    images, labels = data(B, H, W, C, ic, seed=MARGIN_SEED[case])
    eng.set_option("bce_inner_eps", inner_eps)               # per handle: the process-wide default stays 1
    assert eng.handle_option("bce_inner_eps") == inner_eps and _hip.get_option("bce_inner_eps") == 1
    eng.set_bce_dice(True)
    probs, v, mask = bce_step(eng, images, labels, 1.0)
    g = eng.grads.cpu().numpy().astype(np.float64)
    both = [autograd_oracle(cfg, p64, s64, images, labels, mask, 1.0, inner_eps=bool(m)) for m in (0, 1)]
    bce, dice, ref, grads = both[inner_eps]
    clipped = (ref < EPS) | (ref > 1.0 - EPS)
    assert clipped.mean() > 0.2                               # the clips really are active
    Lref = bce + dice
    gref = on.flatten_grads(grads); scale = np.abs(gref).max()
    gerr = np.abs(g - gref).max() / scale
    other = both[1 - inner_eps]
    print(f"bce_inner_eps={inner_eps}: clipped {clipped.mean():.3f}, bce {v[4]} vs {bce} (err {abs(v[4] - bce):.3g}), "
          f"loss {v[6]} vs {Lref} (err {abs(v[6] - Lref):.3g}), gradient err / scale {gerr:.3g}; "
          f"the other setting: loss differs by {abs(other[0] - bce):.3g}, gradient by "
          f"{np.abs(on.flatten_grads(other[3]) - gref).max() / scale:.3g} of the scale")
    assert abs(v[4] - bce) < 2e-5 * max(1.0, bce) and abs(v[6] - Lref) < 2e-5 * max(1.0, Lref)
    assert gerr < 2e-3


def _dice_step(eng, x, lab, macro):
    eng.set_dropout_step(DROP_STEP)
    eng.forward(x, training=True, labels=lab); v = eng.loss_dice().clone(); eng.backward(lab, macro=macro, loss_scale=0.5)
    return v, eng.grads.clone()


def _focal_step(eng, x, lab, macro):
    eng.set_dropout_step(DROP_STEP)
    eng.set_focal_dice(0.35, 2.0, (0.5, 2.0, 1.25))
    eng.forward(x, training=True, labels=lab); v = eng.loss_focal_dice().clone(); eng.backward(lab, macro=macro, loss_scale=0.5)
    return v, eng.grads.clone()


def _bce_step_t(eng, x, lab):
    eng.set_dropout_step(DROP_STEP)
    eng.set_bce_dice(True)
    eng.forward(x, training=True, labels=lab); v = eng.loss_bce_dice().clone(); eng.backward(lab, macro=False, loss_scale=0.5)
    return v, eng.grads.clone()


def test_selection_is_clean():
    """Switching between BCE, focal and plain Dice on one engine gives, bit for bit, what a fresh engine gives; the macro
    combination under BCE is an argument error."""
    from oct_image_segmentation_models_amd.engine import OctError
    case = CASES[0]
    B, H, W, C, sn, P, L, ic = case
    images, labels = data(B, H, W, C, ic, seed=MARGIN_SEED[case])
    x = torch.from_numpy(images).cuda(); lab = torch.from_numpy(labels[..., 0].copy()).cuda()
    fresh = lambda: make(B, H, W, C, sn, P, L, ic, training=True)[1]
    dice_v, dice_g = _dice_step(fresh(), x, lab, True)
    focal_v, focal_g = _focal_step(fresh(), x, lab, True)
    bce_v, bce_g = _bce_step_t(fresh(), x, lab)
    assert not torch.equal(bce_g, dice_g) and not torch.equal(bce_g, focal_g)

    eng = fresh()
    v, g = _bce_step_t(eng, x, lab)
    assert torch.equal(v, bce_v) and torch.equal(g, bce_g)
    with pytest.raises(OctError):
        eng.backward(lab, macro=True, loss_scale=0.5)
    eng.set_bce_dice(False)                                   # BCE -> plain Dice
    assert not eng._bce_active
    v, g = _dice_step(eng, x, lab, True)
    assert torch.equal(v, dice_v) and torch.equal(g, dice_g)
    _bce_step_t(eng, x, lab)
    v, g = _focal_step(eng, x, lab, True)                     # BCE -> focal: set_focal_dice(w > 0) clears BCE
    assert not eng._bce_active and eng._focal_active
    assert torch.equal(v, focal_v) and torch.equal(g, focal_g)
    v, g = _bce_step_t(eng, x, lab)                           # focal -> BCE: set_bce_dice clears focal
    assert eng._bce_active and not eng._focal_active
    assert torch.equal(v, bce_v) and torch.equal(g, bce_g)
    eng.set_bce_dice(False)
    v, g = _dice_step(eng, x, lab, False)                     # ... and neither is left behind
    v2, g2 = _dice_step(fresh(), x, lab, False)
    assert torch.equal(v, v2) and torch.equal(g, g2)


def test_partial_batch_on_a_used_engine():
    """max_batch 4: a BCE step with B = 4, then one with B = 3 -- the mean of the second is over 3 H W C values."""
    case = CASES[1]                                           # B = 3, C = 4: the shared slot is column 20 of a 32-wide row
    B, H, W, C, sn, P, L, ic = case
    cfg, eng, p64, s64 = make(B, H, W, C, sn, P, L, ic, training=True, max_batch=4)
    weights = eng.get_weights()
    eng.set_bce_dice(True)
    full_i, full_l = data(4, H, W, C, ic, seed=MARGIN_SEED[case] + 1000)
    _, v_full, _ = bce_step(eng, full_i, full_l, 0.5)
    assert np.isfinite(v_full).all()
    eng.set_weights(weights)                                  # (the full step updated the moving statistics)
    images, labels = data(B, H, W, C, ic, seed=MARGIN_SEED[case])
    probs, v, mask = bce_step(eng, images, labels, 0.5)
    _, cache = on.forward(cfg, p64, s64, on.preprocess_u8(images, np.float64), training=True, dropout_mask=mask)
    assert relu_margin(cfg, p64, cache) > 2e-5
    bce, dice, ref, grads = autograd_oracle(cfg, p64, s64, images, labels, mask, 0.5)
    assert np.abs(probs.cpu().numpy()[:B] - ref).max() < PROB_TOL
    check_values(v, labels, ref, bce, dice, C)
    check_grads_vs_oracle(eng, grads)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_head_local_in_both_storage_types(dtype):
    """head_bwd_k alone, C = 8, start_neurons 8, from the engine's own stored z and BN record of the last block: y, logits,
    p, the BCE + Dice dlogits, the masked gradient g' of the last block and the head's dW / db recomputed in fp64.
    With the stand-alone BN-backward pass (fuse_* off) the last block's gradient buffer holds dz = ga g' + gb z + gd
    (record rows 6 .. 8) after backward, so g' is compared through that transform with the engine's own coefficients.
    fp32 storage: GRAD_RTOL on the scale of the tensor.  bf16 storage: g' is rounded to bf16 at the store (modelled) and
    the stored value is allowed one bf16 rounding on top (2^-8 relative per element); dW / db are accumulated in fp32 from
    unrounded values: GRAD_RTOL."""
    from oct_image_segmentation_models_amd import _hip
    case = (2, 32, 64, 8, 8, 2, 2, 1)
    B, H, W, C, sn, P, L, ic = case
    try:
        _hip.set_option("fuse_first_apply", 0); _hip.set_option("fuse_bn_apply", 0)
        cfg, eng, p64, s64 = (make_bf16 if dtype == "bf16" else make)(B, H, W, C, sn, P, L, ic)
    finally:
        _hip.set_option("fuse_first_apply", 1); _hip.set_option("fuse_bn_apply", 1)
    images, labels = data(B, H, W, C, ic, seed=HEAD_CASES[case])
    eng.set_bce_dice(True)
    eng.profile_begin()
    probs, v, _ = bce_step(eng, images, labels, 0.5)
    kernels = {e["kernel"] for e in eng.profile_end()}
    at = "unsigned short" if dtype == "bf16" else "float"
    assert {f"head_fwd_k<8,8,{at}>", f"head_bwd_k<8,8,{at}>"} <= kernels, sorted(kernels)
    li = len(eng.layers) - 2
    assert not eng.debug_layer_fused(li)
    z = torch.tensor(eng.debug_activation(li, 0)[:B].cpu().numpy().astype(np.float64))
    rec = eng.debug_bn_record(li).cpu().numpy().astype(np.float64)
    hd = eng.layers[-1]
    w = torch.tensor(p64[-1]["kernel"].reshape(sn, C), requires_grad=True)
    b = torch.tensor(p64[-1]["bias"], requires_grad=True)
    act = torch.relu(torch.tensor(rec[0]) * z + torch.tensor(rec[1])).requires_grad_(True)
    p = torch.softmax(act @ w + b, dim=-1)
    assert np.abs(probs.cpu().numpy() - p.detach().numpy()).max() < PROB_TOL
    y = torch.nn.functional.one_hot(torch.tensor(labels[..., 0].astype(np.int64)), C).to(torch.float64)
    bce = bce_terms(y, p).mean(dim=-1).mean(); dice = ot.dice_loss(y, p, macro=False)
    bce_v, L_v = float(bce.detach()), float((bce + dice).detach())
    assert abs(v[4] - bce_v) < 1e-5 * max(1.0, bce_v) and abs(v[6] - L_v) < 1e-5 * max(1.0, L_v)
    ((bce + dice) * 0.5).backward()
    g = eng.grads.cpu().numpy().astype(np.float64)
    dw, db = w.grad.numpy().ravel(), b.grad.numpy()
    kscale = np.abs(dw).max()
    e_w = np.abs(g[hd["kernel_off"]:hd["kernel_off"] + dw.size] - dw).max() / kscale
    e_b = np.abs(g[hd["bias_off"]:hd["bias_off"] + C] - db).max() / max(np.abs(db).max(), kscale)
    gm = (act.grad * (act.detach() > 0)).numpy()                               # masked gradient g' of the last block
    if dtype == "bf16":
        gm = bf16_round(gm)                                                    # the store rounds g' to bf16
    pred = rec[6] * gm + rec[7] * z.numpy() + rec[8]
    got = eng.debug_activation(li, 1)[:B].cpu().numpy().astype(np.float64)
    err = np.abs(got - pred)
    tight = np.full_like(pred, GRAD_RTOL * np.abs(pred).max())                 # fp32 arithmetic: the fp32-storage bound
    loose = tight
    if dtype == "bf16":
        tight = tight + 2.0 ** -8 * np.abs(pred)                               # + the one rounding of the stored value
        # a g' whose fp32 value and this fp64 one straddle a bf16 rounding boundary is stored one ulp away (rare)
        loose = tight + np.abs(rec[6]) * bf16_ulp(gm) * (gm != 0)
        assert (err <= tight).mean() > 0.999, (err <= tight).mean()
    bound = loose
    print(f"{dtype}: head dW err {e_w:.3g}, db err {e_b:.3g}, dz worst err / bound {(err / bound).max():.3g}")
    assert e_w < GRAD_RTOL and e_b < GRAD_RTOL
    assert (err <= bound).all(), (err / bound).max()


def test_train_model_with_bce_dice_loss(tmp_path):
    """Registry name ``bce_dice_loss`` trains through train_model (which ended at exit(1) before)."""
    from oct_image_segmentation_models_amd import optimizers
    from oct_image_segmentation_models_amd.common import h5io
    from oct_image_segmentation_models_amd.training.training import train_model
    from oct_image_segmentation_models_amd.training.training_parameters import TrainingParams
    tr_i, tr_l = on.synth_scans(8, 32, 64, 3, seed=11)
    va_i, va_l = on.synth_scans(4, 32, 64, 3, seed=12)
    h5io.save(tmp_path / "data.hdf5", {"train_images": tr_i, "train_labels": tr_l, "val_images": va_i, "val_labels": va_l})
    tp = TrainingParams(model_architecture="unet", training_dataset_path=tmp_path / "data.hdf5", initial_model=None,
                        results_location=tmp_path / "results", opt_con=optimizers.Adam, opt_params={"learning_rate": 4e-3},
                        loss="bce_dice_loss", metric="dice_coef_macro", epochs=25, batch_size=4,
                        model_hyperparameters={"pool_layers": 2}, patience=26, seed=3)
    res = train_model(tp, None)
    h = res.history
    print("loss", h["loss"][0], "->", h["loss"][-1], " val_loss", h["val_loss"][0], "->", h["val_loss"][-1])
    assert len(h["loss"]) == 25 and np.isfinite(h["loss"]).all() and np.isfinite(h["val_loss"]).all()
    assert h["loss"][-1] < 0.7 * h["loss"][0]
