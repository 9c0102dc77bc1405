"""The ignore label on the device: head_fwd_k / head_bwd_k, their channel-streaming twins and
dice_finalize_k with ``oct_unet_set_ignore_label``, and padded training through ``Model.fit`` and ``train_model``.

The yardstick of the parity cases is ``oracle/unet_torch.forward`` in fp64 with the masked loss written out below and
differentiated by autograd; the expected loss values also go through ``common.custom_losses.masked_loss_reference``.
Seeds keep every BN pre-activation > 2e-5 from the ReLU kink (tools/find_margin_seed.py; re-asserted), tolerances are the
parity suite's constants: 1e-5 for losses, DICE_TOL for the two coefficients, GRAD_RTOL of each gradient tensor's maximum.
The engine-against-engine comparisons are bit for bit."""
import numpy as np
import pytest
import torch

from oracle import unet_numpy as on
from oracle import unet_torch as ot
from tests.helpers import relu_margin
from tests.layer_local import bf16_round, bf16_ulp
from tests.test_gpu_any_size import _Batches, _cfg, _engine, _scans, _weights
from tests.test_gpu_bce_dice_loss import bce_terms
from tests.test_gpu_head_classes import HEAD_CASES
from tests.test_gpu_parity import (CASES, DICE_TOL, DROP_STEP, GRAD_RTOL, MARGIN_SEED, PROB_TOL, check_grads_vs_oracle, data, make,
                                   make_bf16)
from tests.test_gpu_wide_head import SN40_C8, WIDE_CASES, assert_wide_route

pytestmark = pytest.mark.gpu

IGN = 255
EPS = 1e-7
FOCAL = (0.35, 2.0)                     # focal_loss_weight, gamma
# B, H, W, C, sn, P, L, in_ch: 48 x 80 at four pool levels, batch 3.  Three such images leave a 2e-5 margin at about one seed
# in 20000 with one conv per level (and at none that a search can reach with two), hence conv_layers = 1.  Margin 2.10e-5
CASE_B = (3, 48, 80, 3, 8, 4, 1, 1)
SEED_B = 30989


def _cw(C):
    return tuple(0.5 + 0.25 * ((3 * c) % 7) for c in range(C))


def frame_labels(labels, frame=(5, 3, 4, 6), rects=(), whole=()):
    """``labels`` (B,H,W,1) with a 255 frame (top, bottom, left, right), 255 rectangles (b, y0, y1, x0, x1) and whole images."""
    lab = labels.copy()
    t, b, l, r = frame
    H, W = lab.shape[1:3]
    lab[:, :t] = IGN; lab[:, H - b:] = IGN; lab[:, :, :l] = IGN; lab[:, :, W - r:] = IGN
    for (i, y0, y1, x0, x1) in rects:
        lab[i, y0:y1, x0:x1] = IGN
    for i in whole:
        lab[i] = IGN
    return lab


def masked_loss_t(probs, labels, C, kind, macro, cw=None, smooth=1e-5):
    """The loss over the counted pixels, torch (differentiable): ``kind`` "dice", "focal" (FOCAL, class weights) or "bce"."""
    lab = torch.as_tensor(labels[..., 0].astype(np.int64))
    keep = lab != IGN
    m = keep.to(torch.float64)
    safe = torch.where(keep, lab, torch.zeros_like(lab))
    y = torch.nn.functional.one_hot(safe, C).to(torch.float64) * m[..., None]
    pm = probs * m[..., None]
    I = (y * pm).sum(dim=(1, 2)); D = y.sum(dim=(1, 2)) + pm.sum(dim=(1, 2))
    dice = 1.0 - ((2.0 * I + smooth) / (D + smooth)).mean() if macro else 1.0 - (2.0 * I.sum() + smooth) / (D.sum() + smooth)
    n = float(m.sum())
    inv = 1.0 / n if n > 0 else 0.0
    if kind == "focal":
        fw, gamma = FOCAL
        py = torch.gather(probs, -1, safe[..., None])[..., 0]
        wt = torch.ones_like(py) if cw is None else torch.tensor(np.asarray(cw, np.float64))[safe]
        term = (m * wt * (1.0 - py) ** gamma * -torch.log(torch.clamp(py, EPS, 1.0 - EPS))).sum() * inv
        return fw * term + (1.0 - fw) * dice
    if kind == "bce":
        return (m[..., None] * bce_terms(y, probs)).sum() * (inv / C) + dice
    return dice


def autograd_oracle(cfg, p64, s64, images, labels, mask, kind, macro, cw, loss_scale):
    tp, ts = ot.to_torch(p64, s64, requires_grad=True)
    x = torch.tensor(on.preprocess_u8(images, np.float64))
    probs = ot.forward(cfg, tp, ts, x, training=True, dropout_mask=torch.tensor(mask))
    (masked_loss_t(probs, labels, cfg.num_classes, kind, macro, cw) * loss_scale).backward()
    return probs.detach().numpy(), [{k: v.grad.numpy() for k, v in p.items()} for p in tp]


def select(eng, kind, cw=None):
    if kind == "focal":
        eng.set_focal_dice(FOCAL[0], FOCAL[1], cw)
    elif kind == "bce":
        eng.set_bce_dice(True)
    else:
        eng.set_focal_dice(0.0); eng.set_bce_dice(False)


def step(eng, images, labels, kind, macro, loss_scale=0.5):
    """forward + loss + backward with the replayed dropout mask: (probs, the 8 loss values with zeros behind a plain Dice's
    four, dropout mask)."""
    B = images.shape[0]
    x = torch.from_numpy(images).cuda(); lab = torch.from_numpy(np.ascontiguousarray(labels[..., 0])).cuda()
    eng.set_dropout_step(DROP_STEP)
    mask = eng.dropout_mask(B).cpu().numpy().astype(np.float64)
    probs, _ = eng.forward(x, training=True, labels=lab)
    v = {"focal": eng.loss_focal_dice, "bce": eng.loss_bce_dice, "dice": eng.loss_dice}[kind]()
    eng.backward(lab, macro=macro, loss_scale=loss_scale)
    torch.cuda.synchronize()
    v = v.cpu().numpy()
    return probs, np.concatenate([v, np.zeros(8 - len(v), np.float32)]), mask


def check_against_oracle(case, seed, labels_of, kind, macro, eng_made=None):
    """One masked training step of ``case`` against the fp64 oracle: probabilities, the loss vector, every gradient."""
    from oct_image_segmentation_models_amd.common.custom_losses import masked_loss_reference
    B, H, W, C, sn, P, L, ic = case
    cfg, eng, p64, s64 = eng_made or make(B, H, W, C, sn, P, L, ic, training=True)
    images, labels = data(B, H, W, C, ic, seed=seed)
    labels = labels_of(labels)
    cw = _cw(C) if kind == "focal" else None
    select(eng, kind, cw)
    eng.set_ignore_label(IGN)
    eng.profile_begin()
    probs, v, mask = step(eng, images, labels, kind, macro)
    kernels = {e["kernel"] for e in eng.profile_end()}
    _, cache = on.forward(cfg, p64, s64, on.preprocess_u8(images, np.float64), training=True, dropout_mask=mask)
    assert relu_margin(cfg, p64, cache) > 2e-5
    ref, grads = autograd_oracle(cfg, p64, s64, images, labels, mask, kind, macro, cw, 0.5)
    assert np.abs(probs.cpu().numpy() - ref).max() < PROB_TOL          # probs are written for ignored pixels too
    want = masked_loss_reference(labels, ref, C, IGN, kind, gamma=FOCAL[1], class_weight=cw, focal_loss_weight=FOCAL[0])
    assert abs(float(masked_loss_t(torch.tensor(ref), labels, C, kind, macro, cw)) - want["loss_macro" if macro else "loss_micro"]) < 1e-12
    print(f"{case} {kind} macro={macro}: out8 {v.tolist()} want {want}")
    assert abs(v[0] - want["dice_loss_macro"]) < 1e-5 and abs(v[1] - want["dice_loss_micro"]) < 1e-5
    assert abs(v[2] - want["dice_coef_macro"]) < DICE_TOL and abs(v[3] - want["dice_coef_micro"]) < DICE_TOL
    if kind != "dice":
        assert abs(v[4] - want["term"]) < 1e-5 * max(1.0, want["term"])
        assert abs(v[6] - want["loss_micro"]) < 1e-5 * max(1.0, want["loss_micro"])
        if kind == "focal":
            assert abs(v[5] - want["loss_macro"]) < 1e-5 * max(1.0, want["loss_macro"])
    worst = check_grads_vs_oracle(eng, grads)
    print(f"worst gradient piece error {worst:.3g} (GRAD_RTOL {GRAD_RTOL})")
    return eng, kernels, labels


# ---- a. the predicate never fires ---------------------------------------------------------------------------------------------
def _make_with(options, maker, *args):
    from oct_image_segmentation_models_amd import _hip
    old = {k: _hip.get_option(k) for k in options}
    try:
        for k, v in options.items():
            _hip.set_option(k, v)
        return maker(*args)
    finally:
        for k, v in old.items():
            _hip.set_option(k, v)


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_an_ignore_label_that_does_not_occur_changes_no_bit(dtype, wide):
    """Ignore label 255 on labels without a 255 against the same handle with the mask off: the loss vector, all gradients
    and the BN state, for the three losses (focal and BCE take 1 / count from the device: it must be the host's value)."""
    case = CASES[7]                                   # 36 x 68: a ragged last chunk
    B, H, W, C, sn, P, L, ic = case
    cfg, eng, _, _ = _make_with({"head_wide": 1} if wide else {}, make_bf16 if dtype == "bf16" else make, B, H, W, C, sn, P, L, ic)
    w0 = eng.get_weights()
    images, labels = data(B, H, W, C, ic, seed=MARGIN_SEED[case])
    assert labels.max() < C
    bits = lambda t: t.clone().view(torch.int32)
    for kind, macro in (("dice", True), ("dice", False), ("focal", True), ("focal", False), ("bce", False)):
        got = []
        for ignore in (None, IGN):
            eng.set_weights(w0)
            select(eng, kind, _cw(C) if kind == "focal" else None)
            eng.set_ignore_label(ignore)
            eng.profile_begin()
            _, v, _ = step(eng, images, labels, kind, macro)
            kernels = {e["kernel"] for e in eng.profile_end()}
            got.append((v.view(np.int32), bits(eng.grads), bits(eng.state)))
        at = "unsigned short" if dtype == "bf16" else "float"
        if wide:
            assert_wide_route(kernels, C, sn, at)
        else:
            assert {f"head_fwd_k<{C},{sn},{at}>", f"head_bwd_k<{C},{sn},{at}>"} <= kernels, sorted(kernels)
        assert np.array_equal(got[0][0], got[1][0]), (kind, macro, got[0][0], got[1][0])
        assert torch.equal(got[0][1], got[1][1]) and torch.equal(got[0][2], got[1][2]), (kind, macro)
        assert np.isfinite(v).all() and float(eng.grads.abs().max()) > 0.0


# ---- b. oracle parity -----------------------------------------------------------------------------------------------------------
def _labels_b(labels):
    return frame_labels(labels, (5, 3, 4, 6), rects=((0, 10, 19, 30, 47), (1, 25, 40, 8, 15)), whole=(2,))


@pytest.mark.parametrize("kind, macro", [("dice", True), ("dice", False), ("focal", True), ("bce", False)])
def test_frame_rectangles_and_an_ignored_image_match_the_oracle(kind, macro):
    """48 x 80, four pool levels, batch 3: a 255 frame (5, 3, 4, 6), two ignored rectangles, the third image all 255."""
    eng, kernels, labels = check_against_oracle(CASE_B, SEED_B, _labels_b, kind, macro)
    assert (labels[2] == IGN).all() and (labels[0, 10:19, 30:47] == IGN).all() and (labels[:2] != IGN).sum() > 4000
    assert {"head_fwd_k<3,8,float>", "head_bwd_k<3,8,float>"} <= kernels, sorted(kernels)


# ---- c. shapes where the walk can go wrong -------------------------------------------------------------------------------------
def _labels_c1(labels):
    lab = frame_labels(labels, (0, 0, 0, 0), rects=((0, 0, 1, 0, 1), (0, 20, 30, 11, 50), (1, 35, 36, 0, 68)))
    assert lab[0, 0, 0, 0] == IGN and lab[1, 0, 0, 0] != IGN      # pixel 0: ignored in one image, counted in the other
    return lab


@pytest.mark.parametrize("kind, macro", [("dice", True), ("bce", False)])
def test_ragged_last_chunk_reads_pixel_0s_label(kind, macro):
    """36 x 68 = 2448 pixels: the last 256-pixel chunk holds 144, and its idle lanes read pixel 0's label -- 255 in image
    0 (they must not be taken for counted... nor, in image 1, count)."""
    case = CASES[7]
    assert case[1] * case[2] == 2448 and 2448 % 256 == 144
    check_against_oracle(case, MARGIN_SEED[case], _labels_c1, kind, macro)


@pytest.mark.parametrize("kind, macro", [("focal", True), ("bce", False), ("dice", True)])
def test_channel_streaming_head_with_eight_classes(kind, macro):
    """C = 8, start_neurons 40: head_fwd_wide_k / head_bwd_wide_k; 8 classes fill the per-(b, c) constants buffer, 1 / count
    sits behind its micro pair."""
    case = SN40_C8
    B, H, W, C, sn, P, L, ic = case
    labels_of = lambda lab: frame_labels(lab, (2, 1, 3, 2), rects=((0, 6, 9, 10, 20),))
    eng, kernels, labels = check_against_oracle(case, WIDE_CASES[case], labels_of, kind, macro)
    assert_wide_route(kernels, C, sn)
    assert set(np.unique(labels)) == set(range(C)) | {IGN}


def test_bf16_storage_head_local():
    """head_bwd_k<8, 8, bf16 storage> alone, masked BCE + Dice, from the engine's own stored z and BN record of the last
    block (the method and the bounds of tests/test_gpu_bce_dice_loss.py::test_head_local_in_both_storage_types): the
    stored gradient is rounded to bf16 once, dW / db are fp32 sums.  Under the mask g' is exactly 0."""
    from oct_image_segmentation_models_amd import _hip
    case = (2, 32, 64, 8, 8, 2, 2, 1)
    B, H, W, C, sn, P, L, ic = case
    cfg, eng, p64, s64 = _make_with({"fuse_first_apply": 0, "fuse_bn_apply": 0}, make_bf16, B, H, W, C, sn, P, L, ic)
    images, labels = data(B, H, W, C, ic, seed=HEAD_CASES[case])
    labels = frame_labels(labels, (3, 2, 5, 4), rects=((0, 10, 20, 20, 41), (1, 0, 32, 30, 33)))
    eng.set_bce_dice(True)
    eng.set_ignore_label(IGN)
    probs, v, _ = step(eng, images, labels, "bce", False)
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
    loss = masked_loss_t(p, labels, C, "bce", False)
    assert abs(v[6] - float(loss.detach())) < 1e-5 * max(1.0, float(loss.detach()))
    (loss * 0.5).backward()
    g = eng.grads.cpu().numpy().astype(np.float64)
    dw, db = w.grad.numpy().ravel(), b.grad.numpy()
    kscale = np.abs(dw).max()
    e_w = np.abs(g[hd["kernel_off"]:hd["kernel_off"] + dw.size] - dw).max() / kscale
    e_b = np.abs(g[hd["bias_off"]:hd["bias_off"] + C] - db).max() / max(np.abs(db).max(), kscale)
    gm = (act.grad * (act.detach() > 0)).numpy()
    ignored = labels[..., 0] == IGN
    assert (gm[ignored] == 0.0).all() and ignored.sum() > 500
    gm = bf16_round(gm)
    pred = rec[6] * gm + rec[7] * z.numpy() + rec[8]
    got = eng.debug_activation(li, 1)[:B].cpu().numpy().astype(np.float64)
    err = np.abs(got - pred)
    tight = np.full_like(pred, GRAD_RTOL * np.abs(pred).max()) + 2.0 ** -8 * np.abs(pred)
    loose = tight + np.abs(rec[6]) * bf16_ulp(gm) * (gm != 0)
    print(f"bf16: head dW err {e_w:.3g}, db err {e_b:.3g}, dz worst err / bound {(err / loose).max():.3g}")
    assert (err <= tight).mean() > 0.999, (err <= tight).mean()
    assert e_w < GRAD_RTOL and e_b < GRAD_RTOL
    assert (err <= loose).all(), (err / loose).max()


# ---- d. a batch that is ignored everywhere -------------------------------------------------------------------------------------
@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("kind, macro", [("dice", True), ("dice", False), ("focal", True), ("bce", False)])
def test_whole_batch_ignored(kind, macro, wide):
    case = CASES[0]
    B, H, W, C, sn, P, L, ic = case
    cfg, eng, _, _ = _make_with({"head_wide": 1} if wide else {}, make, B, H, W, C, sn, P, L, ic)
    images, labels = data(B, H, W, C, ic, seed=MARGIN_SEED[case])
    labels = np.full_like(labels, IGN)
    select(eng, kind, _cw(C) if kind == "focal" else None)
    eng.set_ignore_label(IGN)
    eng.grads.fill_(1e30)
    probs, v, _ = step(eng, images, labels, kind, macro)
    print(f"{kind} macro={macro} wide={wide}: out8 {v.tolist()}")
    assert v[0] == 0.0 and v[1] == 0.0                # 1 - s / s
    assert v[2] == 1.0                                # dice_coef_macro's own epsilon: 1e-5 / 1e-5
    assert np.isnan(v[3])                             # dice_coef_micro = 0 / 0, as the reference's formula
    assert (v[4:] == 0.0).all()
    g = eng.grads
    assert torch.isfinite(g).all() and int(torch.count_nonzero(g)) == 0
    assert torch.isfinite(probs).all() and torch.isfinite(eng.state).all() and torch.isfinite(eng.params).all()


def test_set_ignore_label_checks_its_argument():
    from oct_image_segmentation_models_amd._hip import OctError
    case = CASES[1]                                   # C = 4
    B, H, W, C, sn, P, L, ic = case
    cfg, eng, _, _ = make(B, H, W, C, sn, P, L, ic)
    for ok in (4, 200, 255, None):
        eng.set_ignore_label(ok); assert eng.ignore_label == ok
    for bad in (0, 3, 256, -2):
        with pytest.raises(OctError, match="ignore label"):
            eng.set_ignore_label(bad)
    assert eng.ignore_label is None
    # a forward made under another setting cannot be finalized
    images, labels = data(B, H, W, C, ic, seed=MARGIN_SEED[case])
    x = torch.from_numpy(images).cuda(); lab = torch.from_numpy(labels[..., 0].copy()).cuda()
    eng.forward(x, training=True, labels=lab)
    eng.set_ignore_label(IGN)
    with pytest.raises(OctError, match="forward"):
        eng.loss_dice()


# ---- e. padded training equals the native engine ---------------------------------------------------------------------------------
P3 = dict(pool_layers=3)


def _compiled(cfg, w0, ignore_label=None, **pad):
    from oct_image_segmentation_models_amd import optimizers
    from oct_image_segmentation_models_amd.common import custom_losses, custom_metrics
    from oct_image_segmentation_models_amd.models.engine_model import Model
    m = Model(name="unet", config=dict(cfg, seed=2))
    m.set_weights(w0)
    loss = custom_losses.custom_loss_objects["dice_loss_macro"]["function"](num_classes=3, is_y_true_sparse=True)
    metric = custom_metrics.training_monitor_metric_objects["dice_coef_macro"](True, 3)
    m.compile(optimizer=optimizers.Adam(learning_rate=2e-3), loss=loss, metrics=[metric], ignore_label=ignore_label, **pad)
    return m


@pytest.mark.parametrize("mode, value", [("edge", 0), ("constant", 0.25)])
def test_padded_fit_equals_the_native_engine_stepped_by_hand(mode, value):
    """``Model.fit`` for two steps on 36 x 68 with three pool levels (padded: 40 x 72, placement (2, 2)) against a native
    40 x 72 engine stepped by hand on ``pad_reference(x)`` with the labels padded by 255 and the ignore label set: the
    parameters, the moving statistics and the logged loss, bit for bit."""
    from oct_image_segmentation_models_amd import optimizers
    from oct_image_segmentation_models_amd._hip import OctError
    from oct_image_segmentation_models_amd.common.utils import pad_reference, padded_geometry
    assert padded_geometry(36, 68, 3) == (40, 72, 2, 2)
    cfg = _cfg(32, 64, **P3)
    w0 = _weights(cfg, 5)
    tr, va = _scans(4, 36, 68, 31), _scans(2, 36, 68, 32)
    model = _compiled(cfg, w0)
    with pytest.raises(OctError, match="pad_mode"):           # pad_mode None: the error of every size that is no multiple
        model.fit(_Batches(*tr, 2), epochs=1, verbose=0)
    model.pad_mode, model.pad_value = mode, value             # the attributes alone serve inference: fit goes on refusing
    with pytest.raises(OctError, match=r"compile\(pad_mode"):
        model.fit(_Batches(*tr, 2), epochs=1, verbose=0)
    model = _compiled(cfg, w0, pad_mode=mode, pad_value=value)
    assert (model.pad_mode, model.pad_value) == (mode, float(value))
    hist = model.fit(_Batches(*tr, 2), validation_data=_Batches(*va, 2), epochs=1, verbose=0)
    torch.cuda.synchronize()
    h = hist.history
    assert set(h) == {"loss", "dice_coef_macro", "val_loss", "val_dice_coef_macro"} and all(np.isfinite(v).all() for v in h.values())
    eng = model._engines["train"]
    assert (eng.cfg.H, eng.cfg.W) == (40, 72) and eng.opt_step == 2 and eng.ignore_label == IGN
    assert len(eng._pad_bufs) == 1                            # one padded pair for the one batch size, validation included

    native = _engine(_cfg(40, 72, **P3), w0, 2, training=True)
    native.set_ignore_label(IGN)
    opt = optimizers.Adam(learning_rate=2e-3)
    acc = None
    for x, lab in _Batches(*tr, 2).items:
        xp = torch.from_numpy(pad_reference(x, 40, 72, 2, 2, mode, value)).cuda()
        lp = torch.from_numpy(pad_reference(lab, 40, 72, 2, 2, "constant", IGN)).cuda()
        assert xp.dtype == torch.float32 and int((lp == IGN).sum()) == 2 * (40 * 72 - 36 * 68)
        native.forward(xp, training=True, labels=lp, want_probs=False)
        v = native.loss_dice()
        native.backward(lp, macro=True, loss_scale=1.0)
        opt.apply(native)
        acc = v.clone() if acc is None else acc + v
    acc = (acc / 2).cpu().numpy()
    torch.cuda.synchronize()
    assert torch.equal(eng.params, native.params) and torch.equal(eng.state, native.state)
    assert h["loss"][0] == float(acc[0]) and h["dice_coef_macro"][0] == float(acc[2])
    # validation ran on the same padded geometry with the trained weights
    xv, lv = _Batches(*va, 2).items[0]
    native.forward(torch.from_numpy(pad_reference(xv, 40, 72, 2, 2, mode, value)).cuda(), training=False,
                   labels=torch.from_numpy(pad_reference(lv, 40, 72, 2, 2, "constant", IGN)).cuda(), want_probs=False)
    vv = native.loss_dice().cpu().numpy()
    assert h["val_loss"][0] == float(vv[0]) and h["val_dice_coef_macro"][0] == float(vv[2])
    # an engine that the masked model used goes back to counting every pixel when a plain batch comes
    plain = _scans(2, 40, 72, 33)
    model.fit(_Batches(*plain, 2), epochs=1, verbose=0)
    assert model._engines["train"] is eng and eng.ignore_label is None and eng.opt_step == 3


def test_ignore_label_without_padding_in_fit():
    """``compile(ignore_label=200)`` on a size that needs no padding: fit equals the engine stepped by hand with that label."""
    from oct_image_segmentation_models_amd import optimizers
    cfg = _cfg(32, 64)
    w0 = _weights(cfg, 5)
    images, labels = _scans(2, 32, 64, 34)
    labels = labels.copy(); labels[0, 5:20, 10:40] = 200; labels[1, :, 60:] = 200
    model = _compiled(cfg, w0, ignore_label=200)
    hist = model.fit(_Batches(images, labels, 2), epochs=1, verbose=0)
    eng = model._engines["train"]
    assert eng.ignore_label == 200 and eng._pad_bufs == {}
    native = _engine(cfg, w0, 2, training=True)
    native.set_ignore_label(200)
    x, lab = _Batches(images, labels, 2).items[0]
    xd, ld = torch.from_numpy(x).cuda(), torch.from_numpy(np.ascontiguousarray(lab)).cuda()
    native.forward(xd, training=True, labels=ld, want_probs=False)
    v = native.loss_dice().cpu().numpy()
    native.backward(ld, macro=True, loss_scale=1.0)
    optimizers.Adam(learning_rate=2e-3).apply(native)
    torch.cuda.synchronize()
    assert torch.equal(eng.params, native.params) and hist.history["loss"][0] == float(v[0])
    plain = _engine(cfg, w0, 2, training=True)                # ... and the label does make a difference
    plain.forward(xd, training=True, labels=ld, want_probs=False)
    assert float(plain.loss_dice()[0]) != float(v[0])


# ---- f. train_model end to end ---------------------------------------------------------------------------------------------------
def test_train_model_on_a_size_that_is_no_multiple(tmp_path):
    """20 x 34 scans, two pool levels (padded: 20 x 36), device augmentation with a column shift, an ignored region in the
    labels: one epoch, a checkpoint, three classes detected."""
    from oct_image_segmentation_models_amd import optimizers
    from oct_image_segmentation_models_amd.common import h5io
    from oct_image_segmentation_models_amd.training.training import train_model
    from oct_image_segmentation_models_amd.training.training_parameters import TrainingParams
    tr_i, tr_l = on.synth_scans(4, 20, 34, 3, seed=11)
    va_i, va_l = on.synth_scans(2, 20, 34, 3, seed=12)
    tr_l = tr_l.copy(); tr_l[0, 4:9, 20:30] = IGN
    assert set(np.unique(tr_l)) == {0, 1, 2, IGN}
    h5io.save(tmp_path / "data.hdf5", {"train_images": tr_i, "train_labels": tr_l, "val_images": va_i, "val_labels": va_l})
    kw = dict(model_architecture="unet", training_dataset_path=tmp_path / "data.hdf5", initial_model=None,
              results_location=tmp_path / "results", opt_con=optimizers.Adam, opt_params={"learning_rate": 4e-3},
              loss="dice_loss_macro", metric="dice_coef_macro", epochs=1, batch_size=2,
              model_hyperparameters={"pool_layers": 2}, seed=3,
              augmentations=[{"name": "column_shift", "arguments": {"max_shift": 2, "max_tilt": 1, "max_curvature": 1}},
                             {"name": "no_augmentation", "arguments": {}}],
              aug_mode="one", aug_probs=(0.7, 0.3), aug_fly=True, aug_val=True, aug_device=True, ignore_label=IGN)
    res = train_model(TrainingParams(pad_mode="reflect", **kw), None)
    h = res.history
    assert set(h) == {"loss", "dice_coef_macro", "val_loss", "val_dice_coef_macro"}
    assert all(len(v) == 1 and np.isfinite(v).all() for v in h.values())
    assert res.model.config["num_classes"] == 3 and res.model.ignore_label == IGN and res.model.pad_mode == "reflect"
    eng = res.model._engines["train"]
    assert (eng.cfg.H, eng.cfg.W) == (20, 36) and eng.ignore_label == IGN and eng.opt_step == 2
    assert len(res.checkpoints) == 1 and __import__("pathlib").Path(res.checkpoints[0]).exists()
