"""The shaped Dice term on the device (``oct_unet_set_dice_shape``): Tversky weights, the focal-Tversky
exponent and class weights in dice_shape_finalize_k, their gradient through the folded (num, den) pairs that the three head
backward families read.

The oracle is torch-fp64 autograd over ``oracle/unet_torch.forward`` with the loss written out from its definition
(tests/dice_shape_cases.py; the numpy restatement ``shaped_dice_reference`` is held to it too).  Shapes and seeds are the
margin-seed tables of the existing GPU tests (every BN pre-activation > 2e-5 from the ReLU kink, re-asserted); tolerances are
the project's: 1e-5 for losses, DICE_TOL for the coefficients, GRAD_RTOL for every gradient piece."""
import numpy as np
import pytest
import torch

from oracle import unet_numpy as on
from oracle import unet_torch as ot
from tests.dice_shape_cases import SHAPES, drop_class_from_image, shaped_dice_t
from tests.helpers import relu_margin
from tests.test_gpu_bce_dice_loss import bce_terms
from tests.test_gpu_many_classes import C9, CLS_CASES, assert_cls_route
from tests.test_gpu_many_classes import make as make16
from tests.test_gpu_parity import (CASES, DICE_TOL, DROP_STEP, GRAD_RTOL, MARGIN_SEED, PROB_TOL, check_grads_vs_oracle, data,
                                   make, make_bf16)
from tests.test_gpu_wide_head import SN40_C8, WIDE_CASES, assert_wide_route

pytestmark = pytest.mark.gpu

CASE = (2, 32, 64, 3, 8, 2, 2, 1)
assert CASE == CASES[0]
IGN = 255
EPS = 1e-7
FOCAL = (0.35, 2.0)                     # focal_loss_weight, gamma
FOCAL_CW = (0.5, 2.0, 1.25)
FIN, PLAIN_FIN = "dice_shape_finalize_k", "dice_finalize_k"


def loss_t(probs, labels, C, kind, macro, shape, ignore=None, cw=None):
    """``kind`` "dice", "focal" (FOCAL, class weights ``cw``) or "bce" with the shaped Dice term, over the counted pixels."""
    dice = shaped_dice_t(probs, labels, C, macro, ignore=ignore, **shape)
    if kind == "dice":
        return dice
    lab = torch.as_tensor(labels[..., 0].astype(np.int64))
    keep = torch.ones_like(lab, dtype=torch.bool) if ignore is None else lab != ignore
    m = keep.to(torch.float64)
    safe = torch.where(keep, lab, torch.zeros_like(lab))
    n = float(m.sum())
    inv = 1.0 / n if n > 0 else 0.0
    if kind == "focal":
        fw, gamma = FOCAL
        py = torch.gather(probs, -1, safe[..., None])[..., 0]
        wt = torch.ones_like(py) if cw is None else torch.tensor(np.asarray(cw, np.float64))[safe]
        term = (m * wt * (1.0 - py) ** gamma * -torch.log(torch.clamp(py, EPS, 1.0 - EPS))).sum() * inv
        return fw * term + (1.0 - fw) * dice
    y = torch.nn.functional.one_hot(safe, C).to(torch.float64) * m[..., None]
    return (m[..., None] * bce_terms(y, probs)).sum() * (inv / C) + dice


def select(eng, kind, cw=None):
    if kind == "focal":
        eng.set_focal_dice(FOCAL[0], FOCAL[1], cw)
    elif kind == "bce":
        eng.set_bce_dice(True)


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


def check_against_autograd(made, images, labels, shape, kind, macro, ignore=None, cw=None):
    """One shaped training step against the fp64 oracle: probabilities, the loss vector, every gradient piece.  Returns the
    engine and the kernel names of the step."""
    from oct_image_segmentation_models_amd.common.custom_losses import masked_loss_reference, shaped_dice_reference
    cfg, eng, p64, s64 = made
    C = cfg.num_classes
    select(eng, kind, cw)
    if ignore is not None:
        eng.set_ignore_label(ignore)
    eng.set_dice_shape(**shape)
    eng.profile_begin()
    probs, v, mask = step(eng, images, labels, kind, macro)
    ents = eng.profile_end()
    kernels = {e["kernel"] for e in ents}
    assert FIN in kernels and PLAIN_FIN not in kernels, sorted(kernels)
    _, cache = on.forward(cfg, p64, s64, on.preprocess_u8(images, np.float64), training=True, dropout_mask=mask)
    assert relu_margin(cfg, p64, cache) > 2e-5
    tp, ts = ot.to_torch(p64, s64, requires_grad=True)
    pt = ot.forward(cfg, tp, ts, torch.tensor(on.preprocess_u8(images, np.float64)), training=True, dropout_mask=torch.tensor(mask))
    (loss_t(pt, labels, C, kind, macro, shape, ignore, cw) * 0.5).backward()
    grads = [{k: t.grad.numpy() for k, t in p.items()} for p in tp]
    ref = pt.detach()
    assert np.abs(probs.cpu().numpy() - ref.numpy()).max() < PROB_TOL
    want = {(k, mac): float(loss_t(ref, labels, C, k, mac, shape, ignore, cw)) for k in ("dice", kind) for mac in (True, False)}
    rest = shaped_dice_reference(labels, ref.numpy(), C, ignore, **shape)
    assert abs(rest["loss_macro"] - want["dice", True]) < 1e-12 and abs(rest["loss_micro"] - want["dice", False]) < 1e-12
    plain = masked_loss_reference(labels, ref.numpy(), C, ignore)
    print(f"{kind} macro={macro} {shape}: out8 {v.tolist()} want {want} metrics {plain['dice_coef_macro']}, {plain['dice_coef_micro']}")
    assert abs(v[0] - want["dice", True]) < 1e-5 and abs(v[1] - want["dice", False]) < 1e-5
    assert abs(v[2] - plain["dice_coef_macro"]) < DICE_TOL and abs(v[3] - plain["dice_coef_micro"]) < DICE_TOL
    if kind == "focal":
        assert abs(v[5] - want[kind, True]) < 1e-5 * max(1.0, want[kind, True])
    if kind != "dice":
        assert abs(v[6] - want[kind, False]) < 1e-5 * max(1.0, want[kind, False])
    g = eng.grads.cpu().numpy()
    assert np.isfinite(g).all()
    worst = check_grads_vs_oracle(eng, grads)
    print(f"worst gradient piece error {worst:.3g} (GRAD_RTOL {GRAD_RTOL})")
    return eng, kernels


def case_inputs(case, seed, absent=None):
    B, H, W, C, sn, P, L, ic = case
    images, labels = data(B, H, W, C, ic, seed=seed)
    if absent is not None:
        b, c, to = absent
        labels = drop_class_from_image(labels, b, c, to)
        counts = np.stack([np.bincount(labels[i].ravel(), minlength=C) for i in range(B)])
        assert counts[b, c] == 0 and (np.delete(counts, b, axis=0)[:, c] > 0).all()
    return images, labels


# ---- the register head: every shape, macro and micro -------------------------------------------------------------------------------
@pytest.mark.parametrize("macro", [True, False])
@pytest.mark.parametrize("name", ["tversky", "focal_tversky_075", "weights_with_zero", "volume"])
def test_shapes_match_autograd(name, macro):
    """Tversky 0.3 / 0.7; focal-Tversky g = 0.75; fixed weights (0.5, 2.0, 0.0) -- the zero-weight class gets no Dice gradient, and
    nothing in ``grads`` is NaN or inf --; "volume" with class 2 absent from image 1 (it takes the image's largest weight in the
    macro form, and its batch weight in the micro form)."""
    B, H, W, C, sn, P, L, ic = CASE
    images, labels = case_inputs(CASE, MARGIN_SEED[CASE], absent=(1, 2, 1) if name == "volume" else None)
    _, kernels = check_against_autograd(make(B, H, W, C, sn, P, L, ic, training=True), images, labels, SHAPES[name], "dice", macro)
    assert {f"head_fwd_k<{C},{sn},float>", f"head_bwd_k<{C},{sn},float>"} <= kernels, sorted(kernels)


# ---- the other two head families ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("macro", [True, False])
def test_class_streaming_head(macro):
    """9 classes (head_bwd_cls_k): Tversky, g = 0.75 and nine class weights with a zero."""
    B, H, W, C, sn, P, L, ic = C9
    images, labels = case_inputs(C9, CLS_CASES[C9])
    shape = dict(alpha=0.3, beta=0.7, gamma=0.75, class_weight=(0.5, 2.0, 0.0, 1.25, 0.75, 3.0, 1.5, 0.25, 1.75))
    _, kernels = check_against_autograd(make16(B, H, W, C, sn, P, L, ic, training=True), images, labels, shape, "dice", macro)
    assert_cls_route(kernels, C, sn)


@pytest.mark.parametrize("macro", [True, False])
def test_channel_streaming_head(macro):
    """start_neurons 40, 8 classes (head_bwd_wide_k): "volume" weights under Tversky 0.7 / 0.3 and g = 2, class 5 relabelled away
    (one image: the class is absent from the batch, so the micro form's rule for T_c = 0 is met as well)."""
    B, H, W, C, sn, P, L, ic = SN40_C8
    images, labels = data(B, H, W, C, ic, seed=WIDE_CASES[SN40_C8])
    labels = drop_class_from_image(labels, 0, 5, 4)
    shape = dict(alpha=0.7, beta=0.3, gamma=2.0, class_weight="volume")
    _, kernels = check_against_autograd(make(B, H, W, C, sn, P, L, ic, training=True), images, labels, shape, "dice", macro)
    assert_wide_route(kernels, C, sn)


def head_local_check(cfg, eng, p64, images, labels, shape, macro):
    """One shaped step held to the head alone, from the engine's own stored z and BN record of the last block: the shaped losses
    and the head's dW / db (accumulated in fp32 from unrounded values: GRAD_RTOL) recomputed in fp64.  Needs no ReLU margin."""
    B, C, sn = images.shape[0], cfg.num_classes, cfg.start_neurons
    eng.set_dice_shape(**shape)
    eng.profile_begin()
    probs, v, _ = step(eng, images, labels, "dice", macro)
    kernels = {e["kernel"] for e in eng.profile_end()}
    assert FIN in kernels and PLAIN_FIN not in kernels, sorted(kernels)
    li = len(eng.layers) - 2
    z = torch.tensor(eng.debug_activation(li, 0)[:B].cpu().numpy().astype(np.float64))
    rec = eng.debug_bn_record(li).cpu().numpy().astype(np.float64)
    hd = eng.layers[-1]
    w = torch.tensor(p64[-1]["kernel"].reshape(sn, C), requires_grad=True)
    b = torch.tensor(p64[-1]["bias"], requires_grad=True)
    p = torch.softmax(torch.relu(torch.tensor(rec[0]) * z + torch.tensor(rec[1])) @ w + b, dim=-1)
    assert np.abs(probs.cpu().numpy() - p.detach().numpy()).max() < PROB_TOL
    both = {m: shaped_dice_t(p, labels, C, m, **shape) for m in (True, False)}
    print(f"head-local macro={macro}: out4 {v[:4].tolist()} want {float(both[True].detach())}, {float(both[False].detach())}")
    assert abs(v[0] - float(both[True].detach())) < 1e-5 and abs(v[1] - float(both[False].detach())) < 1e-5
    (both[macro] * 0.5).backward()
    g = eng.grads.cpu().numpy().astype(np.float64)
    assert np.isfinite(g).all()
    dw, db = w.grad.numpy().ravel(), b.grad.numpy()
    kscale = np.abs(dw).max()
    e_w = np.abs(g[hd["kernel_off"]:hd["kernel_off"] + dw.size] - dw).max() / kscale
    e_b = np.abs(g[hd["bias_off"]:hd["bias_off"] + C] - db).max() / max(np.abs(db).max(), kscale)
    print(f"head-local macro={macro}: head dW err {e_w:.3g}, db err {e_b:.3g}")
    assert e_w < GRAD_RTOL and e_b < GRAD_RTOL
    return kernels


def test_bf16_storage_head_local():
    """bf16 activation storage, the register head."""
    B, H, W, C, sn, P, L, ic = CASE
    cfg, eng, p64, s64 = make_bf16(B, H, W, C, sn, P, L, ic)
    images, labels = case_inputs(CASE, MARGIN_SEED[CASE])
    shape = dict(alpha=0.3, beta=0.7, gamma=0.75, class_weight=(0.5, 2.0, 0.0))
    kernels = head_local_check(cfg, eng, p64, images, labels, shape, True)
    assert f"head_bwd_k<{C},{sn},unsigned short>" in kernels, sorted(kernels)


@pytest.mark.parametrize("macro", [True, False])
def test_more_than_256_pairs_go_through_the_device_table(macro):
    """B C = 20 x 13 = 260 pairs: four threads of the finalize own two pairs each and the cross-class passes read the sums back from
    the handle's device table instead of LDS.  "volume" weights (every pass reads the table), with class 12 absent from image 3."""
    B, H, W, C, sn, P, L, ic = 20, 16, 32, 13, 8, 1, 1, 1
    cfg, eng, p64, s64 = make16(B, H, W, C, sn, P, L, ic, training=True)
    rng = np.random.default_rng(7)
    images = rng.integers(0, 256, (B, H, W, ic)).astype(np.uint8)
    labels = rng.integers(0, C, (B, H, W, 1)).astype(np.uint8)
    labels = drop_class_from_image(labels, 3, 12, 11)
    assert B * C > 256
    kernels = head_local_check(cfg, eng, p64, images, labels, dict(alpha=0.3, beta=0.7, gamma=0.75, class_weight="volume"), macro)
    assert_cls_route(kernels, C, sn)


# ---- combinations ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("macro", [True, False])
def test_focal_dice_loss_with_a_shape(macro):
    B, H, W, C, sn, P, L, ic = CASE
    images, labels = case_inputs(CASE, MARGIN_SEED[CASE])
    shape = dict(alpha=0.3, beta=0.7, gamma=0.75, class_weight=(0.5, 2.0, 0.0))
    check_against_autograd(make(B, H, W, C, sn, P, L, ic, training=True), images, labels, shape, "focal", macro, cw=FOCAL_CW)


def test_bce_dice_loss_with_a_shape():
    B, H, W, C, sn, P, L, ic = CASE
    images, labels = case_inputs(CASE, MARGIN_SEED[CASE], absent=(1, 2, 1))
    shape = dict(alpha=0.3, beta=0.7, class_weight="volume")
    check_against_autograd(make(B, H, W, C, sn, P, L, ic, training=True), images, labels, shape, "bce", False)


@pytest.mark.parametrize("kind, macro", [("dice", True), ("dice", False), ("focal", True)])
def test_shape_with_an_ignore_label(kind, macro):
    """A 255 frame and a rectangle, class 2 of image 1 ignored altogether (absent from the counted pixels of that image): the
    masked restatement, "volume" weights under Tversky and g = 0.75."""
    B, H, W, C, sn, P, L, ic = CASE
    images, labels = case_inputs(CASE, MARGIN_SEED[CASE])
    labels = labels.copy()
    labels[:, :5] = IGN; labels[:, :, 60:] = IGN; labels[0, 10:20, 8:30] = IGN
    labels[1][labels[1] == 2] = IGN
    shape = dict(alpha=0.3, beta=0.7, gamma=0.75, class_weight="volume")
    eng, _ = check_against_autograd(make(B, H, W, C, sn, P, L, ic, training=True), images, labels, shape, kind, macro, ignore=IGN,
                                    cw=FOCAL_CW if kind == "focal" else None)
    assert eng.ignore_label == IGN


# ---- off is off ------------------------------------------------------------------------------------------------------------------
def _profiled_step(eng, x, lab, macro):
    eng.set_dropout_step(DROP_STEP)
    eng.profile_begin()
    eng.forward(x, training=True, labels=lab); v = eng.loss_dice().clone(); eng.backward(lab, macro=macro, loss_scale=0.5)
    launches = [(e["kernel"], e["layer"], e["launches"]) for e in eng.profile_end()]
    return v, eng.grads.clone(), launches


@pytest.mark.parametrize("macro", [True, False])
def test_off_is_off(macro):
    """After ``set_dice_shape()`` with the defaults, and after ``set_dice_shape(None)`` behind a step under a real shape, the loss
    vector and ``grads`` are a fresh engine's bit for bit and so is the launch list: no shaped finalize."""
    B, H, W, C, sn, P, L, ic = CASE
    images, labels = case_inputs(CASE, MARGIN_SEED[CASE])
    x = torch.from_numpy(images).cuda(); lab = torch.from_numpy(labels[..., 0].copy()).cuda()
    fresh = lambda: make(B, H, W, C, sn, P, L, ic, training=True)[1]      # noqa: E731
    v0, g0, l0 = _profiled_step(fresh(), x, lab, macro)
    assert PLAIN_FIN in {k for k, _, _ in l0} and FIN not in {k for k, _, _ in l0}

    eng = fresh()
    eng.set_dice_shape()
    assert eng.dice_shape is None
    v, g, l = _profiled_step(eng, x, lab, macro)
    assert torch.equal(v, v0) and torch.equal(g, g0) and l == l0

    eng = fresh()
    eng.set_dice_shape(alpha=0.3, beta=0.7, gamma=2.0, class_weight=(0.5, 2.0, 0.0))
    vs, gs, ls = _profiled_step(eng, x, lab, macro)
    assert FIN in {k for k, _, _ in ls} and PLAIN_FIN not in {k for k, _, _ in ls}
    assert not torch.equal(vs[:2], v0[:2]) and torch.equal(vs[2:], v0[2:]) and not torch.equal(gs, g0)     # the metrics never change
    assert [e for e in ls if e[0] != FIN] == [e for e in l0 if e[0] != PLAIN_FIN]      # only the finalize differs
    eng.set_dice_shape(None)
    assert eng.dice_shape is None
    v, g, l = _profiled_step(eng, x, lab, macro)
    assert torch.equal(v, v0) and torch.equal(g, g0) and l == l0


def test_two_shaped_runs_give_the_same_bits():
    B, H, W, C, sn, P, L, ic = CASE
    images, labels = case_inputs(CASE, MARGIN_SEED[CASE], absent=(1, 2, 1))
    x = torch.from_numpy(images).cuda(); lab = torch.from_numpy(labels[..., 0].copy()).cuda()
    eng = make(B, H, W, C, sn, P, L, ic, training=True)[1]
    eng.set_dice_shape(alpha=0.3, beta=0.7, gamma=0.75, class_weight="volume")
    a = _profiled_step(eng, x, lab, False)
    b = _profiled_step(eng, x, lab, False)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_set_dice_shape_checks_its_arguments_and_drops_a_pending_sum():
    from oct_image_segmentation_models_amd import _hip
    from oct_image_segmentation_models_amd._hip import OctError
    B, H, W, C, sn, P, L, ic = CASE
    cfg, eng, _, _ = make(B, H, W, C, sn, P, L, ic)
    for bad in (dict(alpha=-0.1), dict(alpha=0.0, beta=0.0), dict(gamma=0.0), dict(gamma=8.5), dict(class_weight=(1.0, 2.0)),
                dict(class_weight=(1.0, -2.0, 1.0)), dict(class_weight=(0.0, 0.0, 0.0)), dict(class_weight="balanced")):
        with pytest.raises(OctError, match="set_dice_shape"):
            eng.set_dice_shape(**bad)
    assert eng.dice_shape is None
    # the library's own checks, under the Python layer's
    import ctypes as Ct
    zeros = torch.zeros(C, dtype=torch.float32, device="cuda")
    for d in (_hip.DiceShape(-0.1, 0.5, 1.0, 0, None), _hip.DiceShape(0.0, 0.0, 1.0, 0, None), _hip.DiceShape(0.5, 0.5, 0.0, 0, None),
              _hip.DiceShape(0.5, 0.5, 8.5, 0, None), _hip.DiceShape(0.5, 0.5, 1.0, 3, None), _hip.DiceShape(0.5, 0.5, 1.0, 1, None),
              _hip.DiceShape(0.5, 0.5, 1.0, 1, zeros.data_ptr())):
        with pytest.raises(OctError, match="dice_shape"):
            eng._call("oct_unet_set_dice_shape", Ct.byref(d))
    images, labels = case_inputs(CASE, MARGIN_SEED[CASE])
    x = torch.from_numpy(images).cuda(); lab = torch.from_numpy(labels[..., 0].copy()).cuda()
    eng.forward(x, training=True, labels=lab)
    eng.set_dice_shape(alpha=0.3, beta=0.7)                   # between forward and loss: the pending sum is dropped
    with pytest.raises(OctError, match="forward"):
        eng.loss_dice()
    eng.forward(x, training=True, labels=lab)
    assert np.isfinite(eng.loss_dice().cpu().numpy()).all()


# ---- end to end ------------------------------------------------------------------------------------------------------------------
def test_train_model_equals_the_engine_stepped_by_hand(tmp_path):
    """``train_model`` with ``loss_fn_kwargs={"alpha": 0.3, "beta": 0.7}`` and ``apply_class_weight=True`` ("balanced" weights) for two
    epochs: the recorded losses are those of the same engine stepped by hand under ``set_dice_shape``, bit for bit, and
    ``training_params.hdf5`` carries the ``loss_param:`` attributes."""
    from oct_image_segmentation_models_amd import optimizers
    from oct_image_segmentation_models_amd.common import data_generator as data_gen, h5io
    from oct_image_segmentation_models_amd.models import get_model_class
    from oct_image_segmentation_models_amd.models.batch_feed import BatchFeed
    from oct_image_segmentation_models_amd.training.training import _balanced_class_weight, train_model
    from oct_image_segmentation_models_amd.training.training_parameters import TrainingParams
    tr_i, tr_l = on.synth_scans(8, 32, 64, 3, seed=11)
    va_i, va_l = on.synth_scans(4, 32, 64, 3, seed=12)
    h5io.save(tmp_path / "data.hdf5", {"train_images": tr_i, "train_labels": tr_l, "val_images": va_i, "val_labels": va_l})
    kw = dict(model_architecture="unet", training_dataset_path=tmp_path / "data.hdf5", initial_model=None, opt_con=optimizers.Adam,
              opt_params={"learning_rate": 4e-3}, loss="dice_loss_macro", metric="dice_coef_macro", epochs=2, batch_size=4,
              model_hyperparameters={"pool_layers": 2}, seed=3, class_weight="balanced")
    res = train_model(TrainingParams(results_location=tmp_path / "shaped", loss_fn_kwargs={"alpha": 0.3, "beta": 0.7},
                                     apply_class_weight=True, **kw), None)
    torch.cuda.synchronize()
    cw = [float(w) for w in _balanced_class_weight(np.concatenate((tr_l, va_l)))]
    want_shape = dict(alpha=0.3, beta=0.7, gamma=1.0, class_weight=cw)
    assert res.model._dice_shape == want_shape and res.model._engines["train"].dice_shape == want_shape
    attrs = {k[len("attr:"):]: v for k, v in h5io.load(res.save_foldername / "training_params.hdf5").items() if k.startswith("attr:")}
    given = {k: v for k, v in attrs.items() if k.startswith("loss_param: ")}
    assert set(given) == {"loss_param: alpha", "loss_param: beta", "loss_param: dice_class_weight"}
    assert float(given["loss_param: alpha"]) == 0.3 and float(given["loss_param: beta"]) == 0.7
    assert np.asarray(given["loss_param: dice_class_weight"]).tolist() == cw

    # the same engine by hand: the model class's own construction, the generator's own batches
    container = get_model_class("unet")(input_channels=1, num_classes=3, image_height=32, image_width=64, pool_layers=2)
    model = container.build_model()
    model.config["seed"] = 3
    eng = model._ensure_engine(4, True)
    eng.set_dice_shape(**want_shape)
    opt = optimizers.Adam(learning_rate=4e-3)
    gen = data_gen.DataGenerator(tr_i, tr_l, 4, [], "none", (), False, container.get_preprocess_input_fn(), seed=3, device_aug=False)
    feed = BatchFeed("cuda:0")
    losses = []
    for _ in range(2):
        acc = None
        for i in range(len(gen)):
            hb = feed.host_batch(gen, i, 0, 1)
            x = torch.from_numpy(np.ascontiguousarray(hb.x)).cuda(); lab = torch.from_numpy(np.ascontiguousarray(hb.labels)).cuda()
            eng.forward(x, training=True, labels=lab, want_probs=False)
            v = eng.loss_dice()
            eng.backward(lab, macro=True, loss_scale=1.0)
            opt.apply(eng)
            acc = v.clone() if acc is None else acc + v
        gen.on_epoch_end()
        losses.append(float((acc / len(gen)).cpu().numpy()[0]))
    print("train_model", res.history["loss"], "by hand", losses)
    assert res.history["loss"] == losses

    # without the switch and the keywords nothing changes: the weights are recorded, not applied
    plain = train_model(TrainingParams(results_location=tmp_path / "plain", **kw), None)
    assert plain.model._dice_shape is None and plain.model._engines["train"].dice_shape is None
    assert plain.history["loss"] != losses
    pattrs = h5io.load(plain.save_foldername / "training_params.hdf5")
    assert not [k for k in pattrs if "loss_param" in k]
