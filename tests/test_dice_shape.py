"""The shaped Dice term on the host: the loss factories' new keywords, the numpy restatement
``shaped_dice_reference`` against torch-fp64 autograd, the fold of the backward constants into the (num, den) pairs of the head
kernels evaluated in float32, the validation of the parameters and ``TrainingParams(apply_class_weight=...)``.  No GPU."""
import numpy as np
import pytest
import torch

from oct_image_segmentation_models_amd.common import custom_losses as cl
from tests.dice_shape_cases import SHAPES, drop_class_from_image, shaped_dice_t

B, H, W, C = 3, 12, 20, 3
IGN = 255


def _inputs(seed=0):
    rng = np.random.default_rng(seed)
    labels = rng.integers(0, C, (B, H, W, 1)).astype(np.uint8)
    logits = rng.normal(size=(B, H, W, C)) + 2.0 * np.eye(C)[labels[..., 0]]
    probs = np.exp(logits) / np.exp(logits).sum(-1, keepdims=True)
    return labels, probs


LABELS, PROBS = _inputs()


def _variants():
    """(name, labels, probs, ignore, shape): every shape of SHAPES, "volume" with class 2 absent from image 1, an ignore label,
    and a class predicted exactly (u = 0: the clamp of the focal-Tversky power is active)."""
    out = [(k, LABELS, PROBS, None, s) for k, s in SHAPES.items()]
    out.append(("volume_absent", drop_class_from_image(LABELS, 1, 2, 0), PROBS, None, SHAPES["volume"]))
    masked = LABELS.copy(); masked[:, :3] = IGN; masked[2, :, 5:9] = IGN
    out.append(("ignore_tversky", masked, PROBS, IGN, SHAPES["focal_tversky_075"]))
    out.append(("ignore_volume", drop_class_from_image(masked, 0, 1, 2), PROBS, IGN, SHAPES["volume"]))
    exact = PROBS.copy(); exact[0, ..., 1] = LABELS[0, ..., 0] == 1
    out.append(("clamped", LABELS, exact, None, SHAPES["focal_tversky_2"]))
    out.append(("clamped_075", LABELS, exact, None, SHAPES["focal_tversky_075"]))
    return out


VARIANTS = _variants()


def _y(labels, ignore):
    lab = labels[..., 0].astype(np.int64)
    keep = np.ones(lab.shape, bool) if ignore is None else lab != ignore
    return np.eye(C)[np.where(keep, lab, 0)] * keep[..., None], keep


def _grad_from_constants(k, y, keep, macro):
    """dloss/dp = -m (y A - B) / D^2 from the reference's constants; 0 at ignored pixels."""
    bc = (lambda a: np.asarray(a)[:, None, None, :]) if macro else (lambda a: np.asarray(a))
    return -bc(k["m"]) * (y * bc(k["A"]) - bc(k["B"])) / bc(k["D"]) ** 2 * keep[..., None]


@pytest.mark.parametrize("macro", [True, False])
@pytest.mark.parametrize("variant", VARIANTS, ids=[v[0] for v in VARIANTS])
def test_reference_equals_autograd(variant, macro):
    _, labels, probs, ignore, shape = variant
    ref = cl.shaped_dice_reference(labels, probs, C, ignore, **shape)
    p = torch.tensor(probs, requires_grad=True)
    loss = shaped_dice_t(p, labels, C, macro, ignore=ignore, **shape)
    loss.backward()
    want = ref["loss_macro" if macro else "loss_micro"]
    assert abs(float(loss.detach()) - want) < 1e-12 * max(1.0, abs(want))
    y, keep = _y(labels, ignore)
    g = _grad_from_constants(ref["macro" if macro else "micro"], y, keep, macro)
    scale = np.abs(p.grad.numpy()).max()
    assert scale > 0 and np.abs(g - p.grad.numpy()).max() < 1e-10 * scale


def test_plain_shape_is_todays_dice():
    ref = cl.shaped_dice_reference(LABELS, PROBS, C)
    y, _ = _y(LABELS, None)
    I, T, P = (y * PROBS).sum((1, 2)), y.sum((1, 2)), PROBS.sum((1, 2))
    assert abs(ref["loss_macro"] - (1.0 - np.mean((2 * I + 1e-5) / (T + P + 1e-5)))) < 1e-14
    assert abs(ref["loss_micro"] - (1.0 - (2 * I.sum() + 1e-5) / (T.sum() + P.sum() + 1e-5))) < 1e-14
    # the fold of plain Dice is Dice's own pair: num' = 2I + s, den' = T + P + s (the kernels' 1 / (B C) is inside m)
    k = ref["macro"]
    num, den = cl.fold_dice_constants(k["m"] * B * C, k["A"], k["B"], k["D"])
    assert np.allclose(num, 2 * I + 1e-5, rtol=1e-13) and np.allclose(den, T + P + 1e-5, rtol=1e-13)


def _kernel_expression_f32(y, num, den):
    """-(2 y den - num) / den^2 as head_bwd_* form it: float32 operands, float32 operations."""
    y, num, den = np.float32(y), np.asarray(num, np.float32), np.asarray(den, np.float32)
    with np.errstate(over="ignore"):
        return -(np.float32(2.0) * y * den - num) / (den * den)


@pytest.mark.parametrize("macro", [True, False])
@pytest.mark.parametrize("variant", VARIANTS, ids=[v[0] for v in VARIANTS])
def test_fold_in_float32(variant, macro):
    """The folded pair, rounded to float32 and put through the kernels' expression in float32, gives m (yA - B) / D^2 within
    1e-6 relative, and exactly 0 where m = 0 (zero class weight, active clamp)."""
    _, labels, probs, ignore, shape = variant
    k = cl.shaped_dice_reference(labels, probs, C, ignore, **shape)["macro" if macro else "micro"]
    m, A, Bc, D = np.broadcast_arrays(k["m"], k["A"], k["B"], k["D"])
    num, den = cl.fold_dice_constants(m, A, Bc, D)
    for yv in (0.0, 1.0):
        got = _kernel_expression_f32(yv, num, den).astype(np.float64)
        want = -m * (yv * A - Bc) / D ** 2
        assert np.isfinite(got).all()
        assert (got[m == 0] == 0).all()
        nz = m != 0
        assert np.all(np.abs(got[nz] - want[nz]) <= 1e-6 * np.abs(want[nz])), (got, want)
    if "zero" in variant[0] or (macro and "clamped" in variant[0]):      # (the batch's micro triple is not at the clamp)
        assert (m == 0).any()


def test_fold_of_a_vanishing_m_is_the_zero_pair():
    """A den' past 1e18 (its float32 square would near the overflow, 2 y den' - num' could meet inf - inf) is stored as the
    zero pair as well: the gradient it stands for is below 1e-18."""
    num, den = cl.fold_dice_constants(np.array([1e-30, 0.0, 1.0]), 2.0, 0.5, 1.0)
    assert num[0] == 0 and den[0] == 1e30 and num[1] == 0 and den[1] == 1e30 and den[2] == 1.0
    assert (_kernel_expression_f32(1.0, num[:2], den[:2]) == 0).all()


# ---- the factories -----------------------------------------------------------------------------------------------------------
def _dice_micro_before(y_true, y_pred, smooth=1e-05):
    y_true_f = np.asarray(y_true, np.float64).ravel(); y_pred_f = np.asarray(y_pred, np.float64).ravel()
    return 1.0 - (2.0 * np.sum(y_true_f * y_pred_f) + smooth) / (np.sum(y_true_f) + np.sum(y_pred_f) + smooth)


def _dice_macro_before(y_true, y_pred, smooth=1e-05):
    y_true = np.asarray(y_true, np.float64); y_pred = np.asarray(y_pred, np.float64)
    ax = tuple(range(1, y_pred.ndim - 1))
    inter = np.sum(y_true * y_pred, axis=ax)
    return 1.0 - np.mean((2.0 * inter + smooth) / (np.sum(y_true, axis=ax) + np.sum(y_pred, axis=ax) + smooth))


def test_factories_with_defaults_return_what_they_returned():
    y = np.eye(C)[LABELS[..., 0]]
    for explicit in ({}, dict(alpha=0.5, beta=0.5, tversky_gamma=1.0, dice_class_weight=None)):
        mi = cl.dice_loss_micro(is_y_true_sparse=True, num_classes=C, **explicit)
        ma = cl.dice_loss_macro(is_y_true_sparse=True, num_classes=C, **explicit)
        assert mi.oct_dice_shape is None and ma.oct_dice_shape is None
        assert mi(LABELS, PROBS) == _dice_micro_before(y, PROBS) and ma(LABELS, PROBS) == _dice_macro_before(y, PROBS)
        fd = cl.focal_dice_loss(num_classes=C, gamma=2, class_weight=[0.5, 2.0, 1.25], focal_loss_weight=0.35, **explicit)
        py = np.clip(np.take_along_axis(PROBS, LABELS.astype(np.int64), axis=-1)[..., 0], 1e-7, 1 - 1e-7)
        focal = np.sum(np.array([0.5, 2.0, 1.25])[LABELS[..., 0]] * (1.0 - py) ** 2 * -np.log(py)) / LABELS.size
        assert fd(LABELS, PROBS) == 0.35 * focal + (1.0 - 0.35) * _dice_macro_before(y, PROBS) and fd.oct_dice_shape is None
        bd = cl.bce_dice_loss(num_classes=C, **explicit)
        pc, qc = np.clip(PROBS, 1e-7, 1 - 1e-7), np.clip(1.0 - PROBS, 1e-7, 1 - 1e-7)
        bce = np.mean(-(y * np.log(pc + 1e-7) + (1.0 - y) * np.log(qc + 1e-7)))
        assert bd(y, PROBS) == bce + _dice_micro_before(y, PROBS) and bd.oct_dice_shape is None
    assert set(cl.custom_loss_objects) == {"bce_dice_loss", "dice_loss_micro", "dice_loss_macro", "focal_loss", "bce_focal_loss",
                                           "focal_dice_loss"}


def test_factories_take_the_shape_keywords():
    kw = dict(alpha=0.3, beta=0.7, tversky_gamma=0.75, dice_class_weight=[0.5, 2.0, 0.0])
    shape = dict(alpha=0.3, beta=0.7, gamma=0.75, class_weight=[0.5, 2.0, 0.0])
    ref = cl.shaped_dice_reference(LABELS, PROBS, C, **shape)
    mi = cl.dice_loss_micro(is_y_true_sparse=True, num_classes=C, **kw)
    ma = cl.dice_loss_macro(is_y_true_sparse=True, num_classes=C, **kw)
    assert mi.oct_dice_shape == shape and ma.oct_dice_shape == shape
    assert mi.oct_loss == "dice_loss_micro" and ma.oct_loss == "dice_loss_macro"
    assert mi(LABELS, PROBS) == ref["loss_micro"] and ma(LABELS, PROBS) == ref["loss_macro"]
    dense = cl.dice_loss_macro(is_y_true_sparse=False, num_classes=C, **kw)
    assert dense(np.eye(C)[LABELS[..., 0]], PROBS) == ref["loss_macro"]
    plain = cl.focal_dice_loss(num_classes=C, gamma=2, class_weight=[0.5, 2.0, 1.25], focal_loss_weight=0.35)
    plain_dice = _dice_macro_before(np.eye(C)[LABELS[..., 0]], PROBS)
    fd = cl.focal_dice_loss(num_classes=C, gamma=2, class_weight=[0.5, 2.0, 1.25], focal_loss_weight=0.35, **kw)
    assert fd.oct_dice_shape == shape and fd.oct_focal["gamma"] == 2.0 and fd.oct_focal["class_weight"] == [0.5, 2.0, 1.25]
    assert abs(fd(LABELS, PROBS) - (plain(LABELS, PROBS) + 0.65 * (ref["loss_macro"] - plain_dice))) < 1e-14
    bd = cl.bce_dice_loss(num_classes=C, dice_class_weight="volume")
    assert bd.oct_dice_shape == dict(alpha=0.5, beta=0.5, gamma=1.0, class_weight="volume")
    vol = cl.shaped_dice_reference(LABELS, PROBS, C, class_weight="volume")["loss_micro"]
    plain_bd = cl.bce_dice_loss(num_classes=C)
    y = np.eye(C)[LABELS[..., 0]]
    assert abs(bd(y, PROBS) - (plain_bd(y, PROBS) - _dice_micro_before(y, PROBS) + vol)) < 1e-14


@pytest.mark.parametrize("bad", [dict(alpha=-0.1), dict(beta=-1.0), dict(alpha=0.0, beta=0.0), dict(alpha=float("nan")),
                                 dict(tversky_gamma=0.0), dict(tversky_gamma=8.5), dict(tversky_gamma=-1.0),
                                 dict(dice_class_weight=[1.0, 2.0]), dict(dice_class_weight=[1.0, -1.0, 1.0]),
                                 dict(dice_class_weight=[0.0, 0.0, 0.0]), dict(dice_class_weight=[1.0, float("inf"), 1.0]),
                                 dict(dice_class_weight="balanced")])
def test_invalid_parameters_raise(bad):
    for factory in (cl.dice_loss_macro, cl.dice_loss_micro):
        with pytest.raises(ValueError):
            factory(is_y_true_sparse=True, num_classes=C, **bad)
    with pytest.raises(ValueError):
        cl.focal_dice_loss(num_classes=C, **bad)
    with pytest.raises(ValueError):
        cl.bce_dice_loss(num_classes=C, **bad)
    names = {"tversky_gamma": "gamma", "dice_class_weight": "class_weight"}
    with pytest.raises(ValueError):
        cl.shaped_dice_reference(LABELS, PROBS, C, **{names.get(k, k): v for k, v in bad.items()})


def test_valid_edges_are_accepted():
    for ok in (dict(alpha=0.0, beta=1.0), dict(alpha=1.0, beta=0.0), dict(tversky_gamma=8.0), dict(tversky_gamma=1e-3)):
        assert cl.dice_loss_macro(is_y_true_sparse=True, num_classes=C, **ok).oct_dice_shape is not None


# ---- the workflow switch ------------------------------------------------------------------------------------------------------
def _params(tmp_path, **kw):
    from oct_image_segmentation_models_amd import optimizers
    from oct_image_segmentation_models_amd.training.training_parameters import TrainingParams
    return TrainingParams(model_architecture="unet", training_dataset_path=tmp_path / "data.hdf5", initial_model=None,
                          results_location=tmp_path / "results", opt_con=optimizers.Adam, metric="dice_coef_macro", epochs=1,
                          batch_size=2, **kw)


def test_apply_class_weight_reaches_the_factory(tmp_path):
    from oct_image_segmentation_models_amd.training.training import SHAPE_KEYS, loss_factory_kwargs
    cw = np.array([0.5, 2.0, 1.5])
    off = _params(tmp_path, loss="dice_loss_macro", class_weight=[0.5, 2.0, 1.5])
    assert off.apply_class_weight is False and loss_factory_kwargs(off, cw) == {}
    on_ = _params(tmp_path, loss="dice_loss_macro", class_weight=[0.5, 2.0, 1.5], apply_class_weight=True)
    kw = loss_factory_kwargs(on_, cw)
    assert kw == {"dice_class_weight": [0.5, 2.0, 1.5]}
    fn = cl.custom_loss_objects["dice_loss_macro"]["function"](num_classes=C, is_y_true_sparse=False, **kw)
    assert fn.oct_dice_shape == dict(alpha=0.5, beta=0.5, gamma=1.0, class_weight=[0.5, 2.0, 1.5])
    assert loss_factory_kwargs(_params(tmp_path, loss="dice_loss_macro", apply_class_weight=True), None) == {}     # nothing computed
    focal = _params(tmp_path, loss="focal_dice_loss", class_weight=[0.5, 2.0, 1.5], apply_class_weight=True)
    assert loss_factory_kwargs(focal, cw) == {"dice_class_weight": [0.5, 2.0, 1.5], "class_weight": [0.5, 2.0, 1.5]}
    named = _params(tmp_path, loss="focal_dice_loss", class_weight=[0.5, 2.0, 1.5], apply_class_weight=True,
                    loss_fn_kwargs={"class_weight": [1.0, 1.0, 1.0], "dice_class_weight": "volume", "alpha": 0.3})
    assert loss_factory_kwargs(named, cw) == {"class_weight": [1.0, 1.0, 1.0], "dice_class_weight": "volume", "alpha": 0.3}
    assert named.loss_fn_kwargs == {"class_weight": [1.0, 1.0, 1.0], "dice_class_weight": "volume", "alpha": 0.3}
    assert SHAPE_KEYS == ("alpha", "beta", "tversky_gamma", "dice_class_weight")


def test_training_params_file_gains_only_the_given_shape_keys(tmp_path):
    from oct_image_segmentation_models_amd.common import h5io
    from oct_image_segmentation_models_amd.training.training import save_training_params_file

    def attrs_of(folder, tp):
        folder.mkdir()
        save_training_params_file(folder, "summary", {"a": 1}, "md5", None, "stamp", tp, tp.opt_con())
        return {k[len("attr:"):]: v for k, v in h5io.load(folder / "training_params.hdf5").items() if k.startswith("attr:")}

    plain = _params(tmp_path, loss="dice_loss_macro")
    shaped = _params(tmp_path, loss="dice_loss_macro")
    shaped.loss_shape_kwargs = {"alpha": 0.3, "dice_class_weight": [0.5, 2.0, 1.5]}
    a, b = attrs_of(tmp_path / "a", plain), attrs_of(tmp_path / "b", shaped)
    assert not [k for k in a if k.startswith("loss_param")]
    assert set(b) - set(a) == {"loss_param: alpha", "loss_param: dice_class_weight"}
    assert float(np.asarray(b["loss_param: alpha"])) == 0.3
    assert np.asarray(b["loss_param: dice_class_weight"]).tolist() == [0.5, 2.0, 1.5]
