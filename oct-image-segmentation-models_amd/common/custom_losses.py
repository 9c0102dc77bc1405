"""Loss registry with the reference's names and factory signatures
(oct_image_segmentation_models/common/custom_losses.py:47-81,230-255).

On the accelerated path the Dice sums are fused into the HIP head kernel, so ``Model.compile`` selects the
loss by the ``oct_loss`` tag of the callable; the callables themselves are numpy restatements usable on host
arrays (e.g. for evaluation code).  ``focal_dice_loss`` (reference :98-178, built on the third-party ``focal-loss``
package: published formula restated, parity unpinned) and ``bce_dice_loss`` (reference :84-91, Keras 2.9's
``binary_crossentropy`` restated, parity unpinned) are implemented the same way; ``bce_focal_loss`` and the plain
focal loss raise."""
from __future__ import annotations

import numpy as np


def _one_hot(y_true, num_classes):
    lab = np.asarray(y_true)
    if lab.ndim == 4 and lab.shape[-1] == 1:
        lab = lab[..., 0]
    return np.eye(num_classes, dtype=np.float64)[lab.astype(np.int64)]


def dice_loss_micro(*, is_y_true_sparse: bool, num_classes: int, **kwargs):
    def _dice_loss_micro(y_true, y_pred, smooth=1e-05):
        if is_y_true_sparse:
            y_true = _one_hot(y_true, num_classes)
        y_true_f = np.asarray(y_true, np.float64).ravel()
        y_pred_f = np.asarray(y_pred, np.float64).ravel()
        score = (2.0 * np.sum(y_true_f * y_pred_f) + smooth) / (np.sum(y_true_f) + np.sum(y_pred_f) + smooth)
        return 1.0 - score

    _dice_loss_micro.oct_loss = "dice_loss_micro"
    return _dice_loss_micro


def dice_loss_macro(*, is_y_true_sparse: bool, num_classes: int, **kwargs):
    def _dice_loss_macro(y_true, y_pred, smooth=1e-05):
        if is_y_true_sparse:
            y_true = _one_hot(y_true, num_classes)
        y_true = np.asarray(y_true, np.float64)
        y_pred = np.asarray(y_pred, np.float64)
        reduce_axis = tuple(range(1, y_pred.ndim - 1))
        intersection = np.sum(y_true * y_pred, axis=reduce_axis)
        denominator = np.sum(y_true, axis=reduce_axis) + np.sum(y_pred, axis=reduce_axis)
        score = (2.0 * intersection + smooth) / (denominator + smooth)
        return 1.0 - np.mean(score)

    _dice_loss_macro.oct_loss = "dice_loss_macro"
    return _dice_loss_macro


FOCAL_EPS = 1e-7   # keras backend epsilon: probabilities are clipped to [eps, 1 - eps] before the logarithm


def focal_dice_loss(*, num_classes: int, gamma: float = 2, class_weight=None, focal_loss_weight: float = 0.5,
                    dice_macro: bool = True, **kwargs):
    """``focal_dice_loss`` / ``SparseCategoricalFocalDiceLoss`` (reference custom_losses.py:98-178), sparse labels:
    ``w * sum_px[cw[y] (1-p_y)^gamma (-log p_y)] / size(y_true) + (1 - w) * dice_loss_{macro|micro}``."""
    cw = None if class_weight is None else np.asarray(class_weight, np.float64)
    if cw is not None and cw.shape != (num_classes,):
        raise ValueError(f"class_weight must have {num_classes} entries")
    dice_fn = (dice_loss_macro if dice_macro else dice_loss_micro)(is_y_true_sparse=True, num_classes=num_classes)

    def _focal_dice_loss(y_true, y_pred):
        lab = np.asarray(y_true)
        lab = (lab[..., 0] if (lab.ndim == 4 and lab.shape[-1] == 1) else lab).astype(np.int64)
        p = np.asarray(y_pred, np.float64)
        py = np.clip(np.take_along_axis(p, lab[..., None], axis=-1)[..., 0], FOCAL_EPS, 1.0 - FOCAL_EPS)
        w = 1.0 if cw is None else cw[lab]
        focal = np.sum(w * (1.0 - py) ** gamma * -np.log(py)) / lab.size
        return focal_loss_weight * focal + (1.0 - focal_loss_weight) * dice_fn(y_true, y_pred)

    _focal_dice_loss.oct_loss = "focal_dice_loss"
    _focal_dice_loss.oct_focal = {"gamma": float(gamma), "class_weight": None if cw is None else cw.tolist(),
                                  "focal_loss_weight": float(focal_loss_weight), "dice_macro": bool(dice_macro)}
    return _focal_dice_loss


def bce_dice_loss(*, num_classes: int, bce_inner_eps: bool = True, **kwargs):
    """``bce_dice_loss`` (reference custom_losses.py:84-91): ``keras.losses.binary_crossentropy(y, p) + dice_loss_micro``.
    The cross-entropy restates Keras 2.9's ``backend.binary_crossentropy`` (``from_logits=False``) on the clipped
    probabilities, ``-(y ln(pc + e) + (1 - y) ln(1 - pc + e))``, averaged over the class axis and then over the batch
    (one mean over every element).  ``bce_inner_eps=False`` drops the inner ``+ e`` (engine option "bce_inner_eps").
    Sparse ``y_true`` (labels) is accepted as well as the dense one-hot the reference feeds it."""
    dice_fn = dice_loss_micro(is_y_true_sparse=False, num_classes=num_classes)
    e = FOCAL_EPS if bce_inner_eps else 0.0

    def _bce_dice_loss(y_true, y_pred):
        p = np.asarray(y_pred, np.float64)
        y = np.asarray(y_true)
        y = np.asarray(y, np.float64) if y.shape == p.shape else _one_hot(y, num_classes)
        pc = np.clip(p, FOCAL_EPS, 1.0 - FOCAL_EPS)
        qc = np.clip(1.0 - p, FOCAL_EPS, 1.0 - FOCAL_EPS)
        bce = -(y * np.log(pc + e) + (1.0 - y) * np.log(qc + e))
        return np.mean(bce) + dice_fn(y, p)

    _bce_dice_loss.oct_loss = "bce_dice_loss"
    return _bce_dice_loss


def masked_loss_reference(labels, probs, num_classes: int, ignore, kind: str = "dice", *, smooth: float = 1e-05,
                          gamma: float = 2.0, class_weight=None, focal_loss_weight: float = 0.5, bce_inner_eps: bool = True) -> dict:
    """The losses above and the two Dice metrics with an ignore label, as the engine defines them
    (``oct_unet_set_ignore_label``): sparse ``labels`` (B,H,W[,1]), ``probs`` (B,H,W,C), fp64.  A pixel whose label equals
    ``ignore`` (``None``: no such pixel) is dropped from every sum -- its one-hot row AND its probabilities -- and the focal
    / BCE mean divides by the number of counted pixels of the batch (times C for BCE), 0 where there is none.
    ``kind``: ``"dice"``, ``"focal"`` or ``"bce"``.  Returns a dict of ``dice_loss_macro``, ``dice_loss_micro``,
    ``dice_coef_macro``, ``dice_coef_micro``, ``term`` (the focal or BCE mean; 0 for ``"dice"``) and the combined
    ``loss_macro`` / ``loss_micro``: ``w term + (1 - w) dice`` for focal, ``term + dice_loss_micro`` for BCE (whose
    ``loss_macro`` is ``None``: the reference defines that loss with the micro Dice only), the Dice losses themselves for
    ``"dice"``.  A batch without a counted pixel has ``dice_coef_micro = 0/0 = nan``, as the reference's formula gives."""
    if kind not in ("dice", "focal", "bce"):
        raise ValueError(f"masked_loss_reference: unknown kind {kind!r}")
    lab = np.asarray(labels)
    lab = (lab[..., 0] if (lab.ndim == 4 and lab.shape[-1] == 1) else lab).astype(np.int64)
    p = np.asarray(probs, np.float64)
    m = np.ones(lab.shape, bool) if ignore is None else lab != int(ignore)
    safe = np.where(m & (lab < num_classes), lab, 0)
    y = np.eye(num_classes, dtype=np.float64)[safe] * (m & (lab < num_classes))[..., None]   # a value that is no class: all-zero row
    pm = p * m[..., None]
    ph = (p > 0.5) * m[..., None]
    ax = (1, 2)
    I, T, P = np.sum(y * pm, axis=ax), np.sum(y, axis=ax), np.sum(pm, axis=ax)
    Ih, Ph = np.sum(y * ph, axis=ax), np.sum(ph, axis=ax)
    out = {"dice_loss_macro": float(1.0 - np.mean((2.0 * I + smooth) / (T + P + smooth))),
           "dice_loss_micro": float(1.0 - (2.0 * I.sum() + smooth) / (T.sum() + P.sum() + smooth)),
           "dice_coef_macro": float(np.mean((2.0 * Ih + 1e-05) / (T + Ph + 1e-05)))}
    with np.errstate(invalid="ignore", divide="ignore"):
        out["dice_coef_micro"] = float(np.float64(2.0) * Ih.sum() / (T.sum() + Ph.sum()))
    count = int(m.sum())
    inv = 1.0 / count if count else 0.0
    if kind == "focal":
        py = np.clip(np.take_along_axis(p, safe[..., None], axis=-1)[..., 0], FOCAL_EPS, 1.0 - FOCAL_EPS)
        cw = 1.0 if class_weight is None else np.asarray(class_weight, np.float64)[safe]
        term, w = float(np.sum((cw * (1.0 - py) ** gamma * -np.log(py))[m]) * inv), float(focal_loss_weight)
        out.update(term=term, loss_macro=w * term + (1.0 - w) * out["dice_loss_macro"],
                   loss_micro=w * term + (1.0 - w) * out["dice_loss_micro"])
    elif kind == "bce":
        e = FOCAL_EPS if bce_inner_eps else 0.0
        pc, qc = np.clip(p, FOCAL_EPS, 1.0 - FOCAL_EPS), np.clip(1.0 - p, FOCAL_EPS, 1.0 - FOCAL_EPS)
        term = float(np.sum(-(y * np.log(pc + e) + (1.0 - y) * np.log(qc + e))[m]) * inv / num_classes)
        out.update(term=term, loss_macro=None, loss_micro=term + out["dice_loss_micro"])
    else:
        out.update(term=0.0, loss_macro=out["dice_loss_macro"], loss_micro=out["dice_loss_micro"])
    return out


def _out_of_scope(name, why=None):
    def factory(**kwargs):
        raise NotImplementedError(why or f"loss '{name}' is outside the accelerated path (only the Dice losses, "
                                  "focal_dice_loss and bce_dice_loss are implemented; see DESIGN.md section 11)")
    return factory


custom_loss_objects = {
    "bce_dice_loss": {"function": bce_dice_loss, "takes_sparse": False},
    "dice_loss_micro": {"function": dice_loss_micro, "takes_sparse": False},
    "dice_loss_macro": {"function": dice_loss_macro, "takes_sparse": False},
    "focal_loss": {"function": _out_of_scope("focal_loss"), "takes_sparse": True},
    "bce_focal_loss": {"function": _out_of_scope(
        "bce_focal_loss", "loss 'bce_focal_loss': the reference's own registry entry cannot be called through the registry "
        "(its function takes (y_true, y_pred), the registry passes num_classes= / is_y_true_sparse=), so there is "
        "nothing to mirror; see DESIGN.md section 11"), "takes_sparse": False},
    "focal_dice_loss": {"function": focal_dice_loss, "takes_sparse": True},
}
