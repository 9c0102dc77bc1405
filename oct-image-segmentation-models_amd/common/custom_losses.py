"""Loss registry with the reference's names and factory signatures
(oct_image_segmentation_models/common/custom_losses.py:47-81,230-255).

On the accelerated path the Dice sums are fused into the HIP head kernel, so ``Model.compile`` selects the
loss by the ``oct_loss`` tag of the callable; the callables themselves are numpy restatements usable on host
arrays (e.g. for evaluation code).  ``focal_dice_loss`` (reference :98-178, built on the third-party ``focal-loss``
package: published formula restated, parity unpinned) and ``bce_dice_loss`` (reference :84-91, Keras 2.9's
``binary_crossentropy`` restated, parity unpinned) are implemented the same way; ``bce_focal_loss`` and the plain
focal loss raise.

The Dice term of all four takes a SHAPE: ``alpha`` / ``beta`` (Tversky index), ``tversky_gamma``
(focal-Tversky exponent) and ``dice_class_weight`` (a sequence of ``num_classes`` weights, or ``"volume"`` for the
generalized Dice loss).  A factory called with any of them tags its callable with ``oct_dice_shape``, which
``Model.compile`` hands to ``UNetEngine.set_dice_shape``; with none of them the callables are what they were.

The PIXEL term of ``focal_dice_loss`` / ``bce_dice_loss`` takes a per-pixel weight: ``edge_weight``, a
dict ``{"radius", "weight", "profile", "sigma"}`` (``common.utils.check_edge_weight``), weights every pixel by
``lut[squared distance to the nearest class border]`` -- the U-Net paper's weight map, ReLayNet's boundary-weighted
cross-entropy.  The mean still divides by the number of pixels, not by the sum of the weights (Keras ``sample_weight``).  The
factory tags its callable with ``oct_edge_weight``; the Dice factories refuse the keyword (they have no pixel term)."""
from __future__ import annotations

import numpy as np


def _one_hot(y_true, num_classes):
    lab = np.asarray(y_true)
    if lab.ndim == 4 and lab.shape[-1] == 1:
        lab = lab[..., 0]
    return np.eye(num_classes, dtype=np.float64)[lab.astype(np.int64)]


def _edge_weight_spec(edge_weight):
    """The validated spec of the ``edge_weight`` keyword, or None."""
    if edge_weight is None:
        return None
    from .utils import check_edge_weight
    return check_edge_weight(edge_weight)


def _edge_weights(spec, labels, num_classes):
    """float64 (B,H,W) weights of ``spec`` for sparse ``labels`` (1 everywhere for ``spec = None``)."""
    if spec is None:
        return 1.0
    from .utils import edge_weight_lut, edge_weight_reference
    lab = np.asarray(labels)
    lab = lab[..., 0] if (lab.ndim == 4 and lab.shape[-1] == 1) else lab
    lut = edge_weight_lut(spec["radius"], spec["profile"], spec["weight"], spec["sigma"])
    return edge_weight_reference(lab.astype(np.uint8), num_classes, spec["radius"], lut).astype(np.float64)


def _no_edge_weight(name, kwargs):
    if kwargs.get("edge_weight") is not None:
        raise ValueError(f"{name}: edge_weight weights the pixel term of focal_dice_loss / bce_dice_loss; a Dice loss has none")


DICE_CLAMP = 1e-7     # focal-Tversky: L = max(1 - TI, DICE_CLAMP) ** gamma for gamma != 1


def check_dice_shape(num_classes: int, alpha=0.5, beta=0.5, gamma=1.0, class_weight=None):
    """The validated shape ``{"alpha", "beta", "gamma", "class_weight"}`` (``class_weight``: None, ``"volume"`` or a list of
    ``num_classes`` floats), or None where it is plain Dice (alpha = beta = 1/2, gamma = 1, no weights).  ``ValueError`` for
    alpha or beta < 0, alpha + beta = 0, gamma outside (0, 8], weights that are negative, not finite, all zero or of
    another length."""
    alpha, beta, gamma = float(alpha), float(beta), float(gamma)
    if not (np.isfinite(alpha) and np.isfinite(beta) and alpha >= 0.0 and beta >= 0.0 and alpha + beta > 0.0):
        raise ValueError(f"dice shape: alpha, beta must be finite and >= 0 with alpha + beta > 0, not {alpha}, {beta}")
    if not 0.0 < gamma <= 8.0:
        raise ValueError(f"dice shape: gamma must be in (0, 8], not {gamma}")
    if class_weight is not None and not (isinstance(class_weight, str) and class_weight == "volume"):
        if isinstance(class_weight, str):
            raise ValueError(f'dice shape: class_weight must be None, "volume" or {num_classes} weights, not {class_weight!r}')
        w = np.asarray(class_weight, np.float64)
        if w.shape != (num_classes,) or not np.all(np.isfinite(w)) or np.any(w < 0.0) or not np.any(w > 0.0):
            raise ValueError(f"dice shape: class_weight must be {num_classes} finite weights >= 0, not all zero")
        class_weight = w.tolist()
    if alpha == 0.5 and beta == 0.5 and gamma == 1.0 and class_weight is None:
        return None
    return {"alpha": alpha, "beta": beta, "gamma": gamma, "class_weight": class_weight}


def _volume_weights(T):
    """1 / T^2 along the last axis; a T of 0 takes the largest weight of its row, a row of zeros all ones."""
    T = np.asarray(T, np.float64)
    with np.errstate(divide="ignore"):
        w = np.where(T > 0.0, 1.0 / (T * T), 0.0)
    wmax = w.max(axis=-1, keepdims=True)
    return np.where(wmax == 0.0, 1.0, np.where(T > 0.0, w, wmax))


def _shape_term(u, gamma):
    """``(L, dL/du)`` of ``u = 1 - TI``."""
    u = np.asarray(u, np.float64)
    if gamma == 1.0:
        return u, np.ones_like(u)
    on = u > DICE_CLAMP
    uc = np.where(on, u, DICE_CLAMP)
    return uc ** gamma, np.where(on, gamma * uc ** (gamma - 1.0), 0.0)


def fold_dice_constants(m, A, B, D):
    """The pair ``(num', den')`` the head backward kernels read in place of Dice's ``(2I + s, T + P + s)``: they form
    ``-(2 y den' - num') / den'^2`` in float32, and ``den' = 2 D^2 / (A m)``, ``num' = 4 B D^2 / (A^2 m)`` make that
    ``-m (y A - B) / D^2``.  ``m == 0`` -- or a ``den'`` of 1e18 and more -- is stored as ``(0, 1e30)``: the square of 1e30
    overflows float32 to +inf and the quotient is exactly 0."""
    m, A, B, D = np.broadcast_arrays(*(np.asarray(v, np.float64) for v in (m, A, B, D)))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        den, num = 2.0 * D * D / (A * m), 4.0 * B * D * D / (A * A * m)
    zero = ~(m > 0.0) | ~(den < 1e18)
    return np.where(zero, 0.0, num), np.where(zero, 1e30, den)


def _shaped_dice(y, p, smooth, alpha=0.5, beta=0.5, gamma=1.0, class_weight=None) -> dict:
    """The definition on a one-hot ``y`` and probabilities ``p`` (B,H,W,C), ignored pixels already zeroed in both."""
    ax = tuple(range(1, p.ndim - 1))
    I, T, P = np.sum(y * p, axis=ax), np.sum(y, axis=ax), np.sum(p, axis=ax)       # (B, C)
    Bn, C = I.shape
    if class_weight is None:
        w_bc, w_c = np.ones((Bn, C)), np.ones(C)
    elif isinstance(class_weight, str):
        w_bc, w_c = _volume_weights(T), _volume_weights(T.sum(axis=0))
    else:
        w_c = np.asarray(class_weight, np.float64)
        w_bc = np.broadcast_to(w_c, (Bn, C))

    def consts(I, T, P):
        N = 2.0 * I + smooth
        D = 2.0 * I + 2.0 * alpha * (P - I) + 2.0 * beta * (T - I) + smooth
        L, gu = _shape_term(1.0 - N / D, gamma)
        return L, gu, D, 2.0 * D - 2.0 * (1.0 - alpha - beta) * N, 2.0 * alpha * N

    L, gu, D, A, Bc = consts(I, T, P)
    wn = w_bc / w_bc.sum(axis=1, keepdims=True)
    macro = {"w": w_bc, "L": L, "D": D, "A": A, "B": Bc, "m": wn * gu / Bn}
    Lu, guu, Du, Au, Bu = consts(np.sum(w_c * I), np.sum(w_c * T), np.sum(w_c * P))
    micro = {"w": w_c, "L": Lu, "D": Du, "A": Au, "B": Bu, "m": w_c * guu}
    return {"loss_macro": float(np.mean(np.sum(wn * L, axis=1))), "loss_micro": float(Lu), "macro": macro, "micro": micro,
            "I": I, "T": T, "P": P}


def shaped_dice_reference(labels, probs, num_classes: int, ignore=None, *, smooth: float = 1e-05, **shape) -> dict:
    """The shaped Dice term as the engine defines it (``oct_unet_set_dice_shape``), in fp64: sparse
    ``labels`` (B,H,W[,1]), ``probs`` (B,H,W,C), ``ignore`` as in ``masked_loss_reference``, ``shape`` the keywords of
    ``UNetEngine.set_dice_shape`` (``alpha``, ``beta``, ``gamma``, ``class_weight``).  Returns ``loss_macro``, ``loss_micro``,
    the sums ``I``, ``T``, ``P`` (B, C) and, under ``macro`` (arrays (B, C)) and ``micro`` (``w``, ``m`` (C,), the rest
    scalars), the constants ``w``, ``L``, ``D``, ``A``, ``B``, ``m`` of the gradient
    ``dloss/dp = -m (y A - B) / D^2`` for a pixel's class-c probability with one-hot y."""
    sh = check_dice_shape(num_classes, **shape) or {}
    lab = np.asarray(labels)
    lab = (lab[..., 0] if (lab.ndim == 4 and lab.shape[-1] == 1) else lab).astype(np.int64)
    p = np.asarray(probs, np.float64)
    m = np.ones(lab.shape, bool) if ignore is None else lab != int(ignore)
    ok = m & (lab < num_classes)
    y = np.eye(num_classes, dtype=np.float64)[np.where(ok, lab, 0)] * ok[..., None]
    return _shaped_dice(y, p * m[..., None], smooth, **sh)


def dice_loss_micro(*, is_y_true_sparse: bool, num_classes: int, alpha: float = 0.5, beta: float = 0.5,
                    tversky_gamma: float = 1.0, dice_class_weight=None, **kwargs):
    _no_edge_weight("dice_loss_micro", kwargs)
    shape = check_dice_shape(num_classes, alpha, beta, tversky_gamma, dice_class_weight)

    def _dice_loss_micro(y_true, y_pred, smooth=1e-05):
        if is_y_true_sparse:
            y_true = _one_hot(y_true, num_classes)
        if shape:
            return _shaped_dice(np.asarray(y_true, np.float64), np.asarray(y_pred, np.float64), smooth, **shape)["loss_micro"]
        y_true_f = np.asarray(y_true, np.float64).ravel()
        y_pred_f = np.asarray(y_pred, np.float64).ravel()
        score = (2.0 * np.sum(y_true_f * y_pred_f) + smooth) / (np.sum(y_true_f) + np.sum(y_pred_f) + smooth)
        return 1.0 - score

    _dice_loss_micro.oct_loss = "dice_loss_micro"
    _dice_loss_micro.oct_dice_shape = shape
    return _dice_loss_micro


def dice_loss_macro(*, is_y_true_sparse: bool, num_classes: int, alpha: float = 0.5, beta: float = 0.5,
                    tversky_gamma: float = 1.0, dice_class_weight=None, **kwargs):
    _no_edge_weight("dice_loss_macro", kwargs)
    shape = check_dice_shape(num_classes, alpha, beta, tversky_gamma, dice_class_weight)

    def _dice_loss_macro(y_true, y_pred, smooth=1e-05):
        if is_y_true_sparse:
            y_true = _one_hot(y_true, num_classes)
        if shape:
            return _shaped_dice(np.asarray(y_true, np.float64), np.asarray(y_pred, np.float64), smooth, **shape)["loss_macro"]
        y_true = np.asarray(y_true, np.float64)
        y_pred = np.asarray(y_pred, np.float64)
        reduce_axis = tuple(range(1, y_pred.ndim - 1))
        intersection = np.sum(y_true * y_pred, axis=reduce_axis)
        denominator = np.sum(y_true, axis=reduce_axis) + np.sum(y_pred, axis=reduce_axis)
        score = (2.0 * intersection + smooth) / (denominator + smooth)
        return 1.0 - np.mean(score)

    _dice_loss_macro.oct_loss = "dice_loss_macro"
    _dice_loss_macro.oct_dice_shape = shape
    return _dice_loss_macro


FOCAL_EPS = 1e-7   # keras backend epsilon: probabilities are clipped to [eps, 1 - eps] before the logarithm


def focal_dice_loss(*, num_classes: int, gamma: float = 2, class_weight=None, focal_loss_weight: float = 0.5,
                    dice_macro: bool = True, alpha: float = 0.5, beta: float = 0.5, tversky_gamma: float = 1.0,
                    dice_class_weight=None, edge_weight=None, **kwargs):
    """``focal_dice_loss`` / ``SparseCategoricalFocalDiceLoss`` (reference custom_losses.py:98-178), sparse labels:
    ``w * sum_px[cw[y] (1-p_y)^gamma (-log p_y)] / size(y_true) + (1 - w) * dice_loss_{macro|micro}``.  ``gamma`` and
    ``class_weight`` belong to the focal term; ``alpha``, ``beta``, ``tversky_gamma``, ``dice_class_weight`` shape the Dice term.
    ``edge_weight`` (``check_edge_weight``'s dict) multiplies each pixel's focal term by its border weight."""
    ew = _edge_weight_spec(edge_weight)
    cw = None if class_weight is None else np.asarray(class_weight, np.float64)
    if cw is not None and cw.shape != (num_classes,):
        raise ValueError(f"class_weight must have {num_classes} entries")
    dice_fn = (dice_loss_macro if dice_macro else dice_loss_micro)(
        is_y_true_sparse=True, num_classes=num_classes, alpha=alpha, beta=beta, tversky_gamma=tversky_gamma,
        dice_class_weight=dice_class_weight)

    def _focal_dice_loss(y_true, y_pred):
        lab = np.asarray(y_true)
        lab = (lab[..., 0] if (lab.ndim == 4 and lab.shape[-1] == 1) else lab).astype(np.int64)
        p = np.asarray(y_pred, np.float64)
        py = np.clip(np.take_along_axis(p, lab[..., None], axis=-1)[..., 0], FOCAL_EPS, 1.0 - FOCAL_EPS)
        w = (1.0 if cw is None else cw[lab]) * _edge_weights(ew, lab, num_classes)
        focal = np.sum(w * (1.0 - py) ** gamma * -np.log(py)) / lab.size
        return focal_loss_weight * focal + (1.0 - focal_loss_weight) * dice_fn(y_true, y_pred)

    _focal_dice_loss.oct_loss = "focal_dice_loss"
    _focal_dice_loss.oct_focal = {"gamma": float(gamma), "class_weight": None if cw is None else cw.tolist(),
                                  "focal_loss_weight": float(focal_loss_weight), "dice_macro": bool(dice_macro)}
    _focal_dice_loss.oct_dice_shape = dice_fn.oct_dice_shape
    _focal_dice_loss.oct_edge_weight = ew
    return _focal_dice_loss


def bce_dice_loss(*, num_classes: int, bce_inner_eps: bool = True, alpha: float = 0.5, beta: float = 0.5,
                  tversky_gamma: float = 1.0, dice_class_weight=None, edge_weight=None, **kwargs):
    """``bce_dice_loss`` (reference custom_losses.py:84-91): ``keras.losses.binary_crossentropy(y, p) + dice_loss_micro``.
    The cross-entropy restates Keras 2.9's ``backend.binary_crossentropy`` (``from_logits=False``) on the clipped
    probabilities, ``-(y ln(pc + e) + (1 - y) ln(1 - pc + e))``, averaged over the class axis and then over the batch
    (one mean over every element).  ``bce_inner_eps=False`` drops the inner ``+ e`` (engine option "bce_inner_eps").
    Sparse ``y_true`` (labels) is accepted as well as the dense one-hot the reference feeds it.  ``edge_weight``
    (``check_edge_weight``'s dict) multiplies each pixel's cross-entropy by its border weight, taken from the arg-max of a
    dense ``y_true``."""
    ew = _edge_weight_spec(edge_weight)
    dice_fn = dice_loss_micro(is_y_true_sparse=False, num_classes=num_classes, alpha=alpha, beta=beta,
                              tversky_gamma=tversky_gamma, dice_class_weight=dice_class_weight)
    e = FOCAL_EPS if bce_inner_eps else 0.0

    def _bce_dice_loss(y_true, y_pred):
        p = np.asarray(y_pred, np.float64)
        y = np.asarray(y_true)
        y = np.asarray(y, np.float64) if y.shape == p.shape else _one_hot(y, num_classes)
        pc = np.clip(p, FOCAL_EPS, 1.0 - FOCAL_EPS)
        qc = np.clip(1.0 - p, FOCAL_EPS, 1.0 - FOCAL_EPS)
        bce = -(y * np.log(pc + e) + (1.0 - y) * np.log(qc + e))
        if ew is not None:
            sparse = np.asarray(y_true) if np.asarray(y_true).shape != p.shape else np.argmax(y, axis=-1)
            bce = bce * np.asarray(_edge_weights(ew, sparse, num_classes))[..., None]
        return np.mean(bce) + dice_fn(y, p)

    _bce_dice_loss.oct_loss = "bce_dice_loss"
    _bce_dice_loss.oct_dice_shape = dice_fn.oct_dice_shape
    _bce_dice_loss.oct_edge_weight = ew
    return _bce_dice_loss


def masked_loss_reference(labels, probs, num_classes: int, ignore, kind: str = "dice", *, smooth: float = 1e-05,
                          gamma: float = 2.0, class_weight=None, focal_loss_weight: float = 0.5, bce_inner_eps: bool = True,
                          pixel_weight=None) -> dict:
    """The losses above and the two Dice metrics with an ignore label, as the engine defines them
    (``oct_unet_set_ignore_label``): sparse ``labels`` (B,H,W[,1]), ``probs`` (B,H,W,C), fp64.  A pixel whose label equals
    ``ignore`` (``None``: no such pixel) is dropped from every sum -- its one-hot row AND its probabilities -- and the focal
    / BCE mean divides by the number of counted pixels of the batch (times C for BCE), 0 where there is none.
    ``kind``: ``"dice"``, ``"focal"`` or ``"bce"``.  Returns a dict of ``dice_loss_macro``, ``dice_loss_micro``,
    ``dice_coef_macro``, ``dice_coef_micro``, ``term`` (the focal or BCE mean; 0 for ``"dice"``) and the combined
    ``loss_macro`` / ``loss_micro``: ``w term + (1 - w) dice`` for focal, ``term + dice_loss_micro`` for BCE (whose
    ``loss_macro`` is ``None``: the reference defines that loss with the micro Dice only), the Dice losses themselves for
    ``"dice"``.  ``pixel_weight`` (B,H,W), e.g. ``edge_weight_reference``'s map, multiplies each counted pixel's focal / BCE
    term (``oct_unet_set_pixel_weights``); the divisor stays the count, and the Dice sums and metrics never see it.
    A batch without a counted pixel has ``dice_coef_micro = 0/0 = nan``, as the reference's formula gives."""
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
    pw = None if pixel_weight is None else np.asarray(pixel_weight, np.float64).reshape(lab.shape)
    if kind == "focal":
        py = np.clip(np.take_along_axis(p, safe[..., None], axis=-1)[..., 0], FOCAL_EPS, 1.0 - FOCAL_EPS)
        cw = 1.0 if class_weight is None else np.asarray(class_weight, np.float64)[safe]
        px = cw * (1.0 - py) ** gamma * -np.log(py)
        px = px if pw is None else pw * px
        term, w = float(np.sum(px[m]) * inv), float(focal_loss_weight)
        out.update(term=term, loss_macro=w * term + (1.0 - w) * out["dice_loss_macro"],
                   loss_micro=w * term + (1.0 - w) * out["dice_loss_micro"])
    elif kind == "bce":
        e = FOCAL_EPS if bce_inner_eps else 0.0
        pc, qc = np.clip(p, FOCAL_EPS, 1.0 - FOCAL_EPS), np.clip(1.0 - p, FOCAL_EPS, 1.0 - FOCAL_EPS)
        px = -(y * np.log(pc + e) + (1.0 - y) * np.log(qc + e))
        px = px if pw is None else pw[..., None] * px
        term = float(np.sum(px[m]) * inv / num_classes)
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
