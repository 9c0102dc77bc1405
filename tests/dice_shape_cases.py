"""The shaped Dice term written out in torch for autograd, and the shapes the tests walk.  Shared by
tests/test_dice_shape.py (CPU) and tests/test_gpu_dice_shape.py."""
import numpy as np
import torch

CLAMP = 1e-7

# name -> keywords of UNetEngine.set_dice_shape / shaped_dice_reference, for 3 classes
SHAPES = {
    "tversky": dict(alpha=0.3, beta=0.7),
    "focal_tversky_075": dict(alpha=0.3, beta=0.7, gamma=0.75),
    "focal_tversky_2": dict(alpha=0.3, beta=0.7, gamma=2.0),
    "weights_with_zero": dict(class_weight=(0.5, 2.0, 0.0)),
    "volume": dict(class_weight="volume"),
}


def volume_weights_t(T):
    """1 / T^2 along the last axis; T = 0 takes the row's largest weight, a row of zeros all ones (no gradient: labels only)."""
    T = T.detach()
    w = torch.where(T > 0, 1.0 / torch.clamp(T, min=1e-300) ** 2, torch.zeros_like(T))
    wmax = w.max(dim=-1, keepdim=True).values
    return torch.where(wmax == 0, torch.ones_like(w), torch.where(T > 0, w, wmax.expand_as(w)))


def shaped_dice_t(probs, labels, C, macro, *, alpha=0.5, beta=0.5, gamma=1.0, class_weight=None, ignore=None, smooth=1e-5):
    """The definition, differentiable in ``probs`` (B,H,W,C) fp64; ``labels`` (B,H,W[,1]) integers."""
    lab = torch.as_tensor(np.asarray(labels).reshape(probs.shape[:3]).astype(np.int64))
    keep = torch.ones_like(lab, dtype=torch.bool) if ignore is None else lab != ignore
    m = keep.to(torch.float64)
    y = torch.nn.functional.one_hot(torch.where(keep, lab, torch.zeros_like(lab)), C).to(torch.float64) * m[..., None]
    pm = probs * m[..., None]
    I, T, P = (y * pm).sum(dim=(1, 2)), y.sum(dim=(1, 2)), pm.sum(dim=(1, 2))

    def term(I, T, P):
        N = 2.0 * I + smooth
        D = 2.0 * I + 2.0 * alpha * (P - I) + 2.0 * beta * (T - I) + smooth
        u = 1.0 - N / D
        return u if gamma == 1.0 else torch.clamp(u, min=CLAMP) ** gamma

    if class_weight is None:
        w_bc, w_c = torch.ones_like(T), torch.ones(C, dtype=torch.float64)
    elif isinstance(class_weight, str):
        assert class_weight == "volume"
        w_bc, w_c = volume_weights_t(T), volume_weights_t(T.sum(dim=0))
    else:
        w_c = torch.tensor(np.asarray(class_weight, np.float64))
        w_bc = w_c.expand_as(T)
    if macro:
        return ((w_bc * term(I, T, P)).sum(dim=1) / w_bc.sum(dim=1)).mean()
    return term((w_c * I).sum(), (w_c * T).sum(), (w_c * P).sum())


def drop_class_from_image(labels, b, c, to):
    """``labels`` with class ``c`` of image ``b`` relabelled ``to``: the class is absent from that image only."""
    lab = labels.copy()
    img = lab[b]
    img[img == c] = to
    return lab
