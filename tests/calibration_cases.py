"""Shared inputs and tolerances of the calibration tests (tests/test_calibration.py on the host, tests/test_gpu_calibration.py on
the device).  Nothing here touches a GPU."""
import numpy as np

# (B,H,W,C): vector items with tails, npix*C no multiple of 4, C above the vector path, one pixel rows
SHAPES = [(3, 5, 7, 2), (2, 8, 16, 3), (1, 16, 36, 4), (2, 9, 13, 12), (1, 3, 1031, 16), (2, 1, 8, 9), (3, 20, 34, 3), (1, 5, 7, 32)]
BINS = (1, 10, 15, 64)
BETAS = (1.0 / 16.0, 0.25, 0.5, 2.0, 4.0, 16.0)
BETAS8 = (1.0 / 16.0, 0.25, 0.5, 1.0, 1.5, 2.0, 4.0, 16.0)
# the fit: softmax of N(0, s^2) logits with labels drawn at a true temperature T
FITS = [(3.0, 2.0), (1.0, 0.5), (4.0, 3.0), (6.0, 8.0), (0.3, 0.2)]
FIT_SHAPE = (3, 20, 34, 3)


def make(shape, s: float = 2.0, T: float = 1.0, seed: int = 0):
    """``probs`` (B,H,W,C) float32 = softmax of N(0, s^2) logits and ``labels`` (B,H,W) uint8 drawn from softmax(logits / T):
    the temperature that calibrates ``probs`` is T."""
    rng = np.random.default_rng(seed)
    z = rng.normal(0.0, s, shape)
    def softmax(a):
        e = np.exp(a - a.max(-1, keepdims=True))
        return e / e.sum(-1, keepdims=True)
    p, pt = softmax(z), softmax(z / T)
    u = rng.random(shape[:-1] + (1,))
    labels = (pt.cumsum(-1) < u).sum(-1).clip(0, shape[-1] - 1).astype(np.uint8)
    return p.astype(np.float32), labels


def salted(shape, n_bins: int, seed: int = 0):
    """``make`` with pixels overwritten by the cases an implementation can get wrong: a confidence exactly on every bin edge
    k / M that float32 holds exactly enough to land in bin k, confidence 1.0, arg-max ties (two and all classes), an exact 0."""
    p, y = make(shape, 2.0, 1.0, seed)
    B, H, W, C = shape
    flat = p.reshape(-1, C)
    rows = []
    for k in range(1, n_bins + 1):
        conf = np.float32(k) / np.float32(n_bins)
        if conf * C < 1:
            continue                                     # no distribution over C classes has so small a maximum
        rest = (np.float32(1) - conf) / np.float32(C - 1)
        if rest > conf:
            continue
        r = np.full(C, rest, np.float32); r[k % C] = conf
        rows.append(r)
    one = np.zeros(C, np.float32); one[C - 1] = 1.0
    tie2 = np.zeros(C, np.float32); tie2[0] = tie2[C - 1] = 0.5
    rows += [one, tie2, np.full(C, np.float32(1) / np.float32(C), np.float32)]
    rng = np.random.default_rng(seed + 1)
    at = rng.choice(flat.shape[0], size=min(len(rows), flat.shape[0]), replace=False)
    for i, r in zip(at, rows):
        flat[i] = r
    return flat.reshape(shape), y


def with_ignore(labels, num_classes: int, ignore_label: int, seed: int = 0, empty_image=None):
    """``labels`` with about a third of the pixels set to ``ignore_label``; image ``empty_image`` gets no counted pixel."""
    rng = np.random.default_rng(seed + 7)
    y = labels.copy()
    y[rng.random(y.shape) < 0.33] = ignore_label
    if empty_image is not None:
        y[empty_image] = ignore_label
    return y


def sum_tolerance(term32, term64, axis=-1):
    """The bound of the issue for a per-image sum over pixels: 4 x sum |term32 - term64| + 2^-24 x sum |term64| (the L1 form:
    cancellation in the yardstick cannot tighten it).  The factor 4: OCML and the host libm differ by an ulp or two a call."""
    t32, t64 = np.asarray(term32, np.float64), np.asarray(term64, np.float64)
    return 4.0 * np.abs(t32 - t64).sum(axis=axis) + 2.0 ** -24 * np.abs(t64).sum(axis=axis)


def apply_tolerance(q32, q64) -> float:
    """The bound of the issue per element of ``temperature_apply``: 4 x max |q32 - q64| over the case + 2^-23."""
    return 4.0 * float(np.abs(np.asarray(q32, np.float64) - np.asarray(q64, np.float64)).max()) + 2.0 ** -23


PROB_BUDGET = 1e-4          # the project's budget for a class probability (README)
