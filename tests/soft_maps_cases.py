"""Inputs shared by tests/test_soft_maps.py (CPU) and tests/test_gpu_soft_maps.py: the four families of (n,H,W,C) float32
class probabilities the soft boundary maps are checked on, and the pre-cast values behind the wrap assertion."""
import numpy as np

FAMILIES = ("saturated", "layered", "onehot", "constant")
BG = [(True, False), (False, False), (True, True), (False, True)]          # (bg_ilm, bg_csi)


def softmax32(logits):
    z = logits.astype(np.float32)
    e = np.exp(z - z.max(axis=-1, keepdims=True))
    return (e / e.sum(axis=-1, keepdims=True)).astype(np.float32)


def layered_probs(n, H, W, C, seed, width=1.5):
    """What a trained net emits: C stacked layers, a sigmoid ramp of ``width`` rows across each of the C-1 boundaries,
    which wander from column to column.  Rows sum to 1 up to rounding; class 0 is on top."""
    rng = np.random.default_rng(seed)
    base = (np.arange(1, C, dtype=np.float64) * H / C)[None, :, None]                       # (1, C-1, 1)
    walk = np.cumsum(rng.normal(0.0, 0.35, (n, C - 1, W)), axis=2)
    bnd = np.sort(base + walk, axis=1)                                                      # ordered boundaries: probabilities >= 0
    r = np.arange(H, dtype=np.float64)[None, None, :, None]
    s = 1.0 / (1.0 + np.exp(-(r - bnd[:, :, None, :]) / width))                              # (n, C-1, H, W): below boundary k
    below = np.concatenate([np.ones((n, 1, H, W)), s, np.zeros((n, 1, H, W))], axis=1)
    p = below[:, :-1] - below[:, 1:]                                                        # (n, C, H, W)
    return np.ascontiguousarray(np.transpose(p, (0, 2, 3, 1)).astype(np.float32))


def family(name, shape, seed=0):
    n, H, W, C = shape
    rng = np.random.default_rng([seed, n, H, W, C])
    if name == "saturated":           # softmax of N(0, 4^2) logits: many pixels at 0 / 1, rows 0 and H-1 reach the wrap
        return softmax32(rng.normal(0.0, 4.0, shape))
    if name == "layered":
        return layered_probs(n, H, W, C, seed + 1)
    if name == "onehot":
        return np.ascontiguousarray(np.eye(C, dtype=np.float32)[rng.integers(0, C, (n, H, W))])
    if name == "constant":
        return np.full(shape, np.float32(1.0 / C), np.float32)
    raise KeyError(name)


def class_map(shape, seed=0):
    """The class map behind ``family("onehot", shape, seed)``."""
    return family("onehot", shape, seed).argmax(-1).astype(np.uint8)


def scaled_values(probs, bg_ilm, bg_csi):
    """v * 255 of the definition, before the cast to uint8, as float32 (n, C-1, H, W); H >= 2."""
    n, H, W, C = probs.shape
    out = np.zeros((n, C - 1, H, W), np.float32)
    for m in range(1, C):
        flip = (m == 1 and bg_ilm) or (m == C - 1 and bg_csi)
        d = np.gradient(probs[..., m - 1 if flip else m], axis=1)
        g = np.float32(2) * np.maximum(-d if flip else d, np.float32(0))
        out[:, m - 1] = np.maximum(g - np.roll(g, -1, axis=1), np.float32(0)) * np.float32(255)
    return out
