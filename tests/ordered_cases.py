"""Inputs shared by the CPU and GPU tests of the ordered layer decode: the shapes at which the kernel
is held against ``ordered_decode_reference``, the three kinds of probabilities per shape, and the brute-force enumeration the
restatement itself is held against."""
import itertools

import numpy as np

ONE = 1 << 20

# (B, H, W, C): a single pixel; smaller than a float4 item; W past one wave, neither % 4 nor % 64, odd H; float4 path with a
# partial last item (130 % 4 == 2); float4 path at its widest class count with W % 4 == 1; the scalar path above 8 classes
SHAPES = [(1, 1, 1, 2), (2, 5, 3, 3), (3, 17, 70, 3), (2, 33, 130, 4), (1, 64, 65, 8), (2, 9, 67, 9), (1, 12, 64, 16)]
TOP_SHAPE = (1, 4096, 8, 2)          # class 1 at exactly 1.0 everywhere: score 4096 * (2^20 - 1), the top of the uint32 range
KINDS = ("random", "onehot", "equal")


def make(shape, kind: str, seed: int = 0) -> np.ndarray:
    """(B,H,W,C) float32: ``random`` Dirichlet rows, ``onehot`` a random class at 1.0 per pixel (out of depth order: the decode
    has to repair it), ``equal`` 1/C everywhere (every labelling ties)."""
    B, H, W, C = shape
    rng = np.random.default_rng(seed + 1000 * C + H)
    if kind == "random":
        return rng.dirichlet(np.ones(C), size=(B, H, W)).astype(np.float32)
    if kind == "onehot":
        return np.eye(C, dtype=np.float32)[rng.integers(0, C, size=(B, H, W))]
    if kind == "equal":
        return np.full(shape, 1.0 / C, np.float32)
    raise ValueError(kind)


def quantise(p: np.ndarray) -> np.ndarray:
    """The definition's k, written independently of the restatement (per element, in Python numbers)."""
    out = np.empty(p.shape, np.int64)
    for i, v in np.ndenumerate(np.asarray(p, np.float32)):
        q = min(float(v), 1.0) if v > 0 else 0.0                 # NaN > 0 is False
        out[i] = min(int(np.floor(q * ONE)), ONE - 1)
    return out


def brute_force(col: np.ndarray):
    """One column (H, C) -> (best score, the optimal labelling that is smallest when compared from the bottom row upward),
    by enumeration of every non-decreasing labelling."""
    k = quantise(col)
    H, C = k.shape
    best = None
    for lab in itertools.combinations_with_replacement(range(C), H):          # exactly the non-decreasing sequences
        s = sum(int(k[r, lab[r]]) for r in range(H))
        key = (-s, tuple(reversed(lab)))
        if best is None or key < best[0]:
            best = (key, s, lab)
    return best[1], np.array(best[2], np.uint8)


def ordered_onehot(shape, seed: int = 0):
    """One-hot probabilities whose arg-max is already ordered -- class 0 on top of every column; a class may be absent where
    two cuts coincide -- and that arg-max."""
    B, H, W, C = shape
    rng = np.random.default_rng(seed)
    cuts = np.sort(rng.integers(1, H, size=(B, W, C - 1)), axis=-1)            # rows >= 1: class 0 is never empty
    r = np.arange(H)[None, :, None, None]
    labels = (r >= cuts[:, None]).sum(axis=-1).astype(np.uint8)                # (B,H,W)
    return np.eye(C, dtype=np.float32)[labels], labels
