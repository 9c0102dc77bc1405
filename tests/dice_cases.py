"""Inputs shared by tests/test_dice_device.py (CPU) and tests/test_gpu_dice_device.py: delineation families for the
area-label closed form and class-map pairs for the confusion counts."""
import numpy as np

from oracle import unet_numpy as on

SEG_FAMILIES = ("monotone", "crossing", "zeros40", "zero_column", "last_zero", "beyond")


def seg_family(kind: str, n: int, H: int, W: int, C: int, seed: int) -> np.ndarray:
    """(n, C-1, W) uint16 delineations of one family."""
    rng = np.random.default_rng(seed)
    M = C - 1
    monotone = np.sort(rng.integers(1, H, (n, M, W)), axis=1).astype(np.uint16)
    if kind == "monotone":
        return monotone
    crossing = rng.integers(0, H + 1, (n, M, W)).astype(np.uint16)            # uniform in 0..H: crossings, zeros and H
    if kind == "crossing":
        return crossing
    if kind == "zeros40":
        s = crossing.copy()
        s[rng.random(s.shape) < 0.4] = 0
        return s
    if kind == "zero_column":
        s = monotone.copy()
        s[:, :, 0] = 0
        s[:, :, W // 2] = 0
        s[:, :, W - 1] = 0
        return s
    if kind == "last_zero":
        s = crossing.copy()
        s[:, M - 1, :] = 0
        return s
    if kind == "beyond":
        s = crossing.copy()
        m = rng.random(s.shape)
        s[m < 0.15] = H + 5
        s[(m >= 0.15) & (m < 0.3)] = 65535
        s[(m >= 0.3) & (m < 0.4)] = H + rng.integers(0, 6)
        return s
    raise ValueError(kind)


def host_area_labels(segs: np.ndarray, H: int, W: int) -> np.ndarray:
    """``labels_from_delineations`` per image, (n,H,W) uint8."""
    from oct_image_segmentation_models_amd.common.utils import labels_from_delineations
    C = segs.shape[1] + 1
    return np.stack([labels_from_delineations((W, H, 1), s, C)[0] for s in segs]).astype(np.uint8)


def map_pairs(B: int, H: int, W: int, C: int, seed: int) -> dict:
    """name -> (pred, gt), (B,H,W) uint8 each: synthetic scans' labels against a shifted copy, uniform random maps, and
    both maps constant (every lane of a wave on one counter)."""
    _, lab = on.synth_scans(B, H, W, C, seed=seed)
    gt = np.ascontiguousarray(lab[..., 0].astype(np.uint8))
    rng = np.random.default_rng(seed)
    return {"shifted": (np.ascontiguousarray(np.roll(gt, 2, axis=1)), gt),
            "random": (rng.integers(0, C, gt.shape).astype(np.uint8), rng.integers(0, C, gt.shape).astype(np.uint8)),
            "constant": (np.full(gt.shape, C - 1, np.uint8), np.full(gt.shape, 1, np.uint8))}
