"""Metric registry with the reference's names
(oct_image_segmentation_models/common/custom_metrics.py:18-100).  The training-monitor Dice coefficients are
computed on the device by the head kernel (selected through the ``oct_metric`` tag); the numpy bodies here
serve the evaluation code.  The surface-distance metrics (:103-119) are a numpy restatement of the un-vendored
google-deepmind/surface-distance package (2D path), PARITY UNPINNED against it; the evaluation computes them on the
device (``evaluation/surface.py``, csrc/kernels_surface.hpp), which is checked against the functions here."""
from __future__ import annotations

from typing import Tuple

import numpy as np

from . import TRAINING_MONITOR_METRIC_DICE_MACRO, TRAINING_MONITOR_METRIC_DICE_MICRO
from .custom_losses import _one_hot


def dice_coef_micro(is_y_true_sparse: bool, num_classes: int):
    def _dice_coef_micro(y_true, y_pred):
        if is_y_true_sparse:
            y_true = _one_hot(y_true, num_classes)
        y_true_f = np.asarray(y_true, np.float32).ravel()
        y_pred_f = (np.asarray(y_pred, np.float32).ravel() > 0.5).astype(np.float32)
        with np.errstate(invalid="ignore", divide="ignore"):   # no epsilon in the reference: 0/0 -> nan
            return np.float32(2.0) * np.sum(y_true_f * y_pred_f) / (np.sum(y_true_f) + np.sum(y_pred_f))

    _dice_coef_micro.__name__ = "dice_coef_micro"
    _dice_coef_micro.oct_metric = "dice_coef_micro"
    return _dice_coef_micro


def dice_coef_macro(is_y_true_sparse: bool, num_classes: int):
    def _dice_coef_macro(y_true, y_pred, eps=1e-05):
        if is_y_true_sparse:
            y_true = _one_hot(y_true, num_classes)
        y_true = np.asarray(y_true, np.float32)
        y_pred = (np.asarray(y_pred) > 0.5).astype(np.float32)
        reduce_axis = tuple(range(1, y_pred.ndim - 1))
        intersection = np.sum(y_true * y_pred, axis=reduce_axis)
        denominator = np.sum(y_true, axis=reduce_axis) + np.sum(y_pred, axis=reduce_axis)
        return np.mean((2.0 * intersection + eps) / (denominator + eps))

    _dice_coef_macro.__name__ = "dice_coef_macro"
    _dice_coef_macro.oct_metric = "dice_coef_macro"
    return _dice_coef_macro


training_monitor_metric_objects = {
    TRAINING_MONITOR_METRIC_DICE_MACRO: dice_coef_macro,
    TRAINING_MONITOR_METRIC_DICE_MICRO: dice_coef_micro,
}


def soft_dice_class(y_true, y_pred, eps=1e-5):
    """(b, c, X, Y...) inputs -> per-class Dice (b, c)."""
    axes = tuple(range(2, len(y_pred.shape)))
    intersect = np.sum(y_pred * y_true, axis=axes)
    denom = np.sum(y_pred + y_true, axis=axes)
    return ((2.0 * intersect) + eps) / (denom + eps)


# ---- surface distances: restatement of google-deepmind/surface-distance (compute_surface_distances,
# compute_average_surface_distance, compute_robust_hausdorff; 2D), called by the reference at custom_metrics.py:103-119.
# PARITY UNPINNED: the package is not vendored.  numpy only (the package does not depend on scipy): the distance transform
# is an exact column pass + outward row search, the same one the device kernels run (csrc/kernels_surface.hpp).
#
# Cells: the (H+1) x (W+1) grid of 2x2 neighbourhoods of the zero-padded mask, code 8 m[i-1,j-1] + 4 m[i-1,j] +
# 2 m[i,j-1] + m[i,j] (= ndimage.correlate(mask, [[8,4],[2,1]], mode="constant")).  Border cells: code not 0 or 15.  The
# package crops to the bounding box of gt|pred first; distances are translation invariant and every border cell lies in
# that crop, so the full-frame grid gives the same surfels.  Contour length by kind: d = sqrt(v^2+h^2)/2, h, v, 2d.

_SURF_KIND = np.array([255, 0, 0, 1, 0, 2, 3, 0, 0, 3, 2, 0, 1, 0, 0, 255], np.uint8)   # code -> 0:d 1:h 2:v 3:2d


def _surfel_lengths(spacing) -> np.ndarray:
    v, h = float(spacing[0]), float(spacing[1])
    d = 0.5 * np.sqrt(np.float64(v) * np.float64(v) + np.float64(h) * np.float64(h))
    return np.array([d, h, v, 2.0 * d], np.float64)


def _cell_kinds(mask: np.ndarray) -> np.ndarray:
    m = np.pad(np.asarray(mask, bool).astype(np.uint8), 1)
    return _SURF_KIND[8 * m[:-1, :-1] + 4 * m[:-1, 1:] + 2 * m[1:, :-1] + m[1:, 1:]]


def _column_distances(border: np.ndarray) -> np.ndarray:
    """Rows to the nearest border cell in the same column (-1: none in that column)."""
    hc, wc = border.shape
    big = np.int64(1) << 40
    up = np.empty((hc, wc), np.int64)
    last = np.full(wc, -big, np.int64)
    for i in range(hc):
        last = np.where(border[i], i, last)
        up[i] = i - last
    nxt = np.full(wc, 2 * big, np.int64)
    for i in range(hc - 1, -1, -1):
        nxt = np.where(border[i], i, nxt)
        up[i] = np.minimum(up[i], nxt - i)
    up[up >= big] = -1
    return up


def _directed_distances(qi: np.ndarray, qj: np.ndarray, target_border: np.ndarray, spacing) -> np.ndarray:
    """Euclidean distance (physical units) of each query cell to the nearest border cell of ``target_border``:
    min over columns j' of (v dy[j'])^2 + (h (j - j'))^2, searched outward from the query's column until (h dx)^2 alone
    reaches the best value (exact minimum; +inf without target cells)."""
    v, h = np.float64(spacing[0]), np.float64(spacing[1])
    best = np.full(qi.shape, np.inf)
    if qi.size == 0 or not target_border.any():
        return best
    dy = _column_distances(target_border)
    wc = target_border.shape[1]
    active = np.ones(qi.shape, bool)
    for s in range(wc):
        bx = h * np.float64(s)
        bb = bx * bx
        active &= bb < best
        if not active.any():
            break
        for jj in ((qj - s,) if s == 0 else (qj - s, qj + s)):
            sel = np.nonzero(active & (jj >= 0) & (jj < wc))[0]
            u = dy[qi[sel], jj[sel]]
            ok = u >= 0
            sel, a = sel[ok], v * u[ok].astype(np.float64)
            best[sel] = np.minimum(best[sel], a * a + bb)
    return np.sqrt(best)


def _known_cells(valid: np.ndarray) -> np.ndarray:
    """(H, W) validity of the pixels -> (H+1, W+1) bool: the cells none of whose in-image pixels is invalid (the zero
    padding outside the image is known background)."""
    u = np.pad(~np.asarray(valid, bool), 1)
    return ~(u[:-1, :-1] | u[:-1, 1:] | u[1:, :-1] | u[1:, 1:])


def compute_surface_distances(mask_gt: np.ndarray, mask_pred: np.ndarray, spacing, valid=None) -> dict:
    """Surfels of both masks with their distance to the other surface and contour length, sorted by
    (distance, length) as the package sorts them (``sorted(zip(...))``).  Besides the package's four keys the result
    holds ``surfel_kinds_gt`` / ``surfel_kinds_pred`` (0: d, 1: h, 2: v, 3: 2d) for the exact percentile.

    ``valid`` (extension, ``oct_surface_distances_masked``): an (H, W) bool array, False where the ground truth is unknown.
    A cell is then a surfel only if none of its in-image pixels is unknown, in both masks alike: surfaces are those seen
    entirely inside the labelled region, and the rim of an unknown region is never one.  Everything else is unchanged."""
    mask_gt, mask_pred = np.asarray(mask_gt, bool), np.asarray(mask_pred, bool)
    if mask_gt.ndim != 2 or mask_gt.shape != mask_pred.shape:
        raise ValueError("compute_surface_distances: two 2D masks of one shape")
    lengths = _surfel_lengths(spacing)
    kg, kp = _cell_kinds(mask_gt), _cell_kinds(mask_pred)
    if valid is not None:
        valid = np.asarray(valid, bool)
        if valid.shape != mask_gt.shape:
            raise ValueError("compute_surface_distances: valid must have the masks' shape")
        unknown = ~_known_cells(valid)
        kg, kp = np.where(unknown, np.uint8(255), kg), np.where(unknown, np.uint8(255), kp)
    bg, bp = kg != 255, kp != 255
    out = {}
    for name, kinds, border, other in (("gt", kg, bg, bp), ("pred", kp, bp, bg)):
        qi, qj = np.nonzero(border)
        dist = _directed_distances(qi, qj, other, spacing)
        k = kinds[qi, qj]
        area = lengths[k]
        order = np.lexsort((area, dist))
        key = "distances_gt_to_pred" if name == "gt" else "distances_pred_to_gt"
        out[key], out[f"surfel_areas_{name}"], out[f"surfel_kinds_{name}"] = dist[order], area[order], k[order]
    out["surfel_lengths"] = lengths
    return out


def _weighted_length(counts: np.ndarray, lengths: np.ndarray) -> np.ndarray:
    """Contour length of per-kind surfel counts (..., 4): the one expression the device evaluates too."""
    c = counts.astype(np.float64)
    return ((c[..., 0] * lengths[0] + c[..., 1] * lengths[1]) + c[..., 2] * lengths[2]) + c[..., 3] * lengths[3]


def compute_average_surface_distance(surface_distances: dict):
    with np.errstate(invalid="ignore", divide="ignore"):
        res = []
        for d, a in ((surface_distances["distances_gt_to_pred"], surface_distances["surfel_areas_gt"]),
                     (surface_distances["distances_pred_to_gt"], surface_distances["surfel_areas_pred"])):
            res.append(np.sum(d * a) / np.sum(a))
    return tuple(res)


def _robust_percentile(dist: np.ndarray, kinds: np.ndarray, lengths: np.ndarray, percent: float) -> float:
    if dist.size == 0:
        return np.inf
    counts = np.cumsum(np.eye(4, dtype=np.int64)[kinds], axis=0)          # exact per-kind running counts
    cum = _weighted_length(counts, lengths)
    idx = int(np.searchsorted(cum / cum[-1], percent / 100.0))
    return float(dist[min(idx, dist.size - 1)])


def compute_robust_hausdorff(surface_distances: dict, percent: float) -> float:
    """max over both directions of the length-weighted ``percent`` percentile: searchsorted(cumsum(len) / sum(len),
    percent / 100), the cumulative length taken from per-kind integer counts (exact, order-independent within a group of
    equal distances)."""
    lengths = surface_distances["surfel_lengths"]
    a = _robust_percentile(surface_distances["distances_gt_to_pred"], surface_distances["surfel_kinds_gt"], lengths, percent)
    b = _robust_percentile(surface_distances["distances_pred_to_gt"], surface_distances["surfel_kinds_pred"], lengths, percent)
    return max(a, b)


def average_surface_distance(y_true: np.ndarray, y_pred: np.ndarray, spacing: Tuple[float, float]) -> Tuple[float, float]:
    """(gt_to_pred, pred_to_gt) average surface distance of two 2D boolean masks (custom_metrics.py:103-109)."""
    return compute_average_surface_distance(compute_surface_distances(y_true, y_pred, spacing))


def hausdorff_distance(y_true: np.ndarray, y_pred: np.ndarray, spacing: Tuple[float, float], percent: float) -> float:
    """Robust Hausdorff distance at ``percent`` of two 2D boolean masks (custom_metrics.py:112-119)."""
    if not 0.0 <= percent <= 100.0:
        raise ValueError("percent must lie in [0, 100]")
    return compute_robust_hausdorff(compute_surface_distances(y_true, y_pred, spacing), percent)
