"""The evaluation's Dice metrics and graph-search class maps from the device.

Every Dice metric ``evaluate_model`` writes (``dice_coef_classes`` / ``_macro`` / ``_micro``, reference
evaluation/evaluation.py:175-208 and :335-375) is a function of the per-image confusion matrix ``n[g][p]`` -- the number
of pixels with ground truth ``g`` and prediction ``p`` -- and the class map that graph-search delineations enclose
(``common.utils.labels_from_delineations``) has a closed form per pixel.  ``ConfusionCounts`` and ``AreaLabels`` run the
two kernels (``oct_confusion_counts`` / ``oct_area_labels``, include/oct_unet.h) on the current stream;
``confusion_counts_reference`` and ``area_labels_reference`` are the numpy restatements they are tested against, and
``dice_from_counts`` turns one matrix into exactly what ``evaluation._dice_metrics`` returns for the image."""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch

from .. import _hip
from ..common import (EVALUATION_METRIC_DICE_CLASSES, EVALUATION_METRIC_DICE_MACRO, EVALUATION_METRIC_DICE_MICRO)

DICE_METRICS = (EVALUATION_METRIC_DICE_CLASSES, EVALUATION_METRIC_DICE_MACRO, EVALUATION_METRIC_DICE_MICRO)
MAX_CLASSES = 32
# The host sums one-hot float32 arrays: such a sum is exact while it stays <= 2^24.  soft_dice_class sums pred + true
# elementwise, up to 2 H W per class, so the host's own values are order-independent (and dice_from_counts equals them bit
# for bit) while H * W <= 2^23; above that the workflows keep the host path.
MAX_EXACT_PIXELS = 1 << 23


def check_ignore_label(ignore_label, num_classes: int) -> Optional[int]:
    """The public ``ignore_label`` of the evaluation, validated: None, or an int in ``num_classes..255`` (a ground-truth
    value that is no class).  Anything else is a ``ValueError``."""
    if ignore_label is None:
        return None
    if isinstance(ignore_label, (bool, np.bool_)) or not isinstance(ignore_label, (int, np.integer)) \
            or not int(num_classes) <= int(ignore_label) <= 255:
        raise ValueError(f"ignore_label must be None or an int in {int(num_classes)}..255, not {ignore_label!r}")
    return int(ignore_label)


def confusion_counts_reference(pred: np.ndarray, gt: np.ndarray, num_classes: int,
                               ignore_label: Optional[int] = None) -> np.ndarray:
    """(n,H,W) class maps -> (n, C*C + 1) uint32: word ``g*C + p`` counts the pixels with gt == g and pred == p, the last
    word those where either label is >= C (they appear nowhere else in the row).

    With ``ignore_label`` (``oct_confusion_counts_masked``) the rows have C*C + 2 words: a pixel with gt == ignore_label is
    counted in word C*C + 1 and nowhere else, whatever its prediction; the words before it are as above, over the other
    (the counted) pixels."""
    pred, gt, Cc = np.asarray(pred).astype(np.int64), np.asarray(gt).astype(np.int64), int(num_classes)
    if pred.shape != gt.shape or pred.ndim != 3:
        raise ValueError("pred and gt must be (n,H,W) class maps of one shape")
    ignore_label = check_ignore_label(ignore_label, Cc)
    bad = (pred < 0) | (pred >= Cc) | (gt < 0) | (gt >= Cc)
    key = np.where(bad, Cc * Cc, gt * Cc + pred)
    nk = Cc * Cc + 1
    if ignore_label is not None:
        key, nk = np.where(gt == ignore_label, Cc * Cc + 1, key), Cc * Cc + 2
    key = key.reshape(pred.shape[0], -1)
    return np.stack([np.bincount(k, minlength=nk) for k in key]).astype(np.uint32)


def area_labels_reference(segs: np.ndarray, H: int, W: int) -> np.ndarray:
    """Delineations (n, M, W) or (M, W) -> the class maps (n,H,W) / (H,W) uint8 that ``labels_from_delineations`` gives,
    in the (H,W) frame.  Per column: going up in i, a zero s_i becomes the first non-zero s_j with j > i, or H; row r gets
    M if r >= s_{M-1}, else the largest k in 1..M-1 with s_{k-1} <= r < s_k (the host loop's sequential overwrites), else 0."""
    s = np.asarray(segs).astype(np.int64)
    single = s.ndim == 2
    if single:
        s = s[None]
    n, M = s.shape[:2]
    if s.shape[2] != W:
        raise ValueError(f"segs must have {W} columns")
    nxt = np.full((n, W), H, np.int64)
    for i in range(M - 1, -1, -1):
        nxt = np.where(s[:, i] == 0, nxt, s[:, i])
        s[:, i] = nxt
    r = np.arange(H, dtype=np.int64)[None, :, None]
    lab = np.zeros((n, H, W), np.uint8)
    for k in range(1, M):
        lab[(s[:, k - 1, None, :] <= r) & (r < s[:, k, None, :])] = k
    lab[r >= s[:, M - 1, None, :]] = M
    return lab[0] if single else lab


def counts_matrix(rows: np.ndarray, num_classes: int, first_image: int = 0, ignored: bool = False) -> np.ndarray:
    """(n, C*C + 1) rows of the device -> (n, C, C) uint32; a non-zero out-of-range word raises with the image index.
    ``ignored``: the rows are the masked kernel's, C*C + 2 words; the count of ignored pixels is dropped."""
    rows = np.asarray(rows).view(np.uint32) if np.asarray(rows).dtype == np.int32 else np.asarray(rows, np.uint32)
    Cc = int(num_classes)
    if rows.ndim != 2 or rows.shape[1] != Cc * Cc + (2 if ignored else 1):
        raise ValueError(f"rows of {Cc * Cc + (2 if ignored else 1)} words expected, not an array of shape {rows.shape}")
    bad = np.nonzero(rows[:, Cc * Cc])[0]
    if bad.size:
        i = int(bad[0])
        raise ValueError(f"image {first_image + i}: {int(rows[i, Cc * Cc])} pixels carry a label outside 0..{Cc - 1}")
    return rows[:, :Cc * Cc].reshape(-1, Cc, Cc).copy()


def dice_from_counts(counts: np.ndarray, metrics) -> Tuple[Optional[np.ndarray], Optional[np.ndarray], Optional[np.ndarray]]:
    """One image's confusion matrix (C, C) (rows: ground truth, columns: prediction) -> (dice_classes (1, C) float32,
    dice_macro, dice_micro 0-d float32; None for a metric not in ``metrics``): the values, dtypes and shapes of
    ``evaluation._dice_metrics`` for that image, in its plain and its transposed form alike.  The host works in float32 on
    one-hot arrays; its sums are the integers below (exact in float32 up to ``MAX_EXACT_PIXELS``), and the expressions
    that follow them are repeated here operation by operation."""
    n = np.asarray(counts).astype(np.int64)
    if n.ndim != 2 or n.shape[0] != n.shape[1]:
        raise ValueError("counts must be one (C, C) confusion matrix")
    inter = np.diagonal(n).astype(np.float32)[None, :]                 # sum(true * pred) per class
    true, pred = n.sum(axis=1).astype(np.float32)[None, :], n.sum(axis=0).astype(np.float32)[None, :]
    dc = dm = dmi = None
    if EVALUATION_METRIC_DICE_CLASSES in metrics:                      # custom_metrics.soft_dice_class
        dc = ((2.0 * inter) + 1e-5) / ((pred + true) + 1e-5)
    if EVALUATION_METRIC_DICE_MACRO in metrics:                        # custom_metrics.dice_coef_macro
        dm = np.array(np.mean((2.0 * inter + 1e-05) / ((true + pred) + 1e-05)))
    if EVALUATION_METRIC_DICE_MICRO in metrics:                        # custom_metrics.dice_coef_micro
        total = np.float32(n.sum())
        with np.errstate(invalid="ignore", divide="ignore"):
            dmi = np.array(np.float32(2.0) * np.float32(np.trace(n)) / (total + total))
    return dc, dm, dmi


class ConfusionCounts:
    """``oct_confusion_counts`` for up to ``batch`` images of one shape: ``(pred, gt)`` -> (n, C*C + 1) int32 rows on the
    device (the bits are the uint32 counts), queued on the current stream.  With ``ignore_label`` it is
    ``oct_confusion_counts_masked``: rows of C*C + 2 words, ground-truth pixels of that value counted in the last alone."""

    def __init__(self, batch: int, H: int, W: int, num_classes: int, device, ignore_label: Optional[int] = None):
        self.B, self.H, self.W, self.C = int(batch), int(H), int(W), int(num_classes)
        self.ignore_label = check_ignore_label(ignore_label, self.C)
        if not (1 <= self.B <= 65535 and self.H >= 1 and self.W >= 1 and self.H * self.W < 1 << 32
                and 2 <= self.C <= MAX_CLASSES):
            raise _hip.OctError(f"oct_confusion_counts does not support B={batch}, {H}x{W}, {num_classes} classes")
        self.device = torch.device(device)
        self.out = torch.empty((self.B, self.C * self.C + (1 if self.ignore_label is None else 2)), dtype=torch.int32,
                               device=self.device)
        self.outs, self.geometry = (self.out,), (self.B, self.H, self.W, self.C)

    def __call__(self, pred: torch.Tensor, gt: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        n = _hip.expect_map_pair(pred, gt, device=self.device, batch=self.B, H=self.H, W=self.W)
        out = _hip.out_view(out, self.out, n)
        if self.ignore_label is None:
            _hip.call("oct_confusion_counts", self.device, pred.data_ptr(), gt.data_ptr(), n, self.H, self.W, self.C,
                      out.data_ptr(), _hip.stream_ptr(self.device))
        else:
            _hip.call("oct_confusion_counts_masked", self.device, pred.data_ptr(), gt.data_ptr(), n, self.H, self.W, self.C,
                      self.ignore_label, out.data_ptr(), _hip.stream_ptr(self.device))
        return out

    def to_host(self, rows: torch.Tensor, first_image: int = 0) -> np.ndarray:
        """Device rows -> (n, C, C) uint32 on the host (waits for the stream); out-of-range labels raise."""
        return counts_matrix(rows.cpu().numpy(), self.C, first_image, ignored=self.ignore_label is not None)


class AreaLabels:
    """``oct_area_labels`` for up to ``batch`` images: delineations (n, C-1, W) int16 / uint16 on the device (the bits
    are uint16 rows, as the searches emit them) -> (n,H,W) uint8 class maps on the device, queued on the current stream."""

    def __init__(self, batch: int, H: int, W: int, num_classes: int, device):
        self.B, self.H, self.W, self.C = int(batch), int(H), int(W), int(num_classes)
        if not (1 <= self.B <= 65535 and 1 <= self.H <= 65535 and self.W >= 1 and self.H * self.W < 1 << 32
                and 2 <= self.C <= MAX_CLASSES):
            raise _hip.OctError(f"oct_area_labels does not support B={batch}, {H}x{W}, {num_classes} classes")
        self.device = torch.device(device)
        self.out = torch.empty((self.B, self.H, self.W), dtype=torch.uint8, device=self.device)

    def __call__(self, segs: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        _hip.expect(segs, "segs", device=self.device, dtype=(torch.int16, torch.uint16), shape=(None, self.C - 1, self.W))
        n = segs.shape[0]
        if not 1 <= n <= self.B:
            raise _hip.OctError(f"segs needs a count n in 1..{self.B}")
        out = _hip.out_view(out, self.out, n)
        _hip.call("oct_area_labels", self.device, segs.data_ptr(), n, self.H, self.W, self.C, out.data_ptr(),
                  _hip.stream_ptr(self.device))
        return out


class DelineationLabels:
    """The stage behind ``InferenceRun.gs_labels``: a batch's final delineations (n, C-1, W) uint16 on the host -> the
    class maps they enclose, (n,H,W) uint8 on the host, and with the batch's ground-truth class maps (n,H,W) the
    (n, C, C) uint32 confusion counts of those maps against it (else None).  It owns its device buffers and uploads
    both inputs itself; the call waits for the device.  ``ignore_label``: as ``ConfusionCounts``."""

    def __init__(self, batch: int, H: int, W: int, num_classes: int, device, ignore_label: Optional[int] = None):
        self.area = AreaLabels(batch, H, W, num_classes, device)
        self.counts = ConfusionCounts(batch, H, W, num_classes, device, ignore_label=ignore_label)

    def __call__(self, segs: np.ndarray, gt: Optional[np.ndarray] = None,
                 first_image: int = 0) -> Tuple[np.ndarray, Optional[np.ndarray]]:
        a, dev = self.area, self.area.device
        segs = np.ascontiguousarray(segs)
        if segs.dtype != np.uint16 or segs.ndim != 3 or segs.shape[1:] != (a.C - 1, a.W):
            raise ValueError(f"delineations must be uint16 (n,{a.C - 1},{a.W}), not {segs.dtype} {segs.shape}")
        labels_dev = a(torch.from_numpy(segs.view(np.int16)).to(dev))
        counts = None
        if gt is not None:
            gt_u8 = np.ascontiguousarray(gt, dtype=np.uint8)
            if gt_u8.shape != (segs.shape[0], a.H, a.W):
                raise ValueError(f"ground truth of shape {gt_u8.shape}, expected {(segs.shape[0], a.H, a.W)}")
            counts = self.counts.to_host(self.counts(labels_dev, torch.from_numpy(gt_u8).to(dev)), first_image)
        return labels_dev.cpu().numpy(), counts
