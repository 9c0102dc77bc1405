"""Ordered layer decode: for every column of the class probabilities the best labelling whose class
index never decreases with depth, decoded jointly for all classes on the device (``oct_ordered_decode``, include/oct_unet.h;
``common.utils.ordered_decode_reference`` restates it bit for bit).  Here: the wrapper the inference pipeline runs as a stage
and the host formulas of what the result files state about the decode.  The reference has no counterpart."""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np

from ..common.utils import ORDERED_MAX_CLASSES, ORDERED_MAX_H, ORDERED_MIN_CLASSES


def check_ordered(num_classes: int, H: int, what: str = "ordered_decode") -> None:
    """Raise ``ValueError`` for a class count or image height the decode refuses."""
    if not ORDERED_MIN_CLASSES <= int(num_classes) <= ORDERED_MAX_CLASSES:
        raise ValueError(f"{what}: needs {ORDERED_MIN_CLASSES}..{ORDERED_MAX_CLASSES} classes, not {num_classes}")
    if not 1 <= int(H) <= ORDERED_MAX_H:
        raise ValueError(f"{what}: needs an image height in 1..{ORDERED_MAX_H}, not {H}")


def layer_thickness(rows: np.ndarray) -> Tuple[Optional[np.ndarray], Optional[np.ndarray]]:
    """Boundary rows (C-1, W) of one image -> ``(layer_thickness uint16 (C-2, W), mean_layer_thickness float64 (C-2,))`` in
    pixels: ``rows[k] - rows[k-1]``, the number of rows of class k in the column, for the classes 1..C-2 that have a boundary on
    either side.  ``(None, None)`` at C = 2."""
    r = np.asarray(rows).astype(np.int64)
    if r.ndim != 2:
        raise ValueError("layer_thickness: rows must be (C-1, W)")
    if r.shape[0] < 2:
        return None, None
    t = r[1:] - r[:-1]
    if (t < 0).any():
        raise ValueError("layer_thickness: the rows cross")
    return t.astype(np.uint16), t.mean(axis=1, dtype=np.float64)


class OrderedDecode:
    """``oct_ordered_decode`` for up to ``batch`` images of one shape: ``(probs)`` -- (n,H,W,C) float32 class probabilities on
    the device -> ``labels`` (n,H,W) uint8, ``rows`` (n,C-1,W) int16 (the bits are uint16) and ``score`` (n,W) int32 (the bits are
    uint32) on the device, queued on the current stream.  The workspace is the object's own."""

    def __init__(self, batch: int, H: int, W: int, num_classes: int, device):
        import torch
        from .. import _hip
        self.B, self.H, self.W, self.C = int(batch), int(H), int(W), int(num_classes)
        nbytes = int(_hip.lib().oct_ordered_workspace_bytes(self.B, self.H, self.W, self.C))
        if not nbytes:
            raise _hip.OctError(f"oct_ordered_decode does not support B={batch}, {H}x{W}, {num_classes} classes")
        self.device = torch.device(device)
        self.labels = torch.empty((self.B, self.H, self.W), dtype=torch.uint8, device=self.device)
        self.rows = torch.empty((self.B, self.C - 1, self.W), dtype=torch.int16, device=self.device)
        self.score = torch.empty((self.B, self.W), dtype=torch.int32, device=self.device)
        self.ws = torch.empty((nbytes,), dtype=torch.uint8, device=self.device)
        self.outs, self.geometry = (self.labels, self.rows, self.score), (self.B, self.H, self.W, self.C)

    def __call__(self, probs, labels=None, rows=None, score=None):
        import torch
        from .. import _hip
        _hip.expect(probs, "probs", device=self.device, dtype=torch.float32, shape=(None, self.H, self.W, self.C))
        n = probs.shape[0]
        if not 1 <= n <= self.B:
            raise _hip.OctError(f"probs needs a count n in 1..{self.B}, not {n}")
        labels, rows = _hip.out_view(labels, self.labels, n, "labels"), _hip.out_view(rows, self.rows, n, "rows")
        score = _hip.out_view(score, self.score, n, "score")
        _hip.call("oct_ordered_decode", self.device, probs.data_ptr(), n, self.H, self.W, self.C, self.ws.data_ptr(),
                  self.ws.numel(), labels.data_ptr(), rows.data_ptr(), score.data_ptr(), _hip.stream_ptr(self.device))
        return labels, rows, score

    @staticmethod
    def to_host(labels, rows, score, first_image: int = 0) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """Device tensors -> ``(labels (n,H,W) uint8, rows (n,C-1,W) uint16, score (n,W) uint32)`` on the host (waits for the
        stream)."""
        return (labels.cpu().numpy().copy(), rows.cpu().numpy().view(np.uint16).copy(), score.cpu().numpy().view(np.uint32).copy())
