"""Average surface distance and robust Hausdorff distance of class maps on the device
(reference evaluation/evaluation.py:207-262: spacing (0.01111111, 0.01111111), percent 95, every class but the
background).  ``SurfaceDistances`` owns the workspace of ``oct_surface_distances`` (include/oct_unet.h) for one
(batch, H, W, num_classes) and runs it on the current stream; ``datasets`` turns its (n, C-1, 6) rows into the four
per-image result datasets the reference writes (:573-597).  The kernels restate google-deepmind/surface-distance
(PARITY UNPINNED); ``common.custom_metrics`` holds the host restatement they are tested against."""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from .. import _hip

SPACING = (0.01111111, 0.01111111)
PERCENT = 95.0

# columns of one (image, class) row of the device output
ASD_GT_TO_PRED, ASD_PRED_TO_GT, PERC_GT_TO_PRED, PERC_PRED_TO_GT, N_SURFELS_GT, N_SURFELS_PRED = range(6)


class SurfaceDistances:
    def __init__(self, batch: int, H: int, W: int, num_classes: int, device, spacing: Tuple[float, float] = SPACING,
                 percent: float = PERCENT):
        self.B, self.H, self.W, self.C = int(batch), int(H), int(W), int(num_classes)
        self.device = torch.device(device)
        self.spacing, self.percent = (float(spacing[0]), float(spacing[1])), float(percent)
        nbytes = _hip.lib().oct_surface_workspace_bytes(self.B, self.H, self.W, self.C)
        if nbytes == 0:
            raise _hip.OctError(f"oct_surface_distances does not support B={batch}, {H}x{W}, {num_classes} classes")
        self.workspace = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        self.out = torch.empty((self.B, self.C - 1, 6), dtype=torch.float64, device=self.device)

    def __call__(self, pred: torch.Tensor, gt: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """(n,H,W) uint8 predicted and ground-truth class maps on the device, n <= batch -> (n, C-1, 6) float64 on the
        device (``out`` or a view of an internal buffer that the next call overwrites), queued on the current stream."""
        for t in (pred, gt):
            if t.device != self.device or t.dtype != torch.uint8 or not t.is_contiguous() or t.dim() != 3 \
                    or tuple(t.shape[1:]) != (self.H, self.W):
                raise _hip.OctError(f"class maps must be contiguous uint8 (n,{self.H},{self.W}) tensors on {self.device}")
        n = pred.shape[0]
        if gt.shape[0] != n or not 1 <= n <= self.B:
            raise _hip.OctError(f"pred and gt need the same count n in 1..{self.B}")
        if out is None:
            out = self.out[:n]
        elif out.device != self.device or out.dtype != torch.float64 or not out.is_contiguous() \
                or tuple(out.shape) != (n, self.C - 1, 6):
            raise _hip.OctError(f"out must be a contiguous float64 ({n},{self.C - 1},6) tensor on {self.device}")
        stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        with torch.cuda.device(self.device):
            _hip.check(_hip.lib().oct_surface_distances(
                pred.data_ptr(), gt.data_ptr(), n, self.H, self.W, self.C, self.spacing[0], self.spacing[1], self.percent,
                self.workspace.data_ptr(), self.workspace.numel(), out.data_ptr(), stream), "oct_surface_distances")
        return out


def datasets(rows: np.ndarray) -> Dict[str, np.ndarray]:
    """(..., C-1, 6) device rows -> the reference's per-image datasets (float64, (..., C-1)):
    average_surface_distances = (gt_to_pred + pred_to_gt) / 2, both directed averages, and hausdorff_distances = the
    max of the two directed percentile distances."""
    rows = np.asarray(rows, np.float64)
    a, b = rows[..., ASD_GT_TO_PRED], rows[..., ASD_PRED_TO_GT]
    return {"average_surface_distances": (a + b) / 2.0,
            "average_surface_distances_gt_to_pred": a.copy(),
            "average_surface_distances_pred_to_gt": b.copy(),
            "hausdorff_distances": np.maximum(rows[..., PERC_GT_TO_PRED], rows[..., PERC_PRED_TO_GT])}
