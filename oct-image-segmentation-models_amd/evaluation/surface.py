"""Average surface distance and robust Hausdorff distance of class maps on the device
(reference evaluation/evaluation.py:207-262: spacing (0.01111111, 0.01111111), percent 95, every class but the
background).  ``SurfaceDistances`` owns the workspace of ``oct_surface_distances`` (include/oct_unet.h) for one
(batch, H, W, num_classes) and runs it on the current stream; ``datasets`` turns its (n, C-1, 6) rows into the four
per-image result datasets the reference writes (:573-597).  The kernels restate google-deepmind/surface-distance
(PARITY UNPINNED); ``common.custom_metrics`` holds the host restatement they are tested against."""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import numpy as np
import torch

from .. import _hip
from .dice_device import check_ignore_label

SPACING = (0.01111111, 0.01111111)
PERCENT = 95.0

# columns of one (image, class) row of the device output
ASD_GT_TO_PRED, ASD_PRED_TO_GT, PERC_GT_TO_PRED, PERC_PRED_TO_GT, N_SURFELS_GT, N_SURFELS_PRED = range(6)


class SurfaceDistances:
    """``ignore_label`` (None, or an int in num_classes..255) selects ``oct_surface_distances_masked``: ground-truth pixels
    of that value are unknown, and a cell that touches one is a surface element of neither map."""

    def __init__(self, batch: int, H: int, W: int, num_classes: int, device, spacing: Tuple[float, float] = SPACING,
                 percent: float = PERCENT, ignore_label: Optional[int] = None):
        self.B, self.H, self.W, self.C = int(batch), int(H), int(W), int(num_classes)
        self.ignore_label = check_ignore_label(ignore_label, self.C)
        self.device = torch.device(device)
        self.spacing, self.percent = (float(spacing[0]), float(spacing[1])), float(percent)
        nbytes = _hip.lib().oct_surface_workspace_bytes(self.B, self.H, self.W, self.C)
        if nbytes == 0:
            raise _hip.OctError(f"oct_surface_distances does not support B={batch}, {H}x{W}, {num_classes} classes")
        self.workspace = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        self.out = torch.empty((self.B, self.C - 1, 6), dtype=torch.float64, device=self.device)
        self.outs, self.geometry = (self.out,), (self.B, self.H, self.W, self.C)

    def __call__(self, pred: torch.Tensor, gt: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """(n,H,W) uint8 predicted and ground-truth class maps on the device, n <= batch -> (n, C-1, 6) float64 on the
        device (``out`` or a view of an internal buffer that the next call overwrites), queued on the current stream.
        The call waits for that stream once: it checks the labels on the device before the distance passes."""
        n = _hip.expect_map_pair(pred, gt, device=self.device, batch=self.B, H=self.H, W=self.W)
        out = _hip.out_view(out, self.out, n)
        tail = (self.spacing[0], self.spacing[1], self.percent, self.workspace.data_ptr(), self.workspace.numel(),
                out.data_ptr(), _hip.stream_ptr(self.device))
        if self.ignore_label is None:
            _hip.call("oct_surface_distances", self.device, pred.data_ptr(), gt.data_ptr(), n, self.H, self.W, self.C, *tail)
        else:
            _hip.call("oct_surface_distances_masked", self.device, pred.data_ptr(), gt.data_ptr(), n, self.H, self.W, self.C,
                      self.ignore_label, *tail)
        return out

    @staticmethod
    def to_host(rows: torch.Tensor, first_image: int = 0) -> np.ndarray:
        """Device or pinned rows -> a fresh (n, C-1, 6) float64 host array (waits for the stream).  ``first_image`` is
        what the pipeline's stages take in common; nothing here can fail per image."""
        return rows.cpu().numpy().copy()


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
