"""The evaluation / prediction pictures from the device: ``PngRenderer`` runs ``oct_render_rgba``
(include/oct_unet.h; numpy restatement ``common.plotting.render_reference``) over a batch in chunks and hands back host
RGBA arrays, which ``common.png.write_rgba`` turns into files.  ``batch_pictures`` is the set of pictures the two
workflows write for one batch."""
from __future__ import annotations

import ctypes as C
from pathlib import Path
from typing import Dict, Optional, Sequence, Union

import numpy as np
import torch

from .. import _hip
from ..common import plotting, png

STAGING_BYTES = 64 << 20          # pinned host memory of one renderer, whatever the run's batch size


class PngRenderer:
    """``oct_render_rgba`` for up to ``batch`` images of H x W per call, with device and pinned buffers of its own.

    A call renders in chunks of ``self.chunk`` images -- as many as keep the pinned staging buffer (4 H W bytes per image)
    within ``staging_bytes``; seven pictures of 256 x 512 per scan would be 460 MB at batch 128 -- and waits for each
    chunk's download, so what it returns is a fresh host array and nothing of the caller's is referenced afterwards.
    The base layer and the lines may be device tensors (used in place) or host arrays (uploaded into the renderer's own
    buffers)."""

    def __init__(self, batch: int, H: int, W: int, device, staging_bytes: int = STAGING_BYTES):
        self.B, self.H, self.W = int(batch), int(H), int(W)
        if not (1 <= self.B and 1 <= self.H <= plotting.MAX_H and 1 <= self.W <= 1 << 24):
            raise _hip.OctError(f"oct_render_rgba does not support B={batch}, {H}x{W}")
        self.device = torch.device(device)
        per_image = 4 * self.H * self.W
        self.chunk = max(1, min(self.B, 65535, int(staging_bytes) // per_image))
        self.out_dev = torch.empty((self.chunk, self.H, self.W, 4), dtype=torch.uint8, device=self.device)
        self.out_pin = torch.empty((self.chunk, self.H, self.W, 4), dtype=torch.uint8).pin_memory()
        self.rows_dev = torch.empty((self.chunk, plotting.MAX_LINES, self.W), dtype=torch.int16, device=self.device)
        self.base_dev = None                  # flat uint8, grown to the widest base a call has uploaded

    def _upload_base(self, host: np.ndarray) -> torch.Tensor:
        flat = torch.from_numpy(np.ascontiguousarray(host)).reshape(-1)
        if self.base_dev is None or self.base_dev.numel() < flat.numel():
            self.base_dev = torch.empty((flat.numel(),), dtype=torch.uint8, device=self.device)
        view = self.base_dev[:flat.numel()]
        view.copy_(flat)
        return view

    def render(self, base: Union[np.ndarray, torch.Tensor], *, palette=None, lines=None, colours=None, styles=None,
               col_range: Optional[Sequence[int]] = None, half_width: int = plotting.HALF_WIDTH) -> np.ndarray:
        """``base``: (n,H,W,ic) uint8 scans (``ic`` is read from the shape; a (n,H,W) array is one channel), or with
        ``palette`` ((n_cls, 3) RGB) (n,H,W) uint8 class maps.  ``lines``: (n,K,W) 16-bit rows with K ``colours`` and
        ``styles``, as ``render_reference``.  Returns (n,H,W,4) uint8 on the host."""
        labels = palette is not None
        on_dev = isinstance(base, torch.Tensor)
        if not on_dev:
            base = np.asarray(base)
        if (base.dtype != (torch.uint8 if on_dev else np.uint8)) or base.ndim not in (3, 4) or (labels and base.ndim != 3) \
                or tuple(base.shape[1:3]) != (self.H, self.W):
            raise _hip.OctError(f"the base layer must be uint8 (n,{self.H},{self.W}[,ic]), class maps without a channel axis")
        if on_dev:
            _hip.expect(base, "a device base layer", device=self.device, dtype=torch.uint8, shape=(None,) * base.ndim)
        n = int(base.shape[0])
        ic = 1 if base.ndim == 3 else int(base.shape[3])
        K = 0
        if lines is not None:
            lines_dev = isinstance(lines, torch.Tensor)
            if lines.ndim != 3 or lines.shape[0] != n or lines.shape[2] != self.W or \
                    (lines.element_size() if lines_dev else lines.dtype.itemsize) != 2:
                raise _hip.OctError(f"lines must be 16-bit integer ({n},K,{self.W})")
            K = int(lines.shape[1])
            if not lines_dev:
                lines = np.ascontiguousarray(lines).view(np.int16)
            else:
                _hip.expect(lines, "device lines", device=self.device, dtype=(torch.int16, torch.uint16), shape=(n, K, self.W))
        col_lo, col_hi = (0, self.W - 1) if col_range is None else (int(col_range[0]), int(col_range[-1]))
        styles = [plotting.SOLID] * K if styles is None else [int(s) for s in styles]
        colours = np.zeros((0, 3), np.int64) if colours is None else np.asarray(colours, np.int64).reshape(-1, 3)
        pal = np.zeros((1, 3), np.uint8) if not labels else np.asarray(palette, np.uint8).reshape(-1, 3)
        if n < 1 or n > self.B:
            raise _hip.OctError(f"render: needs a count n in 1..{self.B}")
        if K > plotting.MAX_LINES or len(styles) != K or colours.shape[0] != K or pal.shape[0] > plotting.MAX_CLASSES:
            raise _hip.OctError(f"render: at most {plotting.MAX_LINES} lines, each with a colour and a style, and "
                                f"{plotting.MAX_CLASSES} palette entries")
        st = _hip.RenderStyle()
        st.n_cls, st.n_lines, st.col_lo, st.col_hi, st.half_width = pal.shape[0], K, col_lo, col_hi, int(half_width)
        for i, v in enumerate(pal.reshape(-1)):
            st.palette[i] = int(v)
        for i, v in enumerate(colours.reshape(-1)):
            st.line_rgb[i] = int(v)
        for i, v in enumerate(styles):
            st.line_style[i] = int(v) & 255
        mode = _hip.RENDER_BASE_LABELS if labels else _hip.RENDER_BASE_IMAGE
        out = np.empty((n, self.H, self.W, 4), np.uint8)
        for lo in range(0, n, self.chunk):
            hi = min(n, lo + self.chunk)
            m = hi - lo
            b_dev = base[lo:hi] if on_dev else self._upload_base(base[lo:hi])
            r_ptr = None
            if K:
                if isinstance(lines, torch.Tensor):
                    r_dev = lines[lo:hi]
                else:
                    r_dev = self.rows_dev.view(-1)[:m * K * self.W].view(m, K, self.W)
                    r_dev.copy_(torch.from_numpy(lines[lo:hi]))
                r_ptr = r_dev.data_ptr()
            _hip.call("oct_render_rgba", self.device, mode, b_dev.data_ptr(), ic, r_ptr, C.byref(st), m, self.H, self.W,
                      self.out_dev.data_ptr(), _hip.stream_ptr(self.device))
            self.out_pin[:m].copy_(self.out_dev[:m], non_blocking=True)
            torch.cuda.current_stream(self.device).synchronize()
            out[lo:hi] = self.out_pin[:m].numpy()
        return out


# file names of the pictures (the reference's, its spelling of "ovelay" included)
EVALUATION_PNG_NAMES = {"pred": "predicted_segmentation_map.png", "raw": "raw_image.png",
                        "gt": "ground_truth_segmentation_map.png", "truth": "truth_plot.png",
                        "gs_map": "gs_predicted_segmentation_map.png", "gs_both": "gs_pred_and_truth_overlay_plot.png",
                        "gs_bounds": "gs_predicted_boundaries_ovelay_plot.png"}
PREDICTION_PNG_NAMES = {"pred": "segmentation_map.png", "raw": "raw_image.png",
                        "gs_map": "gs_predicted_segmentation_map.png",
                        "gs_bounds": "gs_predicted_boundaries_ovelay_plot.png",
                        "uncertainty": "uncertainty_map.png"}        # (no counterpart in the reference: Monte-Carlo dropout)

# the ordered decode's pictures (no counterpart in the reference), in evaluate_model and predict alike
OD_PNG_NAMES = {"od_map": "od_predicted_segmentation_map.png", "od_bounds": "od_predicted_boundaries_overlay_plot.png"}
# the picture of the component-cleaned class map (likewise)
CC_PNG_NAMES = {"cc_map": "cc_predicted_segmentation_map.png"}


IGNORED_RGB = (128, 128, 128)    # ground-truth pixels that carry the evaluation's ignore_label


def write_pictures(output_dir, pictures: Dict[str, np.ndarray], k: int, names: Dict[str, str]) -> None:
    """Image ``k`` of every picture of a batch -> ``output_dir / names[key]``."""
    for key, arr in pictures.items():
        png.write_rgba(Path(output_dir) / names[key], arr[k])


def batch_pictures(renderer: PngRenderer, num_classes: int, images: np.ndarray, *, pred_labels: Optional[np.ndarray] = None,
                   gt_labels: Optional[np.ndarray] = None, truths: Optional[np.ndarray] = None,
                   gs_segs: Optional[np.ndarray] = None, gs_labels=None, both_overlay: bool = False,
                   col_range: Optional[Sequence[int]] = None, ignore_label: Optional[int] = None) -> Dict[str, np.ndarray]:
    """The pictures of one batch, keyed by what they show; each value is (n,H,W,4) uint8 on the host.

    ``raw``: the scans.  ``pred``: ``pred_labels`` (n,H,W) through the region colours.  ``gt``: ``gt_labels`` likewise.
    ``truth``: the scans with ``truths`` (n,M,W) solid in the truth colours.  With ``gs_segs`` (n,M,W): ``gs_map``, the
    class maps ``gs_labels`` (host array or device tensor) through the region colours; ``gs_bounds``, the scans with
    ``gs_segs`` solid in the truth colours (the reference passes them as truths); and with ``both_overlay`` ``gs_both``,
    ``truths`` solid in the truth colours, then ``gs_segs`` dotted in the prediction colours.

    ``ignore_label``: the value of ``gt_labels`` that means "unknown".  Those pixels are mid-grey, ``IGNORED_RGB``, in ``gt``
    -- remapped on the host to one more palette entry, index ``num_classes``; the classes keep their colours -- and in the
    scan under the truth overlays ``truth`` and ``gs_both``, whose truth lines skip the columns where the boundary is 0 as
    they always do.  No other picture changes."""
    images = np.ascontiguousarray(np.asarray(images).astype(np.uint8, copy=False))
    if images.ndim == 3:
        images = images[..., None]
    scans = images
    images = torch.from_numpy(images).to(renderer.device)          # uploaded once, the base of up to four pictures
    palette = plotting.region_palette(num_classes)
    out = {"raw": renderer.render(images)}

    def u16(a):
        return np.ascontiguousarray(np.asarray(a).astype(np.uint16))

    def u8(a):
        return a if isinstance(a, torch.Tensor) else np.ascontiguousarray(np.asarray(a).astype(np.uint8))

    if pred_labels is not None:
        out["pred"] = renderer.render(u8(pred_labels), palette=palette)
    truth_base = images                                            # the scan under the truth overlays
    if gt_labels is not None and ignore_label is None:
        out["gt"] = renderer.render(u8(gt_labels), palette=palette)
    elif gt_labels is not None:
        if num_classes + 1 > plotting.MAX_CLASSES:
            raise ValueError(f"ignore_label: the ground-truth picture needs a palette entry more than the {num_classes} classes")
        ignored = np.asarray(gt_labels) == ignore_label
        out["gt"] = renderer.render(u8(np.where(ignored, num_classes, gt_labels)),
                                    palette=np.concatenate([palette, np.array([IGNORED_RGB], np.uint8)]))
        if truths is not None and ignored.any():
            grey = scans.copy()
            grey[ignored] = IGNORED_RGB[0]
            truth_base = torch.from_numpy(grey).to(renderer.device)
    if truths is not None:
        truths = u16(truths)
        out["truth"] = renderer.render(truth_base, lines=truths, colours=plotting.TRUTH_COLOURS[:truths.shape[1]])
    if gs_segs is not None:
        gs_segs = u16(gs_segs)
        M = gs_segs.shape[1]
        out["gs_map"] = renderer.render(u8(gs_labels), palette=palette)
        out["gs_bounds"] = renderer.render(images, lines=gs_segs, colours=plotting.TRUTH_COLOURS[:M], col_range=col_range)
        if both_overlay:
            out["gs_both"] = renderer.render(
                truth_base, lines=np.concatenate([truths, gs_segs], axis=1),
                colours=plotting.TRUTH_COLOURS[:truths.shape[1]] + plotting.PREDICT_COLOURS[:M],
                styles=[plotting.SOLID] * truths.shape[1] + [plotting.DOTTED] * M, col_range=col_range)
    return out
