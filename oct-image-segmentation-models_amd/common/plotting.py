"""The evaluation / prediction pictures on the host: the colour tables, ``render_reference`` -- the numpy statement of
``oct_render_rgba`` (include/oct_unet.h), integers only, equal to the kernel bit for bit -- and
``save_image_plot`` / ``save_segmentation_plot`` with the reference's names and argument order
(oct_image_segmentation_models/common/plotting.py:169-278) for callers without a device.  matplotlib is not used.

Against matplotlib: an image picture is H x W RGBA with alpha 255, one output pixel per input pixel, as there; a label map
is ``palette[label]`` (matplotlib normalises by the map's own minimum and maximum, so a map that lacks class 0 or the top
class is coloured differently there: not reproduced); a one-channel scan is the identity R = G = B = level (matplotlib's
resampler gives one less at 24 of the 256 levels: not reproduced); the overlays follow this project's own rule -- one
output pixel per input pixel, no margin, lines by the rule of ``oct_render_rgba`` -- where matplotlib rescales the axes."""
from __future__ import annotations

from pathlib import Path
from typing import Optional, Sequence

import numpy as np

from . import png

# RGB per boundary / region, 12 entries each (the reference's predict_colours, truth_colours, region_colours)
PREDICT_COLOURS = ((66, 133, 244), (219, 68, 55), (244, 180, 0), (15, 157, 88), (255, 109, 0), (70, 189, 198),
                   (171, 48, 196), (253, 232, 255), (66, 133, 244), (219, 68, 55), (244, 180, 0), (15, 157, 88))
TRUTH_COLOURS = ((43, 87, 144), (122, 38, 30), (155, 114, 0), (8, 86, 48), (142, 61, 0), (38, 104, 109),
                 (95, 26, 109), (242, 102, 255), (43, 87, 144), (122, 38, 30), (155, 114, 0), (8, 86, 48))
REGION_COLOURS = ((253, 232, 255), (66, 133, 244), (219, 68, 55), (244, 180, 0), (15, 157, 88), (255, 109, 0),
                  (70, 189, 198), (171, 48, 196), (14, 13, 94), (253, 232, 255), (66, 133, 244), (219, 68, 55))

MAX_CLASSES, MAX_LINES, MAX_H, MAX_HALF_WIDTH = 32, 16, 4096, 64
HALF_WIDTH = 22                 # eighths of a pixel: a 5.5 px line, what the reference's linewidth=4.0 points give at 100 dpi
SOLID, DOTTED = 0, 1
_OFF = np.array([-3, -1, 1, 3], np.int64)


def region_palette(num_classes: int) -> np.ndarray:
    """The first ``num_classes`` region colours, (n, 3) uint8: ``ListedColormap(region_colours, N=num_classes)``."""
    if not 1 <= int(num_classes) <= len(REGION_COLOURS):
        raise ValueError(f"region colours exist for 1..{len(REGION_COLOURS)} classes")
    return np.array(REGION_COLOURS[:int(num_classes)], np.uint8)


# The truth + prediction overlay draws 2 (num_classes - 1) lines out of MAX_LINES, and a picture's lines and regions take
# their colours from the 12-entry tables above: pictures exist up to this class count
PNG_MAX_CLASSES = MAX_LINES // 2 + 1


def check_png_classes(png_plots: bool, num_classes: int) -> bool:
    """``png_plots`` as a bool; ``ValueError`` where pictures are asked for with more classes than the renderer holds.  The
    parameter objects of ``evaluate_model`` / ``predict`` call it, so nothing has run when it raises."""
    if png_plots and int(num_classes) > PNG_MAX_CLASSES:
        raise ValueError(f"png_plots=True needs num_classes <= {PNG_MAX_CLASSES} (an overlay draws 2 (num_classes - 1) lines, the "
                         f"renderer holds {MAX_LINES}), not {int(num_classes)}; png_plots=False works up to 16 classes")
    return bool(png_plots)


def half_width_of(linewidth: float) -> int:
    """A matplotlib line width in points at 100 dpi -> the half width in eighths of a pixel (4.0 -> 22)."""
    return int(round(float(linewidth) * 100.0 / 72.0 * 4.0))


def check_render_args(B, H, W, *, labels: bool, n_cls: int, K: int, col_lo: int, col_hi: int, half_width: int, styles=()):
    """The refusals of ``oct_render_rgba``, as ``ValueError``."""
    if B < 1 or H < 1 or W < 1:
        raise ValueError("render: B, H, W must be positive")
    if H > MAX_H:
        raise ValueError(f"render: H above {MAX_H}")
    if labels and not 1 <= n_cls <= MAX_CLASSES:
        raise ValueError(f"render: need 1 <= n_cls <= {MAX_CLASSES}")
    if not 0 <= K <= MAX_LINES:
        raise ValueError(f"render: need 0 <= n_lines <= {MAX_LINES}")
    if not 1 <= half_width <= MAX_HALF_WIDTH:
        raise ValueError(f"render: need 1 <= half_width <= {MAX_HALF_WIDTH}")
    if col_lo > col_hi or col_lo < 0 or col_hi > W - 1:
        raise ValueError("render: need 0 <= col_lo <= col_hi <= W - 1")
    if any(int(s) not in (SOLID, DOTTED) for s in styles):
        raise ValueError("render: line styles are 0 (solid) or 1 (dotted)")


def line_coverage(rows: np.ndarray, H: int, col_lo: int, col_hi: int, half_width: int, dotted) -> np.ndarray:
    """Polylines, rows (W,) or (N, W) -> the coverage 0..16 of each per pixel, (H, W) or (N, H, W) int64.  ``dotted``: one
    flag, or one per line."""
    rows = np.asarray(rows).astype(np.int64)
    if rows.ndim == 1:
        return line_coverage(rows[None], H, col_lo, col_hi, half_width, dotted)[0]
    N, W = rows.shape
    R = int(half_width)
    dotted = np.broadcast_to(np.asarray(dotted, bool), (N,))
    cols = np.arange(W, dtype=np.int64)
    v = np.where((cols >= col_lo) & (cols <= col_hi) & (rows > 0) & (rows < H), rows, 0)
    cov = np.zeros((N, H, W), np.int64)
    if not ((v[:, :-1] > 0) & (v[:, 1:] > 0)).any():
        return cov
    # a sample at x can be within R of the segment between columns j and j+1 only if 8j - R <= x <= 8j + 8 + R: for a pixel
    # of column c that leaves j = c + d, d in -1-hw .. hw; rows further than R from every vertex hold no sample either
    hw = (R + 3 + 7) // 8
    pad = hw + 2
    used = v[v > 0]
    r_lo = max(0, (8 * int(used.min()) - R - 3 + 7) // 8)
    r_hi = min(H - 1, (8 * int(used.max()) + R + 3) // 8)
    r = np.arange(r_lo, r_hi + 1, dtype=np.int64)
    RR = R * R
    dots = (((8 * (cols - col_lo))[:, None] + _OFF[None, :]) % 120 < 48)[None, None, None, :, :]
    step = max(1, (1 << 21) // (r.size * W * 16))                               # lines per pass: bounds the temporaries
    for n0 in range(0, N, step):
        vn = v[n0:n0 + step]
        vp = np.pad(vn, ((0, 0), (pad, pad)))
        hit = np.zeros((vn.shape[0], r.size, 4, W, 4), bool)                    # (line, row, oy, column, ox)
        for d in range(-1 - hw, hw + 1):
            v0, v1 = vp[:, pad + d:pad + d + W], vp[:, pad + d + 1:pad + d + 1 + W]
            seg = (v0 > 0) & (v1 > 0)
            if not seg.any():
                continue
            wx = (_OFF - 8 * d)[None, None, None, None, :]
            wy = (8 * (r[None, :, None, None] - v0[:, None, None, :]) + _OFF[None, None, :, None])[..., None]
            dy = (8 * (v1 - v0))[:, None, None, :, None]
            t = 8 * wx + wy * dy
            den = 64 + dy * dy
            ww = wx * wx + wy * wy
            end = (wx - 8) * (wx - 8) + (wy - dy) * (wy - dy)
            on = np.where(t <= 0, ww <= RR, np.where(t >= den, end <= RR, ww * den - t * t <= RR * den))
            hit |= on & seg[:, None, None, :, None]
        hit &= dots | ~dotted[n0:n0 + step, None, None, None, None]
        cov[n0:n0 + step, r_lo:r_hi + 1] = hit.sum(axis=(2, 4))
    return cov


def render_reference(base: np.ndarray, palette=None, lines: Optional[np.ndarray] = None, colours=None, styles=None,
                     col_range=None, half_width: int = HALF_WIDTH) -> np.ndarray:
    """``oct_render_rgba`` in numpy.  ``base``: (B,H,W,ic) uint8 scans, or with ``palette`` ((n_cls, 3) RGB) (B,H,W)
    uint8 class maps.  ``lines``: (B,K,W) row per column of K polylines, drawn in index order with ``colours`` (K RGB
    triples) and ``styles`` (K of 0 solid / 1 dotted, default solid) inside the inclusive ``col_range`` (default: the full
    width).  Returns (B,H,W,4) uint8 RGBA, alpha 255."""
    base = np.asarray(base)
    if base.dtype != np.uint8:
        raise ValueError("render: the base layer is uint8")
    labels = palette is not None
    if base.ndim != (3 if labels else 4):
        raise ValueError("render: the base is (B,H,W) class maps with a palette, (B,H,W,ic) scans without")
    B, H, W = base.shape[:3]
    K = 0
    if lines is not None:
        lines = np.asarray(lines)
        if lines.ndim != 3 or lines.shape[0] != B or lines.shape[2] != W:
            raise ValueError(f"render: lines must be (B,K,W) = ({B},K,{W}), not {lines.shape}")
        K = lines.shape[1]
    col_lo, col_hi = (0, W - 1) if col_range is None else (int(col_range[0]), int(col_range[-1]))
    styles = [SOLID] * K if styles is None else [int(s) for s in styles]
    colours = np.zeros((0, 3), np.int64) if colours is None else np.asarray(colours, np.int64).reshape(-1, 3)
    pal = np.zeros((1, 3), np.uint8) if not labels else np.asarray(palette, np.uint8).reshape(-1, 3)
    check_render_args(B, H, W, labels=labels, n_cls=pal.shape[0], K=K, col_lo=col_lo, col_hi=col_hi,
                      half_width=int(half_width), styles=styles)
    if len(styles) != K or colours.shape[0] != K:
        raise ValueError(f"render: {K} lines need {K} colours and styles")
    if labels:
        table = np.zeros((256, 3), np.uint8)
        table[:pal.shape[0]] = pal
        rgb = table[base].astype(np.int64)
    elif base.shape[3] == 3:
        rgb = base.astype(np.int64)
    else:
        rgb = np.repeat(base[..., :1], 3, axis=3).astype(np.int64)
    if K:
        cov = line_coverage(lines.reshape(B * K, W), H, col_lo, col_hi, int(half_width),
                            np.tile(np.array(styles) == DOTTED, B)).reshape(B, K, H, W, 1)
        for k in range(K):
            rgb = (cov[:, k] * colours[k][None, None, None, :] + (16 - cov[:, k]) * rgb + 8) >> 4
    out = np.full((B, H, W, 4), 255, np.uint8)
    out[..., :3] = rgb
    return out


def _as_image(image: np.ndarray) -> np.ndarray:
    image = np.asarray(image)
    if image.ndim == 2:
        image = image[:, :, None]
    if image.ndim != 3:
        raise ValueError("an image is (H,W) or (H,W,channels)")
    return image.astype(np.uint8)[None]


def save_image_plot(image: np.ndarray, filename: Path, cmap=None, vmin: int = None, vmax: int = None) -> None:
    """One picture of ``image``, H x W pixels.  ``cmap`` None or "gray": a scan, (H,W), (H,W,1) or (H,W,3), shown as it is
    (``vmin`` / ``vmax`` are accepted for the reference's signature; the scale is 0..255).  ``cmap`` an (n, 3) RGB table
    (``region_palette(num_classes)``): ``image`` is an (H,W) class map."""
    if cmap is None or isinstance(cmap, str):
        if isinstance(cmap, str) and cmap != "gray":
            raise ValueError('save_image_plot: cmap is None, "gray" or an (n, 3) RGB table')
        rgba = render_reference(_as_image(image))
    else:
        lab = np.asarray(image)
        if lab.ndim == 3 and lab.shape[2] == 1:
            lab = lab[:, :, 0]
        rgba = render_reference(lab.astype(np.uint8)[None], palette=cmap)
    png.write_rgba(filename, rgba[0])


def save_segmentation_plot(image: np.ndarray, image_cmap, filename: Path, truths: Optional[np.ndarray],
                           predictions: Optional[np.ndarray], column_range: Optional[Sequence[int]] = None,
                           linewidth: float = 4.0, color=None) -> None:
    """The scan with boundaries over it: ``truths`` (M, W) solid in the truth colours, then ``predictions`` (M, W) dotted
    in the prediction colours (``color``, an RGB triple, replaces both tables); 0 is "no boundary here".  ``column_range``
    is a range or sequence whose first and last entry bound the columns drawn."""
    if image_cmap is not None and image_cmap != "gray":
        raise ValueError('save_segmentation_plot: image_cmap is None or "gray"')
    if truths is None and predictions is None:
        raise ValueError("save_segmentation_plot: truths or predictions must be given")
    rows, colours, styles = [], [], []
    for segs, table, style in ((truths, TRUTH_COLOURS, SOLID), (predictions, PREDICT_COLOURS, DOTTED)):
        if segs is None:
            continue
        segs = np.asarray(segs)
        for i in range(segs.shape[0]):
            rows.append(np.clip(segs[i], 0, 65535).astype(np.uint16))
            colours.append(table[i] if color is None else tuple(color))
            styles.append(style)
    rgba = render_reference(_as_image(image), lines=np.stack(rows)[None], colours=colours, styles=styles,
                            col_range=column_range, half_width=half_width_of(linewidth))
    png.write_rgba(filename, rgba[0])
