"""Post-step and housekeeping helpers of the reference's ``common/utils.py`` (:19-176), numpy only."""
from __future__ import annotations

import datetime
import hashlib
import json
import logging as log
from pathlib import Path
from typing import Tuple

import numpy as np


def get_timestamp():
    return datetime.datetime.now().strftime("%Y-%m-%d_%H_%M_%S")


def md5(file_path: Path) -> str:
    log.info(f"Calculating md5 of file: {file_path}")
    h = hashlib.md5()
    with open(file_path, "rb") as f:
        for chunk in iter(lambda: f.read(1 << 24), b""):
            h.update(chunk)
    return h.hexdigest()


def result_attrs(model_path, image_name, **times) -> dict:
    """File attributes every per-image result file of ``evaluate_model`` / ``predict`` carries, then the caller's timings."""
    return {"model_filename": np.array(str(model_path), dtype="S1000"),
            "image_name": np.array(str(image_name), dtype="S1000"),
            "timestamp": np.array(get_timestamp(), dtype="S1000"), **times}


def to_categorical(y, num_classes: int) -> np.ndarray:
    """keras.utils.to_categorical: a trailing axis of size 1 is dropped, result float32 (Appendix B.8)."""
    y = np.asarray(y, dtype="int64")
    shape = y.shape
    if shape and shape[-1] == 1 and len(shape) > 1:
        shape = shape[:-1]
    out = np.zeros((y.size, num_classes), dtype=np.float32)
    out[np.arange(y.size), y.ravel()] = 1.0
    return out.reshape(shape + (num_classes,))


def load_model_and_config(model_path: Path, **kwargs):
    """Load a model saved by ``Model.save`` plus its sibling ``model_config.json``
    (reference: utils.py:27-70; the MLflow branch is out of scope)."""
    from ..models.engine_model import load_model
    if kwargs.get("mlflow_tracking_uri"):
        raise NotImplementedError("MLflow model loading is outside the accelerated path")
    model_path = Path(model_path)
    loaded_model = load_model(model_path)
    with open(model_path.parent / Path("model_config.json"), "r") as config_file:
        model_config = json.load(config_file)
    return loaded_model, model_config


def convert_maps_uint8(prob_maps):
    prob_maps *= 255
    return prob_maps.astype("uint8")


def perform_argmax(predictions, bin=True):
    """(n,H,W,C) probabilities -> [argmax (n,H,W), categorical (n,C,H,W)] (utils.py:80-112, channels_last)."""
    num_maps = predictions.shape[3]
    argmax_pred = np.argmax(predictions, axis=3)
    if bin:
        categorical_pred = np.transpose(to_categorical(argmax_pred, num_maps), axes=(0, 3, 1, 2))
    else:
        categorical_pred = np.transpose(predictions, axes=(0, 3, 1, 2))
    return [argmax_pred, categorical_pred]


def labels_to_categorical(label_maps: np.ndarray, num_classes: int) -> np.ndarray:
    """(n,H,W) class maps (e.g. the device arg-max) -> categorical (n,C,H,W) float32, as perform_argmax(bin=True)."""
    return np.transpose(to_categorical(label_maps, num_classes), axes=(0, 3, 1, 2))


def convert_predictions_to_maps_semantic(categorical_pred, bg_ilm=True, bg_csi=False):
    """Vertical-gradient boundary maps, uint8 (n, C-1, H, W) (utils.py:115-168)."""
    num_samples, num_maps, img_height, img_width = categorical_pred.shape
    boundary_maps = np.zeros((num_samples, num_maps - 1, img_height, img_width), dtype="uint8")
    for sample_ind in range(num_samples):
        for map_ind in range(1, num_maps):
            flip = (map_ind == 1 and bg_ilm is True) or (map_ind == num_maps - 1 and bg_csi is True)
            cur_map = categorical_pred[sample_ind, map_ind - 1 if flip else map_ind, :, :]
            grad_map = np.gradient(cur_map, axis=0)
            if flip:
                grad_map = -grad_map
            grad_map[grad_map < 0] = 0
            grad_map *= 2
            grad_map -= np.roll(grad_map, -1, axis=0)
            grad_map[grad_map < 0] = 0
            boundary_maps[sample_ind, map_ind - 1, :, :] = convert_maps_uint8(grad_map)
    return boundary_maps


def soft_boundary_maps_reference(probs_nhwc, bg_ilm=True, bg_csi=False) -> np.ndarray:
    """``oct_boundary_maps_soft`` (include/oct_unet.h) restated element by element: (n,H,W,C) float32 class
    probabilities -> uint8 (n, C-1, H, W), equal to ``convert_predictions_to_maps_semantic(perform_argmax(probs,
    bin=False)[1])``.  Every step is one float32 operation, in the order of the header's definition; a single row
    (where ``np.gradient`` refuses the input) has gradient 0."""
    p = np.asarray(probs_nhwc, dtype=np.float32)
    n, H, W, C = p.shape
    two, zero = np.float32(2.0), np.float32(0.0)
    out = np.zeros((n, C - 1, H, W), dtype=np.uint8)
    rows = np.arange(H)
    lo, hi = np.maximum(rows - 1, 0), np.minimum(rows + 1, H - 1)
    interior = (rows > 0) & (rows < H - 1)
    for m in range(1, C):
        flip = (m == 1 and bool(bg_ilm)) or (m == C - 1 and bool(bg_csi))
        f = p[:, :, :, m - 1 if flip else m]                       # (n,H,W)
        d = f[:, hi, :] - f[:, lo, :]                              # one-sided at the edge rows, 0 where H == 1
        d[:, interior, :] = d[:, interior, :] / two
        if flip:
            d = -d
        g = two * np.maximum(d, zero)
        v = np.maximum(g - g[:, (rows + 1) % H, :], zero)          # the roll wraps: the last row subtracts row 0's g
        # numpy's float32 -> uint8 cast on the hosts the goldens come from: truncate, then wrap (510 -> 254)
        out[:, m - 1] = ((v * np.float32(255.0)).astype(np.int32) & 255).astype(np.uint8)
    return out


def mc_reduce_reference(probs_stack, dtype=np.float32) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """``oct_mc_update`` (include/oct_unet.h) restated step by step: a stack (T, n, H, W, C) of softmax outputs of T
    Monte-Carlo dropout samples -> ``(mean_probs (n,H,W,C), argmax (n,H,W) uint8, entropy (n,H,W), mutual_info (n,H,W))``.
    With ``dtype=np.float32`` every step is one float32 operation in the order of the header's definition, so
    ``mean_probs`` and ``argmax`` equal the kernel's bit for bit (the entropies differ by the rounding of the logarithm);
    ``dtype=np.float64`` runs the same steps in double precision on the same float32 inputs, for the entropy checks."""
    p = np.asarray(probs_stack, dtype=np.float32)
    if p.ndim != 5 or p.shape[0] < 1:
        raise ValueError("mc_reduce_reference: need a (T, n, H, W, C) stack with T >= 1")
    dt = np.dtype(dtype).type
    T, C = p.shape[0], p.shape[-1]
    inv_t = dt(dt(1.0) / dt(T))

    def neg_sum_plogp(q):                      # -(plogp(q_0) + plogp(q_1) + ...), summed in class order
        t = np.zeros_like(q)
        pos = q > 0
        t[pos] = q[pos] * np.log(q[pos])       # p > 0 ? p * log(p) : 0
        acc = t[..., 0].copy()
        for c in range(1, C):
            acc = acc + t[..., c]
        return -acc

    S = E = None
    for t in range(T):
        pt = p[t].astype(dt)
        h = neg_sum_plogp(pt)
        S, E = (pt.copy(), h) if t == 0 else (S + pt, E + h)
    m = S * inv_t
    best, arg = m[..., 0].copy(), np.zeros(m.shape[:-1], np.uint8)
    for c in range(1, C):                      # the lowest index among equal maxima
        gt = m[..., c] > best
        best[gt] = m[..., c][gt]
        arg[gt] = c
    entropy = neg_sum_plogp(m)
    mutual_info = np.maximum(entropy - E * inv_t, dt(0.0))
    return m, arg, entropy, mutual_info


TTA_VIEWS = {"identity": 0, "flip_lr": 1, "flip_ud": 2, "flip_both": 3}    # bit 0 mirrors columns, bit 1 mirrors rows
TTA_VIEW_NAMES = tuple(TTA_VIEWS)                                          # the name of code v is TTA_VIEW_NAMES[v]


def parse_tta(value) -> Tuple[int, ...]:
    """A test-time-augmentation setting -> its view codes: ``None`` or ``()`` (off) -> ``()``; else a sequence of 1..4
    distinct names out of ``TTA_VIEWS``, e.g. ``("identity", "flip_lr")`` -> ``(0, 1)``.  Anything else is a ``ValueError``
    that names the offender."""
    if value is None:
        return ()
    if isinstance(value, str) or not isinstance(value, (tuple, list)):
        raise ValueError(f"tta must be None or a sequence of view names out of {TTA_VIEW_NAMES}, not {value!r}")
    if len(value) > len(TTA_VIEWS):
        raise ValueError(f"tta: at most {len(TTA_VIEWS)} views, not the {len(value)} of {tuple(value)!r}")
    codes = []
    for name in value:
        if not isinstance(name, str) or name not in TTA_VIEWS:
            raise ValueError(f"tta: unknown view {name!r} (the views are {TTA_VIEW_NAMES})")
        if TTA_VIEWS[name] in codes:
            raise ValueError(f"tta: view {name!r} is given twice")
        codes.append(TTA_VIEWS[name])
    return tuple(codes)


def check_tta(tta, mc_samples: int = 0) -> Tuple[str, ...]:
    """The public ``tta`` setting, validated (``parse_tta``): the tuple of its view names, ``()`` for off.
    Together with ``mc_samples`` > 0 it is a ``ValueError``."""
    parse_tta(tta)
    names = () if tta is None else tuple(tta)
    if names and int(mc_samples) > 0:
        raise ValueError(f"tta={names!r} together with mc_samples={mc_samples}: test-time augmentation and Monte-Carlo "
                         "dropout are not combined")
    return names


def flip_reference(a, view: int) -> np.ndarray:
    """``oct_flip_batch`` (include/oct_unet.h) restated with index arrays: ``out[b, y, x] = a[b, yv, xv]`` for a (B,H,W,...)
    array of any dtype; bit 0 of ``view`` mirrors the columns (``xv = W-1-x``), bit 1 the rows (``yv = H-1-y``)."""
    a = np.asarray(a)
    if a.ndim < 3 or not 0 <= int(view) <= 3:
        raise ValueError("flip_reference: need a (B,H,W,...) array and a view in 0..3")
    H, W = a.shape[1:3]
    iy = H - 1 - np.arange(H) if int(view) & 2 else np.arange(H)
    ix = W - 1 - np.arange(W) if int(view) & 1 else np.arange(W)
    return np.ascontiguousarray(a[:, iy][:, :, ix])


def tta_reduce_reference(probs_stack, views, dtype=np.float32) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """``oct_tta_update`` (include/oct_unet.h) restated: a stack (T, n, H, W, C) whose sample t is the softmax output of the
    batch flipped by ``views[t]`` (codes in 0..3) -> ``(mean_probs, argmax, entropy, mutual_info)`` of the views mirrored
    back.  Pixel (b, y, x) of the sums takes sample t's pixel (b, yv, xv), a flip being its own inverse; what follows are
    the float32 steps of ``mc_reduce_reference``, in its order: ``h_t = -sum_c plogp(p_c)`` in class order, ``S = p`` and
    ``E = h_0`` for t == 0 and ``S += p``, ``E += h_t`` after, ``m = S * float32(1 / T)``, the arg-max as the lowest index among
    equal maxima, ``entropy = -sum_c plogp(m_c)`` and ``mutual_info = max(entropy - E * float32(1 / T), 0)``.  So
    ``mean_probs`` and ``argmax`` equal the kernel's bit for bit; ``dtype=np.float64`` is for the entropy checks."""
    p = np.asarray(probs_stack, dtype=np.float32)
    views = tuple(int(v) for v in views)
    if p.ndim != 5 or not 1 <= p.shape[0] <= len(TTA_VIEWS) or len(views) != p.shape[0]:
        raise ValueError("tta_reduce_reference: need a (T, n, H, W, C) stack with T in 1..4 and one view code per sample")
    return mc_reduce_reference(np.stack([flip_reference(p[t], v) for t, v in enumerate(views)]), dtype)


PAD_MODES = ("edge", "reflect", "constant")


def check_pad_mode(pad_mode, pad_value=0):
    """The public ``pad_mode`` / ``pad_value`` pair, validated: ``(None | "edge" | "reflect" | "constant", float)``.
    Anything else is a ``ValueError``."""
    if pad_mode is not None and pad_mode not in PAD_MODES:
        raise ValueError(f'pad_mode must be None, "edge", "reflect" or "constant", not {pad_mode!r}')
    try:
        value = float(pad_value)
    except (TypeError, ValueError):
        raise ValueError(f"pad_value must be a number, not {pad_value!r}") from None
    if not np.isfinite(value):
        raise ValueError(f"pad_value must be finite, not {pad_value!r}")
    return pad_mode, value


def padded_geometry(H: int, W: int, pool_layers: int) -> Tuple[int, int, int, int]:
    """``(Hp, Wp, top, left)``: the smallest multiples of 2^pool_layers that hold an H x W scan, and where the scan sits in
    them.  THE placement rule: ``top = (Hp - H) // 2``, ``left = (Wp - W) // 2`` -- the odd pixel goes to the bottom / right."""
    m = 1 << int(pool_layers)
    Hp, Wp = -(-int(H) // m) * m, -(-int(W) // m) * m
    return Hp, Wp, (Hp - int(H)) // 2, (Wp - int(W)) // 2


def pad_reference(x, Hp: int, Wp: int, top: int, left: int, mode: str, value=0) -> np.ndarray:
    """``oct_pad_batch`` (include/oct_unet.h) restated with index arrays: (B,H,W,ch) of any dtype -> (B,Hp,Wp,ch) with the
    input at (top, left); ``edge`` clamps the index, ``reflect`` mirrors it about the border pixel without repeating it,
    ``constant`` writes ``value`` (cast to the input's dtype) outside.  Equal to ``np.pad`` of the two image axes."""
    x = np.asarray(x)
    B, H, W = x.shape[:3]
    if mode not in PAD_MODES:
        raise ValueError(f"pad_reference: unknown mode {mode!r}")
    if top < 0 or left < 0 or top + H > Hp or left + W > Wp:
        raise ValueError("pad_reference: the image does not fit")

    def index(n_out, n, off):
        i = np.arange(n_out) - off
        if mode == "edge":
            return np.clip(i, 0, n - 1), np.ones(n_out, bool)
        if mode == "reflect":
            if off >= n or n_out - off - n >= n:
                raise ValueError("pad_reference: reflect needs every pad smaller than the dimension")
            return np.where(i < 0, -i, np.where(i >= n, 2 * (n - 1) - i, i)), np.ones(n_out, bool)
        return np.clip(i, 0, n - 1), (i >= 0) & (i < n)

    (iy, oky), (ix, okx) = index(Hp, H, top), index(Wp, W, left)
    out = x[:, iy][:, :, ix]
    if mode == "constant":
        inside = oky[:, None] & okx[None, :]
        out[:, ~inside] = np.asarray(value).astype(x.dtype)
    return np.ascontiguousarray(out)


def crop_reference(t, H: int, W: int, top: int, left: int) -> np.ndarray:
    """``oct_crop_batch`` restated: the (B,H,W,...) window at (top, left) of a (B,Hp,Wp,...) array, contiguous."""
    t = np.asarray(t)
    if top < 0 or left < 0 or top + H > t.shape[1] or left + W > t.shape[2]:
        raise ValueError("crop_reference: the window does not fit")
    return np.ascontiguousarray(t[:, top:top + H, left:left + W])


def entropy_to_u8(entropy, num_classes: int) -> np.ndarray:
    """Predictive entropy (nats) -> uint8 gray levels for ``uncertainty_map.png``: floor(min(entropy / ln C, 1) * 255 + 0.5),
    so 255 is the entropy of the uniform distribution over the ``num_classes`` classes."""
    e = np.asarray(entropy, dtype=np.float64) / np.log(float(num_classes))
    return np.floor(np.minimum(e, 1.0) * 255.0 + 0.5).astype(np.uint8)


def create_area_mask(image_shape: tuple, segs) -> np.ndarray:
    """Boundaries -> stacked-region mask (dataset_construction.py:654-708, channels_last).  ``image_shape`` is
    (width, height[, channels]) of the TRANSPOSED image the graph search works on; regions do not include the
    boundary pixel that ends them."""
    mask_shape = image_shape[:-1] if len(image_shape) == 3 else image_shape
    mask = np.zeros(mask_shape, dtype="uint8")
    image_width, image_height = mask_shape[0], mask_shape[1]
    if len(image_shape) == 3:
        mask = np.expand_dims(mask, axis=-1)
    segs = np.array(segs)
    for col in range(image_width):
        for seg_ind in range(len(segs)):
            seg = segs[seg_ind, col]
            if np.isnan(seg) or seg == 0:
                found_rep = False
                for rep_ind in range(seg_ind + 1, len(segs)):
                    rep_seg = segs[rep_ind, col]
                    if not np.isnan(rep_seg) and not rep_seg == 0:
                        found_rep = True
                        segs[seg_ind, col] = rep_seg
                        break
                if found_rep is False:
                    segs[seg_ind, col] = image_height
        for seg_ind in range(len(segs)):
            cur_seg = segs[seg_ind, col]
            if seg_ind == 0:
                mask[col, 0:cur_seg] = seg_ind
            else:
                mask[col, segs[seg_ind - 1, col]:cur_seg] = seg_ind
        mask[col, segs[len(segs) - 1, col]:] = len(segs)
    return mask


def labels_from_delineations(image_shape_t: tuple, segs, num_classes: int) -> Tuple[np.ndarray, np.ndarray]:
    """Graph-search delineations (C-1, W) -> the class map they enclose, (H, W), and its categorical form
    (1, C, W, H) in the transposed frame the search works in (evaluation.py:317-333, prediction.py:145-158).
    ``image_shape_t`` is the shape of the TRANSPOSED image, as for ``create_area_mask``."""
    mask = create_area_mask(image_shape_t, segs)
    labels_t, categorical = perform_argmax(np.expand_dims(to_categorical(mask, num_classes), axis=0))
    return np.transpose(np.squeeze(labels_t)), categorical


ORDERED_MIN_CLASSES, ORDERED_MAX_CLASSES, ORDERED_MAX_H = 2, 16, 4096      # what oct_ordered_decode accepts
ORDERED_ONE = 1 << 20                                                      # its quantisation scale


def ordered_decode_reference(probs) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """``oct_ordered_decode`` restated (include/oct_unet.h): class probabilities (B,H,W,C) float32, class index == depth
    order -> ``(labels (B,H,W) uint8, rows (B,C-1,W) uint16, score (B,W) uint32)``.  Per column, with rows r = 0..H-1:

        q        = p > 0 ? min(p, 1) : 0                          (NaN -> 0)
        k[r][c]  = min((uint32) floor(q * 2^20), 2^20 - 1)
        F[r][c]  = k[r][c] + M[r-1][c],   M[-1][c] = 0
        M[r][0]  = F[r][0],  s[r][0] = 1
        M[r][c]  = F[r][c] if F[r][c] > M[r][c-1] (s[r][c] = 1) else M[r][c-1] (s[r][c] = 0)
        back-trace: c = C-1;  for r = H-1 down to 0:  while (c > 0 && !s[r][c]) c--;  label[r] = c
        score    = M[H-1][C-1]
        rows[i]  = number of rows with label <= i,  i = 0..C-2

    the labelling that maximises sum_r k[r][label[r]] among those that never decrease with r; of several, the one that is
    smallest when compared from the bottom row upward.  Integers throughout: the kernel gives the same bits."""
    p = np.asarray(probs, dtype=np.float32)
    if p.ndim != 4:
        raise ValueError(f"ordered_decode_reference: probs must be (B,H,W,C), not {p.shape}")
    B, H, W, Cn = p.shape
    if min(B, H, W) < 1 or not ORDERED_MIN_CLASSES <= Cn <= ORDERED_MAX_CLASSES or H > ORDERED_MAX_H or B * H * W >= 1 << 31:
        raise ValueError(f"ordered_decode_reference: need B, H, W >= 1, H <= {ORDERED_MAX_H}, B*H*W < 2^31 and "
                         f"{ORDERED_MIN_CLASSES} <= C <= {ORDERED_MAX_CLASSES}, not {p.shape}")
    with np.errstate(invalid="ignore"):
        q = np.where(p > 0, np.minimum(p, np.float32(1)), np.float32(0)).astype(np.float32)
    k = np.minimum(np.floor(q * np.float32(ORDERED_ONE)).astype(np.uint32), np.uint32(ORDERED_ONE - 1))
    M = np.zeros((B, W, Cn), np.uint32)
    s = np.zeros((H, B, W, Cn), bool)
    for r in range(H):
        F = k[:, r] + M
        M = np.empty_like(F)
        M[..., 0], s[r, ..., 0] = F[..., 0], True
        for c in range(1, Cn):
            take = F[..., c] > M[..., c - 1]
            s[r, ..., c] = take
            M[..., c] = np.where(take, F[..., c], M[..., c - 1])
    score = M[..., Cn - 1].copy()
    c = np.full((B, W), Cn - 1, np.int64)
    labels = np.empty((B, H, W), np.uint8)
    for r in range(H - 1, -1, -1):
        for _ in range(Cn - 1):                    # the while loop, for every column at once
            c = c - ((c > 0) & ~np.take_along_axis(s[r], c[..., None], axis=-1)[..., 0])
        labels[:, r] = c
    rows = np.stack([(labels <= i).sum(axis=1) for i in range(Cn - 1)], axis=1).astype(np.uint16)
    return labels, rows, score


COMPONENTS_MAX_CLASSES, COMPONENTS_MAX_BATCH = 32, 65535                   # what oct_components / oct_component_filter accept
COMPONENTS_FILL_CONSTANT, COMPONENTS_FILL_COLUMN = 0, 1                    # oct_component_rule.fill_mode


def _components_check(name: str, labels, n_cls: int) -> np.ndarray:
    lab = np.asarray(labels)
    if lab.ndim != 3 or lab.dtype != np.uint8:
        raise ValueError(f"{name}: labels must be (B,H,W) uint8, not {lab.dtype} {lab.shape}")
    B, H, W = lab.shape
    if not 1 <= B <= COMPONENTS_MAX_BATCH or min(H, W) < 1 or B * H * W >= 1 << 31:
        raise ValueError(f"{name}: need 1 <= B <= {COMPONENTS_MAX_BATCH}, H, W >= 1 and B*H*W < 2^31, not {lab.shape}")
    if not 1 <= int(n_cls) <= COMPONENTS_MAX_CLASSES:
        raise ValueError(f"{name}: need 1 <= n_cls <= {COMPONENTS_MAX_CLASSES}, not {n_cls}")
    return lab


def components_reference(labels, n_cls: int, connectivity: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """``oct_components`` restated (include/oct_unet.h): a class map (B,H,W) uint8 -> ``(root (B,H,W) uint32, size (B,H,W)
    uint32, stats (B,n_cls,2) uint32)``.

        neighbours   two pixels of ONE image with |dy| + |dx| == 1 (connectivity 4) or max(|dy|, |dx|) == 1 (connectivity 8)
        component    a maximal set of pixels of equal byte value joined by chains of neighbours; any byte value forms
                     components, n_cls bounds only the statistics
        root[b,y,x]  the smallest y*W + x over the pixel's component
        size[b,y,x]  the pixel count of the component at its root pixel, 0 at every other pixel
        stats[b,c]   (number of components of class c in image b, pixels of the largest one), (0, 0) when the class is absent

    The roots are found as the kernels find them -- parents that only ever decrease, the larger of two roots hung under the
    smaller -- but for all pixel pairs at once: hang, jump every pointer to its root, repeat until no pair of neighbours has
    two roots.  The answer does not depend on the order.  Integers throughout: the kernels give the same bits."""
    lab = _components_check("components_reference", labels, n_cls)
    if connectivity not in (4, 8):
        raise ValueError(f"components_reference: connectivity must be 4 or 8, not {connectivity}")
    B, H, W = lab.shape
    idx = np.arange(H * W, dtype=np.int64).reshape(H, W)
    steps = [(0, 1), (1, 0)] + ([(1, 1), (1, -1)] if connectivity == 8 else [])
    root = np.empty((B, H, W), np.uint32)
    size = np.zeros((B, H, W), np.uint32)
    stats = np.zeros((B, int(n_cls), 2), np.uint32)
    for b in range(B):
        pairs = []
        for dy, dx in steps:                       # (y, x) and (y + dy, x + dx), both inside, equal bytes
            ys, xs = slice(0, H - dy), slice(max(0, -dx), W - max(0, dx))
            yt, xt = slice(dy, H), slice(max(0, dx), W + min(0, dx))
            same = lab[b, ys, xs] == lab[b, yt, xt]
            pairs.append((idx[ys, xs][same], idx[yt, xt][same]))
        pa, pb = np.concatenate([p[0] for p in pairs]), np.concatenate([p[1] for p in pairs])
        par = np.arange(H * W, dtype=np.int64)
        while True:
            while True:                            # every pointer to its root
                nxt = par[par]
                if np.array_equal(nxt, par):
                    break
                par = nxt
            ra, rb = par[pa], par[pb]
            differ = ra != rb
            if not differ.any():
                break
            np.minimum.at(par, np.maximum(ra, rb)[differ], np.minimum(ra, rb)[differ])
        root[b] = par.reshape(H, W)
        counts = np.bincount(par, minlength=H * W)
        is_root = par == np.arange(H * W)
        size[b] = np.where(is_root, counts, 0).reshape(H, W)
        cls = lab[b].reshape(-1)[is_root]
        for c in range(int(n_cls)):
            s = counts[is_root][cls == c]
            if s.size:
                stats[b, c] = (s.size, s.max())
    return root, size, stats


def component_filter_reference(labels, root, size, n_cls: int, rule) -> Tuple[np.ndarray, np.ndarray]:
    """``oct_component_filter`` restated (include/oct_unet.h): the class map, the ``root`` and ``size`` of
    ``components_reference`` and a rule -- anything with the fields of ``oct_component_rule``: ``min_pixels`` (a value per
    class), ``keep_largest`` (bit c), ``fill_mode`` (0 constant, 1 column), ``fill_label`` -> ``(labels_out (B,H,W) uint8,
    removed (B,n_cls) uint32)``.

        removed      a pixel of class c < n_cls with root r, if size[r] < min_pixels[c], or if bit c of keep_largest is set and r
                     is not the best root of (b, c): the component of class c with the most pixels, among equals the one with
                     the smallest root.  Pixels with a label >= n_cls are never removed.
        kept         a kept pixel keeps its byte
        fill mode 0  a removed pixel gets fill_label
        fill mode 1  a removed pixel gets the label of the nearest pixel ABOVE it in its column that is kept and has a label
                     < n_cls; if there is none, that of the nearest such pixel below it; if there is none, fill_label
        removed[b,c] the removed pixels whose original class is c

    One pass, not idempotent."""
    lab = _components_check("component_filter_reference", labels, n_cls)
    n_cls = int(n_cls)
    B, H, W = lab.shape
    root, size = np.asarray(root), np.asarray(size)
    if root.shape != lab.shape or size.shape != lab.shape:
        raise ValueError("component_filter_reference: root and size must have the shape of labels")
    min_pixels = [int(v) for v in list(rule.min_pixels)[:n_cls]]
    keep, mode, fill = int(rule.keep_largest), int(rule.fill_mode), int(rule.fill_label)
    if len(min_pixels) < n_cls or mode not in (0, 1) or not 0 <= fill <= 255 or keep >> n_cls:
        raise ValueError("component_filter_reference: the rule needs n_cls min_pixels, fill_mode 0..1, fill_label 0..255 and "
                         "no keep_largest bit at or above n_cls")
    gone = np.zeros(lab.shape, bool)
    removed = np.zeros((B, n_cls), np.uint32)
    for b in range(B):
        r = root[b].reshape(-1).astype(np.int64)
        s = size[b].reshape(-1).astype(np.int64)
        l = lab[b].reshape(-1)
        roots = np.flatnonzero(s)
        for c in range(n_cls):
            of_c = l == c
            g = of_c & (s[r] < min_pixels[c])
            if (keep >> c) & 1:
                rc = roots[l[roots] == c]
                if rc.size:
                    best = rc[np.lexsort((rc, -s[rc]))[0]]         # most pixels, then the smallest root
                    g |= of_c & (r != best)
            gone[b] |= g.reshape(H, W)
            removed[b, c] = g.sum()
    out = lab.copy()
    if mode == COMPONENTS_FILL_CONSTANT:
        out[gone] = fill
        return out, removed
    source = ~gone & (lab < n_cls)
    above = np.full((B, H, W), -1, np.int64)                       # the label of the nearest source above, or -1
    below = np.full((B, H, W), -1, np.int64)
    cur = np.full((B, W), -1, np.int64)
    for y in range(H):
        above[:, y] = cur
        cur = np.where(source[:, y], lab[:, y], cur)
    cur = np.full((B, W), -1, np.int64)
    for y in range(H - 1, -1, -1):
        below[:, y] = cur
        cur = np.where(source[:, y], lab[:, y], cur)
    filled = np.where(above >= 0, above, np.where(below >= 0, below, fill))
    return np.where(gone, filled, lab).astype(np.uint8), removed


# ---- edge weight maps: the table, the spec check and the numpy restatement of oct_edge_weight_map (include/oct_unet.h) ----
EDGE_WEIGHT_MAX_RADIUS = 32
EDGE_WEIGHT_PROFILES = ("box", "gauss", "linear")


def check_edge_weight(spec) -> dict:
    """The validated spec ``{"radius", "weight", "profile", "sigma"}`` of a boundary-weighted pixel loss (``edge_weight=`` of
    ``focal_dice_loss`` / ``bce_dice_loss``): ``radius`` an integer in 1..32, ``weight`` finite and >= 0, ``profile`` one of
    ``"box"`` [default], ``"gauss"``, ``"linear"``, ``sigma`` > 0 (``"gauss"`` only; default ``radius / 2``).  ``ValueError``
    outside that, and for unknown keys."""
    if not isinstance(spec, dict):
        raise ValueError(f"edge_weight must be a dict with the keys radius, weight, profile, sigma, not {spec!r}")
    unknown = sorted(set(spec) - {"radius", "weight", "profile", "sigma"})
    if unknown:
        raise ValueError(f"edge_weight: unknown keys {unknown}")
    if "radius" not in spec or "weight" not in spec:
        raise ValueError("edge_weight needs radius and weight")
    radius, weight, profile, sigma = spec["radius"], spec["weight"], spec.get("profile", "box"), spec.get("sigma")
    if isinstance(radius, bool) or not isinstance(radius, (int, np.integer)) or not 1 <= int(radius) <= EDGE_WEIGHT_MAX_RADIUS:
        raise ValueError(f"edge_weight: radius must be an integer in 1..{EDGE_WEIGHT_MAX_RADIUS}, not {radius!r}")
    try:
        weight = float(weight)
    except (TypeError, ValueError):
        raise ValueError(f"edge_weight: weight must be a number, not {weight!r}") from None
    if not (np.isfinite(weight) and weight >= 0.0):
        raise ValueError(f"edge_weight: weight must be finite and >= 0, not {weight}")
    if profile not in EDGE_WEIGHT_PROFILES:
        raise ValueError(f"edge_weight: profile must be one of {EDGE_WEIGHT_PROFILES}, not {profile!r}")
    if profile == "gauss":
        try:
            sigma = float(radius) / 2.0 if sigma is None else float(sigma)
        except (TypeError, ValueError):
            raise ValueError(f"edge_weight: sigma must be a number, not {sigma!r}") from None
        if not (np.isfinite(sigma) and sigma > 0.0):
            raise ValueError(f"edge_weight: sigma must be finite and > 0, not {sigma}")
    elif sigma is not None:
        raise ValueError(f'edge_weight: sigma belongs to profile "gauss", not {profile!r}')
    return {"radius": int(radius), "weight": weight, "profile": profile, "sigma": sigma}


def edge_weight_lut(radius: int, profile: str, weight: float, sigma=None) -> np.ndarray:
    """The table of ``oct_edge_weight_map``: float32 ``[R^2 + 2]``, entry ``d2`` = the weight at squared distance ``d2`` from
    the nearest class border, entry ``R^2 + 1`` ("far") = 1.  With ``d = sqrt(d2) <= R``:
    ``"box"`` ``1 + weight`` (ReLayNet's ``1 + omega [x near a boundary]``); ``"gauss"`` ``1 + weight exp(-d^2 / (2 sigma^2))``
    (the U-Net paper); ``"linear"`` ``1 + weight (1 - d / (R + 1))``.  Computed in fp64 and cast once."""
    s = check_edge_weight({"radius": radius, "weight": weight, "profile": profile, "sigma": sigma})
    R, w = s["radius"], s["weight"]
    d2 = np.arange(R * R + 1, dtype=np.float64)
    if s["profile"] == "box":
        v = np.full_like(d2, 1.0 + w)
    elif s["profile"] == "gauss":
        v = 1.0 + w * np.exp(-d2 / (2.0 * s["sigma"] ** 2))
    else:
        v = 1.0 + w * (1.0 - np.sqrt(d2) / (R + 1.0))
    return np.concatenate([v, [1.0]]).astype(np.float32)


def edge_index_reference(labels, n_cls: int, radius: int) -> np.ndarray:
    """``idx`` of ``oct_edge_weight_map`` by its definition: int64 (B,H,W), the least ``dx^2 + dy^2 <= R^2`` to an edge pixel
    of the same image, ``R^2 + 1`` where there is none; and ``-1`` at an unknown pixel (label >= n_cls).  An edge pixel is a
    known pixel with a known 4-neighbour inside the image of another label.  Separable, as the kernel: vertical distance per
    column first, then the minimum over the row."""
    lab = np.asarray(labels)
    if lab.ndim == 4 and lab.shape[-1] == 1:
        lab = lab[..., 0]
    if lab.ndim != 3 or lab.dtype != np.uint8:
        raise ValueError("edge_weight_reference: labels must be uint8 (B,H,W) or (B,H,W,1)")
    R = int(radius)
    if not 1 <= R <= EDGE_WEIGHT_MAX_RADIUS or not 1 <= int(n_cls) <= 255:
        raise ValueError("edge_weight_reference: radius must be in 1..32 and n_cls in 1..255")
    B, H, W = lab.shape
    L = lab.astype(np.int64)
    known = L < n_cls
    edge = np.zeros(L.shape, bool)
    for sl_a, sl_b in (((slice(None), slice(1, None)), (slice(None), slice(None, -1))),        # vertical neighbours
                       ((slice(None), slice(None), slice(1, None)), (slice(None), slice(None), slice(None, -1)))):
        diff = known[sl_a] & known[sl_b] & (L[sl_a] != L[sl_b])
        edge[sl_a] |= diff
        edge[sl_b] |= diff
    none = 1 << 20
    v = np.full(L.shape, none, np.int64)                    # vertical distance to the nearest edge pixel of the column
    for d in range(min(R, H - 1), -1, -1):                  # (a radius beyond the image: no such neighbour)
        near = np.zeros_like(edge)
        near[:, d:] |= edge[:, :H - d]
        near[:, :H - d] |= edge[:, d:]
        v[near] = d
    far = R * R + 1
    best = np.full(L.shape, far, np.int64)
    v2 = np.where(v == none, none, v * v)
    for dx in range(-min(R, W - 1), min(R, W - 1) + 1):
        cand = np.full(L.shape, none, np.int64)
        if dx >= 0:
            cand[:, :, :W - dx] = v2[:, :, dx:] + dx * dx
        else:
            cand[:, :, -dx:] = v2[:, :, :W + dx] + dx * dx
        best = np.minimum(best, np.where(cand <= R * R, cand, far))
    return np.where(known, best, -1)


def edge_weight_reference(labels, n_cls: int, radius: int, lut) -> np.ndarray:
    """What ``oct_edge_weight_map`` computes: float32 (B,H,W), ``lut[idx]`` at a known pixel (``edge_index_reference``),
    ``0.0`` at an unknown one.  ``lut``: the ``R^2 + 2`` floats of ``edge_weight_lut``."""
    lut = np.asarray(lut, np.float32)
    if lut.shape != (int(radius) ** 2 + 2,):
        raise ValueError(f"edge_weight_reference: lut must have radius^2 + 2 = {int(radius) ** 2 + 2} entries")
    idx = edge_index_reference(labels, n_cls, radius)
    return np.where(idx >= 0, lut[np.maximum(idx, 0)], np.float32(0.0)).astype(np.float32)


# ---- contrast normalisation: the spec check and the numpy restatement of oct_contrast_batch (include/oct_unet.h) ----
CONTRAST_METHODS = ("clahe", "stretch")
CONTRAST_MAX_TILES, CONTRAST_MIN_TILE, CONTRAST_MAX_DIM = 16, 8, 4096
CONTRAST_FILE = "contrast.json"


def check_contrast(spec, hw=None):
    """The validated spec of the contrast stage (``contrast=`` of ``TrainingParams``, ``EvaluationParameters``,
    ``PredictionParams``, ``Model.predict``): ``None`` (off) stays ``None``; else a dict ``{"method": "clahe" | "stretch",
    "tiles": (ty, tx) [default (8, 8), each in 1..16], "clip": None | 0 (no limit) | a float in 1..255.99, in units of the
    uniform bin height ("clahe" only), "percentiles": (lo, hi) in percent with 0 <= lo < hi <= 100 [default (1, 99)]
    ("stretch" only)}``.  Returns a new dict with every key of its method set, ready for ``json.dumps``.  ``hw = (H, W)``
    also checks the image size: ``H, W <= 4096`` and tiles of at least 8 x 8 pixels (``H // ty >= 8``, ``W // tx >= 8``; a
    one-pixel tile would equalise to a constant).  ``ValueError`` outside that, and for unknown keys."""
    if spec is None:
        return None
    if not isinstance(spec, dict):
        raise ValueError(f"contrast must be None or a dict with the keys method, tiles, clip, percentiles, not {spec!r}")
    unknown = sorted(set(spec) - {"method", "tiles", "clip", "percentiles"})
    if unknown:
        raise ValueError(f"contrast: unknown keys {unknown}")
    method = spec.get("method")
    if method not in CONTRAST_METHODS:
        raise ValueError(f"contrast: method must be one of {CONTRAST_METHODS}, not {method!r}")
    tiles = spec.get("tiles", (8, 8))
    try:
        ty, tx = tiles
        bad = any(isinstance(t, bool) or int(t) != t for t in (ty, tx))
    except (TypeError, ValueError):
        bad = True
    if bad or not (1 <= int(ty) <= CONTRAST_MAX_TILES and 1 <= int(tx) <= CONTRAST_MAX_TILES):
        raise ValueError(f"contrast: tiles must be two integers (ty, tx) in 1..{CONTRAST_MAX_TILES}, not {tiles!r}")
    out = {"method": method, "tiles": [int(ty), int(tx)]}
    if method == "clahe":
        if "percentiles" in spec:
            raise ValueError('contrast: percentiles belong to method "stretch", not "clahe"')
        clip = spec.get("clip")
        if clip is not None:
            try:
                clip = float(clip)
            except (TypeError, ValueError):
                raise ValueError(f"contrast: clip must be None, 0 or a number >= 1, not {clip!r}") from None
            if clip == 0.0:
                clip = None
            elif not (np.isfinite(clip) and clip >= 1.0 and round(clip * 256) <= 65535):
                raise ValueError(f"contrast: clip must be None, 0 (no limit) or in 1..255.99 (units of the uniform bin height), not {clip}")
        out["clip"] = clip
    else:
        if "clip" in spec:
            raise ValueError('contrast: clip belongs to method "clahe", not "stretch"')
        pct = spec.get("percentiles", (1, 99))
        try:
            lo, hi = (float(p) for p in pct)
            lo_bp, hi_bp = round(lo * 100), round(hi * 100)
        except (TypeError, ValueError, OverflowError):
            raise ValueError(f"contrast: percentiles must be two numbers (lo, hi), not {pct!r}") from None
        if not 0 <= lo_bp < hi_bp <= 10000:
            raise ValueError(f"contrast: percentiles need 0 <= lo < hi <= 100 (in steps of 0.01), not {pct!r}")
        out["percentiles"] = [lo, hi]
    if hw is not None:
        H, W = int(hw[0]), int(hw[1])
        if not (1 <= H <= CONTRAST_MAX_DIM and 1 <= W <= CONTRAST_MAX_DIM):
            raise ValueError(f"contrast: images of {H} x {W}: H and W must be in 1..{CONTRAST_MAX_DIM}")
        if H // out["tiles"][0] < CONTRAST_MIN_TILE or W // out["tiles"][1] < CONTRAST_MIN_TILE:
            raise ValueError(f"contrast: tiles {tuple(out['tiles'])} on {H} x {W} images leave tiles of {H // out['tiles'][0]} x "
                             f"{W // out['tiles'][1]} pixels: need at least {CONTRAST_MIN_TILE} x {CONTRAST_MIN_TILE}")
    return out


def contrast_desc(spec) -> Tuple[int, int, int, int, int, int]:
    """The integers of ``oct_contrast_desc`` for a spec: ``(method, tiles_y, tiles_x, clip_q8, lo_bp, hi_bp)`` with
    ``clip_q8 = round(clip * 256)`` (0 = no limit) and the percentiles in basis points."""
    s = check_contrast(spec)
    if s is None:
        raise ValueError("contrast_desc: the spec is None (off)")
    ty, tx = s["tiles"]
    if s["method"] == "clahe":
        return 0, ty, tx, 0 if s["clip"] is None else int(round(s["clip"] * 256)), 0, 0
    lo, hi = s["percentiles"]
    return 1, ty, tx, 0, int(round(lo * 100)), int(round(hi * 100))


def read_contrast_file(model_path):
    """The spec in ``contrast.json`` beside the checkpoint ``model_path`` (written by ``train_model(contrast=)``), validated;
    ``None`` when there is no such file."""
    path = Path(model_path).parent / CONTRAST_FILE
    if not path.is_file():
        return None
    with open(path, "r") as f:
        return check_contrast(json.load(f))


def resolve_contrast(contrast, model_path):
    """What ``contrast=`` of ``EvaluationParameters`` / ``PredictionParams`` means for the checkpoint ``model_path``: a dict
    is validated, ``"model"`` reads ``contrast.json`` beside the checkpoint (``ValueError`` if it is absent), ``None`` stays
    off -- with one warning if the model was trained with a ``contrast.json``."""
    if isinstance(contrast, str):
        if contrast != "model":
            raise ValueError(f'contrast must be None, a dict or "model", not {contrast!r}')
        spec = read_contrast_file(model_path)
        if spec is None:
            raise ValueError(f'contrast="model": no {CONTRAST_FILE} beside {model_path}')
        return spec
    if contrast is None and model_path is not None and (Path(model_path).parent / CONTRAST_FILE).is_file():
        log.warning(f"{Path(model_path).parent / CONTRAST_FILE} says the model was trained on contrast-normalised scans, but "
                    'contrast is None: the scans are used as given (contrast="model" applies the file)')
    return check_contrast(contrast)


def _contrast_input(x, spec, what: str):
    x = np.asarray(x)
    if x.dtype != np.uint8 or x.ndim != 4 or not 1 <= x.shape[3] <= 4 or x.shape[0] < 1:
        raise ValueError(f"{what}: x must be uint8 (B,H,W,ch) with ch in 1..4 and B >= 1, not {x.dtype} {x.shape}")
    return x, check_contrast(spec, hw=x.shape[1:3]), contrast_desc(spec)


def _contrast_axis(n: int, t: int):
    """Cell, next cell, weight of the next cell and span of every position of an axis of ``n`` pixels in ``t`` tiles."""
    e = (np.arange(t + 1, dtype=np.int64) * n) // t
    if t == 1:
        z = np.zeros(n, np.int64)
        return z, z, z, np.ones(n, np.int64)
    cen = e[:-1] + e[1:] - 1                                   # twice the tile centres
    pos = 2 * np.arange(n, dtype=np.int64)
    r = np.clip(np.searchsorted(cen, pos, side="right") - 1, 0, t - 2)
    D = cen[r + 1] - cen[r]
    return r, r + 1, np.clip(pos - cen[r], 0, D), D


def contrast_luts_reference(x, spec) -> np.ndarray:
    """The look-up tables of ``oct_contrast_batch`` by its definition (include/oct_unet.h): uint8 ``(B, ch, ty, tx, 256)``
    for uint8 ``x`` (B,H,W,ch).  Integers only: the kernel leaves the same bytes at the head of its workspace."""
    x, s, (method, ty, tx, clip_q8, lo_bp, hi_bp) = _contrast_input(x, spec, "contrast_luts_reference")
    B, H, W, ch = x.shape
    ey, ex = (np.arange(ty + 1) * H) // ty, (np.arange(tx + 1) * W) // tx
    luts = np.empty((B, ch, ty, tx, 256), np.uint8)
    slots = (np.arange(B * ch, dtype=np.int64) * 256)[:, None]
    i = np.arange(256, dtype=np.int64)
    for r in range(ty):
        for c in range(tx):
            tile = x[:, ey[r]:ey[r + 1], ex[c]:ex[c + 1], :]
            A = int(tile.shape[1] * tile.shape[2])
            flat = tile.reshape(B, A, ch).transpose(0, 2, 1).reshape(B * ch, A).astype(np.int64)
            h = np.bincount((flat + slots).ravel(), minlength=B * ch * 256).reshape(B * ch, 256).astype(np.int64)
            if method == 0:
                L = A if clip_q8 == 0 else max(1, (clip_q8 * A) >> 16)
                E = np.maximum(h - L, 0).sum(axis=1, keepdims=True)
                rem = E % 256
                h = np.minimum(h, L) + E // 256 + ((((i + 1) * rem) // 256) > ((i * rem) // 256))
                lut = (np.cumsum(h, axis=1) * 255 + A // 2) // A
            else:
                cum = np.cumsum(h, axis=1)
                v_lo = (cum <= (lo_bp * A) // 10000).sum(axis=1, keepdims=True)       # cum never decreases
                v_hi = (cum * 10000 < hi_bp * A).sum(axis=1, keepdims=True)
                span = np.maximum(v_hi - v_lo, 1)
                lut = np.where(i <= v_lo, 0, np.where(i >= v_hi, 255, ((i - v_lo) * 255 + span // 2) // span))
                lut = np.where(v_hi <= v_lo, i, lut)
            luts[:, :, r, c, :] = lut.reshape(B, ch, 256).astype(np.uint8)
    return luts


def contrast_reference(x, spec, luts=None) -> np.ndarray:
    """What ``oct_contrast_batch`` computes: uint8 ``x`` (B,H,W,ch) -> the same shape, every byte mapped through the
    look-up tables of the four tiles around it (``contrast_luts_reference``; ``luts``: those, if already computed) and
    blended bilinearly between the tile centres, in integers."""
    x, s, (method, ty, tx, *_) = _contrast_input(x, spec, "contrast_reference")
    B, H, W, ch = x.shape
    r, r1, ay, Dy = (a[None, :, None, None] for a in _contrast_axis(H, ty))
    c, c1, ax, Dx = (a[None, None, :, None] for a in _contrast_axis(W, tx))
    ci = np.arange(ch)[None, None, None, :]
    out = np.empty_like(x)
    for b0 in range(0, B, 16):          # in chunks: the int64 intermediates are eight times the batch
        xb = x[b0:b0 + 16]
        lb = contrast_luts_reference(xb, spec) if luts is None else np.asarray(luts)[b0:b0 + 16]
        bi = np.arange(xb.shape[0])[:, None, None, None]
        v = xb.astype(np.int64)
        v00, v01 = lb[bi, ci, r, c, v].astype(np.int64), lb[bi, ci, r, c1, v].astype(np.int64)
        v10, v11 = lb[bi, ci, r1, c, v].astype(np.int64), lb[bi, ci, r1, c1, v].astype(np.int64)
        num = (Dy - ay) * ((Dx - ax) * v00 + ax * v01) + ay * ((Dx - ax) * v10 + ax * v11) + (Dy * Dx) // 2
        out[b0:b0 + 16] = (num // (Dy * Dx)).astype(np.uint8)
    return out


def contrast_images(images_u8, spec, device=None, chunk: int = 64) -> np.ndarray:
    """A whole dataset array uint8 (N,H,W,ch) through the contrast stage -> a new array of the same shape.  With a GPU
    (``device``: a torch device or its name; default: the current GPU if there is one) the images go through
    ``oct_contrast_batch`` in chunks of ``chunk`` over pinned staging buffers; without one through ``contrast_reference``.
    Both give the same bytes.  ``spec`` None returns the input."""
    if spec is None:
        return images_u8
    x, s, _ = _contrast_input(images_u8, spec, "contrast_images")
    import torch
    if device is None and not torch.cuda.is_available():
        return contrast_reference(x, s)
    from .. import _hip
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if dev.type != "cuda":
        raise ValueError(f"contrast_images: device must be a GPU or None, not {device!r}")
    N = x.shape[0]
    chunk = max(1, min(int(chunk), N, 65535))
    d = _hip.ContrastDesc(*contrast_desc(s))
    import ctypes as C
    need = int(_hip.lib().oct_contrast_workspace_bytes(chunk, x.shape[1], x.shape[2], x.shape[3], C.byref(d)))
    if not need:
        raise _hip.OctError(f"contrast_images: refused: {_hip.lib().oct_last_error().decode()}")
    out = np.empty_like(x)
    with torch.cuda.device(dev):
        stage = [torch.empty((chunk,) + x.shape[1:], dtype=torch.uint8).pin_memory() for _ in range(2)]
        on_dev = [torch.empty((chunk,) + x.shape[1:], dtype=torch.uint8, device=dev) for _ in range(2)]
        done = [None, None]
        ws = torch.empty((need,), dtype=torch.uint8, device=dev)
        for k, n0 in enumerate(range(0, N, chunk)):
            n, s_ = min(chunk, N - n0), k % 2
            if done[s_] is not None:                      # the slot's previous chunk has landed: take it out, refill
                done[s_][0].synchronize()
                out[done[s_][1]:done[s_][1] + done[s_][2]] = stage[s_][:done[s_][2]].numpy()
            stage[s_][:n].copy_(torch.from_numpy(np.ascontiguousarray(x[n0:n0 + n])))
            on_dev[s_][:n].copy_(stage[s_][:n], non_blocking=True)
            _hip.call("oct_contrast_batch", dev, on_dev[s_].data_ptr(), n, x.shape[1], x.shape[2], x.shape[3], C.byref(d),
                      ws.data_ptr(), ws.numel(), on_dev[s_].data_ptr(), _hip.stream_ptr(dev))
            stage[s_][:n].copy_(on_dev[s_][:n], non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
            done[s_] = (ev, n0, n)
        for s_ in (0, 1):
            if done[s_] is not None:
                done[s_][0].synchronize()
                out[done[s_][1]:done[s_][1] + done[s_][2]] = stage[s_][:done[s_][2]].numpy()
    return out
