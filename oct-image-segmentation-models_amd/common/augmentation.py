"""Augmentation functions with the reference's names, signatures and registry
(oct_image_segmentation_models/common/augmentation.py:43-103).

``flip`` is exact.  ``add_noise`` follows the documented semantics of ``skimage.util.random_noise`` (third-party,
not installed here: parity with skimage's RNG stream is unpinned) for the modes gaussian / speckle / s&p / salt /
pepper on images in [0, 1]; the result is clipped to [0, 1] as skimage does for unsigned input."""
from __future__ import annotations

import numpy as np

_rng = np.random.default_rng()


def seed(value) -> None:
    """Seed the module RNG used by ``add_noise`` (the reference is unseeded)."""
    global _rng
    _rng = np.random.default_rng(value)


def no_aug(image, mask, _aug_args, desc_only=False):
    if desc_only is False:
        return image, mask
    return "no aug"


def flip_aug(image, mask, aug_args, desc_only=False):
    flip_type = aug_args["flip_type"]
    if flip_type == "up-down":
        axis = 0
    elif flip_type == "left-right":
        axis = 1
    else:
        raise ValueError(f"flip_type must be 'up-down' or 'left-right', got {flip_type!r}")
    if desc_only is False:
        aug_image = np.flip(image, axis=axis)
        aug_mask = np.flip(mask, axis=axis) if mask is not None else None
        return aug_image, aug_mask
    return "flip aug: " + flip_type


def add_noise_aug(image, mask, aug_args, desc_only=False):
    if desc_only is not False:
        return "add noise: " + str(aug_args)
    mode = aug_args["mode"]
    mean = aug_args.get("mean", 0.0)
    var = aug_args.get("variance", 0.01)
    img = np.asarray(image, dtype=np.float64)
    if mode == "gaussian":
        out = img + _rng.normal(mean, var ** 0.5, img.shape)
    elif mode == "speckle":
        out = img + img * _rng.normal(mean, var ** 0.5, img.shape)
    elif mode in ("s&p", "salt", "pepper"):
        amount = aug_args.get("amount", 0.05)
        svp = {"s&p": aug_args.get("salt_vs_pepper", 0.5), "salt": 1.0, "pepper": 0.0}[mode]
        out = img.copy()
        flipped = _rng.random(img.shape) <= amount
        salted = _rng.random(img.shape) <= svp
        out[flipped & salted] = 1.0
        out[flipped & ~salted] = 0.0
    else:
        raise ValueError(f"add_noise mode {mode!r} is not supported")
    return np.clip(out, 0.0, 1.0), mask


def _public_args(aug_args):
    return {k: v for k, v in (aug_args or {}).items() if k != "op"}


def column_shift_aug(image, mask, aug_args, desc_only=False):
    """Shift every column of the scan along the depth axis: a random translation, tilt and curvature of the retina
    (``max_shift``, ``max_tilt``, ``max_curvature`` in pixels, each drawn uniformly in [-max, max]; ``border`` "wrap" as
    the reference's ``np.roll`` in ``roll_image_offset``, "replicate" or "constant").  uint8 in, uint8 out; a float image
    in [0, 1] (the generator's host path) is taken as float32(u8 / 255) and returned in that form.  Built on
    ``warp_reference``: the device stage ``oct_warp_batch`` gives the same bytes."""
    if desc_only is not False:
        return "column shift: " + str(_public_args(aug_args))
    return _warp_aug(column_shift_aug, image, mask, aug_args)


def affine_aug(image, mask, aug_args, desc_only=False):
    """Rotate, zoom and translate the scan about its centre, bilinear for the image and nearest for the mask
    (``max_rotation`` in degrees, ``scale_range`` (lo, hi), ``max_translate`` (dx, dy) in pixels, each drawn uniformly;
    ``border`` "replicate", "wrap" or "constant" with ``fill`` / ``fill_label``).  Types as ``column_shift_aug``."""
    if desc_only is not False:
        return "affine: " + str(_public_args(aug_args))
    return _warp_aug(affine_aug, image, mask, aug_args)


augmentation_map = {
    "add_noise": add_noise_aug,
    "affine": affine_aug,
    "column_shift": column_shift_aug,
    "flip": flip_aug,
    "no_augmentation": no_aug,
}


def normalize(x):
    x = np.asarray(x)
    return (x - x.min()) / (np.ptp(x))


# ---- augmentation on the device: descriptors and the numpy restatement of oct_augment_batch (include/oct_unet.h) ----------
# One descriptor per sample; the layout is the C struct oct_aug_op (32 bytes).
AUG_OP_DTYPE = np.dtype([("kind", "<i4"), ("p0", "<f4"), ("p1", "<f4"), ("p2", "<f4"), ("noise_id", "<u8"),
                         ("reserved", "<u8")])
AUG_NONE, AUG_FLIP_UD, AUG_FLIP_LR, AUG_GAUSSIAN, AUG_SPECKLE, AUG_SP = range(6)

_PHILOX_M0, _PHILOX_M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_PHILOX_W0, _PHILOX_W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
_MASK32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter4, key2) -> np.ndarray:
    """Philox4x32-10 (Salmon, Moraes, Dror, Shaw, SC'11; Random123): ``counter4`` (..., 4) and ``key2`` (..., 2) uint32
    words (broadcast against each other) -> (..., 4) uint32 output words."""
    c = np.asarray(counter4, dtype=np.uint64)
    k = np.asarray(key2, dtype=np.uint64)
    shape = np.broadcast_shapes(c.shape[:-1], k.shape[:-1])
    c0, c1, c2, c3 = (np.broadcast_to(c[..., i], shape) for i in range(4))
    k0, k1 = (np.broadcast_to(k[..., i], shape) for i in range(2))
    s32 = np.uint64(32)
    for _ in range(10):
        p0, p1 = _PHILOX_M0 * c0, _PHILOX_M1 * c2            # 32 x 32 -> 64 bit products, exact in uint64
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ k0, p1 & _MASK32, (p0 >> s32) ^ c3 ^ k1, p0 & _MASK32
        k0, k1 = (k0 + _PHILOX_W0) & _MASK32, (k1 + _PHILOX_W1) & _MASK32
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def aug_ops_from(aug_fn_args):
    """Descriptor templates (``AUG_OP_DTYPE`` array, one per augmentation, ``noise_id`` 0) of a list of
    ``(function, arguments)`` pairs, or ``None`` if any of them is not one of ``augmentation_map``'s functions with
    arguments the device implements -- such a list keeps the host path.  A ``column_shift`` / ``affine`` entry is kind 0 here:
    its pixels are moved by the stage in front, whose templates ``warp_ops_from`` gives."""
    ops = np.zeros(len(aug_fn_args), dtype=AUG_OP_DTYPE)
    for j, (fn, args) in enumerate(aug_fn_args):
        args = args or {}
        if fn is no_aug:
            ops[j]["kind"] = AUG_NONE
        elif fn is flip_aug and args.get("flip_type") in ("up-down", "left-right"):
            ops[j]["kind"] = AUG_FLIP_UD if args["flip_type"] == "up-down" else AUG_FLIP_LR
        elif fn is add_noise_aug and args.get("mode") in ("gaussian", "speckle"):
            var = float(args.get("variance", 0.01))
            if not var >= 0.0:
                return None
            ops[j]["kind"] = AUG_GAUSSIAN if args["mode"] == "gaussian" else AUG_SPECKLE
            ops[j]["p0"], ops[j]["p1"] = float(args.get("mean", 0.0)), var ** 0.5
        elif fn is add_noise_aug and args.get("mode") in ("s&p", "salt", "pepper"):
            ops[j]["kind"] = AUG_SP
            ops[j]["p0"] = float(args.get("amount", 0.05))
            ops[j]["p1"] = {"s&p": float(args.get("salt_vs_pepper", 0.5)), "salt": 1.0, "pepper": 0.0}[args["mode"]]
        elif fn in (column_shift_aug, affine_aug):
            try:
                _warp_spec(fn, args)
            except ValueError:
                return None
            ops[j]["kind"] = AUG_NONE      # the warp stage in front (warp_ops_from) moves the pixels; this one converts them
        else:
            return None
    return ops


def device_aug_words(n: int, noise_id: int, seed: int):
    """The two random words (w0, w1) of each of the ``n`` elements of one sample: element e owns words 2(e&1), 2(e&1)+1
    of the Philox block with counter (e >> 1, 0, noise_id low, noise_id high) and key (seed low, seed high)."""
    seed, noise_id = int(seed) & 0xFFFFFFFFFFFFFFFF, int(noise_id) & 0xFFFFFFFFFFFFFFFF
    ctr = np.zeros(((n + 1) // 2, 4), dtype=np.uint64)
    ctr[:, 0] = np.arange((n + 1) // 2, dtype=np.uint64)
    ctr[:, 2], ctr[:, 3] = noise_id & 0xFFFFFFFF, noise_id >> 32
    words = philox4x32_10(ctr, np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64)).reshape(-1)
    return words[0::2][:n], words[1::2][:n]


def device_aug_reference(images_u8, labels_u8, ops, seed, dtype=np.float64):
    """What ``oct_augment_batch`` computes, by its definition in include/oct_unet.h, evaluated in ``dtype`` and cast to
    float32 at the end: ``(x float32 (B,H,W,C), labels uint8)`` (``labels_u8`` may be ``None``, (B,H,W) or (B,H,W,1))."""
    images_u8 = np.asarray(images_u8)
    if images_u8.dtype != np.uint8 or images_u8.ndim != 4:
        raise TypeError("device_aug_reference needs (B,H,W,C) uint8 images")
    ops = np.asarray(ops, dtype=AUG_OP_DTYPE)
    if ops.shape != (images_u8.shape[0],):
        raise ValueError("one descriptor per sample")
    dt = np.dtype(dtype).type
    lut = (np.arange(256, dtype=np.float64) / 255.0).astype(np.float32)
    x = np.empty(images_u8.shape, dtype=np.float32)
    labels = None if labels_u8 is None else np.array(labels_u8, dtype=np.uint8)
    sample_shape = images_u8.shape[1:]
    n = int(np.prod(sample_shape))
    for b, op in enumerate(ops):
        kind = int(op["kind"]) if 0 <= int(op["kind"]) <= AUG_SP else AUG_NONE
        img = lut[images_u8[b]]
        if kind in (AUG_FLIP_UD, AUG_FLIP_LR):
            axis = 0 if kind == AUG_FLIP_UD else 1
            x[b] = np.flip(img, axis=axis)
            if labels is not None:
                labels[b] = np.flip(labels[b], axis=axis)
            continue
        if kind == AUG_NONE:
            x[b] = img
            continue
        w0, w1 = device_aug_words(n, op["noise_id"], seed)
        w0, w1 = w0.reshape(sample_shape), w1.reshape(sample_shape)
        two_m24 = dt(2.0 ** -24)
        u2 = (w1 >> np.uint32(8)).astype(dt) * two_m24
        if kind == AUG_SP:
            u1 = (w0 >> np.uint32(8)).astype(dt) * two_m24
            flipped, salted = u2 <= dt(op["p0"]), u1 <= dt(op["p1"])
            x[b] = np.where(flipped, np.where(salted, np.float32(1.0), np.float32(0.0)), img)
            continue
        u1 = ((w0 >> np.uint32(8)).astype(np.uint64) + np.uint64(1)).astype(dt) * two_m24
        z = np.sqrt(dt(-2.0) * np.log(u1)) * np.cos(dt(2.0 * np.pi) * u2)
        noise = dt(op["p0"]) + dt(op["p1"]) * z
        v = img.astype(dt)
        v = v + v * noise if kind == AUG_SPECKLE else v + noise
        x[b] = np.clip(v, dt(0.0), dt(1.0)).astype(np.float32)
    return x, labels


# ---- geometric augmentation: descriptors, parameter draws and the numpy restatement of oct_warp_batch (include/oct_unet.h) ----
# One descriptor per sample; the layout is the C struct oct_warp_op (40 bytes).  Everything is integer arithmetic, so the
# kernel, warp_reference and the host augmentation functions built on it give the same bytes.
WARP_OP_DTYPE = np.dtype([("kind", "<i4"), ("border", "<i4"), ("p", "<i4", (6,)), ("fill", "<i4"), ("fill_label", "<i4")])
WARP_NONE, WARP_COLUMN_SHIFT, WARP_AFFINE = range(3)
WARP_REPLICATE, WARP_WRAP, WARP_CONSTANT = range(3)
WARP_BORDERS = {"replicate": WARP_REPLICATE, "wrap": WARP_WRAP, "constant": WARP_CONSTANT}
# the ranges inside which no intermediate of the definition leaves int64 (OCT_WARP_MAX_* of include/oct_unet.h)
WARP_MAX_DIM, WARP_MAX_SHIFT, WARP_MAX_M = 16384, 1 << 22, 1 << 20
WARP_DRAWS = 4      # uniform numbers a sample's parameters are drawn from, whatever its augmentation


def check_warp_ops(ops, H=None, W=None) -> None:
    """Refuse (``ValueError``) descriptors or image sizes outside the ranges ``oct_warp_batch`` is defined for: the device
    cannot report them."""
    ops = np.asarray(ops)
    if ops.dtype != WARP_OP_DTYPE:
        raise TypeError("warp descriptors must be a WARP_OP_DTYPE array")
    for name, v in (("H", H), ("W", W)):
        if v is not None and not 1 <= int(v) <= WARP_MAX_DIM:
            raise ValueError(f"warp: {name} = {v} outside 1..{WARP_MAX_DIM}")
    if ops.size == 0:
        return
    for name, hi in (("kind", WARP_AFFINE), ("border", WARP_CONSTANT), ("fill", 255), ("fill_label", 255)):
        if ops[name].min() < 0 or ops[name].max() > hi:
            raise ValueError(f"warp: descriptor {name} outside 0..{hi}")
    p = ops["p"].astype(np.int64).reshape(-1, 6)
    kind = ops["kind"].reshape(-1)
    if np.abs(p[kind == WARP_COLUMN_SHIFT, :3]).max(initial=0) > WARP_MAX_SHIFT:
        raise ValueError(f"warp: column shift parameters a, b, c must be within +-{WARP_MAX_SHIFT} (1/256 pixel)")
    if np.abs(p[kind == WARP_AFFINE, :4]).max(initial=0) > WARP_MAX_M:
        raise ValueError(f"warp: affine matrix entries must be within +-{WARP_MAX_M} (Q16)")


def _nonneg(args, key, hi, default=0.0):
    v = float(args.get(key, default))
    if not 0.0 <= v <= hi:
        raise ValueError(f"{key} must be within 0..{hi}, got {args.get(key)!r}")
    return v


def _pair(args, key, default):
    v = args.get(key, default)
    try:
        a, b = (float(e) for e in v)
    except (TypeError, ValueError):
        raise ValueError(f"{key} must be a pair of numbers, got {v!r}") from None
    return a, b


def _warp_spec(fn, args):
    """The validated arguments of one list entry as a dict, ``None`` for a function that is not a warp; ``ValueError``
    for arguments outside what the integer definition covers."""
    if fn is not column_shift_aug and fn is not affine_aug:
        return None
    args = args or {}
    known = {"op", "border", "fill", "fill_label"} | ({"max_shift", "max_tilt", "max_curvature"} if fn is column_shift_aug
                                                     else {"max_rotation", "scale_range", "max_translate"})
    if set(args) - known:
        raise ValueError(f"{fn.__name__}: unknown arguments {sorted(set(args) - known)}")
    border = args.get("border", "wrap" if fn is column_shift_aug else "replicate")
    if border not in WARP_BORDERS:
        raise ValueError(f"border must be one of {sorted(WARP_BORDERS)}, got {border!r}")
    spec = {"border": WARP_BORDERS[border]}
    for key in ("fill", "fill_label"):
        v = args.get(key, 0)
        if int(v) != v or not 0 <= int(v) <= 255:
            raise ValueError(f"{key} must be an integer in 0..255, got {v!r}")
        spec[key] = int(v)
    if fn is column_shift_aug:
        px = WARP_MAX_SHIFT / 256.0
        spec.update(kind=WARP_COLUMN_SHIFT, max_shift=_nonneg(args, "max_shift", px), max_tilt=_nonneg(args, "max_tilt", px),
                    max_curvature=_nonneg(args, "max_curvature", px))
        return spec
    lo, hi = _pair(args, "scale_range", (1.0, 1.0))
    if not 65536.0 / WARP_MAX_M <= lo <= hi < np.inf:
        raise ValueError(f"scale_range must satisfy {65536.0 / WARP_MAX_M} <= lo <= hi, got {(lo, hi)}")
    dx, dy = _pair(args, "max_translate", (0.0, 0.0))
    # |t| <= (1/lo) 2 (dx + dy) 65536 has to fit the descriptor's int32
    if not (dx >= 0.0 and dy >= 0.0 and 2.0 * (dx + dy) * 65536.0 / lo < 2.0 ** 31 - 1):
        raise ValueError(f"max_translate must be non-negative and 2 (dx + dy) / lo below 32768 pixels, got {(dx, dy)}")
    spec.update(kind=WARP_AFFINE, max_rotation=_nonneg(args, "max_rotation", 360.0), scale=(lo, hi), max_translate=(dx, dy))
    return spec


def warp_ops_from(aug_fn_args):
    """Descriptor templates (``WARP_OP_DTYPE`` array, one per augmentation: kind, border and fill values set, parameters 0;
    kind 0 for an entry that is not a warp) of a list of ``(function, arguments)`` pairs, or ``None`` if the list holds no
    ``column_shift`` / ``affine``.  ``ValueError`` for arguments the integer definition does not cover."""
    specs = [_warp_spec(fn, args) for fn, args in aug_fn_args]
    if not any(s is not None for s in specs):
        return None
    ops = np.zeros(len(specs), dtype=WARP_OP_DTYPE)
    for j, s in enumerate(specs):
        if s is not None:
            ops[j]["kind"], ops[j]["border"], ops[j]["fill"], ops[j]["fill_label"] = s["kind"], s["border"], s["fill"], s["fill_label"]
    return ops


def draw_warp_ops(aug_fn_args, j, u):
    """The descriptors of ``len(j)`` samples: sample i gets augmentation ``aug_fn_args[j[i]]`` with parameters taken from
    its ``WARP_DRAWS`` uniform numbers ``u[i]`` in [0, 1).  The one place where parameters are drawn, for the host path
    (one sample at a time) and the device path (a batch at a time) alike; float64, rounded with ``np.rint``.
      column_shift: a, b, c = rint(256 max (2 u - 1)) for shift, tilt, curvature (u[0], u[1], u[2]).
      affine: theta = max_rotation (2 u[0] - 1), s = lo + (hi - lo) u[1], d = max_translate (2 u[2] - 1, 2 u[3] - 1);
        m = (1/s) [[cos, sin], [-sin, cos]], t = -m (2 d); descriptor = rint(65536 (m00, m01, m10, m11, t0, t1))."""
    j = np.asarray(j, dtype=np.int64).reshape(-1)
    u = np.asarray(u, dtype=np.float64).reshape(j.size, WARP_DRAWS)
    ops = np.zeros(j.size, dtype=WARP_OP_DTYPE)
    for k, (fn, args) in enumerate(aug_fn_args):
        spec = _warp_spec(fn, args)
        sel = np.flatnonzero(j == k)
        if spec is None or sel.size == 0:
            continue
        for name in ("kind", "border", "fill", "fill_label"):
            ops[name][sel] = spec[name]
        v = 2.0 * u[sel] - 1.0
        if spec["kind"] == WARP_COLUMN_SHIFT:
            p = 256.0 * np.stack([spec["max_shift"] * v[:, 0], spec["max_tilt"] * v[:, 1], spec["max_curvature"] * v[:, 2]], axis=1)
        else:
            theta = np.radians(spec["max_rotation"] * v[:, 0])
            s = spec["scale"][0] + (spec["scale"][1] - spec["scale"][0]) * u[sel, 1]
            dx, dy = spec["max_translate"][0] * v[:, 2], spec["max_translate"][1] * v[:, 3]
            m00, m01 = np.cos(theta) / s, np.sin(theta) / s
            m10, m11 = -m01, m00
            p = 65536.0 * np.stack([m00, m01, m10, m11, -(m00 * 2.0 * dx + m01 * 2.0 * dy), -(m10 * 2.0 * dx + m11 * 2.0 * dy)], axis=1)
        ops["p"][sel, :p.shape[1]] = np.rint(p).astype(np.int64)
    check_warp_ops(ops)
    return ops


def column_shifts(W: int, a: int, b: int, c: int) -> np.ndarray:
    """s(x) of the column shift for x = 0..W-1 (int64): floor((a D^2 + b t D + c t^2 + 128 D^2) / (256 D^2)) with
    t = 2x - (W-1) and D = max(W-1, 1)."""
    W, a, b, c = int(W), int(a), int(b), int(c)
    D = max(W - 1, 1)
    t = 2 * np.arange(W, dtype=np.int64) - (W - 1)
    return (a * D * D + b * D * t + c * t * t + 128 * D * D) // (256 * D * D)


def _border_index(i, n, border):
    """Source indices of the int64 array ``i`` on an axis of length ``n``: (indices inside 0..n-1, outside mask or None)."""
    if border == WARP_WRAP:
        return np.mod(i, n), None
    inside = np.clip(i, 0, n - 1)
    return inside, ((i < 0) | (i >= n) if border == WARP_CONSTANT else None)


def _any_outside(*masks):
    masks = [m for m in masks if m is not None]
    out = None
    for m in masks:
        out = m if out is None else out | m
    return out


def _warp_positions(H, W, op):
    """Q16 source position (sx, sy), int64 (H, W) arrays, of every output pixel under the affine descriptor ``op``."""
    p = [int(v) for v in op["p"]]
    X = (2 * np.arange(W, dtype=np.int64) - (W - 1))[None, :]
    Y = (2 * np.arange(H, dtype=np.int64) - (H - 1))[:, None]
    U = p[0] * X + p[1] * Y + p[4]
    V = p[2] * X + p[3] * Y + p[5]
    return (U + (W - 1) * 65536) >> 1, (V + (H - 1) * 65536) >> 1


def _warp_kind(op):
    kind, border = int(op["kind"]), int(op["border"])
    return kind if 0 <= kind <= WARP_AFFINE and 0 <= border <= WARP_CONSTANT else WARP_NONE


def warp_label_index(H, W, op):
    """Where every output pixel's LABEL comes from: ``(rows, cols, outside)``, (H, W) int64 index arrays and a bool mask of
    the pixels that read ``fill_label`` (``None`` if there are none by construction)."""
    kind, border = _warp_kind(op), int(op["border"])
    cols = np.broadcast_to(np.arange(W, dtype=np.int64)[None, :], (H, W))
    rows = np.broadcast_to(np.arange(H, dtype=np.int64)[:, None], (H, W))
    if kind == WARP_COLUMN_SHIFT:
        s = column_shifts(W, *op["p"][:3])
        rows, outside = _border_index(rows - s[None, :], H, border)
        return rows, cols, outside
    if kind == WARP_AFFINE:
        sx, sy = _warp_positions(H, W, op)
        cols, ox = _border_index((sx + 32768) >> 16, W, border)
        rows, oy = _border_index((sy + 32768) >> 16, H, border)
        return rows, cols, _any_outside(ox, oy)
    return rows, cols, None


def _warp_image(img, op):
    """One (H, W, C) uint8 image through the descriptor ``op``."""
    kind, border, fill = _warp_kind(op), int(op["border"]), int(op["fill"]) & 255
    H, W = img.shape[:2]
    if kind != WARP_AFFINE:         # a pure gather, the labels' rule
        rows, cols, outside = warp_label_index(H, W, op)
        out = img[rows, cols]
        if outside is not None:
            out[outside] = fill
        return out
    sx, sy = _warp_positions(H, W, op)
    ix, fx, iy, fy = sx >> 16, (sx >> 8) & 255, sy >> 16, (sy >> 8) & 255
    acc = np.zeros(img.shape, dtype=np.int64)
    for dy, wy in ((0, 256 - fy), (1, fy)):
        rows, oy = _border_index(iy + dy, H, border)
        for dx, wx in ((0, 256 - fx), (1, fx)):
            cols, ox = _border_index(ix + dx, W, border)
            tap = img[rows, cols].astype(np.int64)
            outside = _any_outside(ox, oy)
            if outside is not None:
                tap[outside] = fill
            acc += (wx * wy)[..., None] * tap
    return ((acc + 32768) >> 16).astype(np.uint8)


def warp_reference(images_u8, labels_u8, ops):
    """What ``oct_warp_batch`` computes, by its definition in include/oct_unet.h, vectorised in int64: ``(images uint8
    (B,H,W,C), labels uint8)`` (``labels_u8`` may be ``None``, (B,H,W) or (B,H,W,1)).  Refuses what the device entry point
    is not defined for (``check_warp_ops``)."""
    images_u8 = np.asarray(images_u8)
    if images_u8.dtype != np.uint8 or images_u8.ndim != 4:
        raise TypeError("warp_reference needs (B,H,W,C) uint8 images")
    ops = np.asarray(ops)
    B, H, W, _ = images_u8.shape
    check_warp_ops(ops, H, W)
    if ops.shape != (B,):
        raise ValueError("one descriptor per sample")
    labels = None if labels_u8 is None else np.array(labels_u8, dtype=np.uint8)
    if labels is not None and labels.size != B * H * W:
        raise ValueError("labels must be (B,H,W) or (B,H,W,1)")
    out = np.empty_like(images_u8)
    for b, op in enumerate(ops):
        out[b] = _warp_image(images_u8[b], op)
        if labels is not None and _warp_kind(op) != WARP_NONE:
            rows, cols, outside = warp_label_index(H, W, op)
            moved = labels[b].reshape(H, W)[rows, cols]
            if outside is not None:
                moved[outside] = int(op["fill_label"]) & 255
            labels[b] = moved.reshape(labels[b].shape)
    return out, labels


def _warp_aug(fn, image, mask, aug_args):
    """The host side of ``column_shift`` / ``affine``: the sample's descriptor is ``aug_args["op"]`` (a generator that
    walks the device path's parameter stream puts it there) or drawn from the module RNG; the image goes through
    ``warp_reference`` and the mask -- (H,W), (H,W,1) or one-hot (H,W,K), any dtype -- through the label rule."""
    args = aug_args or {}
    op = args.get("op")
    if op is None:
        op = draw_warp_ops([(fn, args)], [0], _rng.random((1, WARP_DRAWS)))
    op = np.asarray(op, dtype=WARP_OP_DTYPE).reshape(1)
    img = np.asarray(image)
    shape = img.shape
    if img.ndim == 2:
        img = img[..., None]
    as_float = img.dtype != np.uint8
    if as_float:        # float32(u8 / 255) -> u8 is exact; anything else is quantised to 8 bits here
        img = np.clip(np.rint(img.astype(np.float64) * 255.0), 0, 255).astype(np.uint8)
    out = warp_reference(img[None], None, op)[0][0].reshape(shape)
    if as_float:
        out = out.astype(np.float32) / np.float32(255.0)
    if mask is None:
        return out, None
    m = np.asarray(mask)
    H, W = img.shape[:2]
    if _warp_kind(op[0]) == WARP_NONE:
        return out, m
    rows, cols, outside = warp_label_index(H, W, op[0])
    moved = m[rows, cols]
    if outside is not None:
        fill = int(op[0]["fill_label"])
        if m.ndim == 3 and m.shape[-1] > 1:     # one-hot: the fill class's row
            if fill >= m.shape[-1]:
                raise ValueError(f"fill_label {fill} is not one of the mask's {m.shape[-1]} classes")
            moved[outside] = np.eye(m.shape[-1], dtype=m.dtype)[fill]
        else:
            moved[outside] = fill
    return out, moved


# ---- elastic deformation: descriptors, parameter draws and the numpy restatement of oct_elastic_batch (include/oct_unet.h) ----
# A stage of its own in FRONT of the warps: applied with probability p to every sample, whatever list entry the sample then
# gets.  One descriptor per sample; the layout is the C struct oct_elastic_op (40 bytes).  Integer arithmetic throughout.
ELASTIC_OP_DTYPE = np.dtype([("kind", "<i4"), ("border", "<i4"), ("spacing", "<i4"), ("amp_x", "<i4"), ("amp_y", "<i4"),
                             ("seed_lo", "<u4"), ("seed_hi", "<u4"), ("fill", "<i4"), ("fill_label", "<i4"), ("reserved", "<i4")])
ELASTIC_NONE, ELASTIC_ON = range(2)
# the ranges inside which no intermediate of the definition leaves int64 (OCT_ELASTIC_MAX_* of include/oct_unet.h)
ELASTIC_MAX_DIM, ELASTIC_MIN_SPACING, ELASTIC_MAX_SPACING, ELASTIC_MAX_AMP = 16384, 2, 128, 8192
ELASTIC_TAG = 0x454C4153    # "ELAS": the last counter word of a control point's Philox block
ELASTIC_DRAWS = 3           # uniform numbers a sample takes from the generator's elastic stream, deformed or not


def check_elastic_ops(ops, H=None, W=None) -> None:
    """Refuse (``ValueError``) descriptors or image sizes outside the ranges ``oct_elastic_batch`` is defined for: the
    device cannot report them."""
    ops = np.asarray(ops)
    if ops.dtype != ELASTIC_OP_DTYPE:
        raise TypeError("elastic descriptors must be an ELASTIC_OP_DTYPE array")
    for name, v in (("H", H), ("W", W)):
        if v is not None and not 1 <= int(v) <= ELASTIC_MAX_DIM:
            raise ValueError(f"elastic: {name} = {v} outside 1..{ELASTIC_MAX_DIM}")
    if ops.size == 0:
        return
    for name, hi in (("kind", ELASTIC_ON), ("border", WARP_CONSTANT), ("fill", 255), ("fill_label", 255), ("reserved", 0)):
        if ops[name].min() < 0 or ops[name].max() > hi:
            raise ValueError(f"elastic: descriptor {name} outside 0..{hi}")
    on = ops[ops["kind"] == ELASTIC_ON]
    if on.size and (on["spacing"].min() < ELASTIC_MIN_SPACING or on["spacing"].max() > ELASTIC_MAX_SPACING):
        raise ValueError(f"elastic: descriptor spacing outside {ELASTIC_MIN_SPACING}..{ELASTIC_MAX_SPACING}")
    for name in ("amp_x", "amp_y"):
        if on.size and (on[name].min() < 0 or on[name].max() > ELASTIC_MAX_AMP):
            raise ValueError(f"elastic: descriptor {name} outside 0..{ELASTIC_MAX_AMP} (1/256 pixel)")


def elastic_spec(args) -> dict:
    """The validated ``elastic`` keyword of the generators and of ``TrainingParams`` as a dict: ``p`` (probability, 0..1),
    ``spacing`` (control-point spacing in pixels, an integer in 2..128), ``amp_x`` / ``amp_y`` (``max_displacement`` in pixels,
    one number or ``(dx, dy)``, each 0..32, as rint(256 v)), ``border`` (the warps' names, default "replicate") and ``fill`` /
    ``fill_label``.  ``ValueError`` for anything else."""
    if not isinstance(args, dict):
        raise ValueError(f"elastic must be a dict of p, spacing, max_displacement[, border, fill, fill_label], got {args!r}")
    known = {"p", "spacing", "max_displacement", "border", "fill", "fill_label"}
    if set(args) - known:
        raise ValueError(f"elastic: unknown keys {sorted(set(args) - known)}")
    for key in ("p", "spacing", "max_displacement"):
        if key not in args:
            raise ValueError(f"elastic: {key} is required")
    p = float(args["p"])
    if not 0.0 <= p <= 1.0:
        raise ValueError(f"elastic: p must be within 0..1, got {args['p']!r}")
    S = args["spacing"]
    if isinstance(S, bool) or int(S) != S or not ELASTIC_MIN_SPACING <= int(S) <= ELASTIC_MAX_SPACING:
        raise ValueError(f"elastic: spacing must be an integer in {ELASTIC_MIN_SPACING}..{ELASTIC_MAX_SPACING}, got {S!r}")
    amp = args["max_displacement"]
    dx, dy = (float(amp), float(amp)) if np.isscalar(amp) else _pair(args, "max_displacement", None)
    px = ELASTIC_MAX_AMP / 256.0
    if not (0.0 <= dx <= px and 0.0 <= dy <= px):
        raise ValueError(f"elastic: max_displacement must be within 0..{px} pixels, got {amp!r}")
    border = args.get("border", "replicate")
    if border not in WARP_BORDERS:
        raise ValueError(f"elastic: border must be one of {sorted(WARP_BORDERS)}, got {border!r}")
    spec = {"p": p, "spacing": int(S), "amp_x": int(np.rint(256.0 * dx)), "amp_y": int(np.rint(256.0 * dy)),
            "border": WARP_BORDERS[border]}
    for key in ("fill", "fill_label"):
        v = args.get(key, 0)
        if int(v) != v or not 0 <= int(v) <= 255:
            raise ValueError(f"elastic: {key} must be an integer in 0..255, got {v!r}")
        spec[key] = int(v)
    return spec


def draw_elastic_ops(spec, u):
    """The descriptors of ``len(u)`` samples from their ``ELASTIC_DRAWS`` uniform numbers ``u[i]`` in [0, 1): sample i is
    deformed iff ``u[i, 0] < p``; its field's key is ``(floor(u[i, 1] 2^32), floor(u[i, 2] 2^32))``.  A sample that is not
    deformed gets the all-zero descriptor.  ``spec``: what ``elastic_spec`` returns."""
    u = np.asarray(u, dtype=np.float64).reshape(-1, ELASTIC_DRAWS)
    ops = np.zeros(u.shape[0], dtype=ELASTIC_OP_DTYPE)
    sel = np.flatnonzero(u[:, 0] < spec["p"])
    ops["kind"][sel] = ELASTIC_ON
    for name in ("border", "spacing", "amp_x", "amp_y", "fill", "fill_label"):
        ops[name][sel] = spec[name]
    ops["seed_lo"][sel] = np.floor(u[sel, 1] * 4294967296.0).astype(np.uint64)
    ops["seed_hi"][sel] = np.floor(u[sel, 2] * 4294967296.0).astype(np.uint64)
    check_elastic_ops(ops)
    return ops


def _elastic_kind(op):
    ok = (int(op["kind"]) == ELASTIC_ON and 0 <= int(op["border"]) <= WARP_CONSTANT
          and ELASTIC_MIN_SPACING <= int(op["spacing"]) <= ELASTIC_MAX_SPACING
          and 0 <= int(op["amp_x"]) <= ELASTIC_MAX_AMP and 0 <= int(op["amp_y"]) <= ELASTIC_MAX_AMP)
    return ELASTIC_ON if ok else ELASTIC_NONE


def elastic_weights(n: int, S: int):
    """``(cell, b)`` of positions 0..n-1 on one axis: the cell ``p // S`` (int64 (n,)) and the four uniform cubic B-spline
    weight numerators over 6 S^3 at offset ``k = p % S`` (int64 (n, 4)), for control points cell..cell+3."""
    p = np.arange(int(n), dtype=np.int64)
    S = int(S)
    k = p % S
    b = np.stack([(S - k) ** 3, 3 * k ** 3 - 6 * S * k ** 2 + 4 * S ** 3, -3 * k ** 3 + 3 * S * k ** 2 + 3 * S * S * k + S ** 3,
                  k ** 3], axis=1)
    return p // S, b


def elastic_control(H: int, W: int, op):
    """The control displacements ``(dx, dy)`` of descriptor ``op`` in 1/256 pixel: int64 arrays over control points
    i = 0..(H-1)//S + 3, j = 0..(W-1)//S + 3, uniform integers in [-amp, amp] from the point's own Philox block."""
    S = int(op["spacing"])
    ny, nx = (int(H) - 1) // S + 4, (int(W) - 1) // S + 4
    ctr = np.zeros((ny, nx, 4), dtype=np.uint64)
    ctr[..., 0], ctr[..., 1], ctr[..., 3] = np.arange(nx, dtype=np.uint64)[None, :], np.arange(ny, dtype=np.uint64)[:, None], ELASTIC_TAG
    r = philox4x32_10(ctr, np.array([int(op["seed_lo"]), int(op["seed_hi"])], dtype=np.uint64)).astype(np.uint64)
    ax, ay = int(op["amp_x"]), int(op["amp_y"])
    dx = ((r[..., 0] * np.uint64(2 * ax + 1)) >> np.uint64(32)).astype(np.int64) - ax
    dy = ((r[..., 1] * np.uint64(2 * ay + 1)) >> np.uint64(32)).astype(np.int64) - ay
    return dx, dy


def elastic_displacement(H: int, W: int, op, control=None):
    """The displacement fields ``(disp_x, disp_y)`` of descriptor ``op`` in 1/256 pixel, int64 (H, W):
    floor((N + 18 S^6) / (36 S^6)) with N the B-spline sum over the 4 x 4 control points of the pixel's cell.  ``control``:
    a caller-given ``(dx, dy)`` pair of control grids in place of ``elastic_control`` (tests)."""
    S = int(op["spacing"])
    dx, dy = elastic_control(H, W, op) if control is None else (np.asarray(c, dtype=np.int64) for c in control)
    (cx, bx), (cy, by) = elastic_weights(W, S), elastic_weights(H, S)
    half = 18 * S ** 6
    out = []
    for d in (dx, dy):
        # columns first: t[r, x] = sum_b bx[x, b] d[r, cx + b], then the rows of t
        t = sum(bx[None, :, b] * d[:, cx + b] for b in range(4))
        N = sum(by[:, a, None] * t[cy + a, :] for a in range(4))
        out.append((N + half) // (2 * half))
    return out[0], out[1]


def elastic_label_index(H, W, op):
    """Where every output pixel's LABEL comes from under descriptor ``op`` (a deformed one): ``(rows, cols, outside)`` as
    ``warp_label_index``."""
    disp_x, disp_y = elastic_displacement(H, W, op)
    sx = 256 * np.arange(W, dtype=np.int64)[None, :] + disp_x
    sy = 256 * np.arange(H, dtype=np.int64)[:, None] + disp_y
    cols, ox = _border_index((sx + 128) >> 8, W, int(op["border"]))
    rows, oy = _border_index((sy + 128) >> 8, H, int(op["border"]))
    return rows, cols, _any_outside(ox, oy)


def _elastic_image(img, op):
    """One (H, W, C) uint8 image through the deformed descriptor ``op``: bilinear in 8-bit fractions, as the affine warp."""
    border, fill = int(op["border"]), int(op["fill"]) & 255
    H, W = img.shape[:2]
    disp_x, disp_y = elastic_displacement(H, W, op)
    sx = 256 * np.arange(W, dtype=np.int64)[None, :] + disp_x
    sy = 256 * np.arange(H, dtype=np.int64)[:, None] + disp_y
    ix, fx, iy, fy = sx >> 8, sx & 255, sy >> 8, sy & 255
    acc = np.zeros(img.shape, dtype=np.int64)
    for dy, wy in ((0, 256 - fy), (1, fy)):
        rows, oy = _border_index(iy + dy, H, border)
        for dx, wx in ((0, 256 - fx), (1, fx)):
            cols, ox = _border_index(ix + dx, W, border)
            tap = img[rows, cols].astype(np.int64)
            outside = _any_outside(ox, oy)
            if outside is not None:
                tap[outside] = fill
            acc += (wx * wy)[..., None] * tap
    return ((acc + 32768) >> 16).astype(np.uint8)


def elastic_reference(images_u8, labels_u8, ops):
    """What ``oct_elastic_batch`` computes, by its definition in include/oct_unet.h, vectorised in int64: ``(images uint8
    (B,H,W,C), labels uint8)`` (``labels_u8`` may be ``None``, (B,H,W) or (B,H,W,1)).  Refuses what the device entry point
    is not defined for (``check_elastic_ops``)."""
    images_u8 = np.asarray(images_u8)
    if images_u8.dtype != np.uint8 or images_u8.ndim != 4:
        raise TypeError("elastic_reference needs (B,H,W,C) uint8 images")
    ops = np.asarray(ops)
    B, H, W, _ = images_u8.shape
    check_elastic_ops(ops, H, W)
    if ops.shape != (B,):
        raise ValueError("one descriptor per sample")
    labels = None if labels_u8 is None else np.array(labels_u8, dtype=np.uint8)
    if labels is not None and labels.size != B * H * W:
        raise ValueError("labels must be (B,H,W) or (B,H,W,1)")
    out = np.array(images_u8)
    for b, op in enumerate(ops):
        if _elastic_kind(op) == ELASTIC_NONE:
            continue
        out[b] = _elastic_image(images_u8[b], op)
        if labels is not None:
            rows, cols, outside = elastic_label_index(H, W, op)
            moved = labels[b].reshape(H, W)[rows, cols]
            if outside is not None:
                moved[outside] = int(op["fill_label"]) & 255
            labels[b] = moved.reshape(labels[b].shape)
    return out, labels


def elastic_sample(image_u8, mask, op):
    """The host generator's side of the stage: one (H,W,C) uint8 image through ``elastic_reference`` and its mask -- (H,W),
    (H,W,1) or one-hot (H,W,K), any dtype -- through the label rule, as ``_warp_aug`` moves a mask."""
    op = np.asarray(op, dtype=ELASTIC_OP_DTYPE).reshape(1)
    out = elastic_reference(np.asarray(image_u8)[None], None, op)[0][0]
    if mask is None or _elastic_kind(op[0]) == ELASTIC_NONE:
        return out, mask
    m = np.asarray(mask)
    rows, cols, outside = elastic_label_index(*out.shape[:2], op[0])
    moved = m[rows, cols]
    if outside is not None:
        fill = int(op[0]["fill_label"])
        if m.ndim == 3 and m.shape[-1] > 1:     # one-hot: the fill class's row
            if fill >= m.shape[-1]:
                raise ValueError(f"fill_label {fill} is not one of the mask's {m.shape[-1]} classes")
            moved[outside] = np.eye(m.shape[-1], dtype=m.dtype)[fill]
        else:
            moved[outside] = fill
    return out, moved


# ---- photometric augmentation: descriptors, parameter draws and the numpy restatement of oct_photo_batch (include/oct_unet.h) ----
# A stage of its own directly BEHIND the elastic stage and in front of the warps, on the uint8 sample: a separable integer
# blur, column shadows and a 256-entry intensity table (gamma, brightness, contrast), in that order.  Images only: labels
# never change.  One descriptor per sample; the layout is the C struct oct_photo_op (320 bytes).  The weights and the table
# are INPUT of the device and of the restatement alike, so both give the same bytes whatever the host's exp and pow do.
PHOTO_OP_DTYPE = np.dtype([("kind", "<i4"), ("radius", "<i4"), ("w", "<u2", (9,)), ("n_shadows", "<u2"), ("cx", "<i2", (4,)),
                           ("hw", "<i2", (4,)), ("y0", "<i2", (4,)), ("strength", "<u2", (4,)), ("reserved", "<u4"),
                           ("lut", "u1", (256,))])
PHOTO_BLUR, PHOTO_SHADOW, PHOTO_LUT = 1, 2, 4
PHOTO_MAX_DIM, PHOTO_MAX_RADIUS, PHOTO_MAX_SHADOWS, PHOTO_MAX_HW, PHOTO_MAX_Y0 = 16384, 8, 4, 4096, 16384
PHOTO_DRAWS = 24            # uniform numbers a sample takes from the generator's photometric stream, whatever it draws


def check_photo_ops(ops, H=None, W=None) -> None:
    """Refuse (``ValueError``) descriptors or image sizes outside what ``oct_photo_batch`` is defined for: the device cannot
    report them.  ``kind``, ``radius``, ``n_shadows`` and ``reserved`` are held to their ranges in every descriptor; the
    weights where the BLUR flag is set (``w[0] + 2 sum_{k>=1} w[k] = 256``, ``w[k] = 0`` for k > radius); ``hw``, ``y0`` and
    ``strength`` of shadows 0..n_shadows-1 where the SHADOW flag is set (``cx`` is any int16)."""
    ops = np.asarray(ops)
    if ops.dtype != PHOTO_OP_DTYPE:
        raise TypeError("photometric descriptors must be a PHOTO_OP_DTYPE array")
    for name, v in (("H", H), ("W", W)):
        if v is not None and not 1 <= int(v) <= PHOTO_MAX_DIM:
            raise ValueError(f"photometric: {name} = {v} outside 1..{PHOTO_MAX_DIM}")
    ops = ops.reshape(-1)
    if ops.size == 0:
        return
    for name, hi in (("kind", PHOTO_BLUR | PHOTO_SHADOW | PHOTO_LUT), ("radius", PHOTO_MAX_RADIUS),
                     ("n_shadows", PHOTO_MAX_SHADOWS), ("reserved", 0)):
        if ops[name].min() < 0 or ops[name].max() > hi:
            raise ValueError(f"photometric: descriptor {name} outside 0..{hi}")
    blur = ops[(ops["kind"] & PHOTO_BLUR) != 0]
    if blur.size:
        w = blur["w"].astype(np.int64)
        if (w[:, 0] + 2 * w[:, 1:].sum(axis=1) != 256).any():
            raise ValueError("photometric: descriptor w must satisfy w[0] + 2 sum(w[1:]) = 256")
        if (w * (np.arange(9)[None, :] > blur["radius"][:, None])).any():
            raise ValueError("photometric: descriptor w[k] must be 0 for k > radius")
    sh = ops[(ops["kind"] & PHOTO_SHADOW) != 0]
    if sh.size:
        live = np.arange(PHOTO_MAX_SHADOWS)[None, :] < sh["n_shadows"][:, None]
        for name, lo, hi in (("hw", 1, PHOTO_MAX_HW), ("y0", 0, PHOTO_MAX_Y0), ("strength", 0, 256)):
            v = sh[name].astype(np.int64)[live]
            if v.size and (v.min() < lo or v.max() > hi):
                raise ValueError(f"photometric: descriptor {name} outside {lo}..{hi}")


def blur_weights(sigma: float):
    """``(radius, w)`` of a Gaussian blur of standard deviation ``sigma`` pixels, 0 < sigma <= 8/3: R = min(8, ceil(3 sigma)),
    g_k = exp(-k^2 / 2 sigma^2) over -R..R normalised to sum 1, ``w[k] = rint(256 g_k)`` for k >= 1 and
    ``w[0] = 256 - 2 sum_{k>=1} w[k]`` (uint16 (9,), zero beyond R)."""
    sigma = float(sigma)
    if not 0.0 < sigma <= 8.0 / 3.0:
        raise ValueError(f"blur sigma must be within (0, 8/3], got {sigma!r}")
    R = min(PHOTO_MAX_RADIUS, int(np.ceil(3.0 * sigma)))
    k = np.arange(-R, R + 1, dtype=np.float64)
    g = np.exp(-(k * k) / (2.0 * sigma * sigma))
    g /= g.sum()
    w = np.zeros(9, dtype=np.int64)
    w[1:R + 1] = np.rint(256.0 * g[R + 1:])
    w[0] = 256 - 2 * w[1:].sum()
    return R, w.astype(np.uint16)


def photo_lut(gamma: float = 1.0, brightness: float = 0.0, contrast: float = 1.0) -> np.ndarray:
    """The intensity table of contrast ``c`` about mid-grey, brightness ``beta`` (units of full scale) and ``gamma``, in
    float64: ``lut[i] = rint(255 clip((i/255 - 0.5) c + 0.5 + beta, 0, 1) ** gamma)`` (uint8 (256,))."""
    i = np.arange(256, dtype=np.float64) / 255.0
    v = np.clip((i - 0.5) * float(contrast) + 0.5 + float(brightness), 0.0, 1.0) ** float(gamma)
    return np.rint(255.0 * v).astype(np.uint8)


_IDENTITY_LUT = np.arange(256, dtype=np.uint8)


def _prob(args, key, what):
    p = float(args.get(key, 1.0))
    if not 0.0 <= p <= 1.0:
        raise ValueError(f"{what}: p must be within 0..1, got {args.get(key)!r}")
    return p


def _range(args, key, lo, hi, what, lo_open=False):
    if key not in args:
        raise ValueError(f"{what}: {key} is required")
    a, b = _pair(args, key, None)
    if not ((lo < a if lo_open else lo <= a) and a <= b <= hi):
        raise ValueError(f"{what}: {key} must be (lo, hi) with {lo} {'<' if lo_open else '<='} lo <= hi <= {hi}, got {args[key]!r}")
    return a, b


def photometric_spec(args) -> dict:
    """The validated ``photometric`` keyword of the generators and of ``TrainingParams`` as a dict.  Every part is optional
    and off unless given: ``p`` (probability that a sample goes through the stage, default 1), ``gamma`` (lo, hi) within
    0.25..4, ``brightness`` b within 0..1, ``contrast`` (lo, hi) within 0.25..4, ``blur`` {``p``, ``sigma`` (lo, hi) within
    (0, 8/3]} and ``shadows`` {``p``, ``max_count`` 1..4 (default 1), ``width`` (lo, hi) half-widths in pixels within 1..4096,
    ``strength`` (lo, hi) within 0..1, ``top`` (lo, hi) fractions of H within 0..1 (default (0, 0))}.  ``ValueError`` for
    anything else, unknown keys included."""
    if not isinstance(args, dict):
        raise ValueError(f"photometric must be a dict of p, gamma, brightness, contrast, blur, shadows, got {args!r}")
    known = {"p", "gamma", "brightness", "contrast", "blur", "shadows"}
    if set(args) - known:
        raise ValueError(f"photometric: unknown keys {sorted(set(args) - known)}")
    spec = {"p": _prob(args, "p", "photometric"), "gamma": None, "brightness": None, "contrast": None, "blur": None,
            "shadows": None}
    if "gamma" in args:
        spec["gamma"] = _range(args, "gamma", 0.25, 4.0, "photometric")
    if "brightness" in args:
        spec["brightness"] = _nonneg(args, "brightness", 1.0)
    if "contrast" in args:
        spec["contrast"] = _range(args, "contrast", 0.25, 4.0, "photometric")
    for part, keys in (("blur", {"p", "sigma"}), ("shadows", {"p", "max_count", "width", "strength", "top"})):
        sub = args.get(part)
        if sub is None:
            continue
        what = f"photometric {part}"
        if not isinstance(sub, dict):
            raise ValueError(f"{what} must be a dict of {sorted(keys)}, got {sub!r}")
        if set(sub) - keys:
            raise ValueError(f"{what}: unknown keys {sorted(set(sub) - keys)}")
        if part == "blur":
            spec[part] = {"p": _prob(sub, "p", what), "sigma": _range(sub, "sigma", 0.0, 8.0 / 3.0, what, lo_open=True)}
            continue
        n = sub.get("max_count", 1)
        if isinstance(n, bool) or int(n) != n or not 1 <= int(n) <= PHOTO_MAX_SHADOWS:
            raise ValueError(f"{what}: max_count must be an integer in 1..{PHOTO_MAX_SHADOWS}, got {n!r}")
        spec[part] = {"p": _prob(sub, "p", what), "max_count": int(n), "width": _range(sub, "width", 1.0, float(PHOTO_MAX_HW), what),
                      "strength": _range(sub, "strength", 0.0, 1.0, what),
                      "top": _range(dict(sub, top=sub.get("top", (0.0, 0.0))), "top", 0.0, 1.0, what)}
    return spec


def draw_photo_ops(spec, u, H, W):
    """The descriptors of ``len(u)`` samples of H x W pixels from their ``PHOTO_DRAWS`` uniform numbers ``u[i]`` in [0, 1);
    float64, rounded with ``np.rint``, as ``draw_warp_ops``.  ``spec``: what ``photometric_spec`` returns.
      u[0] < p: the sample goes through the stage; otherwise, and where it then draws nothing, its ``kind`` is 0.
      u[1], u[2], u[3]: gamma = lo (hi/lo)^u (log-uniform), beta = b (2u - 1), contrast = lo + (hi - lo) u ->
        ``photo_lut``; the LUT flag only where the table is not the identity.
      u[4] < blur p: sigma = lo + (hi - lo) u[5] -> ``blur_weights``.
      u[6] < shadows p: count = 1 + floor(u[7] max_count); shadow s from u[8 + 4s .. 11 + 4s]: cx = floor(u W),
        hw = max(1, rint(width)), y0 = floor(H top), strength = rint(256 strength), each range drawn as lo + (hi - lo) u."""
    H, W = int(H), int(W)
    u = np.asarray(u, dtype=np.float64).reshape(-1, PHOTO_DRAWS)
    ops = np.zeros(u.shape[0], dtype=PHOTO_OP_DTYPE)
    lin = lambda r, t: r[0] + (r[1] - r[0]) * t        # noqa: E731
    for i in np.flatnonzero(u[:, 0] < spec["p"]):
        op, ui, kind = ops[i], u[i], 0
        if spec["gamma"] is not None or spec["brightness"] is not None or spec["contrast"] is not None:
            gamma = 1.0 if spec["gamma"] is None else float(np.exp(lin(np.log(spec["gamma"]), ui[1])))
            beta = 0.0 if spec["brightness"] is None else spec["brightness"] * (2.0 * ui[2] - 1.0)
            c = 1.0 if spec["contrast"] is None else lin(spec["contrast"], ui[3])
            lut = photo_lut(gamma, beta, c)
            if (lut != _IDENTITY_LUT).any():
                kind |= PHOTO_LUT
                op["lut"] = lut
        if spec["blur"] is not None and ui[4] < spec["blur"]["p"]:
            kind |= PHOTO_BLUR
            op["radius"], op["w"] = blur_weights(lin(spec["blur"]["sigma"], ui[5]))
        sh = spec["shadows"]
        if sh is not None and ui[6] < sh["p"]:
            kind |= PHOTO_SHADOW
            n = min(sh["max_count"], 1 + int(np.floor(ui[7] * sh["max_count"])))
            op["n_shadows"] = n
            for s in range(n):
                d = ui[8 + 4 * s:12 + 4 * s]
                op["cx"][s] = min(W - 1, int(np.floor(d[0] * W)))
                op["hw"][s] = max(1, int(np.rint(lin(sh["width"], d[1]))))
                op["y0"][s] = int(np.floor(H * lin(sh["top"], d[2])))
                op["strength"][s] = int(np.rint(256.0 * lin(sh["strength"], d[3])))
        op["kind"] = kind
        if not kind & PHOTO_LUT:
            op["lut"] = _IDENTITY_LUT
    check_photo_ops(ops, H, W)
    return ops


def shadow_gain(H: int, W: int, op) -> np.ndarray:
    """g(y, x) of descriptor ``op``'s shadows, int64 (H, W): the minimum over the shadows with y >= y0_s of
    ``256 - (strength_s max(0, hw_s - |x - cx_s|)) // hw_s``, 256 where there is none."""
    g = np.full((int(H), int(W)), 256, dtype=np.int64)
    x, y = np.arange(int(W), dtype=np.int64), np.arange(int(H), dtype=np.int64)
    for s in range(int(op["n_shadows"])):
        hw = int(op["hw"][s])
        gs = 256 - (int(op["strength"][s]) * np.maximum(0, hw - np.abs(x - int(op["cx"][s])))) // hw
        g = np.where((y >= int(op["y0"][s]))[:, None], np.minimum(g, gs[None, :]), g)
    return g


def _photo_image(img, op):
    """One (H, W, C) uint8 image through descriptor ``op``: blur, shadows, table."""
    kind, H, W = int(op["kind"]), img.shape[0], img.shape[1]
    v = img.astype(np.int64)
    if kind & PHOTO_BLUR:
        R, w = int(op["radius"]), op["w"].astype(np.int64)
        cols = np.clip(np.arange(-R, W + R), 0, W - 1)
        rows = np.clip(np.arange(-R, H + R), 0, H - 1)
        src = v[:, cols]
        h = sum(w[abs(k)] * src[:, R + k:R + k + W] for k in range(-R, R + 1))       # <= 65280: exact
        h = h[rows]
        v = (sum(w[abs(j)] * h[R + j:R + j + H] for j in range(-R, R + 1)) + 32768) >> 16
    if kind & PHOTO_SHADOW:
        v = (v * shadow_gain(H, W, op)[..., None] + 128) >> 8
    if kind & PHOTO_LUT:
        v = op["lut"][v]
    return v.astype(np.uint8)


def photometric_reference(images_u8, ops):
    """What ``oct_photo_batch`` computes, by its definition in include/oct_unet.h, vectorised in int64: (B,H,W,C) uint8 ->
    (B,H,W,C) uint8.  Refuses what the device entry point is not defined for (``check_photo_ops``)."""
    images_u8 = np.asarray(images_u8)
    if images_u8.dtype != np.uint8 or images_u8.ndim != 4:
        raise TypeError("photometric_reference needs (B,H,W,C) uint8 images")
    ops = np.asarray(ops)
    B, H, W, _ = images_u8.shape
    check_photo_ops(ops, H, W)
    if ops.shape != (B,):
        raise ValueError("one descriptor per sample")
    out = np.array(images_u8)
    for b, op in enumerate(ops):
        if op["kind"]:
            out[b] = _photo_image(images_u8[b], op)
    return out


def photometric_sample(image_u8, op):
    """The host generator's side of the stage: one (H,W,C) uint8 image through ``photometric_reference``."""
    op = np.asarray(op, dtype=PHOTO_OP_DTYPE).reshape(1)
    return photometric_reference(np.asarray(image_u8)[None], op)[0]
