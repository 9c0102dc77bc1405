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


augmentation_map = {
    "add_noise": add_noise_aug,
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
    arguments the device implements -- such a list keeps the host path."""
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
