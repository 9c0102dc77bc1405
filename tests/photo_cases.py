"""Shared cases of the photometric tests (test_photometric.py on the CPU, test_gpu_photometric.py on the device): hand-made
descriptors that cover every flag combination, every blur radius with ordinary and extreme weights, 0..4 shadows with the
edge cases of the definition, identity and permutation tables -- and an independent brute-force statement of the definition."""
import itertools

import numpy as np

from oct_image_segmentation_models_amd.common import augmentation as A

# weights of every radius: the rounded Gaussian of sigma = R / 3 (R >= 1), and the extremes -- all the weight in the centre
# (any radius: the identity), none in the centre and all of it at +-8
WEIGHTS = {R: (R, A.blur_weights(R / 3.0)[1]) for R in range(1, 9)}
WEIGHTS[0] = (0, np.array([256, 0, 0, 0, 0, 0, 0, 0, 0], dtype=np.uint16))
WEIGHTS["centre"] = (8, WEIGHTS[0][1])
WEIGHTS["far"] = (8, np.array([0, 0, 0, 0, 0, 0, 0, 0, 128], dtype=np.uint16))
WEIGHTS["box5"] = (5, np.array([26, 23, 23, 23, 23, 23, 0, 0, 0], dtype=np.uint16))       # 26 + 2 * 115 = 256


def shadow_sets(H, W):
    """Lists of (cx, hw, y0, strength): none, one, and up to four with the definition's edge cases -- a centre left and
    right of the image, half-width 1 and 4096, strength 0 and 256, y0 = 0, inside, H and beyond."""
    return [[],
            [(W // 2, 3, 0, 200)],
            [(-3, 6, 0, 256), (W + 2, 5, H // 2, 128)],
            [(0, 1, 0, 256), (W - 1, 4096, H, 255), (W // 3, 2, H - 1, 77)],
            [(W // 2, 7, 1, 0), (W // 2 + 1, 9, 2, 256), (-32768, 4096, 0, 256), (32767, 1, 16384, 256)]]


def tables():
    rng = np.random.default_rng(7)
    return [np.arange(256, dtype=np.uint8), rng.permutation(256).astype(np.uint8), A.photo_lut(2.2, -0.1, 1.7)]


def make_op(kind, weights=0, shadows=(), lut=None):
    op = np.zeros((), dtype=A.PHOTO_OP_DTYPE)
    op["kind"] = kind
    op["radius"], op["w"] = WEIGHTS[weights]
    op["n_shadows"] = len(shadows)
    for s, (cx, hw, y0, strength) in enumerate(shadows):
        op["cx"][s], op["hw"][s], op["y0"][s], op["strength"][s] = cx, hw, y0, strength
    op["lut"] = np.arange(256, dtype=np.uint8) if lut is None else lut
    return op


def combos(H, W):
    """Descriptors for H x W images in a fixed shuffled order: every flag combination x every weight set (cycling through the
    shadow sets and the tables), so neighbours in a batch differ in everything."""
    sh, tb = shadow_sets(H, W), tables()
    ops = [make_op(kind, wk, sh[(i + kind) % len(sh)], tb[(i + 2 * kind) % len(tb)])
           for i, (kind, wk) in enumerate(itertools.product(range(8), list(WEIGHTS)))]
    ops += [make_op(2, 0, s) for s in sh] + [make_op(6, 3, s, tb[1]) for s in sh] + [make_op(7, 8, sh[4], tb[1])]
    ops = np.array(ops, dtype=A.PHOTO_OP_DTYPE)
    return ops[np.random.default_rng(0).permutation(len(ops))]


def batch_ops(all_ops, B, which):
    """B descriptors: sample b takes descriptor ``which + b`` (cyclically)."""
    return all_ops[(which + np.arange(B)) % len(all_ops)].copy()


def brute_force(images, ops):
    """The definition stated independently: the blur as ONE 2-D sum over the (2R+1)^2 window with the outer product of the
    weights and one final rounding, the shadows pixel by pixel from Python integers, then the table."""
    images = np.asarray(images)
    B, H, W, C = images.shape
    out = np.empty_like(images)
    ys, xs = np.arange(H), np.arange(W)
    for b in range(B):
        op = ops[b]
        kind = int(op["kind"])
        v = images[b].astype(np.int64)
        if kind & 1:
            R, w = int(op["radius"]), [int(e) for e in op["w"]]
            acc = np.zeros_like(v)
            for j in range(-R, R + 1):
                for k in range(-R, R + 1):
                    acc += w[abs(j)] * w[abs(k)] * v[np.clip(ys + j, 0, H - 1)][:, np.clip(xs + k, 0, W - 1)]
            v = (acc + 32768) >> 16
        if kind & 2:
            g = np.full((H, W), 256, dtype=np.int64)
            for s in range(int(op["n_shadows"])):
                cx, hw, y0, st = (int(op[f][s]) for f in ("cx", "hw", "y0", "strength"))
                for x in range(W):
                    gs = 256 - (st * max(0, hw - abs(x - cx))) // hw
                    for y in range(max(y0, 0), H):
                        g[y, x] = min(g[y, x], gs)
            v = (v * g[..., None] + 128) >> 8
        if kind & 4:
            v = op["lut"].astype(np.int64)[v]
        assert v.min() >= 0 and v.max() <= 255
        out[b] = v
    return out
