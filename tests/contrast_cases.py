"""Cases and an independent restatement for the contrast tests (tests/test_contrast.py, tests/test_gpu_contrast.py).

``literal_contrast`` is written from the definition in include/oct_unet.h, one tile and one pixel at a time in plain Python
integers; it shares no code with ``common.utils.contrast_reference``."""
import numpy as np

# (H, W, ch, tiles): what each covers is in the GPU test's docstring
SHAPES = [
    (16, 16, 1, (2, 2)),
    (37, 53, 1, (4, 6)),
    (20, 34, 1, (2, 1)),
    (20, 34, 1, (1, 4)),
    (40, 40, 1, (1, 1)),
    (256, 512, 1, (8, 8)),
    (256, 512, 1, (16, 16)),
    (24, 40, 3, (2, 3)),
]
SMALL_SHAPES = [s for s in SHAPES if s[0] * s[1] <= 2048]        # the ones the literal Python loop runs on

SPECS = [
    {"method": "clahe", "clip": None},
    {"method": "clahe", "clip": 1.0},
    {"method": "clahe", "clip": 2.0},
    {"method": "clahe", "clip": 40.0},
    {"method": "stretch", "percentiles": (1, 99)},
    {"method": "stretch", "percentiles": (0, 100)},
]
CONTENTS = ["constant", "halves", "noise", "scan"]


def spec_id(spec) -> str:
    return f"clahe-{spec['clip']}" if spec["method"] == "clahe" else "stretch-%g-%g" % tuple(spec["percentiles"])


def with_tiles(spec, tiles) -> dict:
    return dict(spec, tiles=tiles)


def make_images(content: str, B: int, H: int, W: int, ch: int, seed: int = 0) -> np.ndarray:
    """uint8 (B,H,W,ch) of one kind of content; every image and channel differs where the content allows it."""
    rng = np.random.default_rng([seed, B, H, W, ch, CONTENTS.index(content)])
    if content == "constant":
        return np.full((B, H, W, ch), 37, np.uint8)
    if content == "halves":             # two byte values, thousands of pixels each: the worst contention.  The dark value
        x = np.empty((B, H, W, ch), np.uint8)       # fills the left half of the upper rows only, so that some tiles hold both
        top = H // 2 - 1                            # values and some one: their LUTs differ under every method
        for b in range(B):
            for c in range(ch):
                cut = W // 2 + (b + c) % 3 - 1
                x[b, :, :, c] = 200 - c
                x[b, :top, :cut, c] = 10 + b
        return x
    if content == "noise":              # uniform bytes under a ramp of the mean, so that the tiles' LUTs differ
        ramp = np.linspace(0.0, 1.0, H)[None, :, None, None] * np.linspace(0.2, 1.0, W)[None, None, :, None]
        return (rng.integers(0, 256, (B, H, W, ch)) * (0.25 + 0.75 * ramp)).astype(np.uint8)
    if content == "scan":
        from oct_image_segmentation_models_amd.common.synthetic import make_scans
        imgs = make_scans(B, H, W, 3, seed=seed + 1)[0]
        imgs = (30 + imgs.astype(np.int64) * 2 // 3).astype(np.uint8)       # a low-contrast instrument: bytes in 30..200
        return np.ascontiguousarray(np.concatenate([np.roll(imgs, 3 * c, axis=2) for c in range(ch)], axis=3).astype(np.uint8))
    raise ValueError(content)


def _edges(n, t):
    return [(i * n) // t for i in range(t + 1)]


def _literal_lut(h, A, spec):
    if spec["method"] == "clahe":
        clip = spec.get("clip")
        if clip is None or clip == 0:
            L = A
        else:
            L = max(1, (int(round(clip * 256)) * A) >> 16)
        E = sum(max(v - L, 0) for v in h)
        q, r = divmod(E, 256)
        h2 = [min(h[i], L) + q + (1 if ((i + 1) * r) // 256 > (i * r) // 256 else 0) for i in range(256)]
        lut, c = [], 0
        for i in range(256):
            c += h2[i]
            lut.append((c * 255 + A // 2) // A)
        assert c == A
        return lut
    lo, hi = spec.get("percentiles", (1, 99))
    lo_bp, hi_bp = int(round(lo * 100)), int(round(hi * 100))
    cum, c = [], 0
    for v in h:
        c += v
        cum.append(c)
    v_lo = min(i for i in range(256) if cum[i] > (lo_bp * A) // 10000)
    v_hi = min(i for i in range(256) if cum[i] * 10000 >= hi_bp * A)
    if v_hi <= v_lo:
        return list(range(256))
    d = v_hi - v_lo
    return [0 if i <= v_lo else 255 if i >= v_hi else ((i - v_lo) * 255 + d // 2) // d for i in range(256)]


def _literal_axis(p, edges, t):
    """(cell, next cell, a, D) of position p on an axis."""
    if t == 1:
        return 0, 0, 0, 1
    cen = [edges[i] + edges[i + 1] - 1 for i in range(t)]
    r = min(max(sum(1 for v in cen if v <= 2 * p) - 1, 0), t - 2)
    D = cen[r + 1] - cen[r]
    return r, r + 1, min(max(2 * p - cen[r], 0), D), D


def literal_contrast(x, spec):
    """``(luts (B,ch,ty,tx,256) uint8, out uint8 like x)`` by the definition, pixel by pixel."""
    B, H, W, ch = x.shape
    ty, tx = spec.get("tiles", (8, 8))
    ey, ex = _edges(H, ty), _edges(W, tx)
    luts = np.zeros((B, ch, ty, tx, 256), np.uint8)
    for b in range(B):
        for c in range(ch):
            for r in range(ty):
                for q in range(tx):
                    h = [0] * 256
                    for y in range(ey[r], ey[r + 1]):
                        for xx in range(ex[q], ex[q + 1]):
                            h[int(x[b, y, xx, c])] += 1
                    A = (ey[r + 1] - ey[r]) * (ex[q + 1] - ex[q])
                    luts[b, c, r, q] = _literal_lut(h, A, spec)
    out = np.zeros_like(x)
    for y in range(H):
        r, r1, ay, Dy = _literal_axis(y, ey, ty)
        for xx in range(W):
            q, q1, ax, Dx = _literal_axis(xx, ex, tx)
            for b in range(B):
                for c in range(ch):
                    v = int(x[b, y, xx, c])
                    v00, v01 = int(luts[b, c, r, q, v]), int(luts[b, c, r, q1, v])
                    v10, v11 = int(luts[b, c, r1, q, v]), int(luts[b, c, r1, q1, v])
                    num = (Dy - ay) * ((Dx - ax) * v00 + ax * v01) + ay * ((Dx - ax) * v10 + ax * v11) + (Dy * Dx) // 2
                    assert num < 1 << 32
                    out[b, y, xx, c] = num // (Dy * Dx)
    return luts, out


def interior_pixel_exists(H, W, tiles) -> bool:
    """Is there a pixel with 0 < ay < Dy and 0 < ax < Dx -- one that really blends four tiles?  With a single tile row
    (column) that axis has nothing to blend and only the other one is asked."""
    ty, tx = tiles
    ey, ex = _edges(H, ty), _edges(W, tx)

    def strictly_inside(n, edges, t):
        return t == 1 or any(0 < a < D for a, D in (_literal_axis(p, edges, t)[2:] for p in range(n)))
    return strictly_inside(H, ey, ty) and strictly_inside(W, ex, tx)


def assert_not_vacuous(x, spec, luts_ref, out_ref):
    """The guard of the issue, on the reference alone: the output differs from the input, two tiles' LUTs differ (with more
    than one tile) and some pixel blends -- so an identity or a nearest-tile kernel cannot pass the comparison."""
    B, H, W, ch = x.shape
    ty, tx = spec["tiles"]
    assert (out_ref != x).any(), "reference output equals its input"
    if ty * tx > 1:
        flat = luts_ref.reshape(B, ch, ty * tx, 256)
        assert (flat != flat[:, :, :1]).any(), "all tiles share one LUT"
    assert interior_pixel_exists(H, W, (ty, tx)), "no pixel with 0 < ay < Dy and 0 < ax < Dx"
