"""Inputs shared by the CPU and GPU tests of the connected components: the shapes and patterns at which
the kernels are held against ``components_reference``, and the maps and rules at which the filter is held against
``component_filter_reference``.  The restatement's answers are computed once per case and shared."""
import functools
from types import SimpleNamespace

import numpy as np

# (H, W): a single pixel; a row and a column past one tile; the smallest map with diagonals; within one tile; two tiles side by
# side with a one-pixel remainder; two whole 64x64 tiles plus a remainder in each direction, both ways round
SHAPES = [(1, 1), (1, 67), (67, 1), (2, 2), (16, 16), (33, 65), (131, 133), (133, 131)]
BATCHES = (1, 3)
CONNECTIVITIES = (4, 8)
N_CLS = 16                           # the statistics' class count in the pattern tests; pixels of 255 lie outside it


def _grid(H, W):
    return np.mgrid[0:H, 0:W]


def _spiral(H, W):
    g = np.zeros((H, W), np.uint8)
    y = x = 0
    g[0, 0] = 1
    dy, dx, turns = 0, 1, 0
    inside = lambda r, c: 0 <= r < H and 0 <= c < W      # noqa: E731
    while turns < 2:
        ny, nx, fy, fx = y + dy, x + dx, y + 2 * dy, x + 2 * dx
        if inside(ny, nx) and not g[ny, nx] and not (inside(fy, fx) and g[fy, fx]):
            y, x, turns = ny, nx, 0
            g[y, x] = 1
        else:
            dy, dx, turns = dx, -dy, turns + 1
    return g


def layered(B, H, W, C, seed, noise=0.005):
    """A B-scan-like map: C layers whose boundaries wander with the column, and ``noise`` of the pixels replaced by random
    classes."""
    rng = np.random.default_rng(seed)
    y, x = _grid(H, W)
    out = np.empty((B, H, W), np.uint8)
    for b in range(B):
        cuts = [H * (k + 1) / C + 0.04 * H * np.sin((x[0] + 11 * b) / (7.0 + 3 * k)) for k in range(C - 1)]
        out[b] = sum((y >= c[None, :]).astype(np.uint8) for c in cuts)
        hit = rng.random((H, W)) < noise
        out[b][hit] = rng.integers(0, C, size=int(hit.sum()), dtype=np.uint8)
    return out


def _each(fn):
    """A pattern of one image -> the batch: the image, its transpose-free variants per image (rolled by the image index)."""
    def build(B, H, W, seed):
        return np.stack([np.ascontiguousarray(fn(H, W, b)) for b in range(B)]).astype(np.uint8)
    return build


def _serpentine(H, W, b):
    g = np.zeros((H, W), np.uint8)
    g[0::2] = 1
    g[1::4, W - 1] = 1
    g[3::4, 0] = 1
    return g if b % 2 == 0 else g[:, ::-1]


def _comb(H, W, b):
    g = np.zeros((H, W), np.uint8)
    g[:, 0::2] = 1
    g[H - 1] = 1
    return g if b % 2 == 0 else g[::-1]          # (odd images: the teeth meet in the FIRST row)


def _facing(H, W, b):
    g = np.zeros((H, W), np.uint8)
    g[0] = g[H - 1] = 1
    return g


def _random(classes):
    def build(B, H, W, seed):
        return np.random.default_rng(seed).integers(0, classes, size=(B, H, W), dtype=np.uint8)
    return build


def _with_255(B, H, W, seed):
    rng = np.random.default_rng(seed)
    coarse = rng.integers(0, 3, size=(B, (H + 2) // 3, (W + 3) // 4))
    return np.array([0, 1, 255], np.uint8)[np.kron(coarse, np.ones((1, 3, 4), np.int64))[:, :H, :W]]


PATTERNS = {
    "constant": _each(lambda H, W, b: np.full((H, W), 1 + b)),
    "checkerboard": _each(lambda H, W, b: (sum(_grid(H, W)) + b) % 2),
    "h_stripes": _each(lambda H, W, b: (_grid(H, W)[0] + b) % 2),
    "v_stripes": _each(lambda H, W, b: (_grid(H, W)[1] + b) % 2),
    "diagonals_down": _each(lambda H, W, b: (_grid(H, W)[0] - _grid(H, W)[1] + b) % 3),
    "diagonals_up": _each(lambda H, W, b: (sum(_grid(H, W)) + b) % 3),
    "serpentine": _each(_serpentine),
    "comb": _each(_comb),
    "spiral": _each(lambda H, W, b: _spiral(H, W) if b % 2 == 0 else _spiral(H, W)[::-1, ::-1]),
    "random_2": _random(2),
    "random_3": _random(3),
    "random_16": _random(16),
    "layered_noise": lambda B, H, W, seed: layered(B, H, W, 4, seed),
    "with_255": _with_255,
    "facing_rows": _each(_facing),
}


@functools.lru_cache(maxsize=None)
def pattern(name, B, H, W):
    a = PATTERNS[name](B, H, W, 1000 * H + W)
    assert a.shape == (B, H, W) and a.dtype == np.uint8
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def wanted(name, B, H, W, connectivity):
    """``components_reference`` of a pattern, computed once and left unchanged."""
    from oct_image_segmentation_models_amd.common.utils import components_reference
    out = components_reference(pattern(name, B, H, W), N_CLS, connectivity)
    for a in out:
        a.setflags(write=False)
    return out


# ---- the filter --------------------------------------------------------------------------------------------------------------
def rule(n_cls, min_pixels=0, keep_largest=(), fill_mode=0, fill_label=0):
    """The fields of ``oct_component_rule`` as a plain object."""
    mp = [min_pixels] * n_cls if isinstance(min_pixels, int) else list(min_pixels)
    assert len(mp) == n_cls
    return SimpleNamespace(min_pixels=mp + [0] * (32 - n_cls), keep_largest=sum(1 << c for c in keep_largest),
                           fill_mode=fill_mode, fill_label=fill_label)


def _ties(B):
    """Classes 1 and 2 with two equally large largest components each (and a smaller one), on a background of 0; image b is
    shifted by b so that the roots differ between the images.  70x75: the components lie in different 64x64 tiles."""
    a = np.zeros((B, 70, 75), np.uint8)
    for b in range(B):
        a[b, 2 + b:7 + b, 2:7] = 1
        a[b, 2 + b:7 + b, 66:71] = 1               # same rows: the one to the west has the smaller root
        a[b, 30:33, 30:33] = 1
        a[b, 66:70, 10:14] = 2
        a[b, 40:44, 60:64] = 2                     # the later one in memory order is higher up: rows decide, not columns
        a[b, 50, 50] = 2
    return a


def _crafted(B):
    """3 classes on 70x75.  Column 7 is class 2 from top to bottom (70 pixels; a 10x10 block of class 2 elsewhere is larger):
    removed under keep_largest, it is a column with no kept pixel of a class < 3 -- one of its pixels is 255, which is kept
    and is no source.  Column 12 starts with a two-pixel speck of class 1 over two pixels of 255 over class 0: its kept
    sources lie only below.  Further specks sit inside the layers."""
    a = np.zeros((B, 70, 75), np.uint8)
    a[:, 35:] = 1
    a[:, :, 7] = 2
    a[:, 33, 7] = 255
    a[:, 45:55, 20:30] = 2
    a[:, 0:2, 12] = 1
    a[:, 2:4, 12] = 255
    for b in range(B):
        a[b, 50 + b, 40:42] = 0                    # a speck of class 0 inside class 1: the column rule gives it class 1
        a[b, 10, 63:65] = 1                        # two pixels across a tile border
        a[b, 69, 70] = 0                           # a speck in the last row: sources lie only above
    return a


@functools.lru_cache(maxsize=None)
def filter_cases():
    """name -> (labels (B,H,W), n_cls, connectivity, rule).  Every case removes at least one pixel and keeps at least one, on
    the restatement: asserted here."""
    from oct_image_segmentation_models_amd.common.utils import component_filter_reference, components_reference
    noisy, rnd = layered(3, 131, 133, 4, seed=5), _random(3)(3, 33, 65, 9)
    cases = {
        "min_pixels_constant": (noisy, 4, 8, rule(4, 20, fill_label=2)),
        "min_pixels_column": (noisy, 4, 8, rule(4, [20, 0, 20, 20], fill_mode=1)),
        "min_pixels_column_b1": (noisy[:1], 4, 4, rule(4, 20, fill_mode=1, fill_label=3)),
        "keep_largest_tie_constant": (_ties(3), 3, 8, rule(3, keep_largest=(1, 2), fill_label=0)),
        "keep_largest_tie_column": (_ties(3), 3, 4, rule(3, keep_largest=(1, 2), fill_mode=1, fill_label=9)),
        "both_random_column": (rnd, 3, 4, rule(3, [4, 0, 6], keep_largest=(1,), fill_mode=1, fill_label=1)),
        "both_random_constant": (rnd, 3, 8, rule(3, [4, 2, 600], keep_largest=(0, 1, 2), fill_label=200)),
        "crafted_constant": (_crafted(3), 3, 8, rule(3, [3, 3, 0], keep_largest=(2,), fill_label=7)),
        "crafted_column": (_crafted(3), 3, 8, rule(3, [3, 3, 0], keep_largest=(2,), fill_mode=1, fill_label=9)),
        "crafted_column_n_cls_2": (_crafted(1), 2, 4, rule(2, [3, 3], fill_mode=1, fill_label=5)),
        "one_pixel_images": (np.array([[[1]], [[0]], [[1]]], np.uint8), 2, 8, rule(2, [0, 2], fill_mode=1, fill_label=4)),
    }
    out = {}
    for name, (labels, n_cls, conn, r) in cases.items():
        labels = np.ascontiguousarray(labels)
        root, size, stats = components_reference(labels, n_cls, conn)
        clean, removed = component_filter_reference(labels, root, size, n_cls, r)
        assert removed.sum() >= 1 and removed.sum() == (clean != labels).sum() + _same_label_fills(labels, clean, root, size, n_cls, r)
        assert removed.sum() < (labels < n_cls).sum(), name        # at least one pixel is kept
        for a in (labels, root, size, stats, clean, removed):
            a.setflags(write=False)
        out[name] = SimpleNamespace(labels=labels, n_cls=n_cls, connectivity=conn, rule=r, root=root, size=size, stats=stats,
                                    clean=clean, removed=removed)
    crafted = out["crafted_column"]
    assert (crafted.clean[:, :, 7] == np.where(crafted.labels[:, :, 7] == 255, 255, 9)).all()      # no kept pixel: fill_label
    assert (crafted.clean[:, 0:2, 12] == 0).all() and (crafted.clean[:, 2:4, 12] == 255).all()      # sources only below
    tie = out["keep_largest_tie_constant"]
    assert (tie.clean[0, 2:7, 2:7] == 1).all() and (tie.clean[0, 2:7, 66:71] == 0).all()            # the smaller root stays
    assert (tie.clean[0, 40:44, 60:64] == 2).all() and (tie.clean[0, 66:70, 10:14] == 0).all()
    return out


def _same_label_fills(labels, clean, root, size, n_cls, r):
    """Removed pixels that were filled with the byte they had (a constant fill equal to the class): they do not show in
    ``clean != labels``."""
    from oct_image_segmentation_models_amd.common.utils import component_filter_reference
    other = SimpleNamespace(**{**vars(r), "fill_mode": 0, "fill_label": 254})
    gone = component_filter_reference(labels, root, size, n_cls, other)[0] != labels
    return int((gone & (clean == labels)).sum())
