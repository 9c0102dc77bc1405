"""Shared inputs of tests/test_render.py and tests/test_gpu_render.py: each case is the keyword set of
``common.plotting.render_reference`` (base, palette, lines, colours, styles, col_range, half_width), built from seeds and
closed forms only."""
import numpy as np

LINE_RGB = [(200, 20, 60), (10, 220, 30), (30, 40, 250), (250, 240, 10)]


def scans(B, H, W, ic, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (B, H, W, ic), dtype=np.uint8)


def label_maps(B, H, W, C, seed=0, stray=3):
    """Class maps holding every class 0..C-1 and ``stray`` pixels per image with labels >= C (they render black)."""
    rng = np.random.default_rng(seed)
    lab = rng.integers(0, C, (B, H, W)).astype(np.uint8)
    lab[:, 0, :C] = np.arange(C, dtype=np.uint8)
    for b in range(B):
        for k in range(stray):
            lab[b, (5 * k + 1) % H, (7 * k + 2) % W] = (C, 255, C + 9)[k % 3]
    return lab


def palette(C):
    from oct_image_segmentation_models_amd.common import plotting
    return plotting.region_palette(C)


def flat_line(H=16, W=40, row=8, bg=100, rgb=LINE_RGB[0], **kw):
    """The analytic case: an interior flat line over a constant base."""
    return dict(base=np.full((1, H, W, 1), bg, np.uint8), lines=np.full((1, 1, W), row, np.uint16), colours=[rgb], **kw)


def mixed_lines(B=2, H=36, W=68, **kw):
    """K = 4 on 36x68: line 0 solid with a jump of 30 rows between columns 19 and 20, ten columns of zeros and a run of
    rows >= H; line 1 dotted at row 1 and line 2 solid at row H-1, which clip at the top and bottom edge; line 3 dotted at
    row H-1 as well, drawn over line 2."""
    c = np.arange(W)
    rows = np.zeros((B, 4, W), np.uint16)
    for b in range(B):
        l0 = np.where(c < 20, 1 + (c % 3), H - 3 - (c % 2))
        assert l0[20] - l0[19] >= 30
        l0[40:50] = 0
        l0[55:61] = [H, H + 1, 65535, 4000, H + 7, H]
        rows[b, 0] = np.roll(l0, b)
        rows[b, 1] = 1
        rows[b, 2] = H - 1
        rows[b, 3] = H - 1
    return dict(base=scans(B, H, W, 1, seed=5), lines=rows, colours=LINE_RGB, styles=[0, 1, 0, 1], **kw)


def crossing_lines(H=20, W=34, K=14, B=1):
    """K lines of different slopes that cross each other, alternately solid and dotted; slopes wrap inside the image, so
    steep segments occur."""
    c = np.arange(W)
    rows = np.stack([1 + ((3 * k + (c * (k - 6)) // 2) % (H - 2)) for k in range(K)]).astype(np.uint16)
    colours = [((37 * k) % 256, (91 * k + 50) % 256, (160 * k + 20) % 256) for k in range(K)]
    return dict(base=scans(B, H, W, 3, seed=9), lines=np.tile(rows[None], (B, 1, 1)), colours=colours,
                styles=[k % 2 for k in range(K)])


def wavy_lines(B, H, W, K=3, seed=0, ic=1):
    """Smooth boundaries with holes, as a search emits them."""
    rng = np.random.default_rng(seed)
    c = np.arange(W)
    rows = np.zeros((B, K, W), np.uint16)
    for b in range(B):
        for k in range(K):
            r = (k + 1) * H / (K + 1) + (H / 6.0) * np.sin(c / 5.0 + b + 2 * k)
            r = np.clip(np.rint(r), 0, H + 1).astype(np.uint16)
            r[rng.integers(0, W, 2)] = 0
            rows[b, k] = r
    return dict(base=scans(B, H, W, ic, seed=seed + 1), lines=rows, colours=LINE_RGB[:K], styles=[k % 2 for k in range(K)])


def tall_jump(H=4096, W=12):
    """A 1 -> 4095 jump at 4096 rows: the largest products of the sample test."""
    rows = np.ones((1, 2, W), np.uint16)
    rows[0, 0, W // 2:] = H - 1
    rows[0, 1] = np.where(np.arange(W) % 2 == 0, 1, H - 1)
    return dict(base=scans(1, H, W, 1, seed=3), lines=rows, colours=LINE_RGB[:2], styles=[0, 1])
