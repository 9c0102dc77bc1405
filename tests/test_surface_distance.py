"""CPU tests of the surface-distance metrics' host restatement (common/custom_metrics.py): against a brute-force
pairwise oracle written here (every border cell of one mask against every border cell of the other), closed forms,
and -- where scipy is installed -- a literal restatement of google-deepmind/surface-distance's 2D path."""
import numpy as np
import pytest

from oct_image_segmentation_models_amd.common import custom_metrics as cm
from oracle import unet_numpy as on

REF_SPACING = (0.01111111, 0.01111111)
ANISO = (0.0039, 0.0111)

# contour length by 2x2 code (issue table): codes 1,2,4,7,8,11,13,14 -> d; 3,12 -> h; 5,10 -> v; 6,9 -> 2d
_D_CODES, _H_CODES, _V_CODES, _2D_CODES = (1, 2, 4, 7, 8, 11, 13, 14), (3, 12), (5, 10), (6, 9)


def _code_lengths(spacing):
    v, h = spacing
    d = 0.5 * np.sqrt(v * v + h * h)
    t = np.zeros(16)
    t[list(_D_CODES)], t[list(_H_CODES)], t[list(_V_CODES)], t[list(_2D_CODES)] = d, h, v, 2 * d
    return t


def _codes(mask):
    H, W = mask.shape
    m = np.zeros((H + 2, W + 2), np.int64)
    m[1:-1, 1:-1] = mask
    out = np.zeros((H + 1, W + 1), np.int64)
    for i in range(H + 1):
        for j in range(W + 1):
            out[i, j] = 8 * m[i, j] + 4 * m[i, j + 1] + 2 * m[i + 1, j] + m[i + 1, j + 1]
    return out


def _brute_directed(src_codes, dst_codes, spacing, table):
    si, sj = np.nonzero((src_codes != 0) & (src_codes != 15))
    di, dj = np.nonzero((dst_codes != 0) & (dst_codes != 15))
    lens = table[src_codes[si, sj]]
    if di.size == 0:
        return np.full(si.size, np.inf), lens
    dist = np.empty(si.size)
    for k0 in range(0, si.size, 512):
        a = spacing[0] * (si[k0:k0 + 512, None] - di[None, :]).astype(np.float64)
        b = spacing[1] * (sj[k0:k0 + 512, None] - dj[None, :]).astype(np.float64)
        dist[k0:k0 + 512] = np.sqrt((a * a + b * b).min(axis=1))
    return dist, lens


def _percentile_candidates(dist, lens, percent):
    """The package's selection (plain float cumsum), with both neighbours admitted where cumsum/total lies within 1e-12
    of percent/100 at the chosen group."""
    if dist.size == 0:
        return [np.inf]
    o = np.lexsort((lens, dist))
    d, c = dist[o], np.cumsum(lens[o]) / np.sum(lens)
    q, n = percent / 100.0, d.size
    idx = int(np.searchsorted(c, q))
    cand = {d[min(idx, n - 1)]}
    for k in (idx - 1, idx, idx + 1):
        if 0 <= k < n and abs(c[k] - q) < 1e-12:
            cand.update({d[k], d[min(k + 1, n - 1)]})
    return sorted(cand)


def brute(gt, pred, spacing, percent):
    table = _code_lengths(spacing)
    cg, cp = _codes(gt.astype(np.int64)), _codes(pred.astype(np.int64))
    dg, lg = _brute_directed(cg, cp, spacing, table)
    dp, lp = _brute_directed(cp, cg, spacing, table)
    with np.errstate(invalid="ignore"):
        asd = (np.sum(dg * lg) / np.sum(lg), np.sum(dp * lp) / np.sum(lp))
    return asd, _percentile_candidates(dg, lg, percent), _percentile_candidates(dp, lp, percent), (dg.size, dp.size)


def _close(a, b, rel):
    if np.isnan(a) or np.isnan(b):
        return np.isnan(a) and np.isnan(b)
    if np.isinf(a) or np.isinf(b):
        return a == b
    return abs(a - b) <= rel * max(abs(a), abs(b))


def check_against_brute(gt, pred, spacing, percent):
    asd_ref, cg, cp, _ = brute(gt, pred, spacing, percent)
    sd = cm.compute_surface_distances(gt, pred, spacing)
    asd = cm.average_surface_distance(gt, pred, spacing)
    assert _close(asd[0], asd_ref[0], 1e-12) and _close(asd[1], asd_ref[1], 1e-12), (asd, asd_ref)
    pg = cm._robust_percentile(sd["distances_gt_to_pred"], sd["surfel_kinds_gt"], sd["surfel_lengths"], percent)
    pp = cm._robust_percentile(sd["distances_pred_to_gt"], sd["surfel_kinds_pred"], sd["surfel_lengths"], percent)
    assert any(_close(pg, c, 1e-12) for c in cg), (pg, cg)
    assert any(_close(pp, c, 1e-12) for c in cp), (pp, cp)
    assert cm.hausdorff_distance(gt, pred, spacing, percent) == max(pg, pp)


def _scan_masks(H, W, C, seed):
    _, labels = on.synth_scans(1, H, W, C, seed=seed)
    return labels[0, :, :, 0]


@pytest.mark.parametrize("percent", [0, 50, 95, 100])
@pytest.mark.parametrize("spacing", [REF_SPACING, ANISO])
def test_synthetic_scans_shifted_and_noisy(percent, spacing):
    lab = _scan_masks(48, 96, 3, seed=5)
    rng = np.random.default_rng(3)
    shifted = np.roll(lab, (2, -3), axis=(0, 1))
    noisy = lab.copy()
    flip = rng.random(lab.shape) < 0.05
    noisy[flip] = rng.integers(0, 3, int(flip.sum()))
    for pred in (lab, shifted, noisy):
        for c in (1, 2):
            check_against_brute(lab == c, pred == c, spacing, percent)


@pytest.mark.parametrize("percent", [0, 50, 95, 100])
def test_single_pixels_and_edges(percent):
    H, W = 17, 23
    a = np.zeros((H, W), bool); a[4, 7] = True
    b = np.zeros((H, W), bool); b[12, 19] = True
    check_against_brute(a, b, ANISO, percent)
    edge = np.zeros((H, W), bool); edge[:, :5] = True; edge[0, :] = True        # touches three image edges
    full = np.ones((H, W), bool)
    corner = np.zeros((H, W), bool); corner[-3:, -4:] = True
    for g, p in ((edge, full), (full, corner), (edge, corner), (a, edge)):
        check_against_brute(g, p, ANISO, percent)
        check_against_brute(p, g, REF_SPACING, percent)


def test_random_masks():
    rng = np.random.default_rng(11)
    for _ in range(4):
        g = rng.random((31, 45)) < 0.4
        p = rng.random((31, 45)) < 0.6
        for percent in (0, 50, 95, 100):
            check_against_brute(g, p, ANISO, percent)


def test_closed_forms():
    lab = _scan_masks(40, 64, 3, seed=2) == 1
    assert cm.average_surface_distance(lab, lab, REF_SPACING) == (0.0, 0.0)
    assert cm.hausdorff_distance(lab, lab, REF_SPACING, 95) == 0.0
    empty = np.zeros_like(lab)
    a, b = cm.average_surface_distance(lab, empty, REF_SPACING)
    assert a == np.inf and np.isnan(b)
    assert np.isnan((a + b) / 2) and cm.hausdorff_distance(lab, empty, REF_SPACING, 95) == np.inf
    a, b = cm.average_surface_distance(empty, lab, REF_SPACING)
    assert np.isnan(a) and b == np.inf
    a, b = cm.average_surface_distance(empty, empty, REF_SPACING)
    assert np.isnan(a) and np.isnan(b) and cm.hausdorff_distance(empty, empty, REF_SPACING, 95) == np.inf
    with pytest.raises(ValueError):
        cm.hausdorff_distance(lab, lab, REF_SPACING, 101)


def test_translation_gives_exact_distance():
    g = np.zeros((30, 40), bool); g[5:15, 8:30] = True
    p = np.roll(g, 3, axis=0)                                  # every horizontal edge moves 3 rows
    v, h = ANISO
    sd = cm.compute_surface_distances(g, p, ANISO)
    assert sd["distances_gt_to_pred"].max() <= 3 * v + 1e-15
    assert cm.hausdorff_distance(g, p, ANISO, 100) == pytest.approx(3 * v, rel=1e-12)


def _package_literal(mask_gt, mask_pred, spacing, percent):
    """google-deepmind/surface-distance compute_surface_distances + compute_average_surface_distance +
    compute_robust_hausdorff (2D), restated with scipy as the package runs it: bounding-box crop padded by one row and
    column, ndimage.correlate with [[8,4],[2,1]], distance_transform_edt(sampling=spacing), sorted(zip(...))."""
    ndimage = pytest.importorskip("scipy.ndimage")
    table = _code_lengths(spacing)
    both = mask_gt | mask_pred
    if not both.any():
        return (np.nan, np.nan), np.inf
    rows, cols = np.nonzero(both)
    r0, r1, c0, c1 = rows.min(), rows.max(), cols.min(), cols.max()

    def crop(m):
        out = np.zeros((r1 - r0 + 2, c1 - c0 + 2), np.uint8)
        out[:-1, :-1] = m[r0:r1 + 1, c0:c1 + 1]
        return out

    kernel = np.array([[8, 4], [2, 1]])
    code_gt = ndimage.correlate(crop(mask_gt), kernel, mode="constant", cval=0)
    code_pred = ndimage.correlate(crop(mask_pred), kernel, mode="constant", cval=0)
    border_gt, border_pred = (code_gt != 0) & (code_gt != 15), (code_pred != 0) & (code_pred != 15)
    dist_gt = ndimage.distance_transform_edt(~border_gt, sampling=spacing) if border_gt.any() else np.full(border_gt.shape, np.inf)
    dist_pred = ndimage.distance_transform_edt(~border_pred, sampling=spacing) if border_pred.any() else np.full(border_pred.shape, np.inf)
    d_gp, d_pg = dist_pred[border_gt], dist_gt[border_pred]
    a_g, a_p = table[code_gt][border_gt], table[code_pred][border_pred]
    if d_gp.size:
        d_gp, a_g = map(np.array, zip(*sorted(zip(d_gp, a_g))))
    if d_pg.size:
        d_pg, a_p = map(np.array, zip(*sorted(zip(d_pg, a_p))))
    with np.errstate(invalid="ignore"):
        asd = (np.sum(d_gp * a_g) / np.sum(a_g), np.sum(d_pg * a_p) / np.sum(a_p))

    def perc(d, a):
        if d.size == 0:
            return np.inf
        idx = np.searchsorted(np.cumsum(a) / np.sum(a), percent / 100.0)
        return d[min(idx, d.size - 1)]
    return asd, (perc(d_gp, a_g), perc(d_pg, a_p))


@pytest.mark.parametrize("spacing", [REF_SPACING, ANISO])
def test_matches_package_literal_with_scipy(spacing):
    pytest.importorskip("scipy")
    lab = _scan_masks(64, 128, 4, seed=9)
    rng = np.random.default_rng(4)
    noisy = lab.copy()
    flip = rng.random(lab.shape) < 0.05
    noisy[flip] = rng.integers(0, 4, int(flip.sum()))
    for pred in (lab, np.roll(lab, 2, axis=0), noisy, rng.integers(0, 4, lab.shape)):
        for c in (1, 2, 3):
            g, p = lab == c, pred == c
            for percent in (0, 50, 95, 100):
                asd_ref, perc_ref = _package_literal(g, p, spacing, percent)
                asd = cm.average_surface_distance(g, p, spacing)
                assert _close(asd[0], asd_ref[0], 1e-12) and _close(asd[1], asd_ref[1], 1e-12), (asd, asd_ref)
                sd = cm.compute_surface_distances(g, p, spacing)
                pg = cm._robust_percentile(sd["distances_gt_to_pred"], sd["surfel_kinds_gt"], sd["surfel_lengths"], percent)
                pp = cm._robust_percentile(sd["distances_pred_to_gt"], sd["surfel_kinds_pred"], sd["surfel_lengths"], percent)
                # the package's float cumsum can land on the other side of percent/100 only within rounding of it
                ok_g = _close(pg, perc_ref[0], 1e-12) or any(_close(pg, c, 1e-12) for c in _percentile_candidates(
                    sd["distances_gt_to_pred"], sd["surfel_areas_gt"], percent))
                ok_p = _close(pp, perc_ref[1], 1e-12) or any(_close(pp, c, 1e-12) for c in _percentile_candidates(
                    sd["distances_pred_to_gt"], sd["surfel_areas_pred"], percent))
                assert ok_g and ok_p, (pg, pp, perc_ref)
