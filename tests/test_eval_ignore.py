"""CPU tests of the evaluation's ignore label: the numpy restatements the masked kernels are tested
against -- masked confusion counts, ``compute_surface_distances(..., valid=)``, ``generate_boundary_masked`` -- and the
``EvaluationParameters`` switch.  The brute-force surface oracle is the one of tests/test_surface_distance.py, restricted to
the cells that rule 3 keeps."""
import json

import numpy as np
import pytest

from oct_image_segmentation_models_amd.common import custom_metrics as cm
from oct_image_segmentation_models_amd.evaluation import dice_device as dd
from oct_image_segmentation_models_amd.min_path_processing.utils import generate_boundary, generate_boundary_masked
from oracle import unet_numpy as on
from tests import test_surface_distance as tsd

ANISO = tsd.ANISO


# ---- rule 2: confusion counts and Dice of the counted pixels ----

def _maps(C, ignore, seed, shape=(3, 19, 27), frac=0.15):
    rng = np.random.default_rng(seed)
    gt = rng.integers(0, C, shape).astype(np.uint8)
    pred = rng.integers(0, C, shape).astype(np.uint8)
    gt[rng.random(shape) < frac] = ignore
    return pred, gt


@pytest.mark.parametrize("C", [3, 8])
@pytest.mark.parametrize("ignore_at", ["255", "C"])
def test_masked_confusion_against_brute_force(C, ignore_at):
    ignore = 255 if ignore_at == "255" else C
    pred, gt = _maps(C, ignore, seed=C)
    pred[0, 0, :5] = C + 1                       # out-of-range predictions: two on counted pixels, three on ignored ones
    gt[0, 0, :2], gt[0, 0, 2:5] = 1, ignore
    rows = dd.confusion_counts_reference(pred, gt, C, ignore)
    assert rows.dtype == np.uint32 and rows.shape == (3, C * C + 2)
    for b in range(3):
        brute = np.zeros(C * C + 2, np.int64)
        for p, g in zip(pred[b].ravel(), gt[b].ravel()):
            brute[C * C + 1 if g == ignore else C * C if (p >= C or g >= C) else g * C + p] += 1
        assert np.array_equal(rows[b], brute)
    assert rows[0, C * C] == 2 and (rows[1:, C * C] == 0).all() and (rows[:, C * C + 1] > 0).all()
    assert rows.sum(axis=1).tolist() == [19 * 27] * 3
    with pytest.raises(ValueError, match="image 5"):
        dd.counts_matrix(rows, C, first_image=5, ignored=True)
    m = dd.counts_matrix(rows[1:], C, ignored=True)
    assert m.shape == (2, C, C) and np.array_equal(m.reshape(2, -1), rows[1:, :C * C])
    # without the switch the rows and the unmasked restatement are today's
    assert dd.confusion_counts_reference(pred, np.minimum(gt, C - 1), C).shape == (3, C * C + 1)


def test_other_out_of_range_value_still_raises():
    pred, gt = _maps(3, 255, seed=1)
    gt[2, 4, 4] = 200
    rows = dd.confusion_counts_reference(pred, gt, 3, 255)
    with pytest.raises(ValueError, match="image 2: 1 pixels carry a label outside 0..2"):
        dd.counts_matrix(rows, 3, ignored=True)
    for bad in (2, 256, -1, 3.0, True, "255"):
        with pytest.raises(ValueError, match="ignore_label"):
            dd.confusion_counts_reference(pred, gt, 3, bad)
    with pytest.raises(ValueError, match="words"):
        dd.counts_matrix(rows, 3)                # masked rows read as unmasked ones


@pytest.mark.parametrize("C,ignore", [(3, 255), (3, 3), (8, 255), (8, 8)])
def test_dice_from_masked_counts_equals_host_masked_dice(C, ignore):
    from oct_image_segmentation_models_amd.common import utils
    from oct_image_segmentation_models_amd.evaluation.evaluation import _dice_metrics, _masked_onehot
    pred, gt = _maps(C, ignore, seed=10 + C, shape=(2, 24, 40))
    gt[1] = ignore                                # an image without a counted pixel: micro 0/0 = NaN on both sides
    counts = dd.counts_matrix(dd.confusion_counts_reference(pred, gt, C, ignore), C, ignored=True)
    for b in range(2):
        onehot, keep = _masked_onehot(gt[b], C, ignore)
        assert np.array_equal(keep, gt[b] != ignore) and not onehot[~keep].any() and (onehot[keep].sum(axis=-1) == 1).all()
        cat = utils.labels_to_categorical(pred[b:b + 1].astype(np.int64), C) * keep.astype(np.float32)      # (1,C,H,W)
        plain = _dice_metrics(dd.DICE_METRICS, C, onehot, cat)
        transposed = _dice_metrics(dd.DICE_METRICS, C, onehot, np.transpose(cat, (0, 1, 3, 2)), transposed=True)
        got = dd.dice_from_counts(counts[b], dd.DICE_METRICS)
        for host in (plain, transposed):
            for h, g in zip(host, got):
                assert np.asarray(h).dtype == np.asarray(g).dtype and np.shape(h) == np.shape(g)
                assert np.asarray(h).tobytes() == np.asarray(g).tobytes()
    assert np.isnan(got[2])


# ---- rule 3: surface distances inside the labelled region ----

def _brute_masked(gt, pred, valid, spacing, percent):
    """tests/test_surface_distance.py::brute over the kept cells: a cell with an unknown in-image pixel gets code 0."""
    table = tsd._code_lengths(spacing)
    unknown = np.pad(~valid, 1)
    drop = unknown[:-1, :-1] | unknown[:-1, 1:] | unknown[1:, :-1] | unknown[1:, 1:]
    cg, cp = tsd._codes(gt.astype(np.int64)), tsd._codes(pred.astype(np.int64))
    cg[drop], cp[drop] = 0, 0
    dg, lg = tsd._brute_directed(cg, cp, spacing, table)
    dp, lp = tsd._brute_directed(cp, cg, spacing, table)
    with np.errstate(invalid="ignore"):
        asd = (np.sum(dg * lg) / np.sum(lg), np.sum(dp * lp) / np.sum(lp))
    return asd, tsd._percentile_candidates(dg, lg, percent), tsd._percentile_candidates(dp, lp, percent), (dg.size, dp.size)


def _check_masked(gt, pred, valid, spacing, percent, want_surfels=True):
    asd_ref, cg, cp, n = _brute_masked(gt, pred, valid, spacing, percent)
    sd = cm.compute_surface_distances(gt, pred, spacing, valid=valid)
    assert (sd["distances_gt_to_pred"].size, sd["distances_pred_to_gt"].size) == n
    assert not want_surfels or min(n) > 0
    asd = cm.compute_average_surface_distance(sd)
    assert tsd._close(asd[0], asd_ref[0], 1e-12) and tsd._close(asd[1], asd_ref[1], 1e-12), (asd, asd_ref)
    L = sd["surfel_lengths"]
    pg = cm._robust_percentile(sd["distances_gt_to_pred"], sd["surfel_kinds_gt"], L, percent)
    pp = cm._robust_percentile(sd["distances_pred_to_gt"], sd["surfel_kinds_pred"], L, percent)
    assert any(tsd._close(pg, c, 1e-12) for c in cg) and any(tsd._close(pp, c, 1e-12) for c in cp)
    return sd


def test_valid_all_true_is_the_unmasked_call():
    lab = tsd._scan_masks(40, 64, 3, seed=2)
    pred = np.roll(lab, (2, -3), axis=(0, 1))
    for c in (1, 2):
        a = cm.compute_surface_distances(lab == c, pred == c, ANISO)
        b = cm.compute_surface_distances(lab == c, pred == c, ANISO, valid=np.ones(lab.shape, bool))
        assert sorted(a) == sorted(b)
        for k in a:
            assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), k
    with pytest.raises(ValueError, match="valid"):
        cm.compute_surface_distances(lab == 1, pred == 1, ANISO, valid=np.ones((3, 3), bool))


@pytest.mark.parametrize("percent", [0, 50, 95, 100])
@pytest.mark.parametrize("region", ["rectangle", "left_strip", "last_row", "scattered"])
def test_masked_surface_distances_against_brute_force(region, percent):
    H, W = 33, 47
    lab = tsd._scan_masks(H, W, 3, seed=5)
    rng = np.random.default_rng(3)
    noisy = lab.copy()
    flip = rng.random(lab.shape) < 0.05
    noisy[flip] = rng.integers(0, 3, int(flip.sum()))
    valid = np.ones((H, W), bool)
    if region == "rectangle":                    # crosses both class surfaces
        valid[5:28, 10:20] = False
    elif region == "left_strip":
        valid[:, :4] = False
    elif region == "last_row":
        valid[-1, :] = False
    else:
        valid[rng.random((H, W)) < 0.1] = False
    removed = 0
    for pred in (np.roll(lab, (2, -3), axis=(0, 1)), noisy):
        for c in (1, 2):
            for spacing in (tsd.REF_SPACING, ANISO):
                sd = _check_masked(lab == c, pred == c, valid, spacing, percent)
                full = cm.compute_surface_distances(lab == c, pred == c, spacing)
                assert sd["distances_gt_to_pred"].size <= full["distances_gt_to_pred"].size
                removed += full["distances_gt_to_pred"].size - sd["distances_gt_to_pred"].size
    assert removed > 0                           # the mask took surfels away
    # the rim of the unknown region is no surface: a mask that is constant wherever it is known has no surfel at all
    blob = np.zeros((H, W), bool)
    blob[~valid] = True
    sd = cm.compute_surface_distances(blob, blob, ANISO, valid=valid)
    assert sd["distances_gt_to_pred"].size == 0 and sd["distances_pred_to_gt"].size == 0


def test_everything_ignored_gives_nan_nan_inf():
    lab = tsd._scan_masks(20, 30, 3, seed=4) == 1
    valid = np.zeros(lab.shape, bool)
    sd = _check_masked(lab, np.roll(lab, 2, axis=0), valid, ANISO, 95, want_surfels=False)
    a, b = cm.compute_average_surface_distance(sd)
    assert np.isnan(a) and np.isnan(b) and cm.compute_robust_hausdorff(sd, 95) == np.inf
    # every second row and column unknown: every cell touches an unknown pixel
    valid = np.ones(lab.shape, bool)
    valid[::2, :], valid[:, ::2] = False, False
    sd = cm.compute_surface_distances(lab, lab, ANISO, valid=valid)
    assert sd["distances_gt_to_pred"].size == 0 and cm.compute_robust_hausdorff(sd, 95) == np.inf


# ---- rule 4: truth boundaries ----

def _layers(H, W, tops):
    """A (H, W) map of len(tops) + 1 stacked classes: class i starts at row tops[i-1][col]."""
    lab = np.zeros((H, W), np.int64)
    for i, t in enumerate(tops, start=1):
        lab[np.arange(H)[:, None] >= np.asarray(t)[None, :]] = i
    return lab


def test_generate_boundary_masked_equals_generate_boundary_without_ignored_pixels():
    for C, seed in ((3, 1), (4, 2), (8, 3)):
        _, lab = on.synth_scans(3, 32, 48, C, seed=seed)
        maps = lab[..., 0]
        assert maps.max() == C - 1
        for axis, m in ((1, maps), (0, maps[0])):
            a, b = generate_boundary(m, axis=axis), generate_boundary_masked(m, C, 255, axis=axis)
            assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)
    # the masked form always has C - 1 rows; generate_boundary follows the largest value present
    two = np.minimum(maps, 1)
    assert generate_boundary(two, axis=1).shape[0] == 1 and generate_boundary_masked(two, 8, 255, axis=1).shape[0] == 7
    assert not generate_boundary_masked(two, 8, 255, axis=1)[1:].any()


def test_generate_boundary_masked_rules():
    H, W = 12, 6
    tops = [np.full(W, 3), np.full(W, 6), np.full(W, 9)]
    lab = _layers(H, W, tops)
    clean = generate_boundary_masked(lab, 4, 255)
    assert np.array_equal(clean, np.stack(tops))
    strip = lab.copy()
    strip[10:, :] = 255                          # an ignored strip at the bottom: every boundary lies above it
    assert np.array_equal(generate_boundary_masked(strip, 4, 255), clean)
    hole = lab.copy()
    hole[4, 2] = 255                             # inside class 1, column 2: above boundaries 2 and 3, below boundary 1
    got = generate_boundary_masked(hole, 4, 255)
    expect = clean.copy()
    expect[1:, 2] = 0
    assert np.array_equal(got, expect)
    top = lab.copy()
    top[0, 5] = 255                              # at the top of column 5: all three boundaries lie under it
    expect = clean.copy()
    expect[:, 5] = 0
    assert np.array_equal(generate_boundary_masked(top, 4, 255), expect)
    on_boundary = lab.copy()
    on_boundary[6, 1] = 255                      # the boundary pixel itself is unknown: the first KNOWN row of class 2 lies under it
    expect = clean.copy()
    expect[1:, 1] = 0
    assert np.array_equal(generate_boundary_masked(on_boundary, 4, 255), expect)
    column = lab.copy()
    column[:, 3] = 255                           # a fully ignored column
    expect = clean.copy()
    expect[:, 3] = 0
    assert np.array_equal(generate_boundary_masked(column, 4, 255), expect)
    # ignore == C, and the batched form evaluate_model uses (axis 1 of (n, H, W))
    hole4 = np.where(hole == 255, 4, hole)
    assert np.array_equal(generate_boundary_masked(hole4, 4, 4), got)
    batch = np.stack([lab, hole, column])
    b = generate_boundary_masked(batch, 4, 255, axis=1)
    assert b.shape == (3, 3, W) and np.array_equal(b[:, 1], got) and np.array_equal(b[:, 0], clean)


# ---- the switch ----

def test_evaluation_parameters_validates_ignore_label(tmp_path):
    """The constructor loads a model: a freshly saved untrained one will do (no device is touched)."""
    from oct_image_segmentation_models_amd.evaluation.evaluation_parameters import EvaluationParameters, EvaluationSaveParams
    from oct_image_segmentation_models_amd.models.engine_model import Model
    cfg = dict(input_channels=1, num_classes=3, image_height=16, image_width=16, pool_layers=2)
    model = Model(name="unet", config=cfg)
    model.set_weights(on.keras_weight_list(*on.init_params(on.UNetConfig(num_classes=3, pool_layers=2), seed=3, dtype=np.float32)))
    model.save(tmp_path / "model.npz")
    with open(tmp_path / "model_config.json", "w") as fh:
        json.dump(cfg, fh)

    def make(**kw):
        return EvaluationParameters(tmp_path / "model.npz", None, None, tmp_path / "d.hdf5", tmp_path / "e",
                                    EvaluationSaveParams(), False, ["dice_coef_macro"], **kw)

    assert make().ignore_label is None and make(ignore_label=None).ignore_label is None
    for ok in (3, 200, 255, np.uint8(255)):
        p = make(ignore_label=ok)
        assert p.ignore_label == int(ok) and type(p.ignore_label) is int
    for bad in (0, 2, -1, 256, 1000, 255.0, "255", True):
        with pytest.raises(ValueError, match="ignore_label"):
            make(ignore_label=bad)


def test_ignore_label_is_on_every_layer_of_the_evaluation():
    import inspect
    from oct_image_segmentation_models_amd.evaluation.evaluation_parameters import EvaluationParameters
    from oct_image_segmentation_models_amd.evaluation.pipeline import BatchedPredictor, InferenceRun, host_batches
    from oct_image_segmentation_models_amd.evaluation.surface import SurfaceDistances
    for fn in (EvaluationParameters.__init__, InferenceRun.__init__, InferenceRun.render_pngs, SurfaceDistances.__init__,
               dd.ConfusionCounts.__init__, dd.DelineationLabels.__init__, dd.confusion_counts_reference):
        assert inspect.signature(fn).parameters["ignore_label"].default is None, fn
    assert inspect.signature(dd.counts_matrix).parameters["ignored"].default is False
    for fn in (BatchedPredictor.__init__, host_batches):                 # the sources hold no per-stage switch
        assert "ignore_label" not in inspect.signature(fn).parameters
