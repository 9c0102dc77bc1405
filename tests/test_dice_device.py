"""CPU tests of evaluation/dice_device.py: the numpy restatements the kernels are held to
(tests/test_gpu_dice_device.py) against the host code they replace -- ``area_labels_reference`` against
``labels_from_delineations``, ``dice_from_counts(confusion_counts_reference(...))`` against ``_dice_metrics`` bit for
bit -- the out-of-range word, and the evaluation's Dice selection over an injected ``Batch.confusion``."""
import numpy as np
import pytest

from tests.dice_cases import SEG_FAMILIES, host_area_labels, map_pairs, seg_family

METRICS = ["dice_coef_classes", "dice_coef_macro", "dice_coef_micro"]
AREA_SHAPES = [(16, 16, 2), (16, 24, 3), (32, 40, 2), (20, 34, 5), (16, 16, 8), (36, 68, 8), (48, 80, 3), (48, 80, 4)]


@pytest.mark.parametrize("H,W,C", AREA_SHAPES)
def test_area_labels_reference_equals_labels_from_delineations(H, W, C):
    from oct_image_segmentation_models_amd.evaluation.dice_device import area_labels_reference
    for f, kind in enumerate(SEG_FAMILIES):
        segs = seg_family(kind, 2, H, W, C, seed=100 * C + f)
        before = segs.copy()
        got = area_labels_reference(segs, H, W)
        assert got.dtype == np.uint8 and got.shape == (2, H, W)
        assert np.array_equal(segs, before)                                  # the input is left alone
        assert np.array_equal(got, host_area_labels(segs, H, W)), kind
        assert np.array_equal(area_labels_reference(segs[0], H, W), got[0])   # one image, (M, W)


def test_area_labels_reference_families_hold_what_they_name():
    H, W, C = 20, 34, 5
    assert (np.diff(seg_family("monotone", 2, H, W, C, 1).astype(int), axis=1) >= 0).all()
    assert (np.diff(seg_family("crossing", 2, H, W, C, 1).astype(int), axis=1) < 0).any()
    z = seg_family("zeros40", 4, H, W, C, 1)
    assert 0.3 < (z == 0).mean() < 0.5
    assert (seg_family("zero_column", 2, H, W, C, 1)[:, :, W // 2] == 0).all()
    assert (seg_family("last_zero", 2, H, W, C, 1)[:, C - 2] == 0).all()
    b = seg_family("beyond", 2, H, W, C, 1)
    assert (b == H + 5).any() and (b == 65535).any()


def _host_dice(pred, gt, C, transposed):
    """``_dice_metrics`` as evaluate_model calls it: plain on the arg-max maps, transposed on the graph-search maps."""
    from oct_image_segmentation_models_amd.common import utils
    from oct_image_segmentation_models_amd.evaluation.evaluation import _dice_metrics
    label = utils.to_categorical(gt[..., None], C)                                           # (H,W,C)
    if transposed:
        cat = utils.perform_argmax(np.expand_dims(utils.to_categorical(pred.T[..., None], C), axis=0))[1]   # (1,C,W,H)
    else:
        cat = utils.labels_to_categorical(pred[None].astype(np.int64), C)                    # (1,C,H,W)
    return _dice_metrics(METRICS, C, label, cat, transposed=transposed)


def _dice_pairs():
    rng = np.random.default_rng(4)
    for B, H, W, C in ((2, 20, 34, 5), (1, 36, 68, 8), (1, 64, 128, 3)):
        for name, (pred, gt) in map_pairs(B, H, W, C, seed=C).items():
            yield f"{name}-{H}x{W}x{C}", pred[0], gt[0], C
    pred, gt = map_pairs(1, 256, 512, 8, seed=9)["shifted"]
    yield "shifted-256x512x8", pred[0], gt[0], 8
    gt = rng.integers(0, 3, (24, 40)).astype(np.uint8)                      # class 3 absent from both, class 2 from pred
    pred = np.where(gt == 2, 1, gt).astype(np.uint8)
    yield "absent", pred, gt, 4
    yield "identical", gt.copy(), gt, 4
    yield "disjoint", ((gt + 1) % 3).astype(np.uint8), gt, 3


@pytest.mark.parametrize("transposed", [False, True])
def test_dice_from_counts_equals_dice_metrics_bit_for_bit(transposed):
    from oct_image_segmentation_models_amd.evaluation.dice_device import confusion_counts_reference, counts_matrix, dice_from_counts
    seen = 0
    for name, pred, gt, C in _dice_pairs():
        counts = counts_matrix(confusion_counts_reference(pred[None], gt[None], C), C)[0]
        assert counts.dtype == np.uint32 and counts.shape == (C, C) and counts.sum() == pred.size
        got, want = dice_from_counts(counts, METRICS), _host_dice(pred, gt, C, transposed)
        for g, w, what in zip(got, want, METRICS):
            g, w = np.asarray(g), np.asarray(w)
            assert g.dtype == w.dtype and g.shape == w.shape, (name, what, g.dtype, w.dtype, g.shape, w.shape)
            assert g.tobytes() == w.tobytes(), (name, what, g, w)
        seen += 1
    assert seen >= 13
    only = dice_from_counts(counts, ["dice_coef_macro"])
    assert only[0] is None and only[2] is None and only[1] is not None


def test_out_of_range_word():
    from oct_image_segmentation_models_amd.evaluation.dice_device import confusion_counts_reference, counts_matrix
    C = 3
    pred, gt = map_pairs(3, 16, 16, C, seed=2)["random"]
    clean = confusion_counts_reference(pred, gt, C)
    assert clean.shape == (3, C * C + 1) and clean.dtype == np.uint32 and not clean[:, -1].any()
    assert (clean.sum(axis=1) == 256).all()
    pred, gt = pred.copy(), gt.copy()
    pred[0, 0, 0], gt[2, -1, -1], gt[2, 0, 0], pred[2, 0, 0] = C, 255, 200, 7     # one pixel with both labels out of range
    rows = confusion_counts_reference(pred, gt, C)
    assert list(rows[:, -1]) == [1, 0, 2] and (rows.sum(axis=1) == 256).all()       # counted once, and nowhere else
    assert np.array_equal(rows[1], clean[1])
    with pytest.raises(ValueError, match="image 12"):
        counts_matrix(rows[2:], C, first_image=12)
    with pytest.raises(ValueError, match="image 0"):
        counts_matrix(rows.view(np.int32), C)                                       # the device's int32 rows
    assert np.array_equal(counts_matrix(clean.view(np.int32), C), clean[:, :-1].reshape(3, C, C))


def test_injected_confusion_drives_the_dice_selection():
    """An InferenceRun over ready records (no device): where a batch carries confusion counts the evaluation's Dice values
    come from them -- matching the host values for true counts, following the field for altered ones -- and from the
    one-hot arrays where it carries none."""
    from oct_image_segmentation_models_amd.common import utils
    from oct_image_segmentation_models_amd.evaluation.dice_device import confusion_counts_reference, counts_matrix, dice_from_counts
    from oct_image_segmentation_models_amd.evaluation.evaluation import _batch_dice, _dice_metrics
    from oct_image_segmentation_models_amd.evaluation.pipeline import Batch, InferenceRun
    n, H, W, C, B = 6, 32, 64, 4, 4
    pred, gt = map_pairs(n, H, W, C, seed=6)["shifted"]
    true = counts_matrix(confusion_counts_reference(pred, gt, C), C)
    altered = true.copy()
    altered[:, 0, 0] += 7
    images = np.empty((n, H, W, 1), np.uint8)

    def values(confusion):
        records = [Batch(lo, min(lo + B, n), pred[lo:lo + B], None, None, None,
                         None if confusion is None else confusion[lo:lo + B]) for lo in range(0, n, B)]
        out = []
        with InferenceRun(None, images, B, C, gt=gt, confusion=confusion is not None, batches=records) as run:
            for b in run:
                for k in range(b.hi - b.lo):
                    label = utils.to_categorical(gt[b.lo + k][..., None], C)
                    cat = utils.labels_to_categorical(b.labels[k:k + 1].astype(np.int64), C)
                    out.append(_batch_dice(METRICS, C, b, k, label, cat))
        return out

    host, dev, alt = values(None), values(true), values(altered)
    assert len(host) == len(dev) == n
    for i in range(n):
        label = utils.to_categorical(gt[i][..., None], C)
        want = _dice_metrics(METRICS, C, label, utils.labels_to_categorical(pred[i:i + 1].astype(np.int64), C))
        for h, d, a, w, e in zip(host[i], dev[i], alt[i], want, dice_from_counts(altered[i], METRICS)):
            assert h.tobytes() == w.tobytes() == d.tobytes() and h.dtype == d.dtype and h.shape == d.shape
            assert a.tobytes() == e.tobytes() and a.tobytes() != w.tobytes()
    assert Batch(0, 1, pred[:1]).confusion is None and Batch._fields[-1] == "confusion" and len(Batch._fields) == 7


def test_switches_default_to_off():
    import inspect
    from oct_image_segmentation_models_amd.evaluation.evaluation_parameters import EvaluationParameters
    from oct_image_segmentation_models_amd.prediction.prediction_parameters import PredictionParams
    assert inspect.signature(EvaluationParameters.__init__).parameters["metrics_device"].default is False
    assert inspect.signature(PredictionParams.__init__).parameters["gs_labels_device"].default is False
