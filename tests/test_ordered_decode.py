"""CPU tests of the ordered layer decode: ``common.utils.ordered_decode_reference`` against brute-force
enumeration, its invariants, the clamp, its relation to the arg-max, ``generate_boundary`` and ``area_labels_reference``, and
the parameter validation of the switches.  The kernel is held against the restatement in tests/test_gpu_ordered_decode.py."""
import numpy as np
import pytest

from tests.ordered_cases import ONE, brute_force, make, ordered_onehot, quantise


def _ref():
    from oct_image_segmentation_models_amd.common.utils import ordered_decode_reference
    return ordered_decode_reference


def _columns(kind: str, n: int, seed: int):
    """n random columns (H, C) with H <= 6, C <= 4."""
    rng = np.random.default_rng(seed)
    for _ in range(n):
        H, C = int(rng.integers(1, 7)), int(rng.integers(2, 5))
        if kind == "dirichlet":
            yield rng.dirichlet(np.ones(C), size=H).astype(np.float32)
        elif kind == "onehot":
            yield np.eye(C, dtype=np.float32)[rng.integers(0, C, size=H)]
        else:                                                               # coarse values: many ties
            yield (rng.integers(0, 3, size=(H, C)) / 2.0).astype(np.float32)


@pytest.mark.parametrize("kind", ["dirichlet", "onehot", "coarse"])
def test_restatement_equals_brute_force(kind):
    """Score, labelling and the bottom-up tie rule: among the optimal labellings the one that is smallest when compared
    from the bottom row upward."""
    ref = _ref()
    for col in _columns(kind, 1000, seed={"dirichlet": 1, "onehot": 2, "coarse": 3}[kind]):
        labels, rows, score = ref(col[None, :, None, :])
        want_score, want_labels = brute_force(col)
        assert int(score[0, 0]) == want_score, col
        assert np.array_equal(labels[0, :, 0], want_labels), (col, labels[0, :, 0], want_labels)
        k = quantise(col)
        assert sum(int(k[r, labels[0, r, 0]]) for r in range(col.shape[0])) == want_score


@pytest.mark.parametrize("C", [2, 3, 9, 16])
def test_labels_and_rows_are_ordered(C):
    p = make((2, 23, 11, C), "random", seed=5)
    labels, rows, score = _ref()(p)
    assert labels.dtype == np.uint8 and rows.dtype == np.uint16 and score.dtype == np.uint32
    assert labels.shape == (2, 23, 11) and rows.shape == (2, C - 1, 11) and score.shape == (2, 11)
    assert (np.diff(labels.astype(int), axis=1) >= 0).all() and labels.max() < C
    assert (np.diff(rows.astype(int), axis=1) >= 0).all() and rows.max() <= 23
    for i in range(C - 1):
        assert np.array_equal(rows[:, i], (labels <= i).sum(axis=1))
    k = quantise(p)
    assert np.array_equal(score, np.take_along_axis(k, labels[..., None].astype(np.int64), axis=-1)[..., 0].sum(axis=1))
    argmax_score = k.max(axis=-1).sum(axis=1)                      # an upper bound: the unconstrained optimum
    assert (score <= argmax_score).all()


def test_ordered_onehot_input_is_left_alone():
    from oct_image_segmentation_models_amd.min_path_processing.utils import generate_boundary
    p, want = ordered_onehot((2, 19, 13, 5), seed=4)
    labels, rows, score = _ref()(p)
    assert np.array_equal(labels, want) and np.array_equal(labels, p.argmax(axis=-1))
    assert (score == 19 * (ONE - 1)).all()
    full = np.concatenate([want, np.full((2, 1, 13), 4, np.uint8)], axis=1)      # (generate_boundary sizes itself by the maximum)
    truth = np.swapaxes(generate_boundary(full, axis=1), 0, 1)                    # (B, C-1, W)
    assert truth.shape == rows.shape and (truth != 0).any()
    assert np.array_equal(rows[truth != 0], truth[truth != 0])


def test_clamp_of_nan_negative_and_large_entries():
    ref = _ref()
    p = make((1, 7, 5, 3), "random", seed=9)
    bad = p.copy()
    bad[0, 1, 2, 0], bad[0, 2, 2, 1], bad[0, 3, 2, 2], bad[0, 4, 1, 0] = np.nan, -3.0, 7.5, np.inf
    bad[0, 5, 1, 1], bad[0, 6, 1, 2] = -np.inf, -0.0
    clamped = bad.copy()
    clamped[0, 1, 2, 0], clamped[0, 2, 2, 1], clamped[0, 3, 2, 2], clamped[0, 4, 1, 0] = 0.0, 0.0, 1.0, 1.0
    clamped[0, 5, 1, 1], clamped[0, 6, 1, 2] = 0.0, 0.0
    for a, b in zip(ref(bad), ref(clamped)):
        assert np.array_equal(a, b)
    # 1.0 and everything above it count 2^20 - 1, not 2^20
    _, _, score = ref(np.array([[[[0.0, 1.0]]], ], np.float32))
    assert int(score[0, 0]) == ONE - 1
    _, _, score = ref(np.full((1, 4096, 1, 2), 1.0, np.float32))
    assert int(score[0, 0]) == 4096 * (ONE - 1) < 1 << 32


def test_area_labels_reproduce_the_map_where_no_row_is_zero():
    from oct_image_segmentation_models_amd.evaluation.dice_device import area_labels_reference
    p = make((3, 21, 40, 4), "random", seed=12)
    labels, rows, _ = _ref()(p)
    again = area_labels_reference(rows, 21, 40)
    ok = (rows != 0).all(axis=1)                                    # (B, W) columns without a 0 row
    assert ok.any() and not ok.all()                                 # both kinds occur in the sample
    assert np.array_equal(np.swapaxes(again, 1, 2)[ok], np.swapaxes(labels, 1, 2)[ok])
    assert not np.array_equal(again, labels)                         # a column that starts below a boundary reads otherwise


def test_refusals():
    from oct_image_segmentation_models_amd.evaluation.ordered import check_ordered, layer_thickness
    ref = _ref()
    for shape in ((4, 4, 3), (1, 4, 4, 1), (1, 4, 4, 17), (1, 4097, 1, 2), (0, 4, 4, 3)):
        with pytest.raises(ValueError):
            ref(np.zeros(shape, np.float32))
    for C, H in ((1, 8), (17, 8), (3, 4097), (3, 0)):
        with pytest.raises(ValueError):
            check_ordered(C, H)
    check_ordered(2, 1); check_ordered(16, 4096)
    assert layer_thickness(np.zeros((1, 5), np.uint16)) == (None, None)
    t, m = layer_thickness(np.array([[0, 2, 3], [4, 2, 9], [4, 7, 9]], np.uint16))
    assert t.dtype == np.uint16 and np.array_equal(t, [[4, 0, 6], [0, 5, 0]]) and m.dtype == np.float64
    assert np.array_equal(m, [10 / 3, 5 / 3])
    with pytest.raises(ValueError, match="cross"):
        layer_thickness(np.array([[5, 5], [4, 6]], np.uint16))


def test_batch_record_and_stage_list():
    """``Batch.ordered`` is an attribute beside the seven fields, carried through the other ``with_`` methods; the stage reads
    the probabilities alone, so it runs without a ground truth."""
    from oct_image_segmentation_models_amd.evaluation.pipeline import Batch, _stages
    b = Batch(0, 1, np.zeros((1, 2, 2), np.uint8))
    assert len(b) == 7 and b.ordered is None
    o = b.with_ordered(("l", "r", "s")).with_calibration("c").with_uncertainty("e", "m")
    assert len(o) == 7 and tuple(o) == tuple(b)
    assert (o.ordered, o.calibration, o.entropy, o.mutual_info) == (("l", "r", "s"), "c", "e", "m")
    run = object()
    assert [st.field for st in _stages(None, run, None, have_gt=False, calibration=run, ordered=run)] == ["ordered"]
    assert [st.field for st in _stages(None, run, run, have_gt=True, calibration=run, ordered=run)] == \
        ["confusion", "calibration", "ordered", "minpath"]
    got = []
    st = _stages(None, None, None, have_gt=False, ordered=lambda *a: got.append(a))[0]
    st.launch(1, ("L", "R"), "lab", None, None, "P")
    assert got == [("P", "L", "R")]


def test_inference_run_refuses_what_the_decode_cannot_take():
    from oct_image_segmentation_models_amd.evaluation.pipeline import InferenceRun
    with pytest.raises(ValueError, match="classes"):
        InferenceRun(None, np.zeros((1, 8, 8, 1), np.uint8), 1, 17, batches=[], ordered_decode=True)
    with pytest.raises(ValueError, match="height"):
        InferenceRun(None, np.zeros((1, 4097, 1, 1), np.uint8), 1, 3, batches=[], ordered_decode=True)
    InferenceRun(None, np.zeros((1, 8, 8, 1), np.uint8), 1, 17, batches=[]).close()
