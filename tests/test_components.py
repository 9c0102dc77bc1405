"""CPU tests of the connected components: the numpy restatements against ``scipy.ndimage.label`` and
against closed forms, ``ComponentRule``, the refusals of the parameter classes and the switch's default."""
import numpy as np
import pytest

from tests.components_cases import BATCHES, CONNECTIVITIES, N_CLS, PATTERNS, SHAPES, filter_cases, pattern, rule, wanted

ids = lambda c: "x".join(map(str, c))      # noqa: E731


def _utils():
    from oct_image_segmentation_models_amd.common import utils
    return utils


# ---- 1. the restatement ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("connectivity", CONNECTIVITIES)
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_restatement_equals_scipy_label(shape, connectivity):
    """Same partition as ``scipy.ndimage.label`` run per byte value and image, the root is the component's smallest index,
    the size sits at the root, and the statistics count what the partition holds."""
    ndimage = pytest.importorskip("scipy").ndimage
    structure = np.ones((3, 3), int) if connectivity == 8 else ndimage.generate_binary_structure(2, 1)
    H, W = shape
    B = 3
    for name in PATTERNS:
        labels = pattern(name, B, H, W)
        root, size, stats = wanted(name, B, H, W, connectivity)
        assert root.dtype == size.dtype == stats.dtype == np.uint32 and stats.shape == (B, N_CLS, 2)
        for b in range(B):
            want_root = np.empty((H, W), np.int64)
            want_stats = np.zeros((N_CLS, 2), np.int64)
            for v in np.unique(labels[b]):
                comp, n = ndimage.label(labels[b] == v, structure=structure)
                flat = comp.reshape(-1)
                first = np.full(n + 1, H * W, np.int64)
                np.minimum.at(first, flat, np.arange(H * W))
                want_root[comp > 0] = first[flat][flat > 0]
                if v < N_CLS:
                    want_stats[v] = (n, np.bincount(flat)[1:].max())
            assert np.array_equal(root[b], want_root), (name, b)
            counts = np.bincount(want_root.reshape(-1), minlength=H * W).reshape(H, W)
            assert np.array_equal(size[b], np.where(want_root == np.arange(H * W).reshape(H, W), counts, 0)), (name, b)
            assert np.array_equal(stats[b], want_stats), (name, b)


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_closed_forms(shape):
    H, W = shape
    for B in BATCHES:
        for conn in CONNECTIVITIES:
            root, size, stats = wanted("constant", B, H, W, conn)
            assert not root.any() and (size[:, 0, 0] == H * W).all() and size.sum() == B * H * W
            for b in range(B):                                   # image b is the constant 1 + b
                assert stats[b, 1 + b].tolist() == [1, H * W] and stats[b].sum() == 1 + H * W
        root, size, stats = wanted("checkerboard", B, H, W, 4)
        assert np.array_equal(root, np.broadcast_to(np.arange(H * W, dtype=np.uint32).reshape(H, W), (B, H, W)))
        assert (size == 1).all() and stats[:, :2, 0].sum() == B * H * W
        if H >= 2 and W >= 2:
            root, size, stats = wanted("checkerboard", B, H, W, 8)
            assert set(np.unique(root)) == {0, 1} and stats[:, :2, 0].tolist() == [[1, 1]] * B
            assert sorted(stats[0, :2, 1].tolist()) == [H * W // 2, (H * W + 1) // 2]
        # the serpentine's class 1 is one component (its path is about H*W/2 pixels long); diagonals join only at 8
        if H >= 2 and W >= 2:
            for conn in CONNECTIVITIES:
                assert (wanted("serpentine", B, H, W, conn)[2][:, 1, 0] == 1).all()
                assert (wanted("comb", B, H, W, conn)[2][:, 1, 0] == 1).all()
            for name in ("diagonals_down", "diagonals_up"):
                assert (wanted(name, B, H, W, 4)[1] == 1).all()
                assert wanted(name, B, H, W, 8)[2][:, :3, 0].sum() < B * H * W
        # components never join across images: the facing rows of two images have the same class
        root, size, stats = wanted("facing_rows", B, H, W, 8)
        assert (size.reshape(B, -1).sum(axis=1) == H * W).all() and (root < H * W).all()


def test_restatement_refuses():
    u = _utils()
    ok = np.zeros((1, 2, 2), np.uint8)
    for bad in (lambda: u.components_reference(ok, 3, 6), lambda: u.components_reference(ok, 0, 4),
                lambda: u.components_reference(ok, 33, 4), lambda: u.components_reference(ok[0], 3, 4),
                lambda: u.components_reference(ok.astype(np.int32), 3, 4), lambda: u.components_reference(ok[:, :0], 3, 4)):
        with pytest.raises(ValueError):
            bad()
    root, size, _ = u.components_reference(ok, 3, 4)
    for r in (rule(3, fill_mode=2), rule(3, fill_label=256), rule(3, fill_label=-1), rule(4, keep_largest=(3,))):
        with pytest.raises(ValueError):
            u.component_filter_reference(ok, root, size, 3, r)
    with pytest.raises(ValueError):
        u.component_filter_reference(ok, root[:, :1], size, 3, rule(3))
    assert (u.COMPONENTS_MAX_CLASSES, u.COMPONENTS_MAX_BATCH) == (32, 65535)


def test_filter_cases_remove_and_keep():
    """The case builder asserts that every case removes and keeps something; here: what the definition says about the result."""
    cases = filter_cases()
    assert {c.rule.fill_mode for c in cases.values()} == {0, 1}
    for name, c in cases.items():
        gone_by_class = [(c.labels == k).sum(axis=(1, 2)) - ((c.clean == k) & (c.labels == k)).sum(axis=(1, 2)) for k in range(c.n_cls)]
        assert (np.stack(gone_by_class, axis=1) <= c.removed).all(), name         # (a fill may restate the byte it replaces)
        assert np.array_equal(c.clean[c.labels >= c.n_cls], c.labels[c.labels >= c.n_cls]), name
        if c.rule.fill_mode == 0:
            changed = c.clean != c.labels
            assert (c.clean[changed] == c.rule.fill_label).all(), name


# ---- 2. the rule ---------------------------------------------------------------------------------------------------------------
def _rule_cls():
    from oct_image_segmentation_models_amd.evaluation.components import ComponentRule
    return ComponentRule


def test_component_rule_validates_and_packs():
    import __graft_entry__ as ge
    ge.build()
    R = _rule_cls()
    r = R()
    assert (r.connectivity, r.min_pixels, r.keep_largest, r.fill) == (8, 0, (), "column")
    p = r.pack(3)
    assert list(p.min_pixels) == [0] * 32 and (p.keep_largest, p.fill_mode, p.fill_label) == (0, 1, 0)
    p = R(connectivity=4, min_pixels=[5, 0, 7], keep_largest=[2, 0], fill=200).pack(3)
    assert list(p.min_pixels)[:4] == [5, 0, 7, 0] and (p.keep_largest, p.fill_mode, p.fill_label) == (0b101, 0, 200)
    p = R(min_pixels=9, keep_largest="all").pack(16)
    assert list(p.min_pixels) == [9] * 16 + [0] * 16 and p.keep_largest == 0xFFFF
    assert R(min_pixels=1, keep_largest="all").pack(32).keep_largest == 0xFFFFFFFF
    assert R.coerce(None) is None and R.coerce(r) is r
    assert R.coerce(dict(connectivity=4, min_pixels=3)) == R(4, 3) and R(4, 3) != R(8, 3)
    assert R(**R(4, [1, 2], "all", 7).as_dict()) == R(4, [1, 2], "all", 7)
    for bad in (dict(connectivity=6), dict(connectivity=True), dict(min_pixels=-1), dict(min_pixels=[]), dict(min_pixels=1.5),
                dict(min_pixels=[1, "a"]), dict(min_pixels=1 << 32), dict(keep_largest="largest"), dict(keep_largest=[1, 1]),
                dict(keep_largest=[32]), dict(keep_largest=[-1]), dict(keep_largest=3), dict(fill="row"), dict(fill=256),
                dict(fill=-1), dict(fill=1.0)):
        with pytest.raises(ValueError):
            R(**bad)
    with pytest.raises(ValueError):
        R.coerce(dict(conectivity=4))
    with pytest.raises(ValueError):
        R.coerce("column")
    for rule_, n in ((R(min_pixels=[1, 2]), 3), (R(keep_largest=[3]), 3), (R(), 0), (R(), 33)):
        with pytest.raises(ValueError):
            rule_.check(n)
        with pytest.raises(ValueError):
            rule_.pack(n)
    R(min_pixels=[1, 2, 3], keep_largest=[2]).check(3)


def test_host_formulas():
    import __graft_entry__ as ge
    ge.build()
    from oct_image_segmentation_models_amd.evaluation import components as cc
    c = filter_cases()["crafted_column"]
    r = cc.ComponentRule(connectivity=8, min_pixels=[3, 3, 0], keep_largest=[2], fill="column")
    clean, stats, removed = cc.components_host(c.labels, 3, r)
    # (the case's own rule falls back to 9 where a column has no source; the public rule's fallback is 0)
    assert np.array_equal(stats, c.stats) and np.array_equal(removed, c.removed)
    assert np.array_equal(clean[:, :, :7], c.clean[:, :, :7]) and (clean[:, :, 7][c.labels[:, :, 7] == 2] == 0).all()
    assert cc.changed_pixels(clean[0], c.labels[0]) == int((clean[0] != c.labels[0]).sum()) > 0
    cc.check_components(16, 1, 1)
    for bad in ((0, 4, 4), (33, 4, 4), (3, 0, 4), (3, 4, 0), (3, 1 << 16, 1 << 15)):
        with pytest.raises(ValueError):
            cc.check_components(*bad)


# ---- 3. the switch ---------------------------------------------------------------------------------------------------------------
def test_batch_record_and_stage_list():
    """``Batch.components`` is an attribute beside the seven fields, carried through the other ``with_`` methods; the stage
    reads the arg-max maps alone, so it runs without a ground truth; with the switch off the stage list is what it was."""
    import __graft_entry__ as ge
    ge.build()
    from oct_image_segmentation_models_amd.evaluation.pipeline import Batch, _stages
    b = Batch(0, 1, np.zeros((1, 2, 2), np.uint8))
    assert len(b) == 7 and b.components is None
    o = b.with_components(("l", "s", "r")).with_ordered("o").with_calibration("c").with_uncertainty("e", "m")
    assert o.components == ("l", "s", "r") and (o.ordered, o.calibration, o.entropy) == ("o", "c", "e") and len(o) == 7
    assert tuple(o) == tuple(b) and b.with_ordered("o").components is None
    run = object()
    assert [st.field for st in _stages(None, run, run, have_gt=True, calibration=run, ordered=run)] == \
        ["confusion", "calibration", "ordered", "minpath"]
    assert [st.field for st in _stages(None, run, run, have_gt=True, calibration=run, ordered=run, components=None)] == \
        ["confusion", "calibration", "ordered", "minpath"]
    assert [st.field for st in _stages(run, run, run, have_gt=False, calibration=run, ordered=run, components=run)] == \
        ["ordered", "components", "minpath"]
    got = []
    st = _stages(None, None, None, have_gt=False, components=lambda *a: got.append(a))[0]
    assert not st.reads_gt and not st.on_probs and not st.on_maps
    st.launch(1, ("L", "S", "R"), "lab", None, None, "P")
    assert got == [("l", "L", "S", "R")]             # (the stage slices its inputs to n)


def test_inference_run_and_parameter_classes_refuse(tmp_path):
    import __graft_entry__ as ge
    ge.build()
    from oct_image_segmentation_models_amd.evaluation.evaluation_parameters import EvaluationParameters, EvaluationSaveParams
    from oct_image_segmentation_models_amd.evaluation.pipeline import InferenceRun
    from oct_image_segmentation_models_amd.prediction.prediction_parameters import PredictionParams, PredictionSaveParams
    from tests.helpers import save_untrained_model
    R = _rule_cls()
    imgs = np.zeros((1, 8, 8, 1), np.uint8)
    for bad in (R(min_pixels=[1, 2]), dict(keep_largest=[3]), dict(connectivity=5), "column"):
        with pytest.raises(ValueError):
            InferenceRun(None, imgs, 1, 3, batches=[], components=bad)
    run = InferenceRun(None, imgs, 1, 3, batches=[], components=dict(min_pixels=[1, 2, 3], keep_largest=[2]))
    assert list(run) == []
    model = save_untrained_model(tmp_path, 16, 32, 3, 8, 2)

    def evaluation(**kw):
        return EvaluationParameters(model_path=model, mlflow_tracking_uri=None, mlflow_run_uuid=None,
                                    test_dataset_path=tmp_path / "none.hdf5", save_foldername=tmp_path / "out",
                                    save_params=EvaluationSaveParams(), graph_search=False, metrics=[], **kw)

    def prediction(**kw):
        return PredictionParams(model_path=model, mlflow_tracking_uri=None, mlflow_run_uuid=None, dataset=None,
                                config_output_dir=tmp_path / "out", save_params=PredictionSaveParams(),
                                col_error_range=range(32), **kw)
    for make in (evaluation, prediction):
        assert make().components is None
        assert make(components=dict(min_pixels=[4, 0, 4], keep_largest="all", fill=0)).components == R(8, [4, 0, 4], "all", 0)
        assert make(components=R(4, 5)).components == R(4, 5)
        for bad in (dict(min_pixels=[1, 2]), dict(min_pixels=[1, 2, 3, 4]), dict(keep_largest=[3]), R(keep_largest=[0, 31]),
                    dict(connectivity=6), dict(fill="above"), dict(pixels=3), 8):
            with pytest.raises(ValueError):
                make(components=bad)
