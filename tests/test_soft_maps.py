"""CPU tests of the soft boundary maps (``binarize=False``): the elementwise numpy restatement of
``oct_boundary_maps_soft`` against the reference's ``convert_predictions_to_maps_semantic`` on class probabilities,
``InferenceRun`` over injected soft maps in the three search modes, and the public switches.  Every comparison is exact."""
import inspect

import numpy as np
import pytest

import __graft_entry__ as ge
from tests.soft_maps_cases import BG, FAMILIES, class_map, family, scaled_values

SHAPES = [(1, 1, 4, 2), (1, 2, 5, 2), (1, 3, 4, 4), (3, 20, 34, 5), (2, 36, 68, 8)]


def _cu():
    from oct_image_segmentation_models_amd.common import utils as cu
    return cu


def _semantic(cu, p, bg_ilm, bg_csi):
    return cu.convert_predictions_to_maps_semantic(np.transpose(p, (0, 3, 1, 2)).copy(), bg_ilm, bg_csi)


@pytest.mark.parametrize("fam", FAMILIES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_restatement_equals_the_reference_function_on_probabilities(shape, fam):
    cu = _cu()
    p = family(fam, shape)
    assert p.dtype == np.float32 and p.shape == shape and np.isfinite(p).all() and p.min() >= 0 and p.max() <= 1
    for bg_ilm, bg_csi in BG:
        got = cu.soft_boundary_maps_reference(p, bg_ilm, bg_csi)
        assert got.dtype == np.uint8 and got.shape == (shape[0], shape[3] - 1, shape[1], shape[2])
        if shape[1] == 1:
            # np.gradient refuses a single row, so the reference function has no value there; the definition says d = 0
            with pytest.raises(ValueError):
                _semantic(cu, p, bg_ilm, bg_csi)
            assert not got.any()
            continue
        assert np.array_equal(got, _semantic(cu, p, bg_ilm, bg_csi)), (bg_ilm, bg_csi)
        # perform_argmax(bin=False) hands over exactly that transpose
        _, cat = cu.perform_argmax(p, bin=False)
        assert np.array_equal(got, cu.convert_predictions_to_maps_semantic(cat.copy(), bg_ilm, bg_csi))


@pytest.mark.parametrize("shape", SHAPES[1:], ids=lambda s: "x".join(map(str, s)))
def test_on_one_hot_floats_the_soft_maps_are_the_binary_maps(shape):
    cu = _cu()
    p = family("onehot", shape)
    lab = class_map(shape)
    assert np.array_equal(p.argmax(-1), lab)
    for bg_ilm, bg_csi in BG:
        want = cu.convert_predictions_to_maps_semantic(cu.labels_to_categorical(lab, shape[3]), bg_ilm, bg_csi)
        assert np.array_equal(cu.soft_boundary_maps_reference(p, bg_ilm, bg_csi), want)


@pytest.mark.parametrize("shape", [(3, 20, 34, 5), (2, 36, 68, 8)], ids=lambda s: "x".join(map(str, s)))
def test_saturated_family_reaches_the_edge_rows_and_the_wrap(shape):
    """The uint8 cast is only interesting above 255, which probabilities reach in rows 0 and H-1 alone."""
    cu = _cu()
    p = family("saturated", shape)
    H = shape[1]
    for bg_ilm, bg_csi in BG:
        out = cu.soft_boundary_maps_reference(p, bg_ilm, bg_csi)
        v = scaled_values(p, bg_ilm, bg_csi)
        assert (out[:, :, [0, H - 1], :] > 127).any()
        assert (v >= 256).any() and not (v[:, :, 1:H - 1, :] >= 256).any()
        wrapped = v >= 256
        assert np.array_equal(out[wrapped], (v[wrapped].astype(np.int32) - 256).astype(np.uint8))


# ---- InferenceRun over injected soft maps ----------------------------------------------------------------------------
N, M, H, W, B = 5, 2, 24, 40, 2


def _soft_maps():
    cu = _cu()
    p = np.concatenate([family("layered", (3, H, W, M + 1)), family("saturated", (2, H, W, M + 1))])
    maps = cu.soft_boundary_maps_reference(p, True, False)
    assert len(np.unique(maps)) > 4                      # graded, not the 0 / 127 / 254 / 255 of a binary map
    return maps


def _run(maps, truths, **kw):
    from oct_image_segmentation_models_amd.evaluation.pipeline import Batch, InferenceRun
    from oct_image_segmentation_models_amd.min_path_processing.device_search import delineate_dp
    device = kw.get("gs_device", False)
    batches = [Batch(lo, min(lo + B, N), np.zeros((min(lo + B, N) - lo, H, W), np.uint8), maps[lo:lo + B], None,
                     delineate_dp(maps[lo:lo + B], 1) if device else None) for lo in range(0, N, B)]
    out = []
    with InferenceRun(None, np.empty((N, H, W, 1), np.uint8), B, M + 1, graph_search=True, gsgrad=1, gs_workers=1,
                      batches=batches, soft_maps=True, **kw) as run:
        for b in run:
            out += run.graph_search(b, truths[b.lo:b.hi])
    return out


def test_inference_run_searches_injected_soft_maps_in_all_three_modes():
    ge.build()
    from oct_image_segmentation_models_amd.min_path_processing import graph_search
    from oct_image_segmentation_models_amd.min_path_processing.device_search import delineate_dp
    maps = _soft_maps()
    truths = np.random.default_rng(5).integers(0, H + 1, (N, M, W)).astype(np.float64)
    graph = graph_search.create_graph_structure((W, H), 1)
    want = [graph_search.segment_maps(np.transpose(maps[i], (0, 2, 1)), truths[i], graph)[:2] for i in range(N)]
    tied = delineate_dp(maps, 1)[2]
    for kw in ({}, {"gs_device": True, "gs_device_ties": "host"}):
        got = _run(maps, truths, **kw)
        assert len(got) == N
        for i in range(N):
            assert got[i][0].dtype == np.uint16 and np.array_equal(got[i][0], want[i][0]), (kw, i)
            assert np.array_equal(got[i][1], want[i][1], equal_nan=True), (kw, i)
    got = _run(maps, truths, gs_device=True, gs_device_ties="device")
    assert (~tied).any()
    for i in range(N):
        for m in np.nonzero(~tied[i])[0]:
            assert np.array_equal(got[i][0][m], want[i][0][m]), (i, m)
            assert np.array_equal(got[i][1][m], want[i][1][m], equal_nan=True), (i, m)


# ---- the public switches -------------------------------------------------------------------------------------------
def test_parameters_expose_binarize_and_soft_maps_needs_maps():
    from oct_image_segmentation_models_amd.evaluation.evaluation_parameters import EvaluationParameters
    from oct_image_segmentation_models_amd.evaluation.pipeline import BatchedPredictor, InferenceRun, host_batches
    from oct_image_segmentation_models_amd.models.engine_model import Model
    from oct_image_segmentation_models_amd.prediction.prediction_parameters import PredictionParams
    for cls in (EvaluationParameters, PredictionParams):
        assert inspect.signature(cls.__init__).parameters["binarize"].default is True
    for fn in (InferenceRun.__init__, BatchedPredictor.__init__, host_batches, Model.predict_labels):
        assert inspect.signature(fn).parameters["soft_maps"].default is False
    # (InferenceRun always asks its source for maps: the refusal lives in the two sources)
    with pytest.raises(ValueError, match="soft_maps"):
        BatchedPredictor(None, 2, want_maps=False, soft_maps=True)
    with pytest.raises(ValueError, match="soft_maps"):
        Model.predict_labels(None, np.zeros((1, 8, 8, 1), np.uint8), want_maps=False, soft_maps=True)


def test_binarize_is_stored_by_both_parameter_classes(tmp_path):
    """The two constructors load a model: a freshly saved untrained one will do (no device is touched)."""
    import json
    from pathlib import Path
    from oct_image_segmentation_models_amd.common.dataset import Dataset
    from oct_image_segmentation_models_amd.evaluation.evaluation_parameters import EvaluationParameters, EvaluationSaveParams
    from oct_image_segmentation_models_amd.models.engine_model import Model
    from oracle import unet_numpy as on
    from oct_image_segmentation_models_amd.prediction.prediction_parameters import PredictionParams, PredictionSaveParams
    cfg = dict(input_channels=1, num_classes=3, image_height=16, image_width=16, pool_layers=2)
    model = Model(name="unet", config=cfg)
    model.set_weights(on.keras_weight_list(*on.init_params(on.UNetConfig(num_classes=3, pool_layers=2), seed=3, dtype=np.float32)))
    model.save(tmp_path / "model.npz")
    with open(tmp_path / "model_config.json", "w") as fh:
        json.dump(cfg, fh)
    ds = Dataset(np.zeros((1, 16, 16, 1), np.uint8), [Path("a")], [tmp_path / "out"])
    for flag in (True, False):
        ep = EvaluationParameters(tmp_path / "model.npz", None, None, tmp_path / "d.hdf5", tmp_path / "e",
                                  EvaluationSaveParams(), True, [], binarize=flag)
        pp = PredictionParams(tmp_path / "model.npz", None, None, ds, tmp_path / "p", PredictionSaveParams(), binarize=flag)
        assert ep.binarize is flag and pp.binarize is flag
    assert EvaluationParameters(tmp_path / "model.npz", None, None, tmp_path / "d.hdf5", tmp_path / "e",
                                EvaluationSaveParams(), True, []).binarize is True
