"""Contrast normalisation off the GPU: ``contrast_reference`` against a literal per-pixel loop written
from the definition, known answers, ``check_contrast``'s refusals, and the public switches -- ``TrainingParams`` /
``train_model`` on the CPU path (``contrast_images`` falls back to the numpy restatement), ``EvaluationParameters`` and
``PredictionParams(contrast="model")``."""
import json
from pathlib import Path

import numpy as np
import pytest

import __graft_entry__ as ge
import contrast_cases as cc
from helpers import save_untrained_model


@pytest.fixture(scope="module")
def U():
    ge.build()
    from oct_image_segmentation_models_amd.common import utils
    return utils


# ---- 1. the vectorised restatement against the literal loop -----------------------------------------------------------------
@pytest.mark.parametrize("shape", cc.SMALL_SHAPES, ids=lambda s: "%dx%dx%d-%dx%d" % (s[0], s[1], s[2], s[3][0], s[3][1]))
@pytest.mark.parametrize("spec", cc.SPECS, ids=cc.spec_id)
def test_reference_equals_the_literal_loop(U, shape, spec):
    H, W, ch, tiles = shape
    s = cc.with_tiles(spec, tiles)
    for content in cc.CONTENTS:
        x = cc.make_images(content, 2, H, W, ch)
        luts, out = cc.literal_contrast(x, s)
        got_luts = U.contrast_luts_reference(x, s)
        assert got_luts.shape == (2, ch) + tuple(tiles) + (256,) and got_luts.dtype == np.uint8
        assert np.array_equal(got_luts, luts), content
        assert np.array_equal(U.contrast_reference(x, s), out), content
        assert np.array_equal(U.contrast_reference(x, s, luts=got_luts), out), content
        assert (np.diff(got_luts.astype(np.int64), axis=-1) >= 0).all(), "a LUT is not monotone"


def test_every_committed_case_is_not_vacuous(U):
    """The guard of the GPU comparison, for every case the GPU test runs: checked here too, where a seed that breaks it
    shows without a GPU."""
    for H, W, ch, tiles in cc.SHAPES:
        for spec in cc.SPECS:
            s = U.check_contrast(cc.with_tiles(spec, tiles), hw=(H, W))
            for content in cc.CONTENTS[1:]:
                x = cc.make_images(content, 1, H, W, ch)
                luts = U.contrast_luts_reference(x, s)
                cc.assert_not_vacuous(x, s, luts, U.contrast_reference(x, s, luts=luts))


# ---- 2. known answers ---------------------------------------------------------------------------------------------------------
def test_one_tile_without_clip_is_textbook_equalisation(U):
    x = cc.make_images("noise", 2, 37, 53, 1)
    out = U.contrast_reference(x, {"method": "clahe", "tiles": (1, 1), "clip": None})
    for b in range(2):
        h = np.bincount(x[b].ravel(), minlength=256)
        A = x[b].size
        lut = (np.cumsum(h) * 255 + A // 2) // A          # floor(cdf * 255 / A + 1/2)
        assert np.array_equal(out[b], lut[x[b]].astype(np.uint8))
    # clip 0 means no limit as well
    assert np.array_equal(out, U.contrast_reference(x, {"method": "clahe", "tiles": (1, 1), "clip": 0}))


def test_stretch_known_answers(U):
    x = np.full((1, 16, 32, 1), 60, np.uint8)
    x[:, :, 16:] = 180
    for tiles in ((1, 1), (2, 1)):                     # (tiles that hold both levels)
        out = U.contrast_reference(x, {"method": "stretch", "tiles": tiles, "percentiles": (0, 100)})
        assert (out[:, :, :16] == 0).all() and (out[:, :, 16:] == 255).all()           # the two levels go to 0 and 255
    # (2,2) tiles hold one level each: every LUT is the identity
    assert np.array_equal(U.contrast_reference(x, {"method": "stretch", "tiles": (2, 2), "percentiles": (0, 100)}), x)
    const = np.full((2, 24, 40, 3), 91, np.uint8)
    for pct in ((1, 99), (0, 100), (25, 75)):
        assert np.array_equal(U.contrast_reference(const, {"method": "stretch", "tiles": (2, 3), "percentiles": pct}), const)
    luts = U.contrast_luts_reference(const, {"method": "stretch", "tiles": (2, 3)})
    assert np.array_equal(luts, np.broadcast_to(np.arange(256, dtype=np.uint8), luts.shape))      # the identity


def test_clip_one_on_the_smallest_tile(U):
    """clip_q8 = 256 on an 8 x 8 tile: L = max(1, (256 * 64) >> 16) = 1 -- every occupied bin is cut to one pixel and the
    excess spread over all 256 bins."""
    assert U.contrast_desc({"method": "clahe", "clip": 1.0, "tiles": (2, 2)}) == (0, 2, 2, 256, 0, 0)
    assert max(1, (256 * 64) >> 16) == 1
    x = np.zeros((1, 16, 16, 1), np.uint8)
    x[0, :8, :8, 0] = np.arange(64, dtype=np.uint8).reshape(8, 8) // 16 * 50       # four values, 16 pixels each
    lut = U.contrast_luts_reference(x, {"method": "clahe", "clip": 1.0, "tiles": (2, 2)})[0, 0, 0, 0].astype(np.int64)
    h = np.zeros(256, np.int64)
    h[[0, 50, 100, 150]] = 16
    E = int(np.maximum(h - 1, 0).sum())
    assert E == 60
    i = np.arange(256)
    h2 = np.minimum(h, 1) + E // 256 + ((((i + 1) * (E % 256)) // 256) > ((i * (E % 256)) // 256))
    assert h2.sum() == 64
    assert np.array_equal(lut, (np.cumsum(h2) * 255 + 32) // 64)


def test_desc_packs_the_integers(U):
    assert U.contrast_desc({"method": "clahe"}) == (0, 8, 8, 0, 0, 0)
    assert U.contrast_desc({"method": "clahe", "clip": 2.5, "tiles": [4, 6]}) == (0, 4, 6, 640, 0, 0)
    assert U.contrast_desc({"method": "stretch"}) == (1, 8, 8, 0, 100, 9900)
    assert U.contrast_desc({"method": "stretch", "percentiles": (0.5, 99.95), "tiles": (1, 16)}) == (1, 1, 16, 0, 50, 9995)


# ---- 3. refusals --------------------------------------------------------------------------------------------------------------
def test_check_contrast_refusals(U):
    assert U.check_contrast(None) is None
    ok = U.check_contrast({"method": "clahe", "clip": 2}, hw=(256, 512))
    assert ok == {"method": "clahe", "tiles": [8, 8], "clip": 2.0} and U.check_contrast(json.loads(json.dumps(ok))) == ok
    ok = U.check_contrast({"method": "stretch"}, hw=(64, 64))
    assert ok == {"method": "stretch", "tiles": [8, 8], "percentiles": [1.0, 99.0]}
    bad = [
        ({"method": "clahe", "tiles": (8, 8)}, (63, 64)),                 # 63 // 8 = 7 rows per tile
        ({"method": "clahe", "tiles": (2, 5)}, (16, 39)),                 # 39 // 5 = 7 columns per tile
        ({"method": "clahe", "tiles": (17, 2)}, (512, 512)),              # ty > 16
        ({"method": "clahe", "tiles": (0, 2)}, None),
        ({"method": "clahe", "tiles": (2.5, 2)}, None),
        ({"method": "clahe", "tiles": 8}, None),
        ({"method": "clahe", "clip": 0.5}, None),                         # clip in (0, 1)
        ({"method": "clahe", "clip": 0.999}, None),
        ({"method": "clahe", "clip": 256.0}, None),                       # clip_q8 > 65535
        ({"method": "clahe", "clip": float("nan")}, None),
        ({"method": "clahe", "percentiles": (1, 99)}, None),
        ({"method": "stretch", "clip": 2.0}, None),
        ({"method": "stretch", "percentiles": (50, 50)}, None),           # lo >= hi
        ({"method": "stretch", "percentiles": (60, 40)}, None),
        ({"method": "stretch", "percentiles": (-1, 99)}, None),
        ({"method": "stretch", "percentiles": (1, 100.01)}, None),
        ({"method": "stretch", "percentiles": (1,)}, None),
        ({"method": "equalize"}, None),                                   # unknown method
        ({}, None),
        ({"method": "clahe", "tile": (8, 8)}, None),                      # unknown key
        ("clahe", None),
        ({"method": "clahe"}, (4097, 512)),
    ]
    for spec, hw in bad:
        with pytest.raises(ValueError, match="contrast"):
            U.check_contrast(spec, hw=hw)
    for x in (np.zeros((1, 16, 16, 1), np.float32), np.zeros((16, 16, 1), np.uint8), np.zeros((1, 16, 16, 5), np.uint8)):
        with pytest.raises(ValueError):
            U.contrast_reference(x, {"method": "clahe", "tiles": (2, 2)})


def test_pipeline_refusals(U):
    from oct_image_segmentation_models_amd.evaluation.pipeline import InferenceRun, host_batches
    with pytest.raises(ValueError, match="contrast needs raw uint8 images"):
        next(host_batches(None, np.zeros((1, 16, 32, 1), np.float32), 1, contrast={"method": "clahe", "tiles": (2, 4)}))
    with pytest.raises(ValueError, match="contrast needs raw uint8 images"):
        InferenceRun(None, np.zeros((1, 16, 32, 1), np.float32), 1, 3, contrast={"method": "clahe", "tiles": (2, 4)})
    with pytest.raises(ValueError, match="contrast"):
        InferenceRun(None, np.zeros((1, 16, 32, 1), np.uint8), 1, 3, contrast={"method": "clahe"})        # 16 // 8 = 2 rows per tile


# ---- 4. the public switches ---------------------------------------------------------------------------------------------------
def _eval_params(tmp_path, name, data, **kw):
    from oct_image_segmentation_models_amd.evaluation.evaluation_parameters import EvaluationParameters, EvaluationSaveParams
    return EvaluationParameters(model_path=tmp_path / "model" / "model.npz", mlflow_tracking_uri=None, mlflow_run_uuid=None,
                                test_dataset_path=data, save_foldername=tmp_path / name, save_params=EvaluationSaveParams(),
                                graph_search=False, metrics=["dice_coef_macro"], batch_size=2, **kw)


def test_evaluation_and_prediction_parameters(U, tmp_path, caplog):
    from oct_image_segmentation_models_amd.common.dataset import Dataset
    from oct_image_segmentation_models_amd.prediction.prediction_parameters import PredictionParams, PredictionSaveParams
    save_untrained_model(tmp_path, 16, 32, 3, 8, 2)
    data = Path(ge.ROOT) / "tests" / "golden" / "dataset_small.hdf5"

    def pp(**kw):
        ds = Dataset(np.zeros((1, 16, 32, 1), np.uint8), [Path("scan_0")], [tmp_path / "out" / "image_0"])
        return PredictionParams(tmp_path / "model" / "model.npz", None, None, ds, tmp_path / "p", PredictionSaveParams(), **kw)
    spec = {"method": "clahe", "tiles": (2, 4), "clip": 2.0}
    want = {"method": "clahe", "tiles": [2, 4], "clip": 2.0}
    assert _eval_params(tmp_path, "a", data).contrast is None and pp().contrast is None
    assert _eval_params(tmp_path, "a", data, contrast=spec).contrast == want and pp(contrast=spec).contrast == want
    for make in (lambda **kw: _eval_params(tmp_path, "a", data, **kw), pp):
        with pytest.raises(ValueError, match="contrast.json"):
            make(contrast="model")                                         # no file beside the checkpoint
        with pytest.raises(ValueError, match="contrast"):
            make(contrast="auto")
        with pytest.raises(ValueError, match="contrast"):
            make(contrast={"method": "clahe", "clip": 0.5})
    with open(tmp_path / "model" / "contrast.json", "w") as fh:
        json.dump(want, fh)
    assert _eval_params(tmp_path, "a", data, contrast="model").contrast == want and pp(contrast="model").contrast == want
    import logging
    with caplog.at_level(logging.WARNING):
        caplog.clear()
        assert _eval_params(tmp_path, "a", data).contrast is None          # the file is there, the keyword is not: a warning
        assert sum("contrast.json" in r.getMessage() for r in caplog.records) == 1


def test_train_model_on_the_cpu_path(U, tmp_path, monkeypatch):
    """``train_model(contrast=)`` up to ``fit`` without a GPU: the arrays the generators get are ``contrast_reference`` of the
    dataset's, ``contrast.json`` lies in the run folder and ``EvaluationParameters(contrast="model")`` reads it there; a
    dataset that is not uint8 is refused."""
    import torch
    from oct_image_segmentation_models_amd import optimizers as O
    from oct_image_segmentation_models_amd.common import data_generator, dataset_loader as dl, h5io
    from oct_image_segmentation_models_amd.models import engine_model
    from oct_image_segmentation_models_amd.training import training
    from oct_image_segmentation_models_amd.training.training_parameters import TrainingParams
    if torch.cuda.is_available():
        monkeypatch.setattr(torch.cuda, "is_available", lambda: False)       # this test is about the numpy path
    data = Path(ge.ROOT) / "tests" / "golden" / "dataset_small.hdf5"
    seen = {}

    class Stop(Exception):
        pass

    real_gen = data_generator.DataGenerator

    def spy_gen(images, labels, *a, **kw):
        seen.setdefault("images", []).append(np.array(images))
        return real_gen(images, labels, *a, **kw)

    def no_fit(self, *a, **kw):
        raise Stop()
    monkeypatch.setattr(training.data_gen, "DataGenerator", spy_gen)
    monkeypatch.setattr(engine_model.Model, "fit", no_fit)

    def params(name, path=data, **kw):
        return TrainingParams(model_architecture="unet", training_dataset_path=path, initial_model=None,
                              results_location=tmp_path / name, opt_con=O.Adam, opt_params={"learning_rate": 1e-3},
                              loss="dice_loss_macro", metric="dice_coef_macro", epochs=1, batch_size=2,
                              model_hyperparameters={"pool_layers": 2}, seed=3, **kw)
    spec = {"method": "clahe", "tiles": (2, 4), "clip": 2.0}
    with pytest.raises(Stop):
        training.train_model(params("on", contrast=spec), None)
    d = dl.open_dataset(data)
    tr, va = dl.load_training_data(d)[0], dl.load_validation_data(d)[0]
    assert np.array_equal(seen["images"][0], U.contrast_reference(tr, spec)) and (seen["images"][0] != tr).any()
    assert np.array_equal(seen["images"][1], U.contrast_reference(va, spec))
    (run,) = list((tmp_path / "on").iterdir())
    with open(run / "contrast.json") as fh:
        assert json.load(fh) == {"method": "clahe", "tiles": [2, 4], "clip": 2.0}
    # the file travels with the checkpoint: put an untrained model beside it and ask for "model"
    save_untrained_model(tmp_path, 16, 32, 3, 8, 2)
    (tmp_path / "model" / "contrast.json").write_text((run / "contrast.json").read_text())
    assert _eval_params(tmp_path, "e", data, contrast="model").contrast == {"method": "clahe", "tiles": [2, 4], "clip": 2.0}
    (tmp_path / "model" / "contrast.json").unlink()
    with pytest.raises(ValueError, match="contrast.json"):
        _eval_params(tmp_path, "e", data, contrast="model")

    seen.clear()
    with pytest.raises(Stop):
        training.train_model(params("off"), None)
    assert np.array_equal(seen["images"][0], tr)
    (run_off,) = list((tmp_path / "off").iterdir())
    assert not (run_off / "contrast.json").exists()

    # a dataset that is not uint8
    vals = {k: np.asarray(d[k][:]) for k in ("train_images", "train_labels", "val_images", "val_labels")}
    vals["train_images"] = vals["train_images"].astype(np.float32)
    h5io.save(tmp_path / "float.hdf5", vals)
    with pytest.raises(ValueError, match="uint8"):
        training.train_model(params("float", path=tmp_path / "float.hdf5", contrast=spec), None)
    with pytest.raises(ValueError, match="contrast"):
        params("bad", contrast={"method": "clahe", "clip": 0.25})
