"""GPU tests of the calibration feature: ``oct_calibration_counts``, ``oct_temperature_apply`` and
``oct_temperature_nll`` against their numpy restatements -- integer words bit for bit, float outputs within the bound worked
out from the restatements themselves (tests/calibration_cases.py) --, the engine-driven temperature fit against the
reference fit, and the switches through ``InferenceRun``, ``Model``, ``evaluate_model``, ``predict`` and ``train_model``."""
import json
from pathlib import Path

import numpy as np
import pytest
import torch

from oracle import unet_numpy as on
from tests.calibration_cases import (BETAS, BETAS8, BINS, FIT_SHAPE, FITS, PROB_BUDGET, SHAPES, apply_tolerance, make, salted,
                                     sum_tolerance, with_ignore)
from tests.helpers import save_untrained_model, tree_equal

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
IGNORE = 255
ids = lambda c: "x".join(map(str, c))      # noqa: E731


def _cal():
    from oct_image_segmentation_models_amd.evaluation import calibration
    return calibration


def _up(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()


def _unaligned(a):
    """``a`` on the device, one pixel (C floats) off a fresh allocation's base: 16-byte aligned only where 4 C % 16 == 0."""
    flat = torch.empty(a.size + a.shape[-1], dtype=torch.float32, device="cuda")
    view = flat[a.shape[-1]:].view(a.shape)
    view.copy_(torch.from_numpy(np.ascontiguousarray(a)))
    return view


@pytest.fixture(scope="module")
def eng():
    from oct_image_segmentation_models_amd.engine import UNetEngine
    cfg = on.UNetConfig(num_classes=3, start_neurons=8, pool_layers=2)
    params, state = on.init_params(cfg, seed=0, dtype=np.float32, randomize_bn=True)
    e = UNetEngine(device="cuda:0", input_channels=1, num_classes=3, image_height=16, image_width=32, start_neurons=8,
                   pool_layers=2, max_batch=1, seed=100)
    e.set_weights(on.keras_weight_list(params, state))
    return e


def _counts(eng, p_dev, y_dev, M, ignore):
    c, s = eng.calibration_counts(p_dev, y_dev, M, ignore)
    torch.cuda.synchronize()
    return c.cpu().numpy().view(np.uint64), s.cpu().numpy()


def _check_counts(eng, p, y, M, ignore, p_dev=None, note=None):
    cal = _cal()
    want_c, want_s, (nll64, br64) = cal.calibration_counts_reference(p, y, M, ignore, dtype=np.float64, terms=True)
    _, _, (nll32, br32) = cal.calibration_counts_reference(p, y, M, ignore, dtype=np.float32, terms=True)
    p_dev, y_dev = _up(p) if p_dev is None else p_dev, _up(y)
    got_c, got_s = _counts(eng, p_dev, y_dev, M, ignore)
    assert got_c.shape == want_c.shape and got_c.tobytes() == want_c.tobytes(), (note, M)
    assert np.array_equal(got_s[:, 2:], want_s[:, 2:]), (note, M)
    for j, (t32, t64) in enumerate(((nll32, nll64), (br32, br64))):
        err, tol = np.abs(got_s[:, j] - want_s[:, j]), sum_tolerance(t32, t64)
        print(f"counts {note} M={M} ignore={ignore} sum {j}: max err {err.max():.3e} bound {tol.min():.3e}")
        assert np.all(err <= tol), (note, M, j, err, tol)
    again_c, again_s = _counts(eng, p_dev, y_dev, M, ignore)               # a second call yields the same bytes
    assert again_c.tobytes() == got_c.tobytes() and again_s.tobytes() == got_s.tobytes()
    return got_c, got_s


# ---- 1. the counts --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ignore", [None, IGNORE], ids=["all", "ignore"])
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_counts_equal_the_reference(eng, shape, ignore):
    """Inputs salted with exact bin-edge confidences, 1.0 and arg-max ties; with ``ignore`` a third of the pixels and the
    whole last image are ignored; the same input one pixel off its base takes the unaligned (scalar) path."""
    for M in BINS:
        p, y = salted(shape, M, seed=sum(shape) + M)
        if ignore is not None:
            y = with_ignore(y, shape[-1], ignore, seed=M, empty_image=shape[0] - 1)
        c, s = _check_counts(eng, p, y, M, ignore, note=ids(shape))
        if ignore is not None:
            assert not c[-1].any() and not s[-1].any()
        c2, s2 = _check_counts(eng, p, y, M, ignore, p_dev=_unaligned(p), note=ids(shape) + " unaligned")
        assert c2.tobytes() == c.tobytes()


def test_counts_where_a_thread_walks_several_items(eng):
    """The launcher gives an image at most max(1, 2048 // B) blocks of 256 threads.  With B = 9 that is 227 blocks = 58112
    threads for the 512 * 512 / 4 = 65536 float4 items of an image: threads walk two items, and blocks of all nine images
    share the partial-row workspace."""
    shape = (9, 512, 512, 3)
    assert (2048 // shape[0]) * 256 < shape[1] * shape[2] // 4
    p, y = make(shape, 2.0, 1.5, seed=9)
    y[3, :7, :11] = 77                                           # labels that are no class: counted in sums[:, 3] alone
    c, s = _check_counts(eng, p, y, 15, None, note="large")
    assert s[3, 3] == 77 and s[:, 3].sum() == 77 and c[..., 0].sum() == 9 * 512 * 512 - 77


def test_counts_argument_errors(eng):
    from oct_image_segmentation_models_amd._hip import OctError
    p, y = (_up(a) for a in make((1, 4, 4, 3)))
    for kw in (dict(n_bins=0), dict(n_bins=65), dict(n_bins=10, ignore_label=256)):
        with pytest.raises(OctError):
            eng.calibration_counts(p, y, **kw)
    with pytest.raises(OctError):
        eng.calibration_counts(p, y[:, :2], 10)
    with pytest.raises(OctError, match="workspace"):
        eng.calibration_counts(p, y, 10, ws=torch.empty(8, dtype=torch.uint8, device="cuda"))
    with pytest.raises(OctError):
        eng.temperature_nll(p, y, [1.0] * 9)
    with pytest.raises(OctError):
        eng.temperature_nll(p, y, [0.0])
    with pytest.raises(OctError):
        eng.temperature_apply(p, float("nan"))


# ---- 2. temperature_apply -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_temperature_apply_equals_the_reference(eng, shape):
    cal = _cal()
    p, _ = salted(shape, 10, seed=sum(shape))
    for beta in BETAS:
        q64, q32 = cal.temperature_apply_reference(p, beta, np.float64), cal.temperature_apply_reference(p, beta, np.float32)
        tol = apply_tolerance(q32, q64)
        assert tol < PROB_BUDGET
        for src in (_up(p), _unaligned(p)):
            out = eng.temperature_apply(src, beta)
            inplace = eng.temperature_apply(src, beta, out=src)
            torch.cuda.synchronize()
            got = out.cpu().numpy()
            err = np.abs(got.astype(np.float64) - q64).max()
            print(f"apply {ids(shape)} beta={beta}: max err {err:.3e} bound {tol:.3e}")
            assert err <= tol, (beta, err, tol)
            assert inplace.data_ptr() == src.data_ptr() and src.cpu().numpy().tobytes() == got.tobytes()


# ---- 3. temperature_nll -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ignore", [None, IGNORE], ids=["all", "ignore"])
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_temperature_nll_equals_the_reference(eng, shape, ignore):
    cal = _cal()
    p, y = make(shape, 2.0, 1.5, seed=sum(shape))
    if ignore is not None:
        y = with_ignore(y, shape[-1], ignore, seed=1, empty_image=shape[0] - 1)
    want, cnt, t64 = cal.temperature_nll_reference(p, y, BETAS8, ignore, np.float64, terms=True)
    _, _, t32 = cal.temperature_nll_reference(p, y, BETAS8, ignore, np.float32, terms=True)
    tol = sum_tolerance(t32, t64)                                        # (B, K, 3)
    for p_dev in (_up(p), _unaligned(p)):
        y_dev = _up(y)
        s8, n8 = eng.temperature_nll(p_dev, y_dev, BETAS8, ignore)
        s8, n8 = s8.cpu().numpy(), n8.cpu().numpy()
        assert np.array_equal(n8, cnt)
        err = np.abs(s8 - want)
        print(f"nll {ids(shape)} ignore={ignore}: max err/bound {np.max(err / np.maximum(tol, 1e-300)):.3f}")
        assert np.all(err <= tol), (err, tol)
        for i in (0, 3, 7):                                              # K = 1: the row of a beta is the same bytes
            s1, n1 = eng.temperature_nll(p_dev, y_dev, [BETAS8[i]], ignore)
            assert s1.cpu().numpy()[:, 0].tobytes() == s8[:, i].tobytes() and np.array_equal(n1.cpu().numpy(), cnt)
        s8b, _ = eng.temperature_nll(p_dev, y_dev, BETAS8, ignore)
        assert s8b.cpu().numpy().tobytes() == s8.tobytes()


# ---- 4. the fit ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s,T", FITS)
def test_engine_driven_fit_equals_the_reference_fit(eng, s, T):
    cal = _cal()
    p, y = make(FIT_SHAPE, s, T, seed=11)
    p_dev, y_dev = _up(p), _up(y)

    def sums_at(beta):
        sums, cnt = eng.temperature_nll(p_dev, y_dev, [beta])
        sums, cnt = sums.cpu().numpy(), cnt.cpu().numpy()
        tot = np.zeros(3)
        for b in range(sums.shape[0]):
            tot = tot + sums[b, 0]
        return tot, float(cnt.sum())

    got, want = cal.fit_with(sums_at), cal.fit_temperature_reference(p, y)
    print(f"fit s={s} T={T}: device beta {got.beta:.9g} reference {want.beta:.9g} steps {got.steps}/{want.steps}")
    assert abs(got.beta - want.beta) <= 1e-3 * want.beta and got.steps <= 20 and got.at_bound == want.at_bound
    assert got.counted == want.counted == np.prod(FIT_SHAPE[:3])
    g_at = lambda b: abs(sums_at(b)[0][1]) / got.counted      # noqa: E731
    assert g_at(got.beta) <= g_at(1.0)


# ---- 5. the pipeline ------------------------------------------------------------------------------------------------------------
N_IMG, CC, SN, P_, BATCH, M_ = 5, 3, 8, 2, 3, 15


def _model(tmp_path, H, W):
    from oct_image_segmentation_models_amd.models.engine_model import load_model
    return load_model(save_untrained_model(tmp_path, H, W, CC, SN, P_))


def _run(model, imgs, gt, **kw):
    from oct_image_segmentation_models_amd.evaluation.pipeline import InferenceRun
    with InferenceRun(model, imgs, BATCH, CC, gt=gt, surface=False, **kw) as run:
        return list(run)


def _same_counts(batches, probs, gt, ignore=None):
    cal = _cal()
    want_c, want_s, (nll64, br64) = cal.calibration_counts_reference(probs, gt, M_, ignore, dtype=np.float64, terms=True)
    _, _, (nll32, br32) = cal.calibration_counts_reference(probs, gt, M_, ignore, dtype=np.float32, terms=True)
    assert [(b.lo, b.hi) for b in batches] == [(0, 3), (3, 5)]
    got_c, got_s = (np.concatenate([b.calibration[i] for b in batches]) for i in (0, 1))
    assert got_c.dtype == np.uint64 and got_c.tobytes() == want_c.tobytes()
    assert np.array_equal(got_s[:, 2:], want_s[:, 2:])
    for j, (t32, t64) in enumerate(((nll32, nll64), (br32, br64))):
        assert np.all(np.abs(got_s[:, j] - want_s[:, j]) <= sum_tolerance(t32, t64))


@pytest.mark.parametrize("case", ["plain", "padded", "tta", "mc"])
def test_inference_run_fills_batch_calibration(tmp_path, case):
    """The counts are those of the probabilities the corresponding ``Model`` call returns: the plain ones, the cropped ones
    of a padded size, the MEAN ones of a test-time-augmented or Monte-Carlo prediction."""
    H, W = (20, 34) if case == "padded" else (16, 32)
    imgs, labels = on.synth_scans(N_IMG, H, W, CC, seed=21)
    gt = labels[..., 0].copy()
    model = _model(tmp_path, 32 if case == "padded" else H, 64 if case == "padded" else W)
    if case == "plain":
        gt[1, :5] = IGNORE
        batches = _run(model, imgs, gt, calibration_bins=M_, ignore_label=IGNORE)
        _same_counts(batches, model.predict(imgs, batch_size=BATCH), gt, IGNORE)
        off = _run(model, imgs, None)
        assert all(b.calibration is None for b in off)
        assert all(np.array_equal(a.labels, b.labels) and np.array_equal(a.maps, b.maps) for a, b in zip(batches, off))
    elif case == "padded":
        batches = _run(model, imgs, gt, calibration_bins=M_, pad_mode="edge")
        _same_counts(batches, model.predict(imgs, batch_size=BATCH, pad_mode="edge"), gt)
    elif case == "tta":
        views = ("identity", "flip_lr")
        batches = _run(model, imgs, gt, calibration_bins=M_, tta=views)
        _same_counts(batches, model.predict_tta(imgs, views, batch_size=BATCH)[0], gt)
        assert batches[0].entropy is not None
    else:
        batches = _run(model, imgs, gt, calibration_bins=M_, mc_samples=2, mc_step0=3)
        _same_counts(batches, model.predict_mc(imgs, 2, batch_size=BATCH, step0=3)[0], gt)


def test_temperature_in_the_pipeline_and_in_predict(tmp_path):
    from oct_image_segmentation_models_amd.common.utils import soft_boundary_maps_reference
    cal = _cal()
    imgs, labels = on.synth_scans(N_IMG, 16, 32, CC, seed=21)
    model = _model(tmp_path, 16, 32)
    plain, tempered = model.predict(imgs, batch_size=BATCH), model.predict(imgs, batch_size=BATCH, temperature=2.0)
    assert np.array_equal(model.predict(imgs, batch_size=BATCH, temperature=1.0), plain)
    q64, q32 = cal.temperature_apply_reference(plain, 0.5, np.float64), cal.temperature_apply_reference(plain, 0.5, np.float32)
    assert np.abs(tempered.astype(np.float64) - q64).max() <= apply_tolerance(q32, q64) < PROB_BUDGET
    batches = _run(model, imgs, labels[..., 0], temperature=2.0, soft_maps=True, calibration_bins=M_)
    maps = np.concatenate([b.maps for b in batches])
    assert maps.tobytes() == soft_boundary_maps_reference(tempered).tobytes()
    assert maps.tobytes() != soft_boundary_maps_reference(plain).tobytes()
    _same_counts(batches, tempered, labels[..., 0])                      # the counts see the tempered probabilities too
    for kw in (dict(tta=("identity", "flip_lr")), dict(mc_samples=2)):
        with pytest.raises(ValueError, match="temperature"):
            _run(model, imgs, None, temperature=2.0, **kw)
    with pytest.raises(ValueError, match="uint8"):
        _run(model, imgs.astype(np.float32), labels[..., 0], calibration_bins=M_)


def test_switches_off_launch_no_new_kernel(tmp_path):
    """With every switch at its default the engine's launch profiler sees no kernel of this feature; with them on it sees
    them.  (The profiler records eager launches only: the pipeline runs its Monte-Carlo chain, which is eager, and
    ``Model.predict`` is.)"""
    from oct_image_segmentation_models_amd.evaluation.pipeline import InferenceRun
    imgs, labels = on.synth_scans(3, 16, 32, CC, seed=2)
    model = _model(tmp_path, 16, 32)
    mine = lambda ks: {k for k in ks if "calib" in k or "temperature" in k}      # noqa: E731

    def pipeline(**kw):
        with InferenceRun(model, imgs, BATCH, CC, gt=labels[..., 0], confusion=True, surface=False, mc_samples=2, **kw) as run:
            e = model._ensure_engine(BATCH, False)
            e.profile_begin()
            list(run)
            return {r["kernel"] for r in e.profile_end()}

    def predict(**kw):
        e = model._ensure_engine(BATCH, False)
        e.profile_begin()
        model.predict(imgs, batch_size=BATCH, **kw)
        return {r["kernel"] for r in e.profile_end()}
    off, on_ = pipeline(), pipeline(calibration_bins=M_)
    assert off and not mine(off) and on_ - off == mine(on_) == {"calib_counts_k<C>", "calib_rows_sum_k"}
    off, on_ = predict(), predict(temperature=2.0)
    assert off and not mine(off) and on_ - off == mine(on_) == {"temperature_apply_k<C>"}


# ---- 6. evaluate_model and predict end to end -----------------------------------------------------------------------------------------
def test_evaluate_model_and_predict_end_to_end(tmp_path):
    from oct_image_segmentation_models_amd.common import dataset_loader as dl, h5io
    from oct_image_segmentation_models_amd.common.dataset import Dataset
    from oct_image_segmentation_models_amd.evaluation import eval_model
    from oct_image_segmentation_models_amd.evaluation.evaluation_parameters import EvaluationParameters, EvaluationSaveParams
    from oct_image_segmentation_models_amd.prediction import predict
    from oct_image_segmentation_models_amd.prediction.prediction_parameters import PredictionParams, PredictionSaveParams
    cal = _cal()
    data = ROOT / "tests" / "golden" / "dataset_small.hdf5"
    images, labels, _ = dl.load_testing_data(dl.open_dataset(data))
    n, H, W = images.shape[:3]
    save_untrained_model(tmp_path, H, W, CC, SN, P_)

    def evaluate(name, **kw):
        ep = EvaluationParameters(model_path=tmp_path / "model" / "model.npz", mlflow_tracking_uri=None, mlflow_run_uuid=None,
                                  test_dataset_path=data, save_foldername=tmp_path / name, save_params=EvaluationSaveParams(),
                                  graph_search=False, metrics=["dice_coef_classes", "dice_coef_macro", "dice_coef_micro"],
                                  batch_size=2, **kw)
        eval_model(ep)
        return tmp_path / name

    plain, off, on_ = evaluate("plain"), evaluate("off", calibration_bins=0, temperature=1.0), evaluate("on", calibration_bins=M_)
    tree_equal(plain, off, ["evaluation_results.hdf5", "overall_evaluation_results.hdf5", "eval_params.hdf5"])
    from oct_image_segmentation_models_amd.models.engine_model import load_model
    probs = load_model(tmp_path / "model" / "model.npz").predict(images, batch_size=2)
    want_c, _ = cal.calibration_counts_reference(probs, labels[..., 0], M_)
    names = lambda d: {k for k in d if not k.startswith("attr:")}      # noqa: E731
    tables, nll, brier = [], [], []
    for i in range(n):
        f, g = h5io.load(on_ / f"image_{i}" / "evaluation_results.hdf5"), h5io.load(off / f"image_{i}" / "evaluation_results.hdf5")
        assert names(f) - names(g) == {"calibration_counts", "ece", "mce", "nll", "brier"} and names(g) <= names(f)
        assert all(np.array_equal(f[k], g[k]) for k in names(g))
        assert np.array_equal(f["calibration_counts"], cal.counts_as_float(want_c[i]))
        tables.append(f["calibration_counts"]); nll.append(f["nll"][0]); brier.append(f["brier"][0])
    o, o_off = h5io.load(on_ / "overall_evaluation_results.hdf5"), h5io.load(off / "overall_evaluation_results.hdf5")
    assert all(np.array_equal(o[k], o_off[k]) for k in o_off)
    assert {k for k in o if k not in o_off} == {"calibration_counts"} | {f"{p}{k}" for k in cal.CALIBRATION_METRICS
                                                                         for p in ("", "mean_", "sd_", "pooled_")}
    total, pooled = cal.pooled_calibration(np.stack(tables), nll, brier)
    assert np.array_equal(o["calibration_counts"], np.stack(tables).sum(0)) and np.array_equal(total, o["calibration_counts"])
    direct = cal.calibration_from_counts(total, [sum(a * t[:, 0].sum() for a, t in zip(nll, tables)),
                                                 sum(b * t[:, 0].sum() for b, t in zip(brier, tables)), total[:, 0].sum(), 0])
    for k in cal.CALIBRATION_METRICS:
        assert o[f"pooled_{k}"][0] == pooled[k] and np.isclose(pooled[k], direct[k], rtol=1e-12)

    def run_predict(name, **kw):
        ds = Dataset(images, [Path(f"volume_{i}.tiff") for i in range(n)], [tmp_path / name / f"image_{i}" for i in range(n)])
        pp = PredictionParams(model_path=tmp_path / "model" / "model.npz", mlflow_tracking_uri=None, mlflow_run_uuid=None,
                              dataset=ds, config_output_dir=tmp_path / name, save_params=PredictionSaveParams(),
                              graph_search=False, batch_size=2, binarize=False, **kw)
        return predict(pp)
    p_plain, p_off, p_on = run_predict("p_plain"), run_predict("p_off", temperature=1.0), run_predict("p_on", temperature=2.0)
    tree_equal(tmp_path / "p_plain", tmp_path / "p_off", ["prediction_info.hdf5", "prediction_params.hdf5"])
    assert any(not np.array_equal(a.boundary_maps, b.boundary_maps) for a, b in zip(p_off, p_on))
    assert all(np.array_equal(a.predicted_labels, b.predicted_labels) for a, b in zip(p_off, p_on))
    assert float(h5io.load(tmp_path / "p_on" / "prediction_params.hdf5")["attr:temperature"]) == 2.0
    assert float(h5io.load(p_on[0].image_output_dir / "prediction_info.hdf5")["attr:temperature"]) == 2.0
    assert "attr:temperature" not in h5io.load(p_off[0].image_output_dir / "prediction_info.hdf5")


# ---- 7. train_model(fit_temperature=True) ---------------------------------------------------------------------------------------------
def test_train_model_writes_the_fitted_temperature(tmp_path):
    from oct_image_segmentation_models_amd import optimizers as O
    from oct_image_segmentation_models_amd.common import dataset_loader as dl
    from oct_image_segmentation_models_amd.training.training import train_model
    from oct_image_segmentation_models_amd.training.training_parameters import TrainingParams
    cal = _cal()
    data = ROOT / "tests" / "golden" / "dataset_small.hdf5"                    # 16 x 32 scans

    def train(name, **kw):
        tp = TrainingParams(model_architecture="unet", training_dataset_path=data, initial_model=None,
                            results_location=tmp_path / name, opt_con=O.Adam, opt_params={"learning_rate": 1e-3},
                            loss="dice_loss_macro", metric="dice_coef_macro", epochs=1, batch_size=2,
                            model_hyperparameters={"pool_layers": 2}, seed=3, **kw)
        return train_model(tp, None)
    res = train("on", fit_temperature=True)
    rec = cal.read_temperature(Path(res.save_foldername) / "temperature.json")
    val_x, val_y = dl.load_validation_data(dl.open_dataset(data))
    want = res.model.fit_temperature(val_x, val_y, 2)
    assert vars(rec) == vars(want) and rec.counted == val_y.size and 1 / 16 <= rec.temperature <= 16 and rec.steps >= 1
    ref = cal.fit_temperature_reference(res.model.predict(val_x, batch_size=2), val_y[..., 0])
    assert abs(rec.beta - ref.beta) <= 1e-3 * ref.beta
    with open(Path(res.save_foldername) / "temperature.json") as fh:
        assert set(json.load(fh)) == {"temperature", "beta", "nll_before", "nll_after", "steps", "counted", "at_bound"}
    off = train("off")
    assert not (Path(off.save_foldername) / "temperature.json").exists()
    assert sorted(p.name for p in Path(off.save_foldername).iterdir()) == \
        sorted(p.name for p in Path(res.save_foldername).iterdir() if p.name != "temperature.json")
