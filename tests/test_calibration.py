"""CPU tests of the calibration feature: the numpy restatements of ``oct_calibration_counts`` /
``oct_temperature_apply`` / ``oct_temperature_nll`` against a plain per-pixel loop and known answers, the derivatives against
central differences, THE fit rule against a dense grid search, the public parameters and their refusals, and the host side of
``evaluate_model`` over injected records."""
import inspect
import json
import math
from pathlib import Path

import numpy as np
import pytest

import __graft_entry__ as ge
from tests.calibration_cases import BETAS8, FIT_SHAPE, FITS, make, salted, with_ignore
from tests.helpers import save_untrained_model, tree_equal

EPS = np.float32(1e-7)


@pytest.fixture(scope="module")
def cal():
    ge.build()
    from oct_image_segmentation_models_amd.evaluation import calibration
    return calibration


# ---- the restatements against a per-pixel loop --------------------------------------------------------------------------------
def _loop_counts(p, y, M, ignore):
    B, C = p.shape[0], p.shape[-1]
    pf, yf = p.reshape(B, -1, C), y.reshape(B, -1)
    counts, sums = np.zeros((B, M, 3), np.uint64), np.zeros((B, 4))
    for b in range(B):
        for px in range(pf.shape[1]):
            lab = int(yf[b, px])
            if lab == ignore:
                continue
            if lab >= C:
                sums[b, 3] += 1
                continue
            q = pf[b, px]
            m = 0
            for c in range(1, C):
                if q[c] > q[m]:
                    m = c
            conf = min(max(q[m], np.float32(0)), np.float32(1))
            k = int(math.floor(float(conf) * 2.0 ** 28))
            bin_ = min(M - 1, (k * M) >> 28)
            counts[b, bin_] += np.array([1, int(m == lab), k], np.uint64)
            sums[b, 0] += float(-np.log(min(max(q[lab], EPS), np.float32(1) - EPS)))
            br = np.float32(0)
            for c in range(C):
                d = q[c] - np.float32(c == lab)
                br = d * d if c == 0 else br + d * d
            sums[b, 1] += float(br)
            sums[b, 2] += 1
    return counts, sums


@pytest.mark.parametrize("shape,M,ignore", [((2, 5, 7, 3), 10, None), ((1, 4, 9, 12), 15, 200), ((2, 3, 5, 2), 1, 2), ((1, 6, 6, 4), 64, None)])
def test_counts_restatement_equals_the_pixel_loop(cal, shape, M, ignore):
    p, y = salted(shape, M, seed=3)
    if ignore is not None:
        y = with_ignore(y, shape[-1], ignore, seed=3)
    y[0, 0, 0] = 250                                           # a label that is no class and not the ignore label
    counts, sums = cal.calibration_counts_reference(p, y, M, ignore)
    want_c, want_s = _loop_counts(p, y, M, -1 if ignore is None else ignore)
    assert counts.dtype == np.uint64 and np.array_equal(counts, want_c)
    assert np.array_equal(sums[:, 2:], want_s[:, 2:]) and sums[0, 3] == 1
    assert np.allclose(sums[:, :2], want_s[:, :2], rtol=1e-12, atol=0)
    c64, s64 = cal.calibration_counts_reference(p, y, M, ignore, dtype=np.float64)
    assert np.array_equal(c64, counts) and np.allclose(s64, sums, rtol=1e-5)


def test_temperature_restatements_equal_the_pixel_loop(cal):
    p, y = make((2, 4, 5, 5), 2.0, 1.0, seed=4)
    y = with_ignore(y, 5, 9, seed=4)
    for beta in (0.25, 1.0, 3.0):
        q = cal.temperature_apply_reference(p, beta, np.float64)
        sums, cnt = cal.temperature_nll_reference(p, y, [beta], 9, np.float64)
        want = np.zeros((2, 3)); n = np.zeros(2)
        b32 = float(np.float32(beta))
        for b in range(2):
            for i in range(4):
                for j in range(5):
                    l = np.log(np.maximum(p[b, i, j].astype(np.float64), float(EPS)))
                    e = np.exp(b32 * (l - l.max()))
                    qq = e / e.sum()
                    assert np.allclose(q[b, i, j], qq, rtol=1e-14)
                    if y[b, i, j] == 9:
                        continue
                    mu = (qq * l).sum()
                    want[b] += [np.log(e.sum()) - b32 * (l[y[b, i, j]] - l.max()), mu - l[y[b, i, j]], (qq * (l - mu) ** 2).sum()]
                    n[b] += 1
        assert np.allclose(sums[:, 0], want, rtol=1e-12) and np.array_equal(cnt, n)


# ---- known answers --------------------------------------------------------------------------------------------------------------
def test_known_answers(cal):
    p = np.tile(np.array([0.75, 0.25], np.float32), (1, 2, 2, 1))
    y = np.array([[[0, 0], [0, 1]]], np.uint8)                                        # 3 of 4 right
    c, s = cal.calibration_counts_reference(p, y, 10)
    m = cal.calibration_from_counts(c[0], s[0])
    assert m["ece"] == 0.0 and m["mce"] == 0.0 and c[0, 7].tolist() == [4, 3, 4 * 3 * 2 ** 26]
    p = np.full((1, 2, 2, 2), 0.5, np.float32)
    c, s = cal.calibration_counts_reference(p, np.zeros((1, 2, 2), np.uint8), 10)     # ties take class 0: all right
    m = cal.calibration_from_counts(c[0], s[0])
    assert m["ece"] == 0.5 and m["mce"] == 0.5 and c[0, 5, 1] == 4
    assert math.isclose(m["nll"], math.log(2), rel_tol=1e-6) and math.isclose(m["brier"], 0.5)
    # conf = 1.0 lands in the last bin, conf = k / M in bin k
    for M in (1, 8, 10, 64):
        one = np.array([[[[0.0, 1.0]]]], np.float32)
        assert cal.calibration_counts_reference(one, np.ones((1, 1, 1), np.uint8), M)[0][0, M - 1].tolist() == [1, 1, 2 ** 28]
    for k in range(4, 8):
        edge = np.array([[[[k / 8, 1 - k / 8]]]], np.float32)
        assert cal.calibration_counts_reference(edge, np.zeros((1, 1, 1), np.uint8), 8)[0][0, k, 0] == 1
    half = np.array([[[[0.5, 0.25, 0.25]]]], np.float32)
    assert cal.calibration_counts_reference(half, np.zeros((1, 1, 1), np.uint8), 10)[0][0, 5, 0] == 1
    # arg-max ties take the lowest index
    tie = np.array([[[[0.2, 0.4, 0.4]]]], np.float32)
    c, _ = cal.calibration_counts_reference(tie, np.array([[[2]]], np.uint8), 5)
    assert c[0, 2].tolist() == [1, 0, int(np.float32(0.4) * 2 ** 28)]
    c, _ = cal.calibration_counts_reference(tie, np.array([[[1]]], np.uint8), 5)
    assert c[0, 2, 1] == 1


def test_temperature_known_answers(cal):
    for C in (2, 3, 7):
        u = np.full((1, 2, 2, C), 1.0 / C, np.float32)
        for beta in (1 / 16, 0.5, 3.0, 16.0):
            for dt in (np.float32, np.float64):
                q = cal.temperature_apply_reference(u, beta, dt)
                assert q.dtype == dt and np.all(q == q[..., :1]) and np.allclose(q, 1.0 / C, rtol=1e-6)
    p = np.linspace(0.01, 0.99, 23, dtype=np.float32)
    two = np.stack([p, np.float32(1) - p], -1)[None]
    for beta in (0.25, 2.0, 5.0):
        q = cal.temperature_apply_reference(two, beta, np.float64)[0, :, 0]
        a, b = two[0, :, 0].astype(np.float64) ** beta, two[0, :, 1].astype(np.float64) ** beta
        assert np.allclose(q, a / (a + b), rtol=1e-12)
    assert np.allclose(cal.temperature_apply_reference(two, 1.0, np.float64), two, atol=1e-7)


def test_image_without_a_counted_pixel(cal):
    p, y = make((2, 4, 4, 3), seed=1)
    y[1] = 7
    c, s = cal.calibration_counts_reference(p, y, 15, 7)
    assert not c[1].any() and s[1].tolist() == [0, 0, 0, 0] and c[0, :, 0].sum() == 16
    m = cal.calibration_from_counts(c[1], s[1])
    assert set(m) == {"ece", "mce", "nll", "brier"} and all(math.isnan(v) for v in m.values())
    sums, cnt = cal.temperature_nll_reference(p, y, [1.0, 2.0], 7)
    assert cnt.tolist() == [16, 0] and not sums[1].any()
    r = cal.fit_temperature_reference(p[1:], y[1:], 7)
    assert r.counted == 0 and r.beta == 1.0 and math.isnan(r.nll_before) and r.steps == 0 and not r.at_bound
    total, pooled = cal.pooled_calibration(cal.counts_as_float(c), [1.0, np.nan], [0.5, np.nan])
    assert np.array_equal(total, cal.counts_as_float(c[0])) and pooled["nll"] == 1.0 and pooled["brier"] == 0.5


# ---- derivatives and the fit ------------------------------------------------------------------------------------------------------
def test_g_and_h_are_the_derivatives_of_the_nll(cal):
    p, y = make((2, 6, 7, 4), 2.0, 1.5, seed=5)
    d = 1e-4
    for beta in (0.3, 1.0, 4.0):
        # (beta is rounded to float32 inside, as on the device: take betas float32 holds)
        b0, bm, bp = (float(np.float32(v)) for v in (beta, beta - d, beta + d))
        (s0, sm, sp), _ = zip(*[cal.temperature_nll_reference(p, y, [b], None, np.float64) for b in (b0, bm, bp)])
        nll = lambda s: s[:, 0, 0].sum()      # noqa: E731
        g, h = s0[:, 0, 1].sum(), s0[:, 0, 2].sum()
        g_fd = (nll(sp) - nll(sm)) / (bp - bm)
        h_fd = (sp[:, 0, 1].sum() - sm[:, 0, 1].sum()) / (bp - bm)
        assert abs(g - g_fd) <= 1e-5 * max(1.0, abs(g)) and abs(h - h_fd) <= 1e-5 * max(1.0, abs(h)) and h > 0


def test_rows_do_not_depend_on_position(cal):
    p, y = make((1, 5, 6, 3), seed=2)
    all8, _ = cal.temperature_nll_reference(p, y, BETAS8, None, np.float32)
    for i, b in enumerate(BETAS8):
        one, _ = cal.temperature_nll_reference(p, y, [b], None, np.float32)
        assert one[:, 0].tobytes() == all8[:, i].tobytes()


@pytest.mark.parametrize("s,T", FITS)
def test_fit_beta_against_a_grid_search(cal, s, T):
    p, y = make(FIT_SHAPE, s, T, seed=11)
    r = cal.fit_temperature_reference(p, y)
    grid = np.exp(np.linspace(math.log(1 / 16), math.log(16), 2049))
    nll = lambda b: cal.temperature_nll_reference(p, y, [b], None, np.float64)[0][:, 0, 0].sum()      # noqa: E731
    coarse = np.array([nll(b) for b in grid])
    i = int(coarse.argmin())
    fine = np.exp(np.linspace(math.log(grid[max(i - 1, 0)]), math.log(grid[min(i + 1, 2048)]), 41))
    best = fine[int(np.argmin([nll(b) for b in fine]))]
    assert abs(r.beta - best) <= 1e-3 * best and 1 <= r.steps <= 20 and not r.at_bound
    assert r.temperature == 1.0 / r.beta and r.nll_after <= r.nll_before and r.counted == np.prod(FIT_SHAPE[:3])
    assert 0.5 / T < r.beta < 2.0 / T                                   # it finds the temperature the labels were drawn at
    r32 = cal.fit_temperature_reference(p, y, dtype=np.float32)
    assert abs(r32.beta - r.beta) <= 1e-4 * r.beta


def test_the_bracket_ends_set_at_bound(cal):
    for sign, end in ((1.0, 1 / 16), (-1.0, 16.0)):                       # g > 0 everywhere: the optimum lies below the bracket
        beta, steps, at_bound = cal.fit_beta(lambda b: (sign, 0.0))
        assert at_bound and abs(beta - end) <= 1e-3 * end and steps <= 20
    beta, steps, at_bound = cal.fit_beta(lambda b: (b * b - 6.25, 2.0 * b))     # Newton's square root: quadratic convergence
    assert abs(beta - 2.5) <= 1e-4 * 2.5 and steps <= 6 and not at_bound
    # a Newton step that leaves the bracket is replaced by the bisection in log space
    beta, steps, at_bound = cal.fit_beta(lambda b: ((b - 0.5) * 1e-3, 1e-6 if b == 1.0 else 1e-3))
    assert abs(beta - 0.5) <= 1e-3 and not at_bound


# ---- parameters and refusals ------------------------------------------------------------------------------------------------------
def test_checks(cal):
    assert cal.check_bins(0) == 0 and cal.check_bins(64) == 64 and cal.check_temperature(1) == 1.0
    assert cal.check_temperature(1 / 16) == 1 / 16 and cal.check_temperature(16) == 16.0
    for bad in (-1, 65, 1.5, True, None, "3"):
        with pytest.raises(ValueError, match="calibration_bins"):
            cal.check_bins(bad)
    for bad in (0, 0.06, 16.5, -1.0, float("nan"), None, "2", True):
        with pytest.raises(ValueError, match="temperature"):
            cal.check_temperature(bad)


def test_switches_default_to_off_on_every_layer(cal):
    from oct_image_segmentation_models_amd.evaluation.evaluation_parameters import EvaluationParameters
    from oct_image_segmentation_models_amd.evaluation.pipeline import Batch, BatchedPredictor, InferenceRun, host_batches
    from oct_image_segmentation_models_amd.models.engine_model import Model
    from oct_image_segmentation_models_amd.prediction.prediction_parameters import PredictionParams
    from oct_image_segmentation_models_amd.training.training_parameters import TrainingParams
    sig = lambda f: inspect.signature(f).parameters      # noqa: E731
    for fn in (EvaluationParameters.__init__, InferenceRun.__init__, host_batches):
        assert sig(fn)["calibration_bins"].default == 0 and sig(fn)["temperature"].default == 1.0
    assert sig(BatchedPredictor.__init__)["calibration"].default is None and sig(BatchedPredictor.__init__)["temperature"].default == 1.0
    assert sig(PredictionParams.__init__)["temperature"].default == 1.0 and sig(Model.predict)["temperature"].default is None
    assert sig(TrainingParams.__init__)["fit_temperature"].default is False
    assert list(sig(Model.fit_temperature))[1:] == ["x_u8", "labels", "batch_size", "ignore_label", "pad_mode"]
    plain = Batch(0, 1, np.zeros((1, 2, 2), np.uint8))
    assert plain.calibration is None and len(Batch._fields) == 7 and "calibration" not in Batch._fields
    rec = plain.with_calibration(("c", "s"))
    assert rec.calibration == ("c", "s") and rec == plain and rec.entropy is None and plain.calibration is None
    both = rec.with_uncertainty(1, 2)
    assert both.calibration == ("c", "s") and both.entropy == 1


def test_pipeline_refusals(cal):
    from oct_image_segmentation_models_amd.evaluation.pipeline import BatchedPredictor, InferenceRun, host_batches
    u8, f32 = np.zeros((2, 8, 8, 1), np.uint8), np.zeros((2, 8, 8, 1), np.float32)
    for kw in (dict(mc_samples=2), dict(tta=("identity", "flip_lr"))):
        with pytest.raises(ValueError, match="temperature"):
            InferenceRun(None, u8, 2, 3, batches=[], temperature=2.0, **kw)
        with pytest.raises(ValueError, match="temperature"):
            BatchedPredictor(None, 2, temperature=2.0, **kw)
    for kw in (dict(calibration_bins=15), dict(temperature=2.0)):
        with pytest.raises(ValueError, match="uint8"):
            InferenceRun(None, f32, 2, 3, batches=[], **kw)
        with pytest.raises(ValueError, match="uint8"):
            next(host_batches(None, f32, 2, **kw))
    for kw in (dict(calibration_bins=65), dict(temperature=17.0), dict(temperature=0.0)):
        with pytest.raises(ValueError):
            InferenceRun(None, u8, 2, 3, batches=[], **kw)
    InferenceRun(None, u8, 2, 3, batches=[], calibration_bins=15, temperature=2.0).close()      # accepted together


def _eval_params(tmp_path, name, data, **kw):
    from oct_image_segmentation_models_amd.evaluation.evaluation_parameters import EvaluationParameters, EvaluationSaveParams
    return EvaluationParameters(model_path=tmp_path / "model" / "model.npz", mlflow_tracking_uri=None, mlflow_run_uuid=None,
                                test_dataset_path=data, save_foldername=tmp_path / name, save_params=EvaluationSaveParams(),
                                graph_search=False, metrics=["dice_coef_macro"], batch_size=2, **kw)


def test_public_parameters_validate(cal, tmp_path):
    from oct_image_segmentation_models_amd.common.dataset import Dataset
    from oct_image_segmentation_models_amd.prediction.prediction_parameters import PredictionParams, PredictionSaveParams
    save_untrained_model(tmp_path, 16, 32, 3, 8, 2)
    data = Path(ge.ROOT) / "tests" / "golden" / "dataset_small.hdf5"
    ep = _eval_params(tmp_path, "a", data)
    assert ep.calibration_bins == 0 and ep.temperature == 1.0
    ep = _eval_params(tmp_path, "a", data, calibration_bins=15, temperature=2)
    assert ep.calibration_bins == 15 and ep.temperature == 2.0 and isinstance(ep.temperature, float)
    for kw in (dict(calibration_bins=65), dict(calibration_bins=-1), dict(calibration_bins=1.0), dict(temperature=0.01),
               dict(temperature=32), dict(temperature=2.0, tta=("identity", "flip_lr"))):
        with pytest.raises(ValueError):
            _eval_params(tmp_path, "a", data, **kw)
    _eval_params(tmp_path, "a", data, calibration_bins=10, tta=("identity", "flip_lr"))       # counts of the mean: allowed

    def pp(**kw):
        ds = Dataset(np.zeros((1, 16, 32, 1), np.uint8), [Path("scan_0")], [tmp_path / "out" / "image_0"])
        return PredictionParams(tmp_path / "model" / "model.npz", None, None, ds, tmp_path / "p", PredictionSaveParams(), **kw)
    assert pp().temperature == 1.0 and pp(temperature=0.5).temperature == 0.5
    for kw in (dict(temperature=0.0), dict(temperature=2.0, mc_samples=2), dict(temperature=2.0, tta=("flip_lr",))):
        with pytest.raises(ValueError, match="temperature"):
            pp(**kw)


def test_read_temperature_round_trip(cal, tmp_path):
    rec = cal.fit_record(0.5, 4, False, 1.25, 1.0, 100)
    cal.write_temperature(tmp_path / cal.TEMPERATURE_FILENAME, rec)
    back = cal.read_temperature(tmp_path / "temperature.json")
    assert vars(back) == vars(rec) and back.temperature == 2.0 and set(vars(back)) == {"temperature", "beta", "nll_before", "nll_after",
                                                                                     "steps", "counted", "at_bound"}
    with open(tmp_path / "bad.json", "w") as fh:
        json.dump(dict(vars(rec), temperature=100.0), fh)
    with pytest.raises(ValueError, match="temperature"):
        cal.read_temperature(tmp_path / "bad.json")


# ---- the host side of evaluate_model over injected records ---------------------------------------------------------------------------
def test_evaluate_model_host_side_with_injected_records(cal, tmp_path, monkeypatch):
    """``evaluate_model`` with its ``InferenceRun`` fed from hand-made records (no device): with the switch on the new datasets
    are there and hold what ``calibration_from_counts`` says; everything else equals a run with it off."""
    from oct_image_segmentation_models_amd.common import dataset_loader as dl, h5io
    from oct_image_segmentation_models_amd.evaluation import evaluation
    from oct_image_segmentation_models_amd.evaluation.pipeline import Batch, InferenceRun
    data = Path(ge.ROOT) / "tests" / "golden" / "dataset_small.hdf5"
    images, labels, _ = dl.load_testing_data(dl.open_dataset(data))
    n, H, W = images.shape[:3]
    C, M, B = 3, 15, 2
    save_untrained_model(tmp_path, H, W, C, 8, 2)
    probs, _ = make((n, H, W, C), 2.0, 1.0, seed=8)
    pred = probs.argmax(-1).astype(np.uint8)
    gt = labels[..., 0]
    counts, sums = cal.calibration_counts_reference(probs, gt, M)
    maps = np.zeros((n, C - 1, H, W), np.uint8)

    def run(name, **kw):
        def records():
            for lo in range(0, n, B):
                b = Batch(lo, min(lo + B, n), pred[lo:lo + B], maps[lo:lo + B])
                yield b.with_calibration((counts[lo:lo + B], sums[lo:lo + B])) if kw.get("calibration_bins") else b

        def injected(model, imgs, batch, num_classes, **rest):
            assert rest["calibration_bins"] == kw.get("calibration_bins", 0) and rest["temperature"] == kw.get("temperature", 1.0)
            assert (rest["gt"] is not None) == bool(kw.get("calibration_bins"))
            return InferenceRun(None, imgs, batch, num_classes, batches=records(), **rest)
        monkeypatch.setattr(evaluation, "InferenceRun", injected)
        evaluation.evaluate_model(_eval_params(tmp_path, name, data, **kw))
        return tmp_path / name

    off, plain, on = run("off", calibration_bins=0, temperature=1.0), run("plain"), run("on", calibration_bins=M, temperature=2.0)
    tree_equal(plain, off, ["evaluation_results.hdf5", "overall_evaluation_results.hdf5", "eval_params.hdf5"])
    new = {"calibration_counts", "ece", "mce", "nll", "brier"}
    for i in range(n):
        f, g = h5io.load(on / f"image_{i}" / "evaluation_results.hdf5"), h5io.load(off / f"image_{i}" / "evaluation_results.hdf5")
        names = lambda d: {k for k in d if not k.startswith("attr:")}      # noqa: E731
        assert names(f) - names(g) == new and names(g) <= names(f)
        assert all(np.array_equal(f[k], g[k]) for k in names(g))
        t = f["calibration_counts"]
        assert t.dtype == np.float64 and t.shape == (M, 3) and np.array_equal(t, cal.counts_as_float(counts[i]))
        want = cal.calibration_from_counts(counts[i], sums[i])
        for k in ("ece", "mce", "nll", "brier"):
            assert f[k].dtype == np.float64 and f[k].shape == (1,) and f[k][0] == want[k]
    o, o_off = h5io.load(on / "overall_evaluation_results.hdf5"), h5io.load(off / "overall_evaluation_results.hdf5")
    added = {k for k in o if k not in o_off}
    assert added == {"calibration_counts"} | {f"{p}{k}" for k in ("ece", "mce", "nll", "brier") for p in ("", "mean_", "sd_", "pooled_")}
    assert all(np.array_equal(o[k], o_off[k]) for k in o_off)
    total = cal.counts_as_float(counts).sum(0)
    assert np.array_equal(o["calibration_counts"], total)
    pooled = cal.calibration_from_counts(total, sums.sum(0))
    for k in ("ece", "mce"):
        assert o[f"pooled_{k}"][0] == pooled[k]
    for k in ("nll", "brier"):
        assert math.isclose(o[f"pooled_{k}"][0], pooled[k], rel_tol=1e-12)
    assert np.array_equal(o["mean_ece"], np.mean([cal.calibration_from_counts(c, s)["ece"] for c, s in zip(counts, sums)], keepdims=True))
    cfg, cfg_off = h5io.load(on / "eval_params.hdf5"), h5io.load(off / "eval_params.hdf5")
    assert int(cfg["attr:calibration_bins"]) == M and float(cfg["attr:temperature"]) == 2.0
    assert "attr:calibration_bins" not in cfg_off and "attr:temperature" not in cfg_off
    csv = (on / "overall_evaluation_results.csv").read_text()
    assert "Mean ece," in csv and "Pooled ece," in csv and "ece" not in (off / "overall_evaluation_results.csv").read_text()
