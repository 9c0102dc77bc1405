"""CPU tests of the Monte-Carlo dropout prediction: the numpy restatement ``mc_reduce_reference`` on hand-made stacks, the
workspace size, the argument errors of ``oct_mc_update`` / ``oct_unet_infer`` that return before any launch, the
public parameters, and ``InferenceRun`` carrying the uncertainty maps of injected batches to ``predict``'s savers."""
import ctypes as C
import inspect
import json
from pathlib import Path

import numpy as np
import pytest

import __graft_entry__ as ge
from tests.mc_cases import ENTROPY_TOL, softmax_stack


@pytest.fixture(scope="module")
def hip():
    ge.build()
    from oct_image_segmentation_models_amd import _hip
    return _hip


def _ref(stack, dtype=np.float32):
    from oct_image_segmentation_models_amd.common.utils import mc_reduce_reference
    return mc_reduce_reference(stack, dtype)


def _entropy64(p):
    p = p.astype(np.float64)
    return -np.where(p > 0, p * np.log(np.where(p > 0, p, 1.0)), 0.0).sum(-1)


# ---- the restatement ---------------------------------------------------------------------------------------------------
def test_identical_samples_have_no_mutual_information():
    one = softmax_stack((1, 2, 5, 7, 4), seed=1)
    for T in (1, 2, 3, 8):
        m, am, ent, mi = _ref(np.repeat(one, T, axis=0))
        assert m.dtype == np.float32 and am.dtype == np.uint8 and ent.dtype == np.float32 and mi.dtype == np.float32
        assert m.shape == (2, 5, 7, 4) and am.shape == ent.shape == mi.shape == (2, 5, 7)
        assert np.abs(m - one[0]).max() < 1e-6 and np.array_equal(am, one[0].argmax(-1))
        assert np.allclose(ent, _entropy64(one[0]), atol=ENTROPY_TOL, rtol=0)
        assert np.abs(mi).max() <= ENTROPY_TOL and (mi >= 0).all()
        if T <= 2:                       # p + p and 2p * 0.5 are exact: the mean IS the sample, entropy and E / T the same float
            assert np.array_equal(m, one[0]) and (mi == 0).all()


@pytest.mark.parametrize("Cn", [2, 3, 8, 32])
def test_uniform_probabilities_give_ln_c(Cn):
    p = np.full((3, 1, 2, 3, Cn), 1.0 / Cn, np.float32)
    m, am, ent, mi = _ref(p)
    assert np.allclose(ent, np.log(Cn), atol=ENTROPY_TOL, rtol=0) and (am == 0).all()      # lowest index among equal maxima
    assert np.abs(mi).max() <= ENTROPY_TOL


def test_disagreeing_one_hot_samples_are_all_mutual_information():
    p = np.zeros((2, 1, 1, 4, 3), np.float32)
    p[0, ..., 0] = 1.0
    p[1, ..., 2] = 1.0
    m, am, ent, mi = _ref(p)
    assert np.array_equal(m[0, 0, 0], [0.5, 0.0, 0.5]) and (am == 0).all()
    assert (ent > 0).all() and np.allclose(ent, np.log(2.0), atol=ENTROPY_TOL, rtol=0)
    assert np.array_equal(mi, ent)       # every sample's entropy is exactly 0


def test_zeros_contribute_nothing_and_nothing_is_nan():
    p = np.zeros((3, 1, 2, 2, 5), np.float32)
    p[..., 1] = 0.25
    p[..., 4] = 0.75
    got = _ref(p)
    assert all(np.isfinite(a).all() for a in got)
    q = np.ascontiguousarray(p[..., [1, 4]])
    want = _ref(q)
    assert np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3]) and (got[1] == 4).all()
    assert (_ref(np.zeros((2, 1, 1, 1, 3), np.float32))[2] == 0).all()


@pytest.mark.parametrize("shape", [(1, 3, 5, 7, 3), (2, 1, 16, 32, 2), (5, 2, 9, 13, 8), (64, 1, 3, 17, 32)],
                         ids=lambda s: "x".join(map(str, s)))
def test_fp32_and_fp64_variants_agree_within_the_bound(shape):
    p = softmax_stack(shape, seed=7)
    assert (p == 0).any() and (p == 1).any()
    m32, a32, e32, i32 = _ref(p, np.float32)
    m64, a64, e64, i64 = _ref(p, np.float64)
    assert m64.dtype == np.float64 and np.abs(m32 - m64).max() < 5e-6    # T 2^-24 relative, T <= 64
    assert np.abs(e32 - e64).max() <= ENTROPY_TOL and np.abs(i32 - i64).max() <= ENTROPY_TOL
    ok = np.abs(p.astype(np.float64).sum(-1) - 1.0).max(0) < 1e-6       # (the pixels with a zeroed class are no distributions)
    assert (i32 >= 0).all() and (e64[ok] <= np.log(shape[-1]) + 1e-9).all() and (i64[ok] <= e64[ok] + 1e-9).all()
    differ = a32 != a64                  # the arg-max may only differ where the two largest means are a rounding apart
    top2 = np.sort(m64, -1)[..., -2:]
    assert (top2[differ, 1] - top2[differ, 0] < 1e-5).all()


def test_restatement_refuses_a_stack_without_samples():
    with pytest.raises(ValueError):
        _ref(np.zeros((2, 3, 4, 3), np.float32))


# ---- the library's host side -------------------------------------------------------------------------------------------
def test_workspace_bytes(hip):
    f = hip.lib().oct_mc_workspace_bytes
    assert f(32, 256, 512, 3) == 32 * 256 * 512 * 4 * 4
    assert f(1, 1, 1, 2) == 12 and f(3, 5, 7, 32) == 105 * 33 * 4
    for bad in ((0, 4, 4, 3), (1, 0, 4, 3), (1, 4, -1, 3), (1, 4, 4, 1), (1, 4, 4, 33), (2, 32768, 32768, 3)):
        assert f(*bad) == 0, bad


def _update(hip, probs=0x10000, B=2, H=4, W=8, n_cls=3, t=0, T=4, ws=0x20000, ws_bytes=None, out="default"):
    """``oct_mc_update`` over made-up addresses: every call here must return before it launches anything."""
    lib = hip.lib()
    if ws_bytes is None:
        ws_bytes = B * H * W * (n_cls + 1) * 4
    if out == "default":
        out = hip.McOut(0x40000, 0x50000, 0x60000, 0x70000)
    rc = lib.oct_mc_update(probs, B, H, W, n_cls, t, T, ws, ws_bytes, None if out is None else C.byref(out), None)
    return rc, lib.oct_last_error().decode()


@pytest.mark.parametrize("kw, msg", [
    (dict(probs=None), "null"), (dict(ws=None), "null"), (dict(t=3, out=None), "null out"),
    (dict(T=0), "T"), (dict(T=65, t=64), "T"), (dict(t=4), "t < T"), (dict(t=-1), "t < T"),
    (dict(n_cls=1), "n_cls"), (dict(n_cls=33), "n_cls"), (dict(B=0), "positive"), (dict(H=0), "positive"),
    (dict(B=2, H=32768, W=32768, ws_bytes=1 << 40), "2\\^31"),
    (dict(ws_bytes=2 * 4 * 8 * 4 * 4 - 1), "workspace too small"),
    (dict(ws=0x10000 + 2 * 4 * 8 * 3 * 4 - 4), "overlaps the input"),
    (dict(t=3, out=(0x10000 + 64, 0, 0, 0)), "overlaps"), (dict(t=3, out=(0, 0x20000 + 1023, 0, 0)), "overlaps"),
    (dict(t=3, out=(0, 0, 0x60000, 0x60000 + 252)), "two output ranges"), (dict(probs=0x10002), "aligned"),
])
def test_mc_update_argument_errors_return_before_any_launch(hip, kw, msg):
    import re
    if isinstance(kw.get("out"), tuple):
        kw = dict(kw, out=hip.McOut(*(v or None for v in kw["out"])))
    rc, err = _update(hip, **kw)
    assert rc < 0 and re.search(msg, err), (rc, err)


def test_forward_mc_refuses_a_null_handle_and_is_bound(hip):
    lib = hip.lib()
    out = hip.McOut(0x40000, 0x50000, 0x60000, 0x70000)
    d = hip.Infer(x_dev=0x1000, x_is_u8=1, B=1, kind=hip.INFER_MC, T=4, step0=0, probs_scratch_dev=0x2000, ws_dev=0x3000,
                  ws_bytes=1 << 20, out=out)
    assert lib.oct_unet_infer(None, C.byref(d), None) < 0
    assert "null" in lib.oct_last_error().decode()
    assert hip.MC_MAX_SAMPLES == 64


# ---- the public parameters ------------------------------------------------------------------------------------------
def _saved_model(tmp_path, H=16, W=16):
    from oct_image_segmentation_models_amd.models.engine_model import Model
    from oracle import unet_numpy as on
    cfg = dict(input_channels=1, num_classes=3, image_height=H, image_width=W, pool_layers=2)
    model = Model(name="unet", config=cfg)
    model.set_weights(on.keras_weight_list(*on.init_params(on.UNetConfig(num_classes=3, pool_layers=2), seed=3, dtype=np.float32)))
    model.save(tmp_path / "model.npz")
    with open(tmp_path / "model_config.json", "w") as fh:
        json.dump(cfg, fh)
    return tmp_path / "model.npz"


def _params(tmp_path, n=1, H=16, W=16, **kw):
    from oct_image_segmentation_models_amd.common.dataset import Dataset
    from oct_image_segmentation_models_amd.prediction.prediction_parameters import PredictionParams, PredictionSaveParams
    path = tmp_path / "model.npz" if (tmp_path / "model.npz").exists() else _saved_model(tmp_path, H, W)
    ds = Dataset(np.zeros((n, H, W, 1), np.uint8), [Path(f"scan_{i}") for i in range(n)], [tmp_path / "out" / f"image_{i}" for i in range(n)])
    return PredictionParams(path, None, None, ds, tmp_path / "p", PredictionSaveParams(), **kw)


def test_prediction_params_validate_mc_samples(hip, tmp_path):
    from oct_image_segmentation_models_amd.prediction.prediction_parameters import PredictionParams
    sig = inspect.signature(PredictionParams.__init__).parameters
    assert sig["mc_samples"].default == 0 and sig["mc_step0"].default == 0
    pp = _params(tmp_path)
    assert pp.mc_samples == 0 and pp.mc_step0 == 0
    pp = _params(tmp_path, mc_samples=64, mc_step0=5)
    assert pp.mc_samples == 64 and pp.mc_step0 == 5
    for bad in (-1, 65):
        with pytest.raises(ValueError, match="mc_samples"):
            _params(tmp_path, mc_samples=bad)


def test_pipeline_sources_take_mc_samples():
    from oct_image_segmentation_models_amd.evaluation.pipeline import Batch, BatchedPredictor, InferenceRun, host_batches
    from oct_image_segmentation_models_amd.models.engine_model import Model
    for fn in (InferenceRun.__init__, BatchedPredictor.__init__, host_batches, Model.predict_labels):
        sig = inspect.signature(fn).parameters
        assert sig["mc_samples"].default == 0 and sig["mc_step0"].default == 0
    plain = Batch(0, 1, np.zeros((1, 2, 2), np.uint8))
    assert plain.entropy is None and plain.mutual_info is None
    e, m = np.ones((1, 2, 2), np.float32), np.zeros((1, 2, 2), np.float32)
    both = plain.with_uncertainty(e, m)
    assert both.entropy is e and both.mutual_info is m and isinstance(both, Batch) and both == plain and both.maps is None
    assert plain.entropy is None and Batch(0, 1, plain.labels).entropy is None         # set on that one record alone
    assert list(inspect.signature(Model.predict_mc).parameters)[1:] == ["x", "samples", "batch_size", "step0"]
    with pytest.raises(ValueError, match="mc_samples"):
        BatchedPredictor(None, 2, mc_samples=65)


def test_entropy_quantisation_for_the_picture():
    from oct_image_segmentation_models_amd.common.utils import entropy_to_u8
    e = np.array([0.0, np.log(3) * 0.4, np.log(3), 2.0, 0.5 / 255 * np.log(3) * 0.999, 0.5 / 255 * np.log(3) * 1.001], np.float32)
    assert entropy_to_u8(e, 3).tolist() == [0, 102, 255, 255, 0, 1] and entropy_to_u8(e, 3).dtype == np.uint8


# ---- InferenceRun over injected batches -> predict's savers ---------------------------------------------------------------
def test_injected_uncertainty_maps_reach_the_prediction_files(hip, tmp_path):
    """No device is touched: the records come from a list, the savers are ``predict``'s own."""
    from oct_image_segmentation_models_amd.common import h5io
    from oct_image_segmentation_models_amd.evaluation.pipeline import Batch, InferenceRun
    from oct_image_segmentation_models_amd.prediction import prediction
    n, H, W, B, Cn = 3, 16, 16, 2, 3
    stack = softmax_stack((4, n, H, W, Cn), seed=3)
    _, am, ent, mi = _ref(stack)
    pp = _params(tmp_path, n=n, mc_samples=4, mc_step0=9)
    images = np.asarray(pp.dataset.images)
    maps = np.zeros((n, Cn - 1, H, W), np.uint8)
    batches = [Batch(lo, min(lo + B, n), am[lo:lo + B], maps[lo:lo + B]).with_uncertainty(ent[lo:lo + B], mi[lo:lo + B])
               for lo in range(0, n, B)]
    seen = 0
    with InferenceRun(None, images, B, Cn, batches=batches, mc_samples=pp.mc_samples, mc_step0=pp.mc_step0) as run:
        for b in run:
            assert b.entropy.shape == (b.hi - b.lo, H, W) and b.entropy.dtype == np.float32
            for i in range(b.lo, b.hi):
                out_dir = Path(pp.dataset.image_output_dirs[i]); out_dir.mkdir(parents=True)
                prediction.save_image_prediction_results(pp, images[i], pp.dataset.image_names[i], b.labels[i - b.lo].astype(np.int64),
                                                         np.zeros((Cn, H, W)), b.maps[i - b.lo], 0.0, 0.0, out_dir,
                                                         entropy=b.entropy[i - b.lo], mutual_info=b.mutual_info[i - b.lo])
                seen += 1
        with pytest.raises(RuntimeError, match="device"):
            run.render_gray(np.zeros((1, H, W), np.uint8))
    assert seen == n
    for i in range(n):
        f = h5io.load(Path(pp.dataset.image_output_dirs[i]) / "prediction_info.hdf5")
        assert f["predictive_entropy"].dtype == np.float32 and f["predictive_entropy"].shape == (H, W)
        assert np.array_equal(f["predictive_entropy"], ent[i]) and np.array_equal(f["mutual_information"], mi[i])
        assert int(f["attr:mc_samples"]) == 4 and np.array_equal(f["predicted_labels"], am[i])
    # without the maps the file is what it always was: no new dataset, no new attribute
    plain = tmp_path / "plain"; plain.mkdir()
    pp0 = _params(tmp_path, n=n)
    prediction.save_image_prediction_results(pp0, images[0], "a", am[0].astype(np.int64), np.zeros((Cn, H, W)), maps[0], 0.0, 0.0, plain)
    f = h5io.load(plain / "prediction_info.hdf5")
    assert sorted(k for k in f if not k.startswith("attr:")) == ["boundary_maps", "predicted_labels", "raw_image"]
    assert "attr:mc_samples" not in f
    # prediction_params.hdf5 records the two values only when set
    pp.config_output_dir.mkdir()
    prediction.save_predict_config_file(pp)
    cfg = h5io.load(pp.config_output_dir / "prediction_params.hdf5")
    assert int(cfg["attr:mc_samples"]) == 4 and int(cfg["attr:mc_step0"]) == 9
    pp0.config_output_dir = tmp_path / "p0"; pp0.config_output_dir.mkdir()
    prediction.save_predict_config_file(pp0)
    cfg0 = h5io.load(pp0.config_output_dir / "prediction_params.hdf5")
    assert "attr:mc_samples" not in cfg0 and "attr:mc_step0" not in cfg0
    out = prediction.PredictionOutput(images[0], "a", plain, am[0], None, maps[0], None)
    assert out.predictive_entropy is None and out.mutual_information is None
