"""CPU tests of test-time augmentation: the numpy restatements ``flip_reference`` / ``tta_reduce_reference``, ``parse_tta``,
the argument checks of the public parameter classes and of ``InferenceRun``, and the argument errors of the four new entry
points that return before any launch.  The device side is tests/test_gpu_tta.py."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

from tests.helpers import save_untrained_model
from tests.mc_cases import ENTROPY_TOL, softmax_stack


def _utils():
    from oct_image_segmentation_models_amd.common import utils as cu
    return cu


# ---- the numpy restatements ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("view", range(4))
@pytest.mark.parametrize("shape", [(3, 5, 7), (2, 4, 6, 3), (1, 1, 9, 2), (2, 8, 1)], ids=lambda s: "x".join(map(str, s)))
def test_flip_reference_is_np_flip(shape, view):
    a = np.random.default_rng(view + len(shape)).integers(0, 255, shape).astype(np.uint8)
    axes = tuple(ax for ax, bit in ((2, 1), (1, 2)) if view & bit)
    got = _utils().flip_reference(a, view)
    assert got.flags.c_contiguous and np.array_equal(got, np.flip(a, axes) if axes else a)
    assert np.array_equal(_utils().flip_reference(got, view), a)                # a flip is its own inverse


def test_flip_reference_refuses_bad_arguments():
    for a, v in ((np.zeros((2, 3)), 0), (np.zeros((1, 2, 3)), 4), (np.zeros((1, 2, 3)), -1)):
        with pytest.raises(ValueError, match="flip_reference"):
            _utils().flip_reference(a, v)


def _fp32_loop(stack, views):
    """The definition written out pixel source by pixel source: float32 sums in sample order, one product, the first maximum."""
    T, B, H, W, Cn = stack.shape
    S = np.zeros((B, H, W, Cn), np.float32)
    for t, v in enumerate(views):
        ys = np.arange(H)[::-1] if v & 2 else np.arange(H)
        xs = np.arange(W)[::-1] if v & 1 else np.arange(W)
        for y in range(H):
            for x in range(W):
                p = stack[t, :, ys[y], xs[x], :]
                S[:, y, x, :] = p if t == 0 else S[:, y, x, :] + p
    m = S * np.float32(np.float32(1.0) / np.float32(T))
    return m, m.argmax(-1).astype(np.uint8)                                      # np.argmax: the lowest index among equals


@pytest.mark.parametrize("shape,views", [((3, 1, 5, 7, 3), (0, 1, 2)), ((4, 2, 4, 8, 2), (3, 2, 1, 0)), ((1, 2, 3, 5, 4), (3,)),
                                         ((2, 1, 6, 4, 8), (2, 1))], ids=lambda s: "x".join(map(str, s)))
def test_tta_reduce_reference(shape, views):
    cu = _utils()
    stack = softmax_stack(shape, seed=sum(shape))
    m, a, e, mi = cu.tta_reduce_reference(stack, views)
    m_ref, a_ref = _fp32_loop(stack, views)
    assert m.dtype == np.float32 and np.array_equal(m.view(np.uint32), m_ref.view(np.uint32)) and np.array_equal(a, a_ref)
    # entropy and mutual information against an fp64 mean over the un-flipped stack
    un = np.stack([cu.flip_reference(stack[t], v) for t, v in enumerate(views)]).astype(np.float64)
    mean64 = un.mean(0)

    def ent(p):
        return -np.where(p > 0, p * np.log(np.where(p > 0, p, 1.0)), 0.0).sum(-1)
    e64 = ent(mean64)
    i64 = np.maximum(e64 - ent(un).mean(0), 0.0)
    assert np.abs(e - e64).max() <= ENTROPY_TOL and np.abs(mi - i64).max() <= ENTROPY_TOL
    # it IS mc_reduce_reference of the un-flipped stack
    for got, want in zip((m, a, e, mi), cu.mc_reduce_reference(un.astype(np.float32))):
        assert got.tobytes() == want.tobytes()
    if all(v == 0 for v in views):
        return
    assert not np.array_equal(m, cu.mc_reduce_reference(stack)[0])              # and the views matter


def test_tta_reduce_reference_refuses_bad_arguments():
    cu = _utils()
    p = softmax_stack((2, 1, 3, 4, 3), seed=1)
    for stack, views in ((p, (0,)), (p, (0, 1, 2)), (p[0], (0,)), (np.concatenate([p, p, p]), (0, 1, 2, 3, 0, 1)), (p, (0, 4))):
        with pytest.raises(ValueError):
            cu.tta_reduce_reference(stack, views)


# ---- parse_tta ----------------------------------------------------------------------------------------------------------
def test_parse_tta():
    cu = _utils()
    assert cu.TTA_VIEWS == {"identity": 0, "flip_lr": 1, "flip_ud": 2, "flip_both": 3}
    assert cu.parse_tta(None) == () and cu.parse_tta(()) == () and cu.parse_tta([]) == ()
    assert cu.parse_tta(("identity", "flip_lr")) == (0, 1)
    assert cu.parse_tta(["flip_both", "flip_ud", "flip_lr", "identity"]) == (3, 2, 1, 0)
    with pytest.raises(ValueError, match="'rot90'"):
        cu.parse_tta(("identity", "rot90"))
    with pytest.raises(ValueError, match="'flip_lr' is given twice"):
        cu.parse_tta(("flip_lr", "identity", "flip_lr"))
    with pytest.raises(ValueError, match="at most 4 views, not the 5"):
        cu.parse_tta(("identity", "flip_lr", "flip_ud", "flip_both", "identity"))
    for bad in ("flip_lr", 1, {"flip_lr"}, (1,), (None,)):
        with pytest.raises(ValueError, match="tta"):
            cu.parse_tta(bad)
    with pytest.raises(ValueError, match="mc_samples=2"):
        cu.check_tta(("flip_lr",), 2)
    assert cu.check_tta(None, 2) == () and cu.check_tta(["flip_ud"]) == ("flip_ud",)


# ---- the public parameter objects -----------------------------------------------------------------------------------------
H_, W_, CC, SN, P_ = 16, 32, 3, 8, 2


def _prediction_params(tmp_path, **kw):
    from oct_image_segmentation_models_amd.common.dataset import Dataset
    from oct_image_segmentation_models_amd.prediction.prediction_parameters import PredictionParams, PredictionSaveParams
    images = np.zeros((2, H_, W_, 1), np.uint8)
    ds = Dataset(images, [Path("a.tiff"), Path("b.tiff")], [tmp_path / "out" / f"image_{i}" for i in range(2)])
    return PredictionParams(model_path=tmp_path / "model" / "model.npz", mlflow_tracking_uri=None, mlflow_run_uuid=None, dataset=ds,
                            config_output_dir=tmp_path / "out", save_params=PredictionSaveParams(), **kw)


def _evaluation_params(tmp_path, **kw):
    from oct_image_segmentation_models_amd.evaluation.evaluation_parameters import EvaluationParameters, EvaluationSaveParams
    return EvaluationParameters(model_path=tmp_path / "model" / "model.npz", mlflow_tracking_uri=None, mlflow_run_uuid=None,
                                test_dataset_path=tmp_path / "none.hdf5", save_foldername=tmp_path / "eval",
                                save_params=EvaluationSaveParams(), graph_search=False, metrics=[], **kw)


def _public(obj):
    return {k: v for k, v in vars(obj).items() if k not in ("tta", "loaded_model", "dataset", "save_params")}


@pytest.mark.parametrize("make", [_prediction_params, _evaluation_params], ids=["PredictionParams", "EvaluationParameters"])
def test_parameter_objects_take_tta(tmp_path, make):
    save_untrained_model(tmp_path, H_, W_, CC, SN, P_)
    plain = make(tmp_path)
    assert plain.tta == ()
    on = make(tmp_path, tta=["identity", "flip_lr"])
    assert on.tta == ("identity", "flip_lr")
    assert make(tmp_path, tta=()).tta == ()
    # nothing else moves
    a, b = _public(plain), _public(on)
    assert a.keys() == b.keys()
    for k in a:
        assert repr(a[k]) == repr(b[k]), k
    for bad, match in ((("identity", "mirror"), "'mirror'"), (("flip_ud", "flip_ud"), "twice"), ("flip_lr", "sequence")):
        with pytest.raises(ValueError, match=match):
            make(tmp_path, tta=bad)


def test_prediction_params_refuse_tta_with_mc_samples(tmp_path):
    save_untrained_model(tmp_path, H_, W_, CC, SN, P_)
    with pytest.raises(ValueError, match="mc_samples=3"):
        _prediction_params(tmp_path, tta=("flip_lr",), mc_samples=3)
    assert _prediction_params(tmp_path, mc_samples=3).tta == ()


def test_inference_run_checks_tta_before_anything_is_built():
    from oct_image_segmentation_models_amd.evaluation.pipeline import Batch, InferenceRun
    images = np.zeros((2, H_, W_, 1), np.uint8)
    for kw, match in ((dict(tta=("flip_lr", "spin")), "'spin'"), (dict(tta=("flip_lr",), mc_samples=2), "mc_samples=2"),
                      (dict(tta=("identity",) * 2), "twice")):
        with pytest.raises(ValueError, match=match):
            InferenceRun(None, images, 2, CC, **kw)              # model None: nothing of it may be touched
    rec = Batch(0, 2, np.zeros((2, H_, W_), np.uint8))
    with InferenceRun(None, images, 2, CC, batches=[rec], tta=("identity", "flip_ud")) as run:
        assert run.tta == ("identity", "flip_ud") and list(run) == [rec]
    with InferenceRun(None, images, 2, CC, batches=[rec]) as run:
        assert run.tta == ()


# ---- the C ABI: errors that return before any launch -------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hip():
    from oct_image_segmentation_models_amd import _hip
    return _hip, _hip.lib()


def test_flip_batch_argument_errors(hip):
    """Over made-up addresses: every call here must return before it launches anything."""
    _, lib = hip
    src, dst = 0x10000, 0x90000

    def call(src=src, B=2, H=8, W=16, pb=4, view=1, dst=dst):
        return lib.oct_flip_batch(src, B, H, W, pb, view, dst, None), lib.oct_last_error().decode()

    for kw, msg in ((dict(src=None), "null"), (dict(dst=None), "null"), (dict(B=0), "positive"), (dict(H=0), "positive"),
                    (dict(W=-1), "positive"), (dict(pb=0), "pixel_bytes"), (dict(pb=3), "pixel_bytes"), (dict(pb=6), "pixel_bytes"),
                    (dict(pb=36), "pixel_bytes"), (dict(view=4), "view"), (dict(view=-1), "view"),
                    (dict(dst=src), "overlaps"), (dict(dst=src + 2 * 8 * 16 * 4 - 1), "overlaps"), (dict(src=dst + 1), "overlaps"),
                    (dict(W=(1 << 30) // 4 + 1), "overflow"), (dict(B=(1 << 30) + 1, H=1, W=1, pb=1), "overflow")):
        rc, err = call(**kw)
        assert rc < 0 and "flip_batch" in err and msg in err, (kw, rc, err)


def test_tta_update_argument_errors(hip):
    _hip, lib = hip
    B, H, W, Cn = 2, 8, 16, 3
    need = lib.oct_mc_workspace_bytes(B, H, W, Cn)
    probs, ws, o = 0x100000, 0x200000, 0x400000
    out = _hip.McOut(o, o + 0x10000, o + 0x20000, o + 0x30000)

    def call(probs=probs, Cn=Cn, view=1, t=1, T=2, ws=ws, ws_bytes=need, out=out):
        rc = lib.oct_tta_update(probs, B, H, W, Cn, view, t, T, ws, ws_bytes, None if out is None else C.byref(out), None)
        return rc, lib.oct_last_error().decode()

    for kw, msg in ((dict(view=4), "view"), (dict(view=-1), "view"), (dict(T=5, t=4), "T <= 4"), (dict(T=0, t=0), "1 <= T"),
                    (dict(probs=None), "null"), (dict(ws=None), "null"), (dict(out=None), "null out"), (dict(Cn=1), "n_cls"),
                    (dict(Cn=33), "n_cls"), (dict(t=2), "t < T"), (dict(t=-1), "t < T"), (dict(ws_bytes=need - 1), "workspace too small"),
                    (dict(probs=probs + 2), "aligned"), (dict(ws=probs + 16), "overlaps"),
                    (dict(out=_hip.McOut(probs, None, None, None)), "overlaps"), (dict(out=_hip.McOut(o, None, o + 4, None)), "overlap")):
        rc, err = call(**kw)
        assert rc < 0 and err.startswith("tta_update") and msg in err, (kw, rc, err)


def test_engine_calls_refuse_a_null_handle_and_are_bound(hip):
    _hip, lib = hip
    d = _hip.Infer(x_dev=0x1000, x_is_u8=1, B=1, kind=_hip.INFER_TTA, T=2, views=(C.c_int * 4)(0, 1), x_view_dev=0x2000,
                   probs_scratch_dev=0x3000, ws_dev=0x4000, ws_bytes=1 << 20, H=16, W=32, out=_hip.McOut(None, 0x5000, None, None))
    assert lib.oct_unet_infer(None, C.byref(d), None) < 0
    assert "null" in lib.oct_last_error().decode()
    assert lib.oct_unet_graph_capture_infer(None, C.byref(d), None) < 0
    assert "null" in lib.oct_last_error().decode()
    names = [s[0] for s in _hip.SYMBOLS]
    assert all(n in names for n in ("oct_flip_batch", "oct_tta_update", "oct_unet_infer", "oct_unet_graph_capture_infer"))
