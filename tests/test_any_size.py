"""CPU tests of "scans of any size": the numpy restatements ``pad_reference`` / ``crop_reference`` / ``padded_geometry``, the
geometry-independent parameter layout that lets one set of weights move between engines, the validation of ``pad_mode`` on
the public parameter classes, the model's geometry rule, and every argument error of ``oct_pad_batch`` / ``oct_crop_batch``
over made-up addresses: each must return before anything is launched."""
import ctypes as C
import inspect
import json
import re
from pathlib import Path

import numpy as np
import pytest

import __graft_entry__ as ge


@pytest.fixture(scope="module")
def hip():
    ge.build()
    from oct_image_segmentation_models_amd import _hip
    return _hip


def _utils():
    from oct_image_segmentation_models_amd.common import utils
    return utils


# ---- the restatements ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
@pytest.mark.parametrize("shape, out, at", [((2, 5, 7, 1), (8, 8), (1, 0)), ((1, 33, 70, 3), (36, 72), (1, 1)),
                                            ((3, 16, 32, 1), (16, 32), (0, 0)), ((1, 3, 3, 1), (4, 4), (0, 0)),
                                            ((1, 4, 6, 2), (8, 8), (3, 0))])
def test_pad_reference_equals_np_pad_and_crop_reference_inverts_it(dtype, shape, out, at):
    u = _utils()
    x = (np.random.default_rng(3).random(shape) * 255).astype(dtype)
    (Hp, Wp), (top, left) = out, at
    widths = ((0, 0), (top, Hp - top - shape[1]), (left, Wp - left - shape[2]), (0, 0))
    for mode, kw in (("edge", {}), ("reflect", {}), ("constant", {"constant_values": 7})):
        got = u.pad_reference(x, Hp, Wp, top, left, mode, 7)
        assert got.dtype == dtype and got.flags.c_contiguous and np.array_equal(got, np.pad(x, widths, mode=mode, **kw)), mode
        back = u.crop_reference(got, shape[1], shape[2], top, left)
        assert back.flags.c_contiguous and np.array_equal(back, x)


def test_pad_reference_takes_the_largest_legal_reflect_and_refuses_more():
    u = _utils()
    x = np.arange(2 * 19, dtype=np.uint8).reshape(1, 2, 19, 1)
    got = u.pad_reference(x, 4, 32, 1, 6, "reflect")              # top = 1 = H - 1
    assert np.array_equal(got, np.pad(x, ((0, 0), (1, 1), (6, 7), (0, 0)), mode="reflect"))
    with pytest.raises(ValueError, match="reflect"):
        u.pad_reference(x, 6, 32, 2, 6, "reflect")
    with pytest.raises(ValueError, match="mode"):
        u.pad_reference(x, 4, 32, 1, 6, "wrap")
    with pytest.raises(ValueError, match="fit"):
        u.pad_reference(x, 2, 19, 1, 0, "edge")
    with pytest.raises(ValueError, match="fit"):
        u.crop_reference(np.zeros((1, 4, 4)), 4, 4, 1, 0)
    t = np.arange(2 * 4 * 5 * 3).reshape(2, 4, 5, 3)
    assert np.array_equal(u.crop_reference(t, 2, 3, 1, 2), t[:, 1:3, 2:5]) and u.crop_reference(t[..., 0], 4, 5, 0, 0).shape == (2, 4, 5)


def test_padded_geometry_and_its_placement_rule():
    g = _utils().padded_geometry
    assert g(36, 68, 2) == (36, 68, 0, 0)
    assert g(37, 70, 2) == (40, 72, 1, 1)
    assert g(5, 7, 3) == (8, 8, 1, 0)              # the odd pixel goes to the bottom / right
    assert g(500, 760, 4) == (512, 768, 6, 4) and g(885, 512, 4) == (896, 512, 5, 0) and g(496, 1000, 4) == (496, 1008, 0, 4)
    assert g(7, 9, 0) == (7, 9, 0, 0)


# ---- one set of weights: the flat layout does not depend on H, W ----------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(start_neurons=8, pool_layers=2), dict(start_neurons=4, pool_layers=2, num_classes=5),
                                dict(start_neurons=8, pool_layers=3, conv_layers=3, input_channels=3)])
def test_parameter_layout_is_the_same_at_two_geometries(hip, kw):
    from oct_image_segmentation_models_amd.engine import layer_table, make_cfg
    kw = dict(dict(input_channels=1, num_classes=3), **kw)
    sizes = ((32, 64), (48, 80))
    a, b = (make_cfg(image_height=h, image_width=w, **kw) for h, w in sizes)
    lib = hip.lib()
    assert lib.oct_unet_param_count(C.byref(a)) == lib.oct_unet_param_count(C.byref(b)) > 0
    assert lib.oct_unet_state_count(C.byref(a)) == lib.oct_unet_state_count(C.byref(b)) > 0
    ta, tb = layer_table(a), layer_table(b)
    assert len(ta) == len(tb) > 0
    offsets = ("kernel_off", "bias_off", "gamma_off", "beta_off", "moving_mean_off", "moving_var_off")
    for la, lb in zip(ta, tb):
        assert all(la[k] == lb[k] for k in offsets + ("name", "kh", "kw", "cin", "cout", "has_bn")), la["name"]
    assert (ta[0]["out_h"], ta[0]["out_w"]) == sizes[0] and (tb[0]["out_h"], tb[0]["out_w"]) == sizes[1]


# ---- the public parameters ------------------------------------------------------------------------------------------------
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


def _prediction_params(tmp_path, **kw):
    from oct_image_segmentation_models_amd.common.dataset import Dataset
    from oct_image_segmentation_models_amd.prediction.prediction_parameters import PredictionParams, PredictionSaveParams
    path = tmp_path / "model.npz" if (tmp_path / "model.npz").exists() else _saved_model(tmp_path)
    ds = Dataset(np.zeros((1, 13, 18, 1), np.uint8), [Path("scan_0")], [tmp_path / "out" / "image_0"])
    return PredictionParams(path, None, None, ds, tmp_path / "p", PredictionSaveParams(), **kw)


def _evaluation_params(tmp_path, **kw):
    from oct_image_segmentation_models_amd.evaluation.evaluation_parameters import EvaluationParameters, EvaluationSaveParams
    path = tmp_path / "model.npz" if (tmp_path / "model.npz").exists() else _saved_model(tmp_path)
    return EvaluationParameters(path, None, None, tmp_path / "data.hdf5", tmp_path / "e", EvaluationSaveParams(), False,
                                ["dice_coef_macro"], **kw)


@pytest.mark.parametrize("make", [_prediction_params, _evaluation_params], ids=["PredictionParams", "EvaluationParameters"])
def test_parameter_classes_validate_pad_mode(hip, tmp_path, make):
    p = make(tmp_path)
    assert p.pad_mode is None and p.pad_value == 0
    for mode in ("edge", "reflect", "constant"):
        p = make(tmp_path, pad_mode=mode, pad_value=7)
        assert p.pad_mode == mode and p.pad_value == 7
    for bad in ("wrap", "Edge", "", 0, True):
        with pytest.raises(ValueError, match="pad_mode"):
            make(tmp_path, pad_mode=bad)
    for bad in ("x", None, float("nan")):
        with pytest.raises(ValueError, match="pad_value"):
            make(tmp_path, pad_mode="constant", pad_value=bad)


def test_pad_options_are_on_every_public_entry():
    from oct_image_segmentation_models_amd.evaluation.evaluation_parameters import EvaluationParameters
    from oct_image_segmentation_models_amd.evaluation.pipeline import BatchedPredictor, InferenceRun, host_batches
    from oct_image_segmentation_models_amd.models.engine_model import Model
    from oct_image_segmentation_models_amd.prediction.prediction_parameters import PredictionParams
    for fn in (PredictionParams.__init__, EvaluationParameters.__init__, InferenceRun.__init__, BatchedPredictor.__init__,
               host_batches, Model.predict, Model.predict_labels):
        sig = inspect.signature(fn).parameters
        assert sig["pad_mode"].default is None and sig["pad_value"].default == 0, fn
    assert inspect.signature(Model._ensure_engine).parameters["hw"].default is None
    assert list(inspect.signature(Model._ensure_engine).parameters)[1:3] == ["batch", "training"]
    m = Model("unet", dict(input_channels=1, num_classes=3, image_height=32, image_width=64, pool_layers=2))
    assert m.pad_mode is None and m.pad_value == 0            # predict_mc pads by these: its parameter list is fixed
    with pytest.raises(ValueError, match="pad_mode"):
        BatchedPredictor(None, 2, pad_mode="wrap")
    with pytest.raises(ValueError, match="pad_mode"):
        InferenceRun(None, np.zeros((0, 5, 7, 1), np.uint8), 2, 3, pad_mode="mirror")
    with pytest.raises(ValueError, match="pad_mode"):
        m.predict(np.zeros((1, 32, 64, 1), np.uint8), pad_mode="wrap")


def test_recorded_attributes_only_when_set(hip, tmp_path):
    from oct_image_segmentation_models_amd.common import h5io
    from oct_image_segmentation_models_amd.evaluation import evaluation
    from oct_image_segmentation_models_amd.prediction import prediction
    for k, kw in enumerate(({}, dict(pad_mode="constant", pad_value=7))):
        pp = _prediction_params(tmp_path, **kw)
        pp.config_output_dir = tmp_path / f"p{k}"; pp.config_output_dir.mkdir()
        prediction.save_predict_config_file(pp)
        f = h5io.load(pp.config_output_dir / "prediction_params.hdf5")
        ep = _evaluation_params(tmp_path, **kw)
        (tmp_path / "data.hdf5").write_bytes(b"x")
        ep.save_foldername = tmp_path / f"e{k}"; ep.save_foldername.mkdir()
        evaluation.save_eval_config_file(ep)
        g = h5io.load(ep.save_foldername / "eval_params.hdf5")
        for attrs in (f, g):
            if kw:
                assert bytes(attrs["attr:pad_mode"]).rstrip(b"\x00") == b"constant" and float(attrs["attr:pad_value"]) == 7.0
            else:
                assert "attr:pad_mode" not in attrs and "attr:pad_value" not in attrs
    assert sorted(f) == sorted(["attr:model_filename", "attr:error_col_inc_range", "attr:pad_mode", "attr:pad_value"])


# ---- the model's geometry rule (no engine is built) ---------------------------------------------------------------------------
def test_model_geometry_follows_the_data_and_names_what_it_refuses():
    from oct_image_segmentation_models_amd._hip import OctError
    from oct_image_segmentation_models_amd.models.engine_model import Model
    m = Model("unet", dict(input_channels=1, num_classes=3, image_height=32, image_width=64, pool_layers=2))
    assert m._geometry() == ((32, 64), None) and m._geometry((48, 80)) == ((48, 80), None)
    assert m._geometry((48, 80), "edge") == ((48, 80), None)              # a multiple is never padded
    assert m._geometry((37, 70), "reflect") == ((40, 72), (1, 1))
    with pytest.raises(OctError) as e:
        m._geometry((37, 70))
    assert "37x70" in str(e.value) and "multiple of 4" in str(e.value) and "pad_mode" in str(e.value)
    with pytest.raises(OctError, match="pad_mode"):
        m._ensure_engine(1, False, hw=(37, 70))                           # refused before any device is touched
    with pytest.raises(OctError, match="pad_mode"):
        m._ensure_engine(1, True, hw=(40, 70))
    m.release_engines()                                                   # nothing cached: a no-op
    assert m._engine is None and m._engines == {}


# ---- the library's host side: every argument error returns before a launch ---------------------------------------------------
def _pad(hip, src=0x10000, is_u8=1, B=2, H=5, W=7, ch=1, Hp=8, Wp=8, top=1, left=0, mode=0, value=0.0, dst=0x80000):
    lib = hip.lib()
    rc = lib.oct_pad_batch(src, is_u8, B, H, W, ch, Hp, Wp, top, left, mode, value, dst, None)
    return rc, lib.oct_last_error().decode()


def _crop(hip, src=0x10000, B=2, Hp=8, Wp=8, pixel_bytes=1, H=5, W=7, top=1, left=0, dst=0x80000):
    lib = hip.lib()
    rc = lib.oct_crop_batch(src, B, Hp, Wp, pixel_bytes, H, W, top, left, dst, None)
    return rc, lib.oct_last_error().decode()


@pytest.mark.parametrize("kw, msg", [
    (dict(src=None), "null"), (dict(dst=None), "null"),
    (dict(dst=0x10000 + 69), "overlaps"), (dict(src=0x80000 + 127), "overlaps"), (dict(dst=0x10000), "overlaps"),
    (dict(B=0), "positive"), (dict(H=0), "positive"), (dict(W=-1), "positive"), (dict(ch=0), "positive"),
    (dict(Hp=0), "positive"), (dict(Wp=0), "positive"),
    (dict(top=4), "does not fit"), (dict(left=2), "does not fit"), (dict(top=-1), "does not fit"), (dict(left=-1), "does not fit"),
    (dict(Hp=4, top=0), "does not fit"), (dict(top=2**31 - 1), "does not fit"),
    (dict(mode=1, H=2, Hp=8, top=2), "reflect"), (dict(mode=1, H=2, Hp=8, top=1), "reflect"),     # pad above, pad below >= H
    (dict(mode=1, W=2, Wp=8, left=2), "reflect"), (dict(mode=1, W=3, Wp=8, left=2), "reflect"),
    (dict(mode=1, H=1, Hp=2, top=0), "reflect"),
    (dict(mode=3), "unknown mode"), (dict(mode=-1), "unknown mode"),
    (dict(mode=2, value=7.5), "0\\.\\.255"), (dict(mode=2, value=256.0), "0\\.\\.255"), (dict(mode=2, value=-1.0), "0\\.\\.255"),
    (dict(is_u8=0, src=0x10002), "aligned"), (dict(is_u8=0, dst=0x80001), "aligned"),
    (dict(B=2**30 + 1), "overflow"), (dict(is_u8=0, ch=4, W=2**28, Wp=2**28, left=0), "overflow"),
    (dict(ch=2**30, is_u8=0), "overflow"),
    (dict(B=2**30, H=2**29, Hp=2**30, W=2**20, Wp=2**20 + 1, ch=2**9, top=0), "overflow"),
])
def test_pad_batch_argument_errors_return_before_any_launch(hip, kw, msg):
    rc, err = _pad(hip, **kw)
    assert rc < 0 and re.search(msg, err), (rc, err)


@pytest.mark.parametrize("kw, msg", [
    (dict(src=None), "null"), (dict(dst=None), "null"),
    (dict(dst=0x10000 + 127), "overlaps"), (dict(src=0x80000 + 69), "overlaps"),
    (dict(B=0), "positive"), (dict(H=0), "positive"), (dict(W=0), "positive"), (dict(Hp=-3), "positive"), (dict(Wp=0), "positive"),
    (dict(H=8), "does not fit"), (dict(left=2), "does not fit"), (dict(top=-1), "does not fit"), (dict(left=-2), "does not fit"),
    (dict(pixel_bytes=0), "pixel_bytes"), (dict(pixel_bytes=3), "pixel_bytes"), (dict(pixel_bytes=6), "pixel_bytes"),
    (dict(pixel_bytes=36), "pixel_bytes"), (dict(pixel_bytes=-4), "pixel_bytes"),
    (dict(B=2**30 + 1), "overflow"), (dict(pixel_bytes=32, W=2**25 + 1, Wp=2**25 + 1, left=0), "overflow"),
    (dict(B=2**30, Hp=2**30, H=2**30, top=0, Wp=2**24, W=2**24, pixel_bytes=32), "overflow"),
])
def test_crop_batch_argument_errors_return_before_any_launch(hip, kw, msg):
    rc, err = _crop(hip, **kw)
    assert rc < 0 and re.search(msg, err), (rc, err)


def test_pad_modes_are_bound_by_their_public_names(hip):
    assert hip.PAD_MODES == {"edge": 0, "reflect": 1, "constant": 2}
    lib = hip.lib()
    d = hip.Infer(x_dev=0x1000, x_is_u8=1, B=1, kind=hip.INFER_PLAIN, H=5, W=7, top=1, left=0, pad_mode=0, pad_value=0.0, x_pad_dev=0x2000)
    assert lib.oct_unet_graph_capture_infer(None, C.byref(d), None) < 0
    assert "null" in lib.oct_last_error().decode()
