"""CPU tests of num_classes 9 .. 16: the host plan accepts the class counts behind ``max_classes``, its counts and layer table
agree with the oracle's, the workspace of the class counts up to 8 has not moved by a byte, the 32 class-streaming head
kernels (kernels_head_cls.hpp) are in the build without scratch, the host mirror carries 10 and 16 classes, and PNG pictures
are refused above 9 classes before anything runs.  No compute calls."""
import ctypes as C
import glob
import json
import os
import sys
import tempfile
from pathlib import Path

import numpy as np
import pytest

import __graft_entry__ as ge
from oracle import unet_numpy as on

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

# oct_unet_workspace_bytes(256 x 512, max_batch 32, start_neurons 8, pool_layers 4) of the commit before the class-streaming
# head: (num_classes, training) -> bytes
WORKSPACE_BEFORE = {(3, True): 3059258624, (3, False): 1353553664, (8, True): 3059632896, (8, False): 1353553664}


@pytest.fixture(scope="module")
def hip():
    ge.build()
    from oct_image_segmentation_models_amd import _hip
    return _hip


@pytest.mark.parametrize("sn", [8, 64])
@pytest.mark.parametrize("C_", list(range(9, 17)))
def test_class_counts_above_8_are_planned(hip, C_, sn):
    from oct_image_segmentation_models_amd.engine import make_cfg, layer_table
    lib = hip.lib()
    P = 2
    cfg = make_cfg(input_channels=1, num_classes=C_, image_height=64, image_width=128, start_neurons=sn, pool_layers=P,
                   max_batch=2, training=True, max_classes=16)
    ocfg = on.UNetConfig(input_channels=1, num_classes=C_, start_neurons=sn, pool_layers=P, conv_layers=2)
    assert lib.oct_unet_param_count(C.byref(cfg)) == on.param_count(ocfg)[0]
    assert lib.oct_unet_state_count(C.byref(cfg)) == on.param_count(ocfg)[1]
    layers = layer_table(cfg)
    assert layers[-1]["cin"] == sn and layers[-1]["cout"] == C_
    assert [(l["cin"], l["cout"]) for l in layers] == [(p.cin, p.cout) for p in on.build_plan(ocfg)]
    assert lib.oct_unet_workspace_bytes(C.byref(cfg)) > 0
    cfg.training = 0
    assert lib.oct_unet_workspace_bytes(C.byref(cfg)) > 0


def test_limits_of_num_classes_and_max_classes(hip):
    from oct_image_segmentation_models_amd.engine import make_cfg
    from oct_image_segmentation_models_amd._hip import OctError
    base = dict(input_channels=1, image_height=64, image_width=128, pool_layers=2)
    with pytest.raises(OctError, match="max_classes"):
        make_cfg(num_classes=17, max_classes=16, **base)
    with pytest.raises(OctError, match=r"2\.\.16"):
        make_cfg(num_classes=1, max_classes=16, **base)
    with pytest.raises(OctError, match=r"8\.\.16"):
        make_cfg(num_classes=3, max_classes=17, **base)
    with pytest.raises(OctError, match=r"8\.\.16"):
        make_cfg(num_classes=3, max_classes=7, **base)
    with pytest.raises(OctError, match="max_classes"):          # the default stays at 8
        make_cfg(num_classes=9, **base)
    with pytest.raises(OctError, match="max_classes"):
        make_cfg(num_classes=13, max_classes=12, **base)
    assert make_cfg(num_classes=8, **base).n_cls == 8
    assert make_cfg(num_classes=12, max_classes=12, **base).n_cls == 12
    # the library itself refuses 17, whatever the binding lets through
    cfg = make_cfg(num_classes=16, max_classes=16, **base)
    cfg.n_cls = 17
    assert hip.lib().oct_unet_cfg_check(C.byref(cfg)) != 0
    assert "2..16" in hip.lib().oct_last_error().decode()


def test_probability_maps_stay_inside_32_bit_indexing(hip):
    """start_neurons 4 leaves max_batch * H * W < 2^28; with 16 classes the (B,H,W,C) maps would pass 2^31 elements."""
    from oct_image_segmentation_models_amd.engine import make_cfg
    from oct_image_segmentation_models_amd._hip import OctError
    base = dict(input_channels=1, image_height=1024, image_width=1024, start_neurons=4, pool_layers=2, max_classes=16)
    assert make_cfg(num_classes=8, max_batch=255, **base).max_batch == 255        # 255 * 2^20 * 8 < 2^31
    assert make_cfg(num_classes=16, max_batch=127, **base).max_batch == 127
    with pytest.raises(OctError, match=r"n_cls must stay below 2\^31"):
        make_cfg(num_classes=16, max_batch=128, **base)


@pytest.mark.parametrize("key", sorted(WORKSPACE_BEFORE))
def test_workspace_up_to_8_classes_has_not_moved(hip, key):
    from oct_image_segmentation_models_amd.engine import make_cfg
    n_cls, training = key
    cfg = make_cfg(input_channels=1, num_classes=n_cls, image_height=256, image_width=512, max_batch=32, training=training)
    assert hip.lib().oct_unet_workspace_bytes(C.byref(cfg)) == WORKSPACE_BEFORE[key]


def test_class_streaming_head_kernels_are_built_without_scratch():
    import kernel_resources as kr
    objs = sorted(glob.glob(os.path.join(ROOT, "oct-image-segmentation-models_amd", "csrc", "build", "*.o")))
    if not objs:
        pytest.skip("csrc/build/*.o not present (run __graft_entry__.build())")
    cls, wide, read_any = {}, set(), False
    with tempfile.TemporaryDirectory() as tmp:
        for o in objs:
            co = kr.code_objects(o, tmp)
            if not co:
                continue
            for k in kr.kernels(co):
                read_any = True
                if "head_fwd_cls_k" in k["name"] or "head_bwd_cls_k" in k["name"]:
                    cls[k["name"]] = k
                if "head_fwd_wide_k" in k["name"] or "head_bwd_wide_k" in k["name"]:
                    wide.add(k["name"])
    if not read_any:
        pytest.skip("no gfx950 code objects could be read from csrc/build/*.o (llvm tools missing?)")
    want = {f"head_{d}_cls_k<{c}, {at}>" for d in ("fwd", "bwd") for c in range(9, 17) for at in ("float", "unsigned short")}
    assert len(want) == 32
    missing = [w for w in sorted(want) if not any(w in n for n in cls)]
    assert not missing and len(cls) == 32, (missing, sorted(cls))
    bad = {n: (k["spill"], k["scratch"]) for n, k in cls.items()
           if k["spill"] not in ("0", 0) or k["scratch"] not in ("0", 0)}
    assert not bad, f"(vgpr_spill_count, scratch bytes) of the class-streaming head kernels: {bad}"
    assert len(wide) == 28, sorted(wide)                        # the channel-streaming family has not grown


@pytest.mark.parametrize("n_cls", [10, 16])
def test_host_mirror_at_10_and_16_classes(hip, n_cls):
    """UNet(...).build_model(), summary(), count_params() and the Keras-H5 weight layout."""
    from oct_image_segmentation_models_amd.common import keras_h5
    from oct_image_segmentation_models_amd.models import get_model_class
    from tests.test_keras_h5 import FakeH5, weights_for
    cfg = dict(input_channels=1, num_classes=n_cls, image_height=32, image_width=64, start_neurons=8, pool_layers=2)
    unet = get_model_class("unet")(**cfg)
    assert unet.get_config()["num_classes"] == n_cls
    model = unet.build_model()
    assert model.output.shape[-1] == n_cls
    ocfg = on.UNetConfig(input_channels=1, num_classes=n_cls, start_neurons=8, pool_layers=2, conv_layers=2)
    assert model.count_params() == sum(on.param_count(ocfg))
    lines = []
    model.summary(print_fn=lines.append)
    head = next(l for l in lines if l.startswith("head"))
    assert head.split()[2:4] == ["8", str(n_cls)], head
    assert lines[-1] == f"Total params: {sum(on.param_count(ocfg))}"
    full = dict(cfg, conv_layers=2, enc_kernel=(3, 3), dec_kernel=(2, 2))
    assert [(s.kh, s.kw, s.cin, s.cout, s.has_bn) for s in on.build_plan(ocfg)] == keras_h5.conv_plan(full)
    w = weights_for(full)
    assert w[-2].shape == (1, 1, 8, n_cls) and w[-1].shape == (n_cls,)
    be = FakeH5()
    keras_h5.export_keras_h5("m.hdf5", w, full, h5=be)
    back = keras_h5.import_keras_h5("m.hdf5", full, h5=be)
    assert len(back) == len(w) and all(np.array_equal(a, b) for a, b in zip(back, w))


def test_png_plots_are_refused_above_9_classes(hip, tmp_path):
    """The renderer holds 16 lines and the overlay draws 2 (C - 1): both parameter objects refuse png_plots=True with 10
    classes when they are built -- nothing has run -- and name the limit; 9 classes pass, and so does png_plots=False."""
    from oct_image_segmentation_models_amd.common import plotting
    from oct_image_segmentation_models_amd.common.dataset import Dataset
    from oct_image_segmentation_models_amd.evaluation.evaluation_parameters import EvaluationParameters, EvaluationSaveParams
    from oct_image_segmentation_models_amd.models.engine_model import Model
    from oct_image_segmentation_models_amd.prediction.prediction_parameters import PredictionParams, PredictionSaveParams
    assert plotting.PNG_MAX_CLASSES == 9 and 2 * (plotting.PNG_MAX_CLASSES - 1) == plotting.MAX_LINES
    ds = Dataset(np.zeros((1, 16, 16, 1), np.uint8), [Path("a")], [tmp_path / "out"])

    def params(n_cls, png):
        d = tmp_path / f"m{n_cls}"
        if not d.exists():
            d.mkdir()
            cfg = dict(input_channels=1, num_classes=n_cls, image_height=16, image_width=16, pool_layers=2)
            model = Model(name="unet", config=cfg)
            model.set_weights(on.keras_weight_list(*on.init_params(on.UNetConfig(num_classes=n_cls, pool_layers=2), seed=3,
                                                                   dtype=np.float32)))
            model.save(d / "model.npz")
            with open(d / "model_config.json", "w") as fh:
                json.dump(cfg, fh)
        ep = EvaluationParameters(d / "model.npz", None, None, tmp_path / "d.hdf5", tmp_path / "e", EvaluationSaveParams(), True,
                                  [], png_plots=png)
        pp = PredictionParams(d / "model.npz", None, None, ds, tmp_path / "p", PredictionSaveParams(), png_plots=png)
        return ep, pp

    for n_cls in (9, 10):
        ep, pp = params(n_cls, False)
        assert ep.num_classes == pp.num_classes == n_cls and ep.png_plots is False and pp.png_plots is False
    ep, pp = params(9, True)
    assert ep.png_plots is True and pp.png_plots is True
    for build in (lambda: params(10, True)[0], lambda: PredictionParams(tmp_path / "m10" / "model.npz", None, None, ds,
                                                                       tmp_path / "p", PredictionSaveParams(), png_plots=True)):
        with pytest.raises(ValueError, match=r"num_classes <= 9.*16"):
            build()
