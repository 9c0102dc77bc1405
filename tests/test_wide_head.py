"""CPU tests of start_neurons 36 .. 64: the host plan accepts the widths, its counts and layer table agree with the oracle's
restatement of models/unet.py, the "head_wide" routing option exists, and the 28 channel-streaming head kernels
(kernels_head_wide.hpp) are in the build without scratch.  No compute calls."""
import ctypes as C
import glob
import os
import sys
import tempfile

import pytest

import __graft_entry__ as ge
from oracle import unet_numpy as on

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


@pytest.fixture(scope="module")
def hip():
    ge.build()
    from oct_image_segmentation_models_amd import _hip
    return _hip


@pytest.mark.parametrize("sn", list(range(36, 65, 4)))
def test_widths_above_32_are_planned(hip, sn):
    from oct_image_segmentation_models_amd.engine import make_cfg, layer_table
    lib = hip.lib()
    for C_, P in ((3, 4), (8, 1)):
        cfg = make_cfg(input_channels=1, num_classes=C_, image_height=64, image_width=128, start_neurons=sn, pool_layers=P,
                       max_batch=2, training=True)
        ocfg = on.UNetConfig(input_channels=1, num_classes=C_, start_neurons=sn, pool_layers=P, conv_layers=2)
        params, state = on.init_params(ocfg, seed=0)
        n_params = sum(v.size for p in params for v in p.values())
        n_state = sum(v.size for s in state for v in s.values())
        assert lib.oct_unet_param_count(C.byref(cfg)) == n_params == on.param_count(ocfg)[0]
        assert lib.oct_unet_state_count(C.byref(cfg)) == n_state == on.param_count(ocfg)[1]
        layers = layer_table(cfg)
        assert layers[-1]["cin"] == sn and layers[-1]["cout"] == C_
        assert [(l["cin"], l["cout"]) for l in layers] == [(p.cin, p.cout) for p in on.build_plan(ocfg)]
        assert lib.oct_unet_workspace_bytes(C.byref(cfg)) > 0
        cfg.training = 0
        assert lib.oct_unet_workspace_bytes(C.byref(cfg)) > 0


@pytest.mark.parametrize("sn", [68, 66, 128])
def test_widths_outside_the_range_are_rejected(hip, sn):
    from oct_image_segmentation_models_amd.engine import make_cfg
    from oct_image_segmentation_models_amd._hip import OctError
    with pytest.raises(OctError, match=r"4\.\.64"):
        make_cfg(input_channels=1, num_classes=3, image_height=64, image_width=128, start_neurons=sn)


def test_head_wide_option_round_trips(hip):
    assert hip.get_option("head_wide") == 0
    try:
        hip.set_option("head_wide", 1)
        assert hip.get_option("head_wide") == 1
    finally:
        hip.set_option("head_wide", 0)
    assert hip.get_option("head_wide") == 0


def test_wide_head_kernels_are_built_without_scratch():
    import kernel_resources as kr
    objs = sorted(glob.glob(os.path.join(ROOT, "oct-image-segmentation-models_amd", "csrc", "build", "*.o")))
    if not objs:
        pytest.skip("csrc/build/*.o not present (run __graft_entry__.build())")
    found, read_any = {}, False
    with tempfile.TemporaryDirectory() as tmp:
        for o in objs:
            co = kr.code_objects(o, tmp)
            if not co:
                continue
            for k in kr.kernels(co):
                read_any = True
                if "head_fwd_wide_k" in k["name"] or "head_bwd_wide_k" in k["name"]:
                    found[k["name"]] = k
    if not read_any:
        pytest.skip("no gfx950 code objects could be read from csrc/build/*.o (llvm tools missing?)")
    want = {f"head_{d}_wide_k<{c}, {at}>" for d in ("fwd", "bwd") for c in range(2, 9) for at in ("float", "unsigned short")}
    assert len(want) == 28
    missing = [w for w in sorted(want) if not any(w in n for n in found)]
    assert not missing and len(found) == 28, (missing, sorted(found))
    bad = {n: (k["spill"], k["scratch"]) for n, k in found.items()
           if k["spill"] not in ("0", 0) or k["scratch"] not in ("0", 0)}
    assert not bad, f"(vgpr_spill_count, scratch bytes) of the wide head kernels: {bad}"


def test_host_mirror_at_a_width_above_32(hip):
    """UNet(...).build_model(), summary(), count_params() and the Keras-H5 weight layout at start_neurons 40 / 64."""
    import numpy as np
    from oct_image_segmentation_models_amd.common import keras_h5
    from oct_image_segmentation_models_amd.models import get_model_class
    from tests.test_keras_h5 import FakeH5, weights_for
    for sn in (40, 64):
        cfg = dict(input_channels=1, num_classes=3, image_height=32, image_width=64, start_neurons=sn, pool_layers=2)
        unet = get_model_class("unet")(**cfg)
        assert unet.get_config()["start_neurons"] == sn
        model = unet.build_model()
        ocfg = on.UNetConfig(input_channels=1, num_classes=3, start_neurons=sn, pool_layers=2, conv_layers=2)
        assert model.count_params() == sum(on.param_count(ocfg))
        lines = []
        model.summary(print_fn=lines.append)
        head = next(l for l in lines if l.startswith("head"))
        assert head.split()[2:4] == [str(sn), "3"], head
        assert lines[-1] == f"Total params: {sum(on.param_count(ocfg))}"
        full = dict(cfg, conv_layers=2, enc_kernel=(3, 3), dec_kernel=(2, 2))
        assert [(s.kh, s.kw, s.cin, s.cout, s.has_bn) for s in on.build_plan(ocfg)] == keras_h5.conv_plan(full)
        w = weights_for(full)
        be = FakeH5()
        keras_h5.export_keras_h5("m.hdf5", w, full, h5=be)
        assert be.files["m.hdf5"]["model_weights"]["conv2d"]["conv2d"]["kernel:0"].data.shape == (3, 3, 1, sn)
        back = keras_h5.import_keras_h5("m.hdf5", full, h5=be)
        assert len(back) == len(w) and all(np.array_equal(a, b) for a, b in zip(back, w))
