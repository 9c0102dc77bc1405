"""CPU tests of the inference descriptor: ``oct_unet_infer`` and ``oct_unet_graph_capture_infer`` refuse a null handle, a null
descriptor and a kind outside the three, with the reason in ``oct_last_error()``, before anything is launched."""
import ctypes as C

import pytest

import __graft_entry__ as ge


@pytest.fixture(scope="module")
def hip():
    ge.build()
    from oct_image_segmentation_models_amd import _hip
    return _hip


@pytest.mark.parametrize("name", ["oct_unet_infer", "oct_unet_graph_capture_infer"])
def test_infer_refuses_null_arguments_and_an_unknown_kind(hip, name):
    call = getattr(hip.lib(), name)
    d = hip.Infer(x_dev=0x1000, x_is_u8=1, B=1, kind=hip.INFER_PLAIN, H=16, W=32, out=hip.McOut(0x2000, 0x3000, None, None))
    # the kind is looked at before the handle is: zeroed memory stands in for one
    handle = C.cast(C.create_string_buffer(1 << 16), C.c_void_p)
    for h, desc, msg in ((None, C.byref(d), "null"), (handle, None, "null")):
        hip.lib().oct_set_option(b"no_such_option", 0)              # leaves another message behind
        assert call(h, desc, None) < 0
        assert msg in hip.lib().oct_last_error().decode() and "infer" in hip.lib().oct_last_error().decode()
    assert (hip.INFER_PLAIN, hip.INFER_MC, hip.INFER_TTA) == (0, 1, 2)
    for kind in (-1, 3, 7):
        d.kind = kind
        assert call(handle, C.byref(d), None) < 0
        assert f"unknown kind {kind}" in hip.lib().oct_last_error().decode()

