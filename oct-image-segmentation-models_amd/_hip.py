"""ctypes binding of ``liboct_unet_hip.so`` (C ABI declared in ``include/oct_unet.h``).

The library is built in-tree by ``csrc/build.sh`` (``__graft_entry__.build()``).
Importing this module without the built library raises: the product path has
no fallback implementation.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("OCT_UNET_LIB") or os.path.join(_HERE, "liboct_unet_hip.so")     # (OCT_UNET_LIB: kernel experiments)


class OctError(RuntimeError):
    pass


class UNetCfg(C.Structure):
    _fields_ = [
        ("in_ch", C.c_int), ("n_cls", C.c_int), ("H", C.c_int), ("W", C.c_int), ("max_batch", C.c_int),
        ("start_neurons", C.c_int), ("pool_layers", C.c_int), ("conv_layers", C.c_int),
        ("enc_k", C.c_int), ("dec_k", C.c_int), ("dtype", C.c_int), ("training", C.c_int),
        ("bn_eps", C.c_float), ("bn_momentum", C.c_float), ("dropout_rate", C.c_float),
        ("bn_unbiased_moving_var", C.c_int), ("seed", C.c_ulonglong),
    ]


class LayerInfo(C.Structure):
    _fields_ = [
        ("name", C.c_char * 32),
        ("kh", C.c_int), ("kw", C.c_int), ("cin", C.c_int), ("cout", C.c_int), ("has_bn", C.c_int),
        ("out_h", C.c_int), ("out_w", C.c_int),
        ("kernel_off", C.c_size_t), ("bias_off", C.c_size_t), ("gamma_off", C.c_size_t), ("beta_off", C.c_size_t),
        ("moving_mean_off", C.c_size_t), ("moving_var_off", C.c_size_t),
    ]


class ProfileEntry(C.Structure):
    _fields_ = [("kernel", C.c_char * 80), ("layer", C.c_char * 32), ("launches", C.c_int),
                ("total_ms", C.c_double), ("flops", C.c_double), ("bytes", C.c_double)]


class OptDesc(C.Structure):
    _fields_ = [("kind", C.c_int), ("flags", C.c_int), ("clip_mode", C.c_int), ("clip", C.c_float), ("lr", C.c_float),
                ("beta1", C.c_float), ("beta2", C.c_float), ("rho", C.c_float), ("momentum", C.c_float), ("eps", C.c_float)]


# oct_opt_desc.kind / .flags / .clip_mode (include/oct_unet.h)
OPT_SGD, OPT_ADAM, OPT_ADAMAX, OPT_RMSPROP, OPT_ADAGRAD, OPT_ADADELTA = range(6)
OPT_NESTEROV, OPT_AMSGRAD, OPT_CENTERED = 1, 2, 4
CLIP_NONE, CLIP_VALUE, CLIP_NORM, CLIP_GLOBAL_NORM = range(4)


class RenderStyle(C.Structure):
    """``oct_render_style``: palette, line colours and styles of one ``oct_render_rgba`` call, passed by value."""
    _fields_ = [("n_cls", C.c_int), ("n_lines", C.c_int), ("col_lo", C.c_int), ("col_hi", C.c_int), ("half_width", C.c_int),
                ("palette", C.c_ubyte * 96), ("line_rgb", C.c_ubyte * 48), ("line_style", C.c_ubyte * 16)]


RENDER_BASE_IMAGE, RENDER_BASE_LABELS = 0, 1
RENDER_MAX_CLASSES, RENDER_MAX_LINES = 32, 16


class DiceShape(C.Structure):
    """``oct_dice_shape``: the shape of the Dice term for ``oct_unet_set_dice_shape``."""
    _fields_ = [("alpha", C.c_float), ("beta", C.c_float), ("gamma", C.c_float), ("weight_mode", C.c_int),
                ("class_weight_dev", C.c_void_p)]


DICE_WEIGHT_NONE, DICE_WEIGHT_CLASS, DICE_WEIGHT_VOLUME = range(3)


class ComponentRuleC(C.Structure):
    """``oct_component_rule``: what ``oct_component_filter`` removes and how it fills (``evaluation.components.ComponentRule``
    packs it)."""
    _fields_ = [("min_pixels", C.c_uint * 32), ("keep_largest", C.c_uint), ("fill_mode", C.c_int), ("fill_label", C.c_int)]


class ContrastDesc(C.Structure):
    """``oct_contrast_desc``: method, tile grid and clip limit / percentiles of one ``oct_contrast_batch`` call
    (``common.utils.contrast_desc`` packs a validated spec into it)."""
    _fields_ = [("method", C.c_int), ("tiles_y", C.c_int), ("tiles_x", C.c_int), ("clip_q8", C.c_uint), ("lo_bp", C.c_int),
                ("hi_bp", C.c_int)]


CONTRAST_CLAHE, CONTRAST_STRETCH = 0, 1


class UNetIO(C.Structure):
    _fields_ = [("probs", C.c_void_p), ("argmax", C.c_void_p), ("labels", C.c_void_p)]


class McOut(C.Structure):
    """``oct_mc_out``: the maps the last ``oct_mc_update`` of a sequence writes (device pointers, ``None`` = not wanted)."""
    _fields_ = [("mean_probs", C.c_void_p), ("argmax", C.c_void_p), ("entropy", C.c_void_p), ("mutual_info", C.c_void_p)]


class Infer(C.Structure):
    """``oct_infer``: one inference chain -- kind (plain, MC, TTA), padding, buffers -- for ``oct_unet_infer`` / ``oct_unet_graph_capture_infer``."""
    _fields_ = [("x_dev", C.c_void_p), ("x_is_u8", C.c_int), ("B", C.c_int), ("kind", C.c_int), ("T", C.c_int),
                ("step0", C.c_ulonglong), ("views", C.c_int * 4), ("x_view_dev", C.c_void_p), ("probs_scratch_dev", C.c_void_p),
                ("ws_dev", C.c_void_p), ("ws_bytes", C.c_size_t), ("H", C.c_int), ("W", C.c_int), ("top", C.c_int), ("left", C.c_int),
                ("pad_mode", C.c_int), ("pad_value", C.c_float), ("x_pad_dev", C.c_void_p), ("out", McOut), ("out_crop", McOut)]


INFER_PLAIN, INFER_MC, INFER_TTA = range(3)
MC_MAX_SAMPLES = 64

# oct_pad_batch modes (include/oct_unet.h), by the public pad_mode names
PAD_MODES = {"edge": 0, "reflect": 1, "constant": 2}


# every symbol include/oct_unet.h declares: (name, restype, argtypes)
_P = C.POINTER
SYMBOLS = [
    ("oct_unet_cfg_default", None, [_P(UNetCfg)]),
    ("oct_unet_cfg_check", C.c_int, [_P(UNetCfg)]),
    ("oct_unet_param_count", C.c_size_t, [_P(UNetCfg)]),
    ("oct_unet_state_count", C.c_size_t, [_P(UNetCfg)]),
    ("oct_unet_workspace_bytes", C.c_size_t, [_P(UNetCfg)]),
    ("oct_unet_layer_count", C.c_int, [_P(UNetCfg)]),
    ("oct_unet_layer_info", C.c_int, [_P(UNetCfg), C.c_int, _P(LayerInfo)]),
    ("oct_unet_create", C.c_int, [_P(UNetCfg), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                  _P(C.c_void_p)]),
    ("oct_unet_destroy", None, [C.c_void_p]),
    ("oct_unet_forward", C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, _P(UNetIO), C.c_void_p]),
    ("oct_unet_loss_dice", C.c_int, [C.c_void_p, C.c_float, C.c_void_p, C.c_void_p]),
    ("oct_unet_set_focal_dice", C.c_int, [C.c_void_p, C.c_float, C.c_float, C.c_void_p]),
    ("oct_unet_loss_focal_dice", C.c_int, [C.c_void_p, C.c_float, C.c_void_p, C.c_void_p]),
    ("oct_unet_set_bce_dice", C.c_int, [C.c_void_p, C.c_int]),
    ("oct_unet_loss_bce_dice", C.c_int, [C.c_void_p, C.c_float, C.c_void_p, C.c_void_p]),
    ("oct_unet_set_ignore_label", C.c_int, [C.c_void_p, C.c_int]),
    ("oct_unet_set_pixel_weights", C.c_int, [C.c_void_p, C.c_void_p]),
    ("oct_unet_set_dice_shape", C.c_int, [C.c_void_p, _P(DiceShape)]),
    ("oct_unet_backward", C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_void_p]),
    ("oct_unet_set_tail_event", C.c_int, [C.c_void_p, C.c_void_p]),
    ("oct_unet_grad_tail_offset", C.c_size_t, [_P(UNetCfg)]),
    ("oct_adam_step", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_float, C.c_float,
                                C.c_float, C.c_float, C.c_long, C.c_void_p]),
    ("oct_sgd_step", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_float, C.c_float, C.c_void_p]),
    ("oct_opt_slot_count", C.c_int, [_P(OptDesc)]),
    ("oct_opt_scratch_bytes", C.c_size_t, [C.c_size_t, C.c_size_t]),
    ("oct_opt_step", C.c_int, [_P(OptDesc), C.c_void_p, C.c_void_p, _P(C.c_void_p), C.c_size_t, C.c_long, C.c_void_p,
                               C.c_size_t, C.c_void_p, C.c_void_p]),
    ("oct_unet_set_dropout_step", C.c_int, [C.c_void_p, C.c_ulonglong]),
    ("oct_unet_dropout_mask", C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    ("oct_unet_infer", C.c_int, [C.c_void_p, _P(Infer), C.c_void_p]),
    ("oct_unet_graph_capture_infer", C.c_int, [C.c_void_p, _P(Infer), C.c_void_p]),
    ("oct_unet_graph_launch", C.c_int, [C.c_void_p, C.c_void_p]),
    ("oct_unet_profile_begin", C.c_int, [C.c_void_p]),
    ("oct_unet_profile_end", C.c_int, [C.c_void_p, C.c_void_p, C.c_int, _P(C.c_int)]),
    ("oct_boundary_maps", C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    ("oct_boundary_maps_soft", C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    ("oct_mc_workspace_bytes", C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int]),
    ("oct_mc_update", C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t,
                                _P(McOut), C.c_void_p]),
    ("oct_flip_batch", C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    ("oct_tta_update", C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t,
                                 _P(McOut), C.c_void_p]),
    ("oct_surface_workspace_bytes", C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int]),
    ("oct_surface_distances", C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double,
                                        C.c_double, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    ("oct_surface_distances_masked", C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double,
                                               C.c_double, C.c_double, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    ("oct_augment_batch", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_ulonglong,
                                    C.c_void_p, C.c_void_p, C.c_void_p]),
    ("oct_warp_batch", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                 C.c_void_p]),
    ("oct_elastic_batch", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                    C.c_void_p]),
    ("oct_edge_weight_map", C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("oct_contrast_workspace_bytes", C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int, _P(ContrastDesc)]),
    ("oct_contrast_batch", C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, _P(ContrastDesc), C.c_void_p, C.c_size_t,
                                     C.c_void_p, C.c_void_p]),
    ("oct_photo_batch", C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    ("oct_pad_batch", C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                C.c_float, C.c_void_p, C.c_void_p]),
    ("oct_crop_batch", C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                 C.c_void_p]),
    ("oct_minpath_workspace_bytes", C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    ("oct_minpath_device", C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t,
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("oct_confusion_counts", C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    ("oct_confusion_counts_masked", C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                              C.c_void_p]),
    ("oct_area_labels", C.c_int,[C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    ("oct_calibration_workspace_bytes", C.c_size_t, [C.c_int, C.c_size_t, C.c_int, C.c_int]),
    ("oct_calibration_counts", C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    ("oct_temperature_apply", C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_float, C.c_void_p]),
    ("oct_temperature_workspace_bytes", C.c_size_t, [C.c_int, C.c_size_t, C.c_int, C.c_int]),
    ("oct_temperature_nll", C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_size_t, C.c_int, C.c_int, _P(C.c_float), C.c_int,
                                      C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    ("oct_ordered_workspace_bytes", C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int]),
    ("oct_ordered_decode", C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_void_p]),
    ("oct_components_workspace_bytes", C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    ("oct_components", C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p,
                                 C.c_void_p, C.c_void_p, C.c_void_p]),
    ("oct_component_filter", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                       _P(ComponentRuleC), C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("oct_render_rgba", C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_void_p, _P(RenderStyle), C.c_int, C.c_int, C.c_int,
                                  C.c_void_p, C.c_void_p]),
    ("oct_set_option", C.c_int, [C.c_char_p, C.c_int]),
    ("oct_get_option", C.c_int, [C.c_char_p, _P(C.c_int)]),
    ("oct_unet_get_option", C.c_int, [C.c_void_p, C.c_char_p, _P(C.c_int)]),
    ("oct_unet_set_option", C.c_int, [C.c_void_p, C.c_char_p, C.c_int]),
    ("oct_unet_debug_activation", C.c_void_p, [C.c_void_p, C.c_int, C.c_int]),
    ("oct_unet_debug_layer_fused", C.c_int, [C.c_void_p, C.c_int]),
    ("oct_last_error", C.c_char_p, []),
    ("oct_version", C.c_char_p, []),
]

_lib = None


def source_stamp() -> str:
    """SHA-256 (12 hex digits) of csrc/*.hip, csrc/*.hpp and include/*.h in build.sh's order, or '' when the sources
    are not beside the package (an installed copy)."""
    import glob
    import hashlib
    here = os.path.dirname(os.path.abspath(__file__))
    csrc, inc = os.path.join(here, "csrc"), os.path.join(here, "..", "include")
    files = glob.glob(os.path.join(csrc, "*.hip")) + glob.glob(os.path.join(csrc, "*.hpp")) + glob.glob(os.path.join(inc, "*.h"))
    if not files:
        return ""
    # build.sh sorts the names as it lists them: '*.hip *.hpp ../../include/*.h' through `sort`
    rel = sorted((os.path.basename(f) if os.path.dirname(f) == csrc else "../../include/" + os.path.basename(f), f) for f in files)
    h = hashlib.sha256()
    for _, f in rel:
        with open(f, "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:12]


def lib() -> C.CDLL:
    """Load (once) and return the HIP library; raise loudly if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise OctError(
                f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(csrc/build.sh).  There is no fallback implementation.")
        # torch ships its own HIP runtime (libamdhip64): it must be in the process BEFORE this library is loaded, so
        # that both resolve to the same runtime instance (otherwise: "no ROCm-capable device is detected")
        import torch  # noqa: F401
        l = C.CDLL(LIB_PATH)
        for name, res, args in SYMBOLS:
            fn = getattr(l, name)  # AttributeError if the ABI is incomplete
            fn.restype = res
            fn.argtypes = args
        # a stale binary (built from other sources than the ones beside it) must not pass for this tree
        want, have = source_stamp(), l.oct_version().decode()
        if want and f"src:{want}" not in have and not os.environ.get("OCT_ALLOW_STALE_LIB"):
            raise OctError(f"{LIB_PATH} is stale: it reports '{have}' but the sources beside it hash to src:{want}; "
                           "rebuild with csrc/build.sh (OCT_ALLOW_STALE_LIB=1 overrides)")
        _lib = l
        # tuning knobs for experiments: OCT_OPTIONS="name=value,name=value" (oct_set_option; results do not depend on them)
        for kv in filter(None, os.environ.get("OCT_OPTIONS", "").split(",")):
            k, v = kv.split("=")
            if l.oct_set_option(k.strip().encode(), int(v)) != 0:
                raise OctError(f"OCT_OPTIONS: {l.oct_last_error().decode()}")
    return _lib


def set_option(name: str, value: int) -> None:
    check(lib().oct_set_option(name.encode(), int(value)), f"oct_set_option({name})")


def get_option(name: str) -> int:
    v = C.c_int(0)
    check(lib().oct_get_option(name.encode(), C.byref(v)), f"oct_get_option({name})")
    return int(v.value)


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        raise OctError(f"{what} failed (rc={rc}): {lib().oct_last_error().decode()}")


def stream_ptr(device) -> C.c_void_p:
    """The current HIP stream of ``device``, as the ABI's ``stream`` argument."""
    import torch
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def call(name: str, device, *args) -> None:
    """Call the library's ``name(*args)`` with ``device`` current; a non-zero return code raises ``OctError``."""
    import torch
    with torch.cuda.device(device):
        check(getattr(lib(), name)(*args), name)


def expect(t, what: str, *, device, dtype, shape=None, numel=None) -> None:
    """Raise ``OctError`` unless tensor ``t`` may be handed to a kernel as ``what``: on ``device`` (a ``torch.device``),
    of ``dtype`` (one, or a tuple of allowed ones), contiguous, and of ``shape`` -- a tuple in which ``None`` matches
    any extent -- and / or of ``numel`` elements, for the (B,H,W[,1]) arguments that are compared by size."""
    dtypes = dtype if isinstance(dtype, tuple) else (dtype,)
    ok = t.device == device and t.dtype in dtypes and t.is_contiguous() and (numel is None or t.numel() == numel)
    if ok and shape is not None:
        ok = t.dim() == len(shape) and all(e is None or e == s for e, s in zip(shape, t.shape))
    if not ok:
        want = f"{numel} elements" if shape is None else "shape (" + ",".join("n" if e is None else str(e) for e in shape) + ")"
        raise OctError(f"{what} must be a contiguous {' / '.join(map(str, dtypes))} tensor of {want} on {device}, not "
                       f"{'a' if t.is_contiguous() else 'a non-contiguous'} {t.dtype} {tuple(t.shape)} one on {t.device}")


def expect_map_pair(pred, gt, *, device, batch: int, H: int, W: int) -> int:
    """The two arguments of the kernels that compare class maps: uint8 (n,H,W) predictions and ground truth on ``device``
    with one count n in 1..batch, which is returned."""
    import torch
    expect(pred, "pred", device=device, dtype=torch.uint8, shape=(None, H, W))
    n = pred.shape[0]
    expect(gt, "gt", device=device, dtype=torch.uint8, shape=(n, H, W))
    if not 1 <= n <= batch:
        raise OctError(f"pred and gt need a count n in 1..{batch}, not {n}")
    return n


def out_view(out, own, n: int, what: str = "out"):
    """The output of a call over ``n`` images: ``own[:n]``, a view of the wrapper's buffer, unless the caller passes
    ``out``, which must then look exactly like that view."""
    view = own[:n]
    if out is None:
        return view
    expect(out, what, device=own.device, dtype=own.dtype, shape=tuple(view.shape))
    return out
