"""``UNetEngine``: Python owner of one ``oct_unet`` handle (one per GPU rank).

PyTorch-ROCm is used for plumbing only -- device allocations, the current HIP
stream, and (in ``parallel.py``) ``torch.distributed``/RCCL on the flat gradient
tensor.  All arithmetic of the hot path happens inside ``liboct_unet_hip.so``.

Replaces, for the ``"unet"`` architecture, what the reference obtains from
``tf.keras.Model`` (reference call sites: training/training.py:243-266,401-407;
evaluation/evaluation.py:129-135; prediction/prediction.py:75-81).
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import _hip
from ._hip import OctError, UNetCfg, UNetIO, LayerInfo


def _ptr(t: Optional[torch.Tensor]): return None if t is None else t.data_ptr()


def _view_code(view) -> int:
    """A view of ``common.utils.TTA_VIEWS`` by name, or its code 0..3 as it is (the library checks the range)."""
    from .common.utils import TTA_VIEWS
    if isinstance(view, str):
        if view not in TTA_VIEWS:
            raise OctError(f"unknown view {view!r} (the views are {tuple(TTA_VIEWS)})")
        return TTA_VIEWS[view]
    return int(view)


def _require_gpu(device) -> torch.device:
    dev = torch.device(device)
    if dev.type != "cuda" or not torch.cuda.is_available():
        raise OctError("the OCT U-Net engine needs an AMD GPU (torch.cuda.is_available() is False); "
                       "there is no CPU fallback")
    return dev


def make_cfg(*, input_channels: int, num_classes: int, image_height: int, image_width: int,
             start_neurons: int = 8, pool_layers: int = 4, conv_layers: int = 2,
             enc_kernel: Sequence[int] = (3, 3), dec_kernel: Sequence[int] = (2, 2),
             max_batch: int = 1, training: bool = False, seed: int = 0,
             bn_eps: float = 1e-3, bn_momentum: float = 0.99, dropout_rate: float = 0.5,
             bn_unbiased_moving_var: bool = True, dtype="float32", max_classes: int = 8) -> UNetCfg:
    """The checked configuration of an engine.

    ``max_classes`` (8..16) is the largest ``num_classes`` this call accepts.  The library takes 2..16; the default here
    stays at 8, the limit of the register and channel-streaming head kernels, so that a caller written against that limit
    (and the test that pins ``num_classes=9`` as an error) meets it unchanged.  9..16 classes run the class-streaming head
    kernels; ``Model`` always passes ``max_classes=16``, so the model classes, ``train_model``, ``evaluate_model`` and
    ``predict`` need no opt-in."""
    if not 8 <= int(max_classes) <= 16:
        raise OctError(f"max_classes must be in 8..16, got {max_classes}")
    if num_classes > max_classes:
        raise OctError(f"num_classes {num_classes} exceeds max_classes {max_classes} (pass max_classes up to 16)")
    ek, dk = tuple(enc_kernel), tuple(dec_kernel)
    if ek[0] != ek[1] or dk[0] != dk[1]:
        raise OctError("only square kernels are supported")
    cfg = UNetCfg()
    _hip.lib().oct_unet_cfg_default(C.byref(cfg))
    cfg.in_ch, cfg.n_cls, cfg.H, cfg.W = input_channels, num_classes, image_height, image_width
    cfg.max_batch, cfg.start_neurons, cfg.pool_layers, cfg.conv_layers = max_batch, start_neurons, pool_layers, conv_layers
    dmap = {"float32": 0, "f32": 0, 0: 0, "bfloat16": 1, "bf16": 1, 1: 1}
    if dtype not in dmap:
        raise OctError(f"dtype must be 'float32' or 'bfloat16' (activation storage), got {dtype!r}")
    cfg.enc_k, cfg.dec_k, cfg.dtype, cfg.training = ek[0], dk[0], dmap[dtype], int(training)
    cfg.bn_eps, cfg.bn_momentum, cfg.dropout_rate = bn_eps, bn_momentum, dropout_rate
    cfg.bn_unbiased_moving_var, cfg.seed = int(bn_unbiased_moving_var), seed & 0xFFFFFFFFFFFFFFFF
    _hip.check(_hip.lib().oct_unet_cfg_check(C.byref(cfg)), "oct_unet_cfg_check")
    return cfg


def layer_table(cfg: UNetCfg) -> List[dict]:
    """Conv(+BN) nodes in Keras creation order with their flat-buffer offsets (host only, no GPU)."""
    l = _hip.lib()
    out = []
    for i in range(l.oct_unet_layer_count(C.byref(cfg))):
        info = LayerInfo()
        _hip.check(l.oct_unet_layer_info(C.byref(cfg), i, C.byref(info)), "oct_unet_layer_info")
        out.append({k: (getattr(info, k).decode() if k == "name" else int(getattr(info, k))) for k, _ in LayerInfo._fields_})
    return out


def glorot_init(cfg: UNetCfg, seed: int = 0):
    """Keras initial values (glorot_uniform kernels, zero bias, gamma=1, beta=0, moving mean 0 / var 1)."""
    rng = np.random.default_rng(seed)
    l = _hip.lib()
    params = np.zeros(l.oct_unet_param_count(C.byref(cfg)), np.float32)
    state = np.zeros(l.oct_unet_state_count(C.byref(cfg)), np.float32)
    for L in layer_table(cfg):
        n = L["kh"] * L["kw"] * L["cin"] * L["cout"]
        lim = np.sqrt(6.0 / (L["kh"] * L["kw"] * (L["cin"] + L["cout"])))
        params[L["kernel_off"]:L["kernel_off"] + n] = rng.uniform(-lim, lim, n).astype(np.float32)
        if L["has_bn"]:
            params[L["gamma_off"]:L["gamma_off"] + L["cout"]] = 1.0
            state[L["moving_var_off"]:L["moving_var_off"] + L["cout"]] = 1.0
    return params, state


class UNetEngine:
    def __init__(self, *, device="cuda:0", init_seed: int = 0, **cfg_kwargs):
        self._h = None
        self.device = _require_gpu(device)
        self.cfg = make_cfg(**cfg_kwargs)
        self.layers = layer_table(self.cfg)
        l = _hip.lib()
        self.n_params = int(l.oct_unet_param_count(C.byref(self.cfg)))
        self.n_state = int(l.oct_unet_state_count(C.byref(self.cfg)))
        ws_bytes = int(l.oct_unet_workspace_bytes(C.byref(self.cfg)))
        with torch.cuda.device(self.device):
            p0, s0 = glorot_init(self.cfg, init_seed)
            self.params = torch.from_numpy(p0).to(self.device)
            self.state = torch.from_numpy(s0).to(self.device)
            self.grads = torch.zeros(self.n_params, dtype=torch.float32, device=self.device) if self.cfg.training else None
            self.workspace = torch.empty(ws_bytes, dtype=torch.uint8, device=self.device)
            h = C.c_void_p()
            _hip.check(l.oct_unet_create(C.byref(self.cfg), self.params.data_ptr(), _ptr(self.grads), self.state.data_ptr(),
                                         self.workspace.data_ptr(), ws_bytes, C.byref(h)), "oct_unet_create")
        self._h = h
        self._opt: Dict[str, torch.Tensor] = {}
        self.opt_step = 0
        # kept alive: the tensors an in-flight launch and the captured graph refer to, the event of set_tail_event
        self._keep, self._graph_keep, self._tail_event = [], [], None
        self._mc: Dict[int, dict] = {}  # infer's buffer set per batch size
        self._pad_bufs, self._wver = {}, -1  # its Model's: the padded pair per (batch size, image type); the version of the weights held
        # the loss state: what the set_* calls last selected (set_focal_dice's device buffer and parameters by value too); select_loss's kind
        self.ignore_label, self._focal_active, self._bce_active = None, False, False
        self._focal_cw, self._focal_sel, self._loss_kind = None, None, "dice"
        self.dice_shape, self._shape_cw = None, None       # set_dice_shape's validated keywords (None: plain Dice) and its device weights
        # per-pixel loss weights: the map the library holds a pointer to (None: off), the spec select_loss last saw, and the
        # engine's own LUTs per spec and maps per batch size (Model._run_epoch fills them)
        self.pixel_weights, self.edge_weight = None, None
        self._edge_luts, self._edge_maps = {}, {}

    def __del__(self):
        if self._h:
            try:
                _hip.lib().oct_unet_destroy(self._h)
            except Exception:   # interpreter teardown: module globals may already be gone
                pass
            self._h = None

    # ---- plumbing --------------------------------------------------------------------------------
    @property
    def H(self): return self.cfg.H
    @property
    def W(self): return self.cfg.W
    @property
    def num_classes(self): return self.cfg.n_cls

    def _stream(self):
        return _hip.stream_ptr(self.device)

    def _call(self, name: str, *args) -> None:
        """``name(handle, *args)`` of the library, on the engine's device."""
        _hip.call(name, self.device, self._h, *args)

    def _check_x(self, x: torch.Tensor, any_size: bool = False):
        # uint8: raw scans; float32: already / 255; of the engine's size (any_size: the input of a padded infer)
        _hip.expect(x, "input", device=self.device, dtype=(torch.uint8, torch.float32),
                    shape=(None,) + ((None, None) if any_size else (self.cfg.H, self.cfg.W)) + (self.cfg.in_ch,))
        if not 1 <= x.shape[0] <= self.cfg.max_batch:
            raise OctError(f"batch {x.shape[0]} outside 1..max_batch={self.cfg.max_batch}")

    def _check_labels(self, labels: torch.Tensor, B: int):
        _hip.expect(labels, "labels (B,H,W[,1])", device=self.device, dtype=torch.uint8, numel=B * self.cfg.H * self.cfg.W)

    def _io(self, B, labels, want_probs, want_argmax, probs_out=None, argmax_out=None):
        H, W = self.cfg.H, self.cfg.W
        probs = am = None
        if want_probs:
            probs = probs_out if probs_out is not None else torch.empty((B, H, W, self.cfg.n_cls), dtype=torch.float32, device=self.device)
        if want_argmax:
            am = argmax_out if argmax_out is not None else torch.empty((B, H, W), dtype=torch.uint8, device=self.device)
        return UNetIO(_ptr(probs), _ptr(am), _ptr(labels)), probs, am

    # ---- hot path --------------------------------------------------------------------------------
    def forward(self, x: torch.Tensor, training: bool = False, labels: Optional[torch.Tensor] = None,
                want_probs: bool = True, want_argmax: bool = False, probs_out=None, argmax_out=None):
        self._check_x(x)
        B = x.shape[0]
        if labels is not None:
            self._check_labels(labels, B)
        io, probs, am = self._io(B, labels, want_probs, want_argmax, probs_out, argmax_out)
        self._call("oct_unet_forward", x.data_ptr(), int(x.dtype == torch.uint8), B, int(training), C.byref(io), self._stream())
        self._keep = [x, labels, probs, am]
        return probs, am

    def _loss(self, name: str, n: int, smooth: float) -> torch.Tensor:
        out = torch.empty(n, dtype=torch.float32, device=self.device)
        self._call(name, smooth, out.data_ptr(), self._stream())
        return out

    def loss_dice(self, smooth: float = 1e-5) -> torch.Tensor:
        """[dice_loss_macro, dice_loss_micro, dice_coef_macro, dice_coef_micro] of the last forward (device tensor)."""
        return self._loss("oct_unet_loss_dice", 4, smooth)

    def set_focal_dice(self, focal_loss_weight: float = 0.5, gamma: float = 2.0, class_weight=None) -> None:
        """Select ``focal_dice_loss`` (reference custom_losses.py:98-178) for the following forward / loss / backward
        calls: L = w*focal + (1-w)*dice.  ``focal_loss_weight = 0`` restores the plain Dice losses."""
        host = None if class_weight is None else np.asarray(class_weight, np.float32)
        cw = None if host is None else torch.as_tensor(host, device=self.device).contiguous()
        if cw is not None and cw.numel() != self.cfg.n_cls:
            raise OctError(f"class_weight must have {self.cfg.n_cls} entries")
        self._focal_cw = cw          # keep the device buffer alive: the library only stores the pointer
        self._focal_sel = (float(focal_loss_weight), float(gamma), None if host is None else host.tolist())     # by value
        self._focal_active = float(focal_loss_weight) > 0.0
        if self._focal_active:
            self._bce_active = False     # the library clears it too: the two losses share one slot of the Dice rows
        self._call("oct_unet_set_focal_dice", float(focal_loss_weight), float(gamma), _ptr(cw))

    def loss_focal_dice(self, smooth: float = 1e-5) -> torch.Tensor:
        """loss_dice() + [focal term, w*focal+(1-w)*dice_macro, w*focal+(1-w)*dice_micro, 0] (device tensor, 8 floats)."""
        return self._loss("oct_unet_loss_focal_dice", 8, smooth)

    def set_bce_dice(self, on: bool = True) -> None:
        """Select ``bce_dice_loss`` (reference custom_losses.py:84-91) for the following forward / loss / backward calls:
        L = mean over (B,H,W,C) of the binary cross-entropy + dice_loss_micro.  Clears a selected focal_dice_loss;
        ``on=False`` restores the plain Dice losses.  ``backward`` then takes ``macro=False`` only."""
        self._bce_active = bool(on)
        if self._bce_active:
            self._focal_active = False
        self._call("oct_unet_set_bce_dice", int(bool(on)))

    def loss_bce_dice(self, smooth: float = 1e-5) -> torch.Tensor:
        """loss_dice() + [bce mean, 0, bce + dice_loss_micro, 0] (device tensor, 8 floats)."""
        return self._loss("oct_unet_loss_bce_dice", 8, smooth)

    def set_ignore_label(self, label: Optional[int]) -> None:
        """Pixels whose label byte equals ``label`` (``num_classes..255``) do not count in the loss of the following
        forward / loss / backward calls: nothing in the Dice sums and metrics, nothing in the focal / BCE mean -- which then
        divides by the counted pixels -- and a zero gradient (``oct_unet_set_ignore_label``).  ``None`` switches it off."""
        self._call("oct_unet_set_ignore_label", -1 if label is None else int(label))
        self.ignore_label = None if label is None else int(label)

    def set_pixel_weights(self, w: Optional[torch.Tensor]) -> None:
        """Per-pixel weights of the focal / BCE term for the following forward / loss / backward calls
        (``oct_unet_set_pixel_weights``): a float32 (B,H,W[,1]) tensor of the NEXT batch, kept alive by the engine and read
        at the forward and the backward (refill it in place between steps), or ``None`` = off.  The Dice term, the metrics
        and the divisor of the mean (B*H*W, or the counted pixels) do not see it.  Setting another tensor drops a pending
        forward: call ``forward`` again before the loss."""
        if w is not None:
            _hip.expect(w, "pixel weights (B,H,W[,1])", device=self.device, dtype=torch.float32)
            if w.dim() not in (3, 4) or tuple(w.shape[1:3]) != (self.cfg.H, self.cfg.W) or w.numel() != w.shape[0] * self.cfg.H * self.cfg.W \
                    or not 1 <= w.shape[0] <= self.cfg.max_batch:
                raise OctError(f"pixel weights must be (B,{self.cfg.H},{self.cfg.W}[,1]) with B in 1..{self.cfg.max_batch}, not {tuple(w.shape)}")
        self._call("oct_unet_set_pixel_weights", _ptr(w))
        self.pixel_weights = w       # keep the tensor alive: the library only stores the pointer

    def edge_weight_map(self, labels: torch.Tensor, radius: int, lut, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The border weight map of uint8 (B,H,W[,1]) ``labels`` on the device (``oct_edge_weight_map``;
        ``common.utils.edge_weight_reference`` restates it): float32 (B,H,W), ``lut[capped squared distance to the nearest
        class border]`` at a pixel whose label is a class, 0 elsewhere.  ``lut``: ``common.utils.edge_weight_lut``'s
        ``radius^2 + 2`` floats, a numpy array (uploaded) or a float32 device tensor.  Any image size; asynchronous on the
        current stream."""
        _hip.expect(labels, "edge_weight_map: labels (B,H,W[,1])", device=self.device, dtype=torch.uint8)
        if labels.dim() not in (3, 4) or (labels.dim() == 4 and labels.shape[3] != 1) or labels.numel() == 0:
            raise OctError(f"edge_weight_map: labels must be a non-empty (B,H,W) or (B,H,W,1) tensor, not {tuple(labels.shape)}")
        B, H, W = labels.shape[:3]
        if int(radius) != radius or not 1 <= int(radius) <= 32:
            raise OctError(f"edge_weight_map: radius must be an integer in 1..32, not {radius!r}")
        if not torch.is_tensor(lut):
            lut = torch.from_numpy(np.ascontiguousarray(lut, np.float32)).to(self.device)
        _hip.expect(lut, "edge_weight_map: lut (radius^2 + 2 floats)", device=self.device, dtype=torch.float32, shape=(int(radius) ** 2 + 2,))
        if out is None:
            out = torch.empty((B, H, W), dtype=torch.float32, device=self.device)
        else:
            _hip.expect(out, "edge_weight_map: out", device=self.device, dtype=torch.float32, shape=(B, H, W))
        _hip.call("oct_edge_weight_map", self.device, labels.data_ptr(), B, H, W, self.cfg.n_cls, int(radius), lut.data_ptr(),
                  out.data_ptr(), self._stream())
        self._keep = self._keep + [labels, lut, out]
        return out

    def edge_weight_step(self, labels: torch.Tensor, spec: dict) -> torch.Tensor:
        """The map of ``spec`` (``check_edge_weight``'s dict) for this step's ``labels``, in the engine's buffer of that batch
        size, and set as the pixel weights.  The LUT is uploaded once per spec, the buffer made once per batch size."""
        from .common.utils import edge_weight_lut
        key = (spec["radius"], spec["profile"], spec["weight"], spec["sigma"])
        lut = self._edge_luts.get(key)
        if lut is None:
            lut = self._edge_luts[key] = torch.from_numpy(edge_weight_lut(*key)).to(self.device)
        B = labels.shape[0]
        buf = self._edge_maps.get(B)
        if buf is None:
            buf = self._edge_maps[B] = torch.empty((B, self.cfg.H, self.cfg.W), dtype=torch.float32, device=self.device)
        self.edge_weight_map(labels, spec["radius"], lut, out=buf)
        if self.pixel_weights is not buf:
            self.set_pixel_weights(buf)
        return buf

    def set_dice_shape(self, alpha=0.5, beta: float = 0.5, gamma: float = 1.0, class_weight=None) -> None:
        """Shape the Dice term of the following forward / loss / backward calls (``oct_unet_set_dice_shape``, DESIGN.md section
        32): Tversky weights ``alpha`` (false positives) and ``beta`` (false negatives), the focal-Tversky exponent ``gamma``
        and class weights -- ``None``, a sequence of ``num_classes`` weights, or ``"volume"`` (generalized Dice, 1 / T^2 of the
        label volume).  The defaults, or ``set_dice_shape(None)``, restore plain Dice.  A pending forward is dropped: call
        ``forward`` again before the loss."""
        from .common.custom_losses import check_dice_shape
        try:
            shape = None if alpha is None else check_dice_shape(self.cfg.n_cls, alpha, beta, gamma, class_weight)
        except (ValueError, TypeError) as e:
            raise OctError(f"set_dice_shape: {e}") from None
        cw = None
        if shape is None:
            self._call("oct_unet_set_dice_shape", None)
        else:
            w = shape["class_weight"]
            mode = _hip.DICE_WEIGHT_NONE if w is None else _hip.DICE_WEIGHT_VOLUME if w == "volume" else _hip.DICE_WEIGHT_CLASS
            if mode == _hip.DICE_WEIGHT_CLASS:
                cw = torch.as_tensor(np.asarray(w, np.float32), device=self.device).contiguous()
            d = _hip.DiceShape(shape["alpha"], shape["beta"], shape["gamma"], mode, _ptr(cw))
            self._call("oct_unet_set_dice_shape", C.byref(d))
        self._shape_cw = cw          # keep the device buffer alive: the library only stores the pointer
        self.dice_shape = shape

    def select_loss(self, kind: str = "dice", focal_loss_weight=0.5, gamma=2.0, class_weight=None, ignore_label=None,
                    dice_shape=None, edge_weight=None) -> None:
        """Put the handle into the loss state a model asks for: ``kind`` "dice", "focal" (with ``set_focal_dice``'s parameters,
        compared by value) or "bce", the ignore label and the shape of the Dice term (``set_dice_shape``'s keywords as a dict,
        None: plain Dice).  Only the ``set_*`` calls that change what the engine last had selected are issued: an engine last
        used by a focal, BCE, masked or shaped model comes back to plain Dice over every pixel.  ``edge_weight``: the spec of
        the model's border weights (None: none); a model without one takes the pixel weights off an engine that another
        model left weighted (a model with one sets its map per step, ``edge_weight_step``)."""
        if edge_weight is None and self.pixel_weights is not None:
            self.set_pixel_weights(None)
        self.edge_weight = edge_weight
        if self.dice_shape != dice_shape:
            self.set_dice_shape(**dice_shape) if dice_shape else self.set_dice_shape(None)
        if self.ignore_label != ignore_label:
            self.set_ignore_label(ignore_label)
        want = (float(focal_loss_weight), float(gamma), None if class_weight is None else np.asarray(class_weight, np.float32).tolist())
        if kind == "focal" and not (self._focal_active and self._focal_sel == want):
            self.set_focal_dice(*want)
        elif kind != "focal" and self._focal_active:
            self.set_focal_dice(0.0)
        if (kind == "bce") != self._bce_active:
            self.set_bce_dice(kind == "bce")
        self._loss_kind = kind

    def loss_selected(self, smooth: float = 1e-5) -> torch.Tensor:
        """The loss vector of the kind last given to ``select_loss``: ``loss_dice``, ``loss_focal_dice`` or ``loss_bce_dice``."""
        return {"dice": self.loss_dice, "focal": self.loss_focal_dice, "bce": self.loss_bce_dice}[self._loss_kind](smooth)

    def backward(self, labels: torch.Tensor, macro: bool = True, loss_scale: float = 1.0):
        self._check_labels(labels, labels.shape[0])
        self._call("oct_unet_backward", labels.data_ptr(), int(macro), loss_scale, self._stream())

    def adam_step(self, lr=1e-3, beta_1=0.9, beta_2=0.999, epsilon=1e-7):
        if "m" not in self._opt:
            self._opt["m"] = torch.zeros_like(self.params); self._opt["v"] = torch.zeros_like(self.params)
        self.opt_step += 1
        _hip.call("oct_adam_step", self.device, self.params.data_ptr(), self.grads.data_ptr(), self._opt["m"].data_ptr(),
                  self._opt["v"].data_ptr(), self.n_params, lr, beta_1, beta_2, epsilon, self.opt_step, self._stream())

    def sgd_step(self, lr=1e-2, momentum=0.0):
        mom = None
        if momentum != 0.0:
            if "mom" not in self._opt:
                self._opt["mom"] = torch.zeros_like(self.params)
            mom = self._opt["mom"].data_ptr()
        self.opt_step += 1
        _hip.call("oct_sgd_step", self.device, self.params.data_ptr(), self.grads.data_ptr(), mom, self.n_params, lr, momentum,
                  self._stream())

    # state buffers of oct_opt_step by kind, in the ABI's slot order (Adam and SGD share theirs with adam_step / sgd_step)
    _OPT_SLOTS = {_hip.OPT_SGD: ("mom",), _hip.OPT_ADAM: ("m", "v", "vhat"), _hip.OPT_ADAMAX: ("adamax.m", "adamax.u"),
                  _hip.OPT_RMSPROP: ("rmsprop.rms", "rmsprop.mom", "rmsprop.mg"), _hip.OPT_ADAGRAD: ("adagrad.a",),
                  _hip.OPT_ADADELTA: ("adadelta.a", "adadelta.b")}

    def var_offsets(self) -> np.ndarray:
        """The variable table of the flat parameter buffer: n_vars + 1 ascending offsets, variable k being
        [off[k], off[k+1]) -- kernel, bias and (with BN) gamma, beta of every conv, in buffer order."""
        offs = sorted(L[k] for L in self.layers for k in (("kernel_off", "bias_off", "gamma_off", "beta_off") if L["has_bn"]
                                                          else ("kernel_off", "bias_off")))
        return np.asarray(offs + [self.n_params], np.uint64)

    def optimizer_step(self, kind: int, *, lr: float, beta_1: float = 0.9, beta_2: float = 0.999, rho: float = 0.9,
                       momentum: float = 0.0, epsilon: float = 1e-7, flags: int = 0, clip_mode: int = _hip.CLIP_NONE,
                       clip: float = 0.0, initial_accumulator_value: float = 0.1):
        """One step of any optimizer of the family on params / grads (``oct_opt_step``); state buffers, the variable table
        and the clipping scratch are created at the first step that needs them and then live in ``_opt``."""
        l = _hip.lib()
        desc = _hip.OptDesc(kind, flags, clip_mode, clip, lr, beta_1, beta_2, rho, momentum, epsilon)
        ns = l.oct_opt_slot_count(C.byref(desc))
        if ns < 0:
            raise OctError(f"oct_opt_slot_count: {l.oct_last_error().decode()}")
        names = self._OPT_SLOTS[kind]
        if kind == _hip.OPT_RMSPROP:
            names = tuple(n for n, on in zip(names, (True, momentum != 0.0, bool(flags & _hip.OPT_CENTERED))) if on)
        slots = (C.c_void_p * 3)()
        for k, name in enumerate(names[:ns]):
            if name not in self._opt:
                self._opt[name] = torch.full_like(self.params, initial_accumulator_value if kind == _hip.OPT_ADAGRAD else 0.0)
            slots[k] = self._opt[name].data_ptr()
        var_off = scratch = None
        n_vars = 0
        if clip_mode in (_hip.CLIP_NORM, _hip.CLIP_GLOBAL_NORM):
            if "clip.var_off" not in self._opt:
                off = self.var_offsets()
                self._opt["clip.var_off"] = torch.from_numpy(off.astype(np.int64)).to(self.device)
                self._opt["clip.scratch"] = torch.empty(int(l.oct_opt_scratch_bytes(len(off) - 1, self.n_params)),
                                                        dtype=torch.uint8, device=self.device)
            var_off, scratch = self._opt["clip.var_off"].data_ptr(), self._opt["clip.scratch"].data_ptr()
            n_vars = self._opt["clip.var_off"].numel() - 1
        self.opt_step += 1
        _hip.call("oct_opt_step", self.device, C.byref(desc), self.params.data_ptr(), self.grads.data_ptr(), slots, self.n_params,
                  self.opt_step, var_off, n_vars, scratch, self._stream())

    # ---- data-parallel overlap hook ---------------------------------------------------
    def grad_tail_offset(self) -> int:
        """First float of the gradient segment (bottleneck + decoder + head) that is final at the tail event."""
        return int(_hip.lib().oct_unet_grad_tail_offset(C.byref(self.cfg)))

    def set_tail_event(self, event: Optional[torch.cuda.Event]) -> None:
        """``backward`` records ``event`` on its stream once grads[grad_tail_offset():] are final (None disables)."""
        if event is not None and not event.cuda_event:
            with torch.cuda.device(self.device):
                event.record()          # torch creates the HIP event lazily, at its first record
        self._tail_event = event        # keep the handle alive
        self._call("oct_unet_set_tail_event", C.c_void_p(event.cuda_event) if event is not None else None)

    # ---- arithmetic mode of the convolution kernels (reported by bench.py) --------------------------
    def mfma_products(self) -> int:
        """0: the convolutions run on the f32 MFMA pipe.  n > 0: on the bf16 pipe, n bf16 products per product
        (6 = exact three-term split of both fp32 operands, csrc/kernels_bx.hpp; 1 = bf16 operands, cfg.dtype 1)."""
        if not self.handle_option("mfma_mode"):
            return 0
        return 1 if self.cfg.dtype == 1 else 6

    def mfma_mode_name(self) -> str:
        n = self.mfma_products()
        if n == 0:
            return "f32 MFMA (v_mfma_f32_32x32x2_f32 / v_mfma_f32_16x16x4_f32), f32 accumulate"
        if n == 1:
            return "bf16 MFMA (v_mfma_f32_32x32x16_bf16 / 16x16x32), bf16 operands, f32 accumulate"
        return ("fp32 via exact 3-term bf16 split: 6 bf16 MFMAs (v_mfma_f32_32x32x16_bf16 / 16x16x32) per fp32 product, "
                "f32 accumulate (first layer / head: f32 VALU)")

    # ---- per-launch profiler ---------------------------------------------------------------------
    def profile_begin(self):
        self._call("oct_unet_profile_begin")

    def profile_end(self) -> List[dict]:
        """One dict per (kernel instantiation, layer): launches, total_ms, algorithmic flops and bytes."""
        n = C.c_int(0)
        buf = (_hip.ProfileEntry * 1024)()
        self._call("oct_unet_profile_end", buf, 1024, C.byref(n))
        return [dict(kernel=buf[i].kernel.decode(), layer=buf[i].layer.decode(), launches=buf[i].launches,
                     total_ms=buf[i].total_ms, flops=buf[i].flops, bytes=buf[i].bytes) for i in range(min(n.value, 1024))]

    # ---- dropout replay (tests) -------------------------------------------------------------------
    def set_dropout_step(self, step: int):
        self._call("oct_unet_set_dropout_step", step)

    def dropout_mask(self, B: int) -> torch.Tensor:
        P = self.cfg.pool_layers
        m = torch.empty((B, self.cfg.H >> P, self.cfg.W >> P, self.cfg.start_neurons << P), dtype=torch.uint8, device=self.device)
        self._call("oct_unet_dropout_mask", B, m.data_ptr(), self._stream())
        return m

    # ---- inference: one chain -- plain, Monte-Carlo dropout or test-time augmentation; padded or not; eager or captured ----
    _MAPS = ("mean_probs", "argmax", "entropy", "mutual_info")

    def _buf(self, B: int, key, shape, dtype) -> torch.Tensor:
        """Tensor ``key`` of the buffer set of batch size ``B``: made at its first use, kept."""
        b = self._mc.setdefault(B, {})
        if key not in b:
            b[key] = torch.empty(shape, dtype=dtype, device=self.device)
        return b[key]

    def _map(self, B: int, k: str, hw=None) -> torch.Tensor:
        """Map ``k`` of ``_MAPS`` in the buffer set: at the engine's size, or the cropped one of true size ``hw``."""
        H, W = hw or (self.cfg.H, self.cfg.W)
        return self._buf(B, k if hw is None else (k, H, W), (B, H, W) + ((self.cfg.n_cls,) if k == "mean_probs" else ()),
                         torch.uint8 if k == "argmax" else torch.float32)

    def _mc_buffers(self, B: int) -> dict:
        """The buffer set of batch size ``B`` with what every Monte-Carlo / TTA chain needs: scratch probabilities, reduction
        workspace and the four maps at the engine's size."""
        H, W, Cn = self.cfg.H, self.cfg.W, self.cfg.n_cls
        self._buf(B, "scratch", (B, H, W, Cn), torch.float32)
        self._buf(B, "ws", (int(_hip.lib().oct_mc_workspace_bytes(B, H, W, Cn)),), torch.uint8)
        for k in self._MAPS:
            self._map(B, k)
        return self._mc[B]

    def _tta_buffers(self, B: int, x: torch.Tensor) -> dict:
        """``_mc_buffers`` plus ``x_view``, the flipped input of a TTA chain for the input's type."""
        b = self._mc_buffers(B)
        return dict(b, x_view=self._buf(B, "x_view_u8" if x.dtype == torch.uint8 else "x_view_f32",
                                        (B, self.cfg.H, self.cfg.W, self.cfg.in_ch), x.dtype))

    def infer(self, x: torch.Tensor, *, mc=None, tta=None, pad=None, want_probs: bool, want_argmax: bool,
              capture: bool = False) -> Dict[str, torch.Tensor]:
        """THE inference entry (``oct_unet_infer`` / ``oct_unet_graph_capture_infer``): one chain of launches on the current stream.

        * kind -- neither ``mc`` nor ``tta``: one forward; the dict holds ``probs`` (B,H,W,C) float32 and / or ``argmax`` (B,H,W)
          uint8 as wanted.  ``mc=(samples, step0)``: ``samples`` forwards with the bottleneck dropout on (dropout steps ``step0 ..
          step0+samples-1``; the encoder and the bottleneck run once), reduced on the device.  ``tta=views``, 1..4 distinct
          names of ``common.utils.TTA_VIEWS``: one forward per view on the batch flipped by it, mirrored back and averaged on the
          device.  Both give ``entropy`` and ``mutual_info`` (B,H,W) float32, ``argmax`` -- of the mean prediction -- with
          ``want_argmax`` and ``mean_probs`` with ``want_probs``.
        * ``pad=(top, left, mode, value)``: ``x`` has a size that is no multiple of 2^pool_layers and the engine is one built at
          the padded size; the chain pads in front (``oct_pad_batch``), takes the views of the PADDED batch and crops every map
          it returns behind (``oct_crop_batch``).
        * ``capture``: record the chain over the fixed input ``x`` into the graph that ``graph_launch`` replays, instead of
          running it; ``x`` must be refilled in place between launches, and every replay refills the tensors returned here.
          Not with ``mc``: the dropout step travels by value.

        The tensors of an unpadded plain forward are new ones; all others belong to the engine's buffer set for this batch
        size (and true size): the next ``infer`` of that batch size refills them."""
        if mc is not None and tta is not None:
            raise OctError("infer: mc and tta exclude each other")
        self._check_x(x, any_size=pad is not None)
        B, H, W, _ = x.shape
        plain = mc is None and tta is None
        d = _hip.Infer(x_dev=x.data_ptr(), x_is_u8=int(x.dtype == torch.uint8), B=B, H=H, W=W)
        if plain and pad is None:
            _, probs, am = self._io(B, None, want_probs, want_argmax)
            full = {k: t for k, t in (("mean_probs", probs), ("argmax", am)) if t is not None}
        else:
            keys = (("mean_probs",) if want_probs else ()) + (("argmax",) if want_argmax else ()) + (() if plain else self._MAPS[2:])
            full = {k: self._map(B, k) for k in keys}
        if mc is not None:
            samples, step0 = mc
            if not 1 <= int(samples) <= _hip.MC_MAX_SAMPLES:
                raise OctError(f"infer: mc samples must be in 1..{_hip.MC_MAX_SAMPLES}, not {samples}")
            d.kind, d.T, d.step0 = _hip.INFER_MC, int(samples), int(step0) & 0xFFFFFFFFFFFFFFFF
        if tta is not None:
            from .common.utils import parse_tta
            try:
                codes = parse_tta(tta)
            except ValueError as e:
                raise OctError(str(e)) from None
            if not codes:
                raise OctError("tta: at least one view is needed")
            d.kind, d.T, d.views = _hip.INFER_TTA, len(codes), (C.c_int * 4)(*codes)
            d.x_view_dev = self._tta_buffers(B, x)["x_view"].data_ptr()
        if not plain:
            b = self._mc_buffers(B)
            d.probs_scratch_dev, d.ws_dev, d.ws_bytes = b["scratch"].data_ptr(), b["ws"].data_ptr(), b["ws"].numel()
        outs = full
        if pad is not None:
            top, left, mode, value = pad
            if mode not in _hip.PAD_MODES:
                raise OctError(f'infer: the pad mode must be "edge", "reflect" or "constant", not {mode!r}')
            d.top, d.left, d.pad_mode, d.pad_value = int(top), int(left), _hip.PAD_MODES[mode], float(value)
            d.x_pad_dev = self._buf(B, ("x_pad", x.dtype), (B, self.cfg.H, self.cfg.W, self.cfg.in_ch), x.dtype).data_ptr()
            outs = {k: self._map(B, k, (H, W)) for k in full}
            d.out_crop = _hip.McOut(**{k: t.data_ptr() for k, t in outs.items()})
        d.out = _hip.McOut(**{k: t.data_ptr() for k, t in full.items()})
        if plain:
            outs = {("probs" if k == "mean_probs" else k): t for k, t in outs.items()}
        if capture:
            s = torch.cuda.Stream(self.device)                  # a side stream, joined to the current one on both ends
            s.wait_stream(torch.cuda.current_stream(self.device))
            self._call("oct_unet_graph_capture_infer", C.byref(d), C.c_void_p(s.cuda_stream))
            torch.cuda.current_stream(self.device).wait_stream(s)
            # the fixed input, what else the graph refers to outside the buffer set, the arg-max map it refills
            self._graph_keep = [x, full, outs.get("argmax")]
        else:
            self._call("oct_unet_infer", C.byref(d), self._stream())
            self._keep = [x, full]
        return outs

    def forward_mc(self, x: torch.Tensor, samples: int, step0: int = 0, want_mean_probs: bool = False) -> Dict[str, torch.Tensor]:
        """``infer(x, mc=(samples, step0))``: ``argmax``, ``entropy``, ``mutual_info`` and, with ``want_mean_probs``,
        ``mean_probs`` -- the engine's own buffers for this batch size.  Asynchronous on the current stream."""
        return self.infer(x, mc=(samples, step0), want_probs=want_mean_probs, want_argmax=True)

    def forward_tta(self, x: torch.Tensor, views, want_mean_probs: bool = False) -> Dict[str, torch.Tensor]:
        """``infer(x, tta=views)``: a dict like ``forward_mc``'s, in the same buffers."""
        return self.infer(x, tta=views, want_probs=want_mean_probs, want_argmax=True)

    def graph_capture_tta(self, x: torch.Tensor, views, want_mean_probs: bool = False, pad=None) -> Dict[str, torch.Tensor]:
        """``infer(x, tta=views, pad=pad, capture=True)``: the dict of tensors every ``graph_launch`` refills."""
        return self.infer(x, tta=views, pad=pad, want_probs=want_mean_probs, want_argmax=True, capture=True)

    def graph_capture(self, x: torch.Tensor, want_probs=True, want_argmax=False):
        """Capture one inference forward over fixed buffers; returns (probs, argmax) output tensors that every
        ``graph_launch`` refills.  ``x`` must be refilled in place (``x.copy_``) between launches."""
        out = self.infer(x, want_probs=want_probs, want_argmax=want_argmax, capture=True)
        return out.get("probs"), out.get("argmax")

    def graph_capture_padded(self, x: torch.Tensor, top: int, left: int, mode: str, value=0, want_probs=True, want_argmax=False):
        """``graph_capture`` of a (B,H,W,ch) input of a size that is no multiple of 2^pool_layers, on an engine built at the
        padded size: pad, forward and crops in ONE graph; the (probs, argmax) tensors are of size (H, W)."""
        out = self.infer(x, pad=(top, left, mode, value), want_probs=want_probs, want_argmax=want_argmax, capture=True)
        return out.get("probs"), out.get("argmax")

    def mc_update(self, probs: torch.Tensor, t: int, samples: int, ws: torch.Tensor, *, mean_probs=None, argmax=None,
                  entropy=None, mutual_info=None) -> None:
        """Fold softmax sample ``t`` of ``samples`` -- ``probs`` (B,H,W,C) float32, any C in 2..32 -- into the running sums
        in ``ws`` (a uint8 tensor of ``oct_mc_workspace_bytes`` bytes); the call with ``t == samples - 1`` writes the maps
        that are given (``oct_mc_update``; ``common.utils.mc_reduce_reference`` restates it).  Calls go in order of t."""
        out = self._mc_out(probs, ws, mean_probs, argmax, entropy, mutual_info)
        B, H, W, Cn = probs.shape
        _hip.call("oct_mc_update", self.device, probs.data_ptr(), B, H, W, Cn, int(t), int(samples), ws.data_ptr(), ws.numel(),
                  C.byref(out), self._stream())

    def _mc_out(self, probs, ws, mean_probs, argmax, entropy, mutual_info) -> "_hip.McOut":
        """The tensor checks of ``mc_update`` / ``tta_update`` -> the ``oct_mc_out`` of the maps that are given."""
        _hip.expect(probs, "probs (B,H,W,C)", device=self.device, dtype=torch.float32, shape=(None, None, None, None))
        B, H, W, Cn = probs.shape
        _hip.expect(ws, "mc workspace", device=self.device, dtype=torch.uint8, shape=(None,))
        for t_, what, dt, shape in ((mean_probs, "mean_probs", torch.float32, (B, H, W, Cn)), (argmax, "argmax", torch.uint8, (B, H, W)),
                                    (entropy, "entropy", torch.float32, (B, H, W)), (mutual_info, "mutual_info", torch.float32, (B, H, W))):
            if t_ is not None:
                _hip.expect(t_, what, device=self.device, dtype=dt, shape=shape)
        return _hip.McOut(_ptr(mean_probs), _ptr(argmax), _ptr(entropy), _ptr(mutual_info))

    # ---- calibration: reliability counts and temperature on the device (evaluation/calibration.py restates them) ----
    def _cal_inputs(self, what: str, probs: torch.Tensor, labels: torch.Tensor, ignore_label):
        """The tensor checks of ``calibration_counts`` / ``temperature_nll`` -> ``(B, npix, C, ignore_label as the ABI's int)``."""
        if probs.dim() < 3:
            raise OctError(f"{what}: probs must be (B,...,C), not {tuple(probs.shape)}")
        _hip.expect(probs, f"{what}: probs (B,...,C)", device=self.device, dtype=torch.float32, shape=(None,) * probs.dim())
        B, Cn = probs.shape[0], probs.shape[-1]
        npix = probs.numel() // max(B * Cn, 1)
        _hip.expect(labels, f"{what}: labels (B,...)", device=self.device, dtype=torch.uint8, numel=B * npix)
        if ignore_label is not None and not (int(ignore_label) == ignore_label and 0 <= int(ignore_label) <= 255):
            raise OctError(f"{what}: ignore_label must be None or an int in 0..255, not {ignore_label!r}")
        return B, npix, Cn, -1 if ignore_label is None else int(ignore_label)

    def _cal_ws(self, ws, nbytes: int, what: str) -> torch.Tensor:
        if not nbytes:
            raise OctError(f"{what}: unsupported shape (oct_last_error: {_hip.lib().oct_last_error().decode()})")
        if ws is None:
            return torch.empty((nbytes,), dtype=torch.uint8, device=self.device)
        _hip.expect(ws, f"{what}: workspace", device=self.device, dtype=torch.uint8, shape=(None,))
        return ws

    def calibration_counts(self, probs: torch.Tensor, labels: torch.Tensor, n_bins: int, ignore_label: Optional[int] = None, *,
                           counts=None, sums=None, ws=None):
        """Reliability counts of class probabilities ``probs`` (B,...,C) float32, any C in 2..32, against ``labels`` (B,...)
        uint8 in ``n_bins`` = 1..64 confidence bins (``oct_calibration_counts``; ``calibration_counts_reference``): returns
        ``(counts (B, n_bins, 3) int64 -- the bits are uint64 [pixels, correct, sum of floor(conf 2^28)] --, sums (B, 4) float64 =
        [sum nll, sum brier, counted, labels >= C that are not ignore_label])`` on the device.  ``counts`` / ``sums`` / ``ws``
        (uint8, ``oct_calibration_workspace_bytes``): optional tensors to use.  Asynchronous on the current stream."""
        B, npix, Cn, ig = self._cal_inputs("calibration_counts", probs, labels, ignore_label)
        M = int(n_bins)
        ws = self._cal_ws(ws, int(_hip.lib().oct_calibration_workspace_bytes(B, npix, Cn, M)), "calibration_counts")
        counts = torch.empty((B, M, 3), dtype=torch.int64, device=self.device) if counts is None else counts
        sums = torch.empty((B, 4), dtype=torch.float64, device=self.device) if sums is None else sums
        _hip.expect(counts, "calibration_counts: counts", device=self.device, dtype=torch.int64, shape=(B, M, 3))
        _hip.expect(sums, "calibration_counts: sums", device=self.device, dtype=torch.float64, shape=(B, 4))
        _hip.call("oct_calibration_counts", self.device, probs.data_ptr(), labels.data_ptr(), B, npix, Cn, ig, M, counts.data_ptr(),
                  sums.data_ptr(), ws.data_ptr(), ws.numel(), self._stream())
        return counts, sums

    def temperature_apply(self, probs: torch.Tensor, beta: float, out=None) -> torch.Tensor:
        """softmax(beta * log p) over the last axis of ``probs`` (...,C) float32 -- the class probabilities at temperature
        1 / beta, formed from the probabilities alone (``oct_temperature_apply``; ``temperature_apply_reference``).  ``out``:
        optional tensor to write into; it may be ``probs`` itself.  Asynchronous on the current stream."""
        if probs.dim() < 2:
            raise OctError(f"temperature_apply: probs must be (...,C), not {tuple(probs.shape)}")
        _hip.expect(probs, "temperature_apply: probs (...,C)", device=self.device, dtype=torch.float32, shape=(None,) * probs.dim())
        out = torch.empty_like(probs) if out is None else out
        _hip.expect(out, "temperature_apply: out", device=self.device, dtype=torch.float32, shape=tuple(probs.shape))
        Cn = probs.shape[-1]
        _hip.call("oct_temperature_apply", self.device, probs.data_ptr(), out.data_ptr(), probs.numel() // max(Cn, 1), Cn, float(beta),
                  self._stream())
        return out

    def temperature_nll(self, probs: torch.Tensor, labels: torch.Tensor, betas, ignore_label: Optional[int] = None, *,
                        out=None, ws=None):
        """For each of the 1..8 ``betas``: the per-image sums over the counted pixels of the NLL of the probabilities tempered
        by it and of its first and second derivative in beta (``oct_temperature_nll``; ``temperature_nll_reference``).
        Returns ``(sums (B, K, 3) float64, counted (B) float64)``, two views of ``out`` -- optional, float64 of B*K*3 + B
        elements.  Asynchronous on the current stream."""
        B, npix, Cn, ig = self._cal_inputs("temperature_nll", probs, labels, ignore_label)
        bs = [float(b) for b in np.atleast_1d(np.asarray(betas, dtype=np.float64))]
        K = len(bs)
        ws = self._cal_ws(ws, int(_hip.lib().oct_temperature_workspace_bytes(B, npix, Cn, K)), "temperature_nll")
        out = torch.empty((B * K * 3 + B,), dtype=torch.float64, device=self.device) if out is None else out
        _hip.expect(out, "temperature_nll: out", device=self.device, dtype=torch.float64, shape=(B * K * 3 + B,))
        _hip.call("oct_temperature_nll", self.device, probs.data_ptr(), labels.data_ptr(), B, npix, Cn, ig, (C.c_float * K)(*bs), K,
                  out.data_ptr(), ws.data_ptr(), ws.numel(), self._stream())
        return out[:B * K * 3].view(B, K, 3), out[B * K * 3:]

    # ---- ordered layer decode: the best class map per column that never decreases with depth ----------
    def ordered_decode(self, probs: torch.Tensor, *, labels=None, rows=None, score=None, ws=None):
        """The ordered decode of class probabilities ``probs`` (B,H,W,C) float32, C in 2..16, H <= 4096, class index == depth
        order (``oct_ordered_decode``; ``common.utils.ordered_decode_reference`` gives the same bits): returns ``(labels
        (B,H,W) uint8, rows (B,C-1,W) int16 -- the bits are uint16 --, score (B,W) int32 -- the bits are uint32)`` on the
        device.  ``labels`` / ``rows`` / ``score`` / ``ws`` (uint8, ``oct_ordered_workspace_bytes``): optional tensors to use.
        ``probs`` may be a view ``[:n]`` of a larger buffer.  Asynchronous on the current stream."""
        if probs.dim() != 4:
            raise OctError(f"ordered_decode: probs must be (B,H,W,C), not {tuple(probs.shape)}")
        _hip.expect(probs, "ordered_decode: probs (B,H,W,C)", device=self.device, dtype=torch.float32, shape=(None,) * 4)
        B, H, W, Cn = probs.shape
        nbytes = int(_hip.lib().oct_ordered_workspace_bytes(B, H, W, Cn))
        if not nbytes:
            raise OctError(f"ordered_decode: unsupported shape {tuple(probs.shape)}: need H <= 4096, B*H*W < 2^31 and 2..16 classes")
        if ws is None:
            ws = torch.empty((nbytes,), dtype=torch.uint8, device=self.device)
        _hip.expect(ws, "ordered_decode: workspace", device=self.device, dtype=torch.uint8, shape=(None,))
        labels = torch.empty((B, H, W), dtype=torch.uint8, device=self.device) if labels is None else labels
        rows = torch.empty((B, Cn - 1, W), dtype=torch.int16, device=self.device) if rows is None else rows
        score = torch.empty((B, W), dtype=torch.int32, device=self.device) if score is None else score
        _hip.expect(labels, "ordered_decode: labels", device=self.device, dtype=torch.uint8, shape=(B, H, W))
        _hip.expect(rows, "ordered_decode: rows", device=self.device, dtype=torch.int16, shape=(B, Cn - 1, W))
        _hip.expect(score, "ordered_decode: score", device=self.device, dtype=torch.int32, shape=(B, W))
        _hip.call("oct_ordered_decode", self.device, probs.data_ptr(), B, H, W, Cn, ws.data_ptr(), ws.numel(), labels.data_ptr(),
                  rows.data_ptr(), score.data_ptr(), self._stream())
        return labels, rows, score

    # ---- test-time augmentation: flipped views averaged on the device ---------------------------------
    def flip(self, t: torch.Tensor, view, out=None) -> torch.Tensor:
        """(B,H,W[,C]) uint8 or float32 -> the same shape mirrored by ``view`` -- a name of ``common.utils.TTA_VIEWS`` or its
        code 0..3 -- on the device (``oct_flip_batch``, one byte-moving kernel; ``common.utils.flip_reference`` restates it).
        ``out``: optional tensor to write into, never ``t`` itself.  Asynchronous on the current stream."""
        if t.dim() not in (3, 4):
            raise OctError(f"flip: t must be (B,H,W) or (B,H,W,C), not {tuple(t.shape)}")
        _hip.expect(t, "flip: t (B,H,W[,C])", device=self.device, dtype=(torch.uint8, torch.float32), shape=(None,) * t.dim())
        if out is None:
            out = torch.empty_like(t)
        _hip.expect(out, "flip: out", device=self.device, dtype=t.dtype, shape=tuple(t.shape))
        B, H, W = t.shape[:3]
        _hip.call("oct_flip_batch", self.device, t.data_ptr(), B, H, W, t.element_size() * int(np.prod(t.shape[3:], dtype=np.int64)),
                  _view_code(view), out.data_ptr(), self._stream())
        return out

    def tta_update(self, probs: torch.Tensor, view, t: int, samples: int, ws: torch.Tensor, *, mean_probs=None, argmax=None,
                   entropy=None, mutual_info=None) -> None:
        """``mc_update`` for the softmax output ``probs`` of the batch flipped by ``view``: pixel (b, y, x) of the sums and
        of the maps takes the mirrored pixel of ``probs`` (``oct_tta_update``; ``common.utils.tta_reduce_reference``).
        ``samples`` is the number of views, 1..4; calls go in order of t."""
        out = self._mc_out(probs, ws, mean_probs, argmax, entropy, mutual_info)
        B, H, W, Cn = probs.shape
        _hip.call("oct_tta_update", self.device, probs.data_ptr(), B, H, W, Cn, _view_code(view), int(t), int(samples),
                  ws.data_ptr(), ws.numel(), C.byref(out), self._stream())

    # ---- inference hipGraph ------------------------------------------------------------------------
    def graph_launch(self):
        self._call("oct_unet_graph_launch", self._stream())

    # ---- post-step on device ---------------------------------------------------------------------
    def boundary_maps(self, labels: torch.Tensor, bg_ilm: bool = True, bg_csi: bool = False) -> torch.Tensor:
        """(B,H,W) uint8 class maps (e.g. the arg-max output) -> (B, num_classes-1, H, W) uint8 boundary maps."""
        _hip.expect(labels, "labels (B,H,W)", device=self.device, dtype=torch.uint8, shape=(None, None, None))
        return self._maps("oct_boundary_maps", labels, bg_ilm, bg_csi)

    def boundary_maps_soft(self, probs: torch.Tensor, bg_ilm: bool = True, bg_csi: bool = False) -> torch.Tensor:
        """(B,H,W,num_classes) float32 class probabilities (the forward's ``probs``) -> (B, num_classes-1, H, W) uint8
        soft boundary maps: ``convert_predictions_to_maps_semantic`` of the probabilities themselves
        (``oct_boundary_maps_soft``; ``common.utils.soft_boundary_maps_reference`` restates it)."""
        _hip.expect(probs, "probs (B,H,W,C)", device=self.device, dtype=torch.float32, shape=(None, None, None, self.cfg.n_cls))
        return self._maps("oct_boundary_maps_soft", probs, bg_ilm, bg_csi)

    def _maps(self, name: str, src: torch.Tensor, bg_ilm: bool, bg_csi: bool) -> torch.Tensor:
        B, H, W = src.shape[:3]
        out = torch.empty((B, self.cfg.n_cls - 1, H, W), dtype=torch.uint8, device=self.device)
        _hip.call(name, self.device, src.data_ptr(), B, H, W, self.cfg.n_cls, int(bg_ilm), int(bg_csi), out.data_ptr(),
                  self._stream())
        return out

    def augment(self, x_u8: torch.Tensor, labels: Optional[torch.Tensor], ops, seed: int, out=None):
        """The training augmentations on the device (``oct_augment_batch``): (B,H,W,C) uint8 images, (B,H,W[,1]) uint8
        labels or ``None`` and one ``common.augmentation.AUG_OP_DTYPE`` descriptor per sample -> ``(x float32 in [0,1],
        labels uint8)`` (flipped alongside; ``None`` without labels).  ``ops``: a numpy descriptor array (validated, then
        uploaded) or a uint8 device tensor of B*32 bytes that already holds validated descriptors.  ``out``: optional
        ``(x_out, labels_out)`` tensors to write into.  Asynchronous on the current stream."""
        from .common.augmentation import AUG_OP_DTYPE, AUG_SP
        def check(ops, H, W):
            if ops["kind"].min() < 0 or ops["kind"].max() > AUG_SP:
                raise ValueError("augment: descriptor kind outside 0..5")
        ops, x_out, lab_out = self._stage_io("augment", x_u8, labels, ops, "AUG_OP_DTYPE", AUG_OP_DTYPE, check, out, torch.float32)
        _hip.call("oct_augment_batch", self.device, x_u8.data_ptr(), _ptr(labels), ops.data_ptr(), *x_u8.shape,
                  int(seed) & 0xFFFFFFFFFFFFFFFF, x_out.data_ptr(), _ptr(lab_out), self._stream())
        return x_out, lab_out

    def warp(self, x_u8: torch.Tensor, labels: Optional[torch.Tensor], ops, out=None):
        """The geometric augmentations on the device (``oct_warp_batch``): (B,H,W,C) uint8 images, (B,H,W[,1]) uint8 labels
        or ``None`` and one ``common.augmentation.WARP_OP_DTYPE`` descriptor per sample -> ``(images uint8, labels uint8)``
        (moved alongside; ``None`` without labels), the input of ``augment``.  ``ops``: a numpy descriptor array (validated
        with ``check_warp_ops``, then uploaded) or a uint8 device tensor of B*40 bytes that already holds validated
        descriptors.  ``out``: optional ``(x_out, labels_out)`` tensors to write into; the stage gathers, so neither may
        be an input.  Asynchronous on the current stream."""
        from .common.augmentation import WARP_OP_DTYPE, check_warp_ops
        ops, x_out, lab_out = self._stage_io("warp", x_u8, labels, ops, "WARP_OP_DTYPE", WARP_OP_DTYPE, check_warp_ops, out, torch.uint8)
        _hip.call("oct_warp_batch", self.device, x_u8.data_ptr(), _ptr(labels), ops.data_ptr(), *x_u8.shape, x_out.data_ptr(),
                  _ptr(lab_out), self._stream())
        return x_out, lab_out

    def elastic(self, x_u8: torch.Tensor, labels: Optional[torch.Tensor], ops, out=None):
        """The elastic deformation on the device (``oct_elastic_batch``): (B,H,W,C) uint8 images, (B,H,W[,1]) uint8 labels
        or ``None`` and one ``common.augmentation.ELASTIC_OP_DTYPE`` descriptor per sample -> ``(images uint8, labels uint8)``
        (moved alongside; ``None`` without labels), the input of ``warp`` or ``augment``.  ``ops`` and ``out`` as for ``warp``
        (validated with ``check_elastic_ops``; B*40 descriptor bytes).  Asynchronous on the current stream."""
        from .common.augmentation import ELASTIC_OP_DTYPE, check_elastic_ops
        ops, x_out, lab_out = self._stage_io("elastic", x_u8, labels, ops, "ELASTIC_OP_DTYPE", ELASTIC_OP_DTYPE, check_elastic_ops,
                                             out, torch.uint8)
        _hip.call("oct_elastic_batch", self.device, x_u8.data_ptr(), _ptr(labels), ops.data_ptr(), *x_u8.shape, x_out.data_ptr(),
                  _ptr(lab_out), self._stream())
        return x_out, lab_out

    def photometric(self, x_u8: torch.Tensor, ops, out=None) -> torch.Tensor:
        """The photometric augmentation on the device (``oct_photo_batch``): (B,H,W,C) uint8 images and one
        ``common.augmentation.PHOTO_OP_DTYPE`` descriptor per sample -> uint8 images of the same shape through each sample's
        blur, shadows and intensity table; labels never change, so the call takes none.  ``ops``: a numpy descriptor array
        (validated with ``check_photo_ops``, then uploaded) or a uint8 device tensor of B*320 bytes that already holds
        validated descriptors.  ``out``: optional tensor to write into, never ``x_u8`` itself (the blur gathers).
        Asynchronous on the current stream."""
        from .common.augmentation import PHOTO_OP_DTYPE, check_photo_ops
        ops, x_out, _ = self._stage_io("photometric", x_u8, None, ops, "PHOTO_OP_DTYPE", PHOTO_OP_DTYPE, check_photo_ops,
                                       None if out is None else (out, None), torch.uint8)
        _hip.call("oct_photo_batch", self.device, x_u8.data_ptr(), ops.data_ptr(), *x_u8.shape, x_out.data_ptr(), self._stream())
        return x_out

    def _stage_io(self, what, x_u8, labels, ops, op_name, op_dtype, check, out, x_dtype):
        """``augment`` / ``warp`` / ``elastic`` / ``photometric`` (``what``): validates images, labels, descriptors (a numpy array: also by ``check(ops, H, W)``, then
        uploaded) and ``out``, and makes what of it is missing.  Returns ``(descriptor bytes, x_out, labels_out or None)``."""
        u8 = dict(device=self.device, dtype=torch.uint8)
        _hip.expect(x_u8, f"{what}: images (B,H,W,C)", shape=(None, None, None, None), **u8)
        B, H, W, _ = x_u8.shape
        if labels is not None:
            _hip.expect(labels, f"{what}: labels (B,H,W[,1])", numel=B * H * W, **u8)
        if isinstance(ops, np.ndarray):
            if ops.dtype != op_dtype or ops.shape != (B,):
                raise OctError(f"{what}: ops must hold one {op_name} descriptor per sample")
            try:
                check(ops, H, W)
            except ValueError as e:
                raise OctError(str(e)) from None
            ops = torch.from_numpy(np.ascontiguousarray(ops).view(np.uint8).copy()).to(self.device)
        _hip.expect(ops, f"{what}: ops (B*{op_dtype.itemsize} descriptor bytes)", numel=B * op_dtype.itemsize, **u8)
        x_out, lab_out = out if out is not None else (None, None)
        x_out = torch.empty(x_u8.shape, dtype=x_dtype, device=self.device) if x_out is None else x_out
        lab_out = None if labels is None else torch.empty_like(labels) if lab_out is None else lab_out
        _hip.expect(x_out, f"{what}: out[0]", device=self.device, dtype=x_dtype, shape=tuple(x_u8.shape))
        if labels is not None:
            _hip.expect(lab_out, f"{what}: out[1]", numel=labels.numel(), **u8)
        return ops, x_out, lab_out

    # ---- pad and crop: scans whose size is no multiple of 2^pool_layers ------------------------------
    def pad(self, x: torch.Tensor, Hp: int, Wp: int, top: int, left: int, mode: str, value=0, out=None) -> torch.Tensor:
        """(B,H,W,ch) uint8 or float32 -> (B,Hp,Wp,ch) of the same type with ``x`` at (top, left) and the frame filled by
        ``mode`` -- ``"edge"``, ``"reflect"`` or ``"constant"`` (``value``) -- on the device (``oct_pad_batch``;
        ``common.utils.pad_reference`` restates it).  ``out``: optional tensor to write into.  Asynchronous on the
        current stream."""
        _hip.expect(x, "pad: x (B,H,W,ch)", device=self.device, dtype=(torch.uint8, torch.float32), shape=(None, None, None, None))
        if mode not in _hip.PAD_MODES:
            raise OctError(f'pad: mode must be "edge", "reflect" or "constant", not {mode!r}')
        B, H, W, ch = x.shape
        if out is None:
            out = torch.empty((B, int(Hp), int(Wp), ch), dtype=x.dtype, device=self.device)
        _hip.expect(out, "pad: out", device=self.device, dtype=x.dtype, shape=(B, int(Hp), int(Wp), ch))
        _hip.call("oct_pad_batch", self.device, x.data_ptr(), int(x.dtype == torch.uint8), B, H, W, ch, int(Hp), int(Wp), int(top),
                  int(left), _hip.PAD_MODES[mode], float(value), out.data_ptr(), self._stream())
        return out

    def crop(self, t: torch.Tensor, H: int, W: int, top: int, left: int, out=None) -> torch.Tensor:
        """(B,Hp,Wp[,C]) uint8 or float32 -> its (B,H,W[,C]) window at (top, left), on the device (``oct_crop_batch``, one
        byte-generic kernel; ``common.utils.crop_reference`` restates it).  ``out``: optional tensor to write into.
        Asynchronous on the current stream."""
        if t.dim() not in (3, 4):
            raise OctError(f"crop: t must be (B,Hp,Wp) or (B,Hp,Wp,C), not {tuple(t.shape)}")
        _hip.expect(t, "crop: t (B,Hp,Wp[,C])", device=self.device, dtype=(torch.uint8, torch.float32), shape=(None,) * t.dim())
        B, Hp, Wp = t.shape[:3]
        shape = (B, int(H), int(W)) + tuple(t.shape[3:])
        if out is None:
            out = torch.empty(shape, dtype=t.dtype, device=self.device)
        _hip.expect(out, "crop: out", device=self.device, dtype=t.dtype, shape=shape)
        pb = t.element_size() * int(np.prod(t.shape[3:], dtype=np.int64))
        k = pb // 4 if pb > 32 and pb % 4 == 0 else 1      # the call takes pixels of up to 32 bytes: wider ones go as 4-byte pixels
        _hip.call("oct_crop_batch", self.device, t.data_ptr(), B, Hp, Wp * k, pb // k,
                  int(H), int(W) * k, int(top), int(left) * k, out.data_ptr(), self._stream())
        return out

    # ---- contrast normalisation: CLAHE / percentile stretch of uint8 scans ---------------------------
    def contrast(self, x_u8: torch.Tensor, spec, out=None, ws=None) -> torch.Tensor:
        """(B,H,W,ch) uint8, ch in 1..4 -> the same shape through the contrast stage ``spec`` (``common.utils.check_contrast``'s
        dict) on the device (``oct_contrast_batch``; ``common.utils.contrast_reference`` gives the same bytes).  Any image
        size up to 4096 x 4096 whose tiles keep 8 x 8 pixels.  ``out``: optional tensor to write into; it may be ``x_u8``
        itself.  ``ws``: optional uint8 workspace (``oct_contrast_workspace_bytes``), else one kept in the engine's buffer
        set of this batch size; its first B*ch*ty*tx*256 bytes are the look-up tables after the call.  Asynchronous on the
        current stream."""
        from .common.utils import check_contrast, contrast_desc
        _hip.expect(x_u8, "contrast: x (B,H,W,ch)", device=self.device, dtype=torch.uint8, shape=(None, None, None, None))
        B, H, W, ch = x_u8.shape
        try:
            s = check_contrast(spec, hw=(H, W))
            if s is None:
                raise ValueError("contrast: the spec is None (off)")
        except ValueError as e:
            raise OctError(str(e)) from None
        desc = contrast_desc(s)
        d = _hip.ContrastDesc(*desc)
        need = int(_hip.lib().oct_contrast_workspace_bytes(B, H, W, ch, C.byref(d)))
        if not need:
            raise OctError(f"contrast: unsupported shape {tuple(x_u8.shape)}: need 1 <= B <= 65535 and 1..4 channels")
        if ws is None:
            ws = self._buf(B, ("contrast_ws", H, W, ch) + desc[:3], (need,), torch.uint8)
        _hip.expect(ws, "contrast: workspace", device=self.device, dtype=torch.uint8, shape=(None,))
        if out is None:
            out = torch.empty_like(x_u8)
        _hip.expect(out, "contrast: out", device=self.device, dtype=torch.uint8, shape=tuple(x_u8.shape))
        _hip.call("oct_contrast_batch", self.device, x_u8.data_ptr(), B, H, W, ch, C.byref(d), ws.data_ptr(), ws.numel(),
                  out.data_ptr(), self._stream())
        return out

    # ---- weights exchange --------------------------------------------------------------------------
    def get_weights(self) -> List[np.ndarray]:
        """Keras ``get_weights()`` order: Conv2D [kernel HWIO, bias]; BN [gamma, beta, moving_mean, moving_var]."""
        p = self.params.cpu().numpy(); s = self.state.cpu().numpy()
        out = []
        for L in self.layers:
            n = L["kh"] * L["kw"] * L["cin"] * L["cout"]; c = L["cout"]
            out.append(p[L["kernel_off"]:L["kernel_off"] + n].reshape(L["kh"], L["kw"], L["cin"], c).copy())
            out.append(p[L["bias_off"]:L["bias_off"] + c].copy())
            if L["has_bn"]:
                out += [p[L["gamma_off"]:L["gamma_off"] + c].copy(), p[L["beta_off"]:L["beta_off"] + c].copy(),
                        s[L["moving_mean_off"]:L["moving_mean_off"] + c].copy(), s[L["moving_var_off"]:L["moving_var_off"] + c].copy()]
        return out

    def set_weights(self, weights: Sequence[np.ndarray]):
        p = np.empty(self.n_params, np.float32); s = np.empty(self.n_state, np.float32)
        it = iter(weights)
        try:
            for L in self.layers:
                n = L["kh"] * L["kw"] * L["cin"] * L["cout"]; c = L["cout"]
                k = np.asarray(next(it), np.float32)
                if k.shape != (L["kh"], L["kw"], L["cin"], c):
                    raise OctError(f"{L['name']}: kernel shape {k.shape} != {(L['kh'], L['kw'], L['cin'], c)}")
                p[L["kernel_off"]:L["kernel_off"] + n] = k.ravel()
                p[L["bias_off"]:L["bias_off"] + c] = np.asarray(next(it), np.float32)
                if L["has_bn"]:
                    p[L["gamma_off"]:L["gamma_off"] + c] = np.asarray(next(it), np.float32)
                    p[L["beta_off"]:L["beta_off"] + c] = np.asarray(next(it), np.float32)
                    s[L["moving_mean_off"]:L["moving_mean_off"] + c] = np.asarray(next(it), np.float32)
                    s[L["moving_var_off"]:L["moving_var_off"] + c] = np.asarray(next(it), np.float32)
        except StopIteration:
            raise OctError("set_weights: too few arrays") from None
        if next(it, None) is not None:
            raise OctError("set_weights: too many arrays")
        self.params.copy_(torch.from_numpy(p)); self.state.copy_(torch.from_numpy(s))

    def debug_bn_record(self, layer: int) -> torch.Tensor:
        """The (9, cout) f32 BN record of ``layer``: rows a, b, mean, rstd (consumers apply relu(a*z + b) on load), c1, c2
        (BN-backward means) and ga, gb, gd (the BN-backward transform dz = ga*g' + gb*z + gd)."""
        ptr = _hip.lib().oct_unet_debug_activation(self._h, layer, 2)
        if not ptr:
            raise OctError("no BN record for this layer")
        c = self.layers[layer]["cout"]
        off = ptr - self.workspace.data_ptr()
        return self.workspace[off:off + 4 * 9 * c].view(torch.float32).view(9, c)

    def debug_layer_fused(self, layer: int) -> bool:
        """True if, in the last backward, the layer's BN-backward transform was applied on load by its consumers: its
        gradient buffer (``debug_activation(layer, 1)``) then holds the masked gradient g', not dz."""
        r = _hip.lib().oct_unet_debug_layer_fused(self._h, layer)
        if r < 0:
            raise OctError("no such layer")
        return bool(r)

    def debug_dz(self, layer: int) -> torch.Tensor:
        """dz of ``layer`` after a backward, float64: the gradient buffer itself where the stand-alone BN-backward pass
        ran, else the transform of the stored g' and z with the record's rows (what the consumers formed on load)."""
        g = self.debug_activation(layer, 1).double()
        if not self.debug_layer_fused(layer):
            return g
        rec = self.debug_bn_record(layer).double()
        return rec[6] * g + (rec[7] * self.debug_activation(layer, 0).double() + rec[8])

    def set_option(self, name: str, value: int) -> None:
        """Edit this handle's copy of a tuning / arithmetic option (``_hip.set_option`` edits the defaults new handles copy)."""
        _hip.check(_hip.lib().oct_unet_set_option(self._h, name.encode(), int(value)), f"oct_unet_set_option({name})")

    def handle_option(self, name: str) -> int:
        """The value of a tuning option as this handle snapshotted it at creation."""
        v = C.c_int(0)
        _hip.check(_hip.lib().oct_unet_get_option(self._h, name.encode(), C.byref(v)), f"oct_unet_get_option({name})")
        return int(v.value)

    def debug_activation(self, layer: int, which: int = 0) -> torch.Tensor:
        """A layer's saved pre-BN output (which=0) or gradient buffer (which=1), max_batch-sized; a float32 view in
        f32 mode, a float32 COPY of the bf16 storage in bf16 mode."""
        ptr = _hip.lib().oct_unet_debug_activation(self._h, layer, which)
        if not ptr:
            raise OctError("no such activation")
        L = self.layers[layer]
        n = self.cfg.max_batch * L["out_h"] * L["out_w"] * L["cout"]
        off = ptr - self.workspace.data_ptr()
        shape = (self.cfg.max_batch, L["out_h"], L["out_w"], L["cout"])
        if self.cfg.dtype == 1:
            return self.workspace[off:off + 2 * n].view(torch.bfloat16).view(shape).float()
        return self.workspace[off:off + 4 * n].view(torch.float32).view(shape)
