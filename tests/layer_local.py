"""Layer-local fp64 model of one engine step -- test helper, not a conftest.

Every layer is recomputed in float64 FROM THE ENGINE'S OWN STORED INPUTS (pre-BN outputs z, the BN records, the
gradient buffers, the probabilities), so a flipped ReLU mask or pool route upstream cannot spread: each kernel is held to
its own rounding on every element.  Written in torch float64 (matmuls and elementwise ops only, never a project kernel),
so it runs on the CPU for the small tests and on the device at the benched sizes; the batch is processed in chunks of at
most ``chunk`` images while dW, the batch statistics and the BN-backward means are summed in fp64 over the whole batch.

Two arithmetic models:

* ``"f32"`` -- the engine's fp32 mode.  A stored value may differ from the fp64 recomputation by what its accumulation
  can round: ``|err| <= GAMMA * (|x| (*) |w|) + tiny`` per element, where ``|x| (*) |w|`` is the same conv on absolute
  values (the operand magnitudes include the fp32 affine ``a z + b`` before its ReLU, and the three terms of a dz formed
  on load).  Elements whose ReLU mask or pool route is decided within fp32 rounding are excluded explicitly and counted.
* ``"bf16"`` -- the bf16-storage mode: the rounding rules of ``test_bf16_storage_layer_local_rounding_is_exact`` (one
  bf16 rounding per stored tensor and per MFMA operand, mirrored from the host rules in csrc/oct_unet.hip) and its
  one-rounding bounds, applied per layer and per image.  The engine takes every batch statistic (BN mean / variance, the
  BN-backward means, beta and gamma gradients) of its fp32 accumulators BEFORE the storage rounding, so the model sums its
  own unrounded recomputation, not the stored roundings (the two differ by the mean of N rounding errors: nothing at a
  full-size layer, more than the record gates at a 4 x 8 bottleneck).  A stored intermediate (the pooled gradient, the
  raw skip half) whose fp64 value lies within the fp32 accumulation error of a bf16 rounding midpoint may be stored as
  the other neighbour: such an element adds one ulp of that intermediate to the hard bound of the g' it feeds.

``LayerLocal(...).run()`` returns a ``Report``: one row per layer (the worst err/bound of every gate, printed as the
per-layer table) and a list of failures, each naming the layer, the image and the first failing coordinates.
"""
from __future__ import annotations

import dataclasses
from typing import Dict, List, Optional

import numpy as np
import torch
import torch.nn.functional as F

from oracle import unet_numpy as on

U32 = 2.0 ** -24           # fp32 unit roundoff
GAMMA = 2.0 ** -17         # fp32 per-element gate on z, g' and dz: 128 u of the absolute-value accumulation
# fp32 tensor relative L2 gate on z, g' and dz.  Its margin is NOT 3x, by arithmetic: an output of a K = 9 Cin term conv
# on the bf16 pipe takes 6 MFMAs per 16-deep K slice (the exact 3-term split), each adding exact
# products into the fp32 accumulator with one rounding, so n = 6 K / 16 roundings of a running sum of the size of the
# result: relative L2 ~ u sqrt(n / 3).  The widest layers (K = 9 x 128 = 1152: dec0.conv0 and mid.conv1 forward, the
# backward-data into mid.conv0 and enc3.conv1) have n = 432 and an estimate of 7.2e-7; measured 4.7e-7 .. 5.7e-7 (1.8x -
# 2.1x below the gate); K = 576 layers (estimate 5.1e-7) measure <= 3.8e-7, narrower ones less.  A different summation order keeps n and the estimate; a change that raises
# the roundings per output (shorter K slices, more split terms) moves the estimate toward 1e-6 and needs re-measuring.
REL_L2 = 1e-6
REL_L2_RATIO = 1.39        # REL_L2 over that estimate at K = 1152: what the gate allows above u sqrt(n / 3)


def rel_l2_gate(K):
    """The relative L2 gate of a tensor whose elements accumulate K terms: REL_L2 up to K = 1152, beyond that the same
    ratio over the same estimate u sqrt(n / 3), n = 6 K / 16 (start_neurons 20 .. 28: K up to 9 x 448)."""
    return max(REL_L2, REL_L2_RATIO * U32 * (6.0 * K / 16.0 / 3.0) ** 0.5)
PARAM_RTOL = 2e-5          # fp32 dW / bias / gamma / beta, relative to the tensor's scale
REC_RTOL = 1e-5            # fp32 BN record rows
EXCLUDE_MAX = 1e-5         # share of the elements the fp32 mask / route exclusions may remove
TINY = 1e-30


# ---- bf16 rounding rules (numpy; shared with tests/test_gpu_parity.py) ----------------------------------------------

def bf16_round(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.bfloat16).double().numpy()


def bf16_ulp(a):
    """Spacing of bf16 numbers at |a| (8 significant bits)."""
    return 2.0 ** (np.floor(np.log2(np.maximum(np.abs(a), 1e-30))) - 7)


# ---- which arithmetic a layer runs in bf16 mode (dtype=1): mirror of the host rules (csrc/host.hpp: pipe_fit;
# csrc/oct_unet.hip: conv_route, dw_plan).  On the bf16 MFMA pipe (mfma_mode 1, the default) BOTH operands of a
# product are bf16: the activation is rounded once more after BN + ReLU (dz operands are stored bf16 already: exact)
# and the weights are rounded per step; accumulation stays fp32.  Layers outside those rules (first layer, head,
# channel counts that are not multiples of 8, mfma_mode 0) multiply the stored bf16 values with fp32 weights. ----
def _bt_k(k):
    return k in (8, 16, 32)


def bf16_fwd_operands(plan, li, cfg, mfma_mode, training=True):
    sp = plan[li]
    if not mfma_mode or sp.src == "input" or not sp.has_bn:
        return False
    drop = training and sp.name == "dec0.up" and cfg.dropout_rate > 0      # (conv_forward: dropout only in a training forward)
    two_ok = sp.src != "concat" or plan[li - 1].cout % 8 == 0
    thin = sp.cout <= 16 and sp.cout % 4 == 0 and _bt_k(sp.cin) and not drop and two_ok
    wide = sp.cout % 32 == 0 and sp.cin % 8 == 0 and sp.cin <= 512 and two_ok
    return thin or wide


def bf16_dx_weights(plan, li, mfma_mode):
    sp = plan[li]
    if not mfma_mode or sp.src == "input" or not sp.has_bn:
        return False
    cg = sp.cin // 2 if sp.src == "concat" else sp.cin
    wide = cg % 32 == 0 and sp.cout % 8 == 0 and sp.cout <= 512
    thin = cg <= 16 and cg % 4 == 0 and (sp.cout == 8 if sp.src == "up" else _bt_k(sp.cout))
    return wide or thin


def bf16_dw_operands(plan, li, mfma_mode):
    sp = plan[li]
    if not mfma_mode or sp.src == "input" or sp.kh == 1 or not sp.has_bn:
        return False
    if sp.cin % 32 == 0 and sp.cout % 32 == 0:                               # conv_dwbx_k
        return True
    pair = (sp.cin, sp.cout)                                                  # conv_dwbt_k's instantiated shapes
    if sp.src == "up":
        return pair in ((16, 8), (32, 16))
    if sp.src == "concat" and (sp.cin // 2) % 8:
        return False
    return pair in ((8, 8), (8, 16), (16, 8), (16, 16), (16, 32), (32, 16))


def upconv_dx_effective(dz, kernel, round_w):
    """Backward-data of UpSampling2D(2) -> Conv2D(2x2, same) as the engine forms it (prep_wt_k mode 1 + A_DOWN2): a 3x3
    stride-2 gather over dz with effective weights Weff[a][b] = sum of the 2x2 taps that reach that offset; the
    EFFECTIVE weights are what the bf16 pipe rounds."""
    B, H2, W2, Co = dz.shape
    Ci = kernel.shape[2]
    Hl, Wl = H2 // 2, W2 // 2
    sel = {0: (1,), 1: (0, 1), 2: (0,)}
    dzp = np.zeros((B, H2 + 2, W2 + 2, Co)); dzp[:, 1:H2 + 1, 1:W2 + 1] = dz      # index 2y - 1 + a  ->  2y + a
    out = np.zeros((B, Hl, Wl, Ci))
    for a in range(3):
        for b in range(3):
            weff = sum(kernel[ky, kx] for ky in sel[a] for kx in sel[b])         # (Ci, Co)
            if round_w:
                weff = bf16_round(weff.astype(np.float32))                         # prep_wt_k sums in fp32, prep_wb*_k rounds
            out += np.einsum("bhwo,io->bhwi", dzp[:, a:a + 2 * Hl:2, b:b + 2 * Wl:2], weff)
    return out


# ---- torch float64 primitives (NHWC) ---------------------------------------------------------------------------------

def t_bf16(t):
    """Round to bf16 the way the engine stores (fp32 value, round to nearest even), returned as float64."""
    return t.float().to(torch.bfloat16).double()


def t_bf16_ulp(t):
    return torch.exp2(torch.floor(torch.log2(t.abs().clamp_min(1e-30))) - 7)


def t_bf16_may_flip(x, mag):
    """Where the device's fp32 value of x (an accumulation of magnitude ``mag``, within GAMMA * mag of this fp64 one: the
    fp32 gate on the same sums) may round to the other bf16 neighbour: x lies that close to a rounding midpoint."""
    q = t_bf16(x)
    return (0.5 * t_bf16_ulp(q) - (x - q).abs()).abs() <= GAMMA * mag


def t_conv(x, k):
    """Conv2D 'same' at stride 1, HWIO kernel, no bias."""
    kh, kw, ci, co = k.shape
    B, H, W, _ = x.shape
    (pt, pb), (pl, pr) = on.same_pad(kh), on.same_pad(kw)
    xp = F.pad(x, (0, 0, pl, pr, pt, pb))
    out = torch.zeros((B, H, W, co), dtype=x.dtype, device=x.device)
    for ky in range(kh):
        for kx in range(kw):
            out += xp[:, ky:ky + H, kx:kx + W, :] @ k[ky, kx]
    return out


def t_conv_dx(dz, k):
    kh, kw, ci, co = k.shape
    B, H, W, _ = dz.shape
    (pt, pb), (pl, pr) = on.same_pad(kh), on.same_pad(kw)
    gxp = torch.zeros((B, H + kh - 1, W + kw - 1, ci), dtype=dz.dtype, device=dz.device)
    for ky in range(kh):
        for kx in range(kw):
            gxp[:, ky:ky + H, kx:kx + W, :] += dz @ k[ky, kx].T
    return gxp[:, pt:pt + H, pl:pl + W, :]


def t_conv_dw(x, dz, kh, kw):
    B, H, W, ci = x.shape
    co = dz.shape[-1]
    (pt, pb), (pl, pr) = on.same_pad(kh), on.same_pad(kw)
    xp = F.pad(x, (0, 0, pl, pr, pt, pb))
    n = B * H * W
    s = 256                                   # split the pixel sum: a (ci x n)(n x co) product with n in the millions
    while n % s:
        s //= 2
    d3 = dz.reshape(s, n // s, co)
    dk = torch.empty((kh, kw, ci, co), dtype=x.dtype, device=x.device)
    for ky in range(kh):
        for kx in range(kw):
            x3 = xp[:, ky:ky + H, kx:kx + W, :].reshape(s, n // s, ci)
            dk[ky, kx] = torch.bmm(x3.transpose(1, 2), d3).sum(0)
    return dk


def t_upconv_weff(k, round_w):
    """The nine (Ci, Co) effective weights of the up layer's backward-data (see upconv_dx_effective)."""
    sel = {0: (1,), 1: (0, 1), 2: (0,)}
    out = {}
    for a in range(3):
        for b in range(3):
            w = sum(k[ky, kx] for ky in sel[a] for kx in sel[b])
            out[a, b] = t_bf16(w) if round_w else w
    return out


def t_upconv_dx(dz, weff):
    B, H2, W2, Co = dz.shape
    Ci = weff[0, 0].shape[0]
    Hl, Wl = H2 // 2, W2 // 2
    dzp = F.pad(dz, (0, 0, 1, 1, 1, 1))
    out = torch.zeros((B, Hl, Wl, Ci), dtype=dz.dtype, device=dz.device)
    for a in range(3):
        for b in range(3):
            out += dzp[:, a:a + 2 * Hl:2, b:b + 2 * Wl:2, :] @ weff[a, b].T
    return out


def t_upsample(x):
    return x.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)


def _windows(x):
    B, H, W, C = x.shape
    return x.reshape(B, H // 2, 2, W // 2, 2, C).permute(0, 1, 3, 5, 2, 4).reshape(B, H // 2, W // 2, C, 4)


def _unwindows(w):
    B, h, ww, C, _ = w.shape
    return w.reshape(B, h, ww, C, 2, 2).permute(0, 1, 4, 2, 5, 3).reshape(B, 2 * h, 2 * ww, C)


def t_maxpool(x):
    return _windows(x).amax(dim=-1)


def t_pool_route(x, g):
    """Gradient g of the pooled tensor to the first maximum of each 2x2 window of x (row-major scan)."""
    xw = _windows(x)
    idx = xw.argmax(dim=-1, keepdim=True)
    gw = torch.zeros_like(xw).scatter_(-1, idx, g.unsqueeze(-1))
    return _unwindows(gw)


def t_pool_near_tie(x, mag, k):
    """Per input element: its window's two largest values (the larger > 0) lie within k fp32 roundings of the window's
    largest operand magnitude -- the route the device takes there is decided by rounding."""
    top = _windows(x).topk(2, dim=-1).values
    tol = k * U32 * _windows(mag).amax(dim=-1)
    tie = (top[..., 0] - top[..., 1] <= tol) & (top[..., 0] > 0)
    return _unwindows(tie.unsqueeze(-1).expand(*tie.shape, 4).contiguous())


# ---- stored tensors --------------------------------------------------------------------------------------------------

@dataclasses.dataclass
class Stored:
    """What an engine holds after one step (any float dtype, any device; sliced per chunk).

    z[li]     pre-BN output of every BN layer (B, H, W, cout)
    rec[li]   BN record (9, cout): a, b, mean, rstd, c1, c2, ga, gb, gd (training only)
    gbuf[li]  gradient buffer: the masked gradient g' where fused[li], else dz (training only)
    probs     (B, H, W, C) probabilities
    grads[li] dict kernel (HWIO) / bias / gamma / beta (training only)
    argmax    (B, H, W) class map (optional)"""
    z: list
    probs: object
    rec: Optional[list] = None
    gbuf: Optional[list] = None
    fused: Optional[list] = None
    grads: Optional[list] = None
    argmax: object = None


def engine_grads(eng):
    """The gradient buffer of a UNetEngine as one dict per layer (kernel HWIO, bias, gamma, beta), float64 numpy."""
    g = eng.grads.detach().double().cpu().numpy()
    grads = []
    for L in eng.layers:
        n = L["kh"] * L["kw"] * L["cin"] * L["cout"]
        d = {"kernel": g[L["kernel_off"]:L["kernel_off"] + n].reshape(L["kh"], L["kw"], L["cin"], L["cout"]),
             "bias": g[L["bias_off"]:L["bias_off"] + L["cout"]]}
        if L["has_bn"]:
            d["gamma"] = g[L["gamma_off"]:L["gamma_off"] + L["cout"]]
            d["beta"] = g[L["beta_off"]:L["beta_off"] + L["cout"]]
        grads.append(d)
    return grads


def engine_stored(eng, B, probs, training=True, argmax=None):
    """Stored tensors of a UNetEngine after a forward (+ backward when ``training``)."""
    nb = len(eng.layers) - 1
    z = [eng.debug_activation(li, 0)[:B] for li in range(nb)]
    if not training:
        return Stored(z=z, probs=probs, argmax=argmax)
    grads = engine_grads(eng)
    return Stored(z=z, probs=probs, rec=[eng.debug_bn_record(li).clone() for li in range(nb)],
                  gbuf=[eng.debug_activation(li, 1)[:B] for li in range(nb)],
                  fused=[bool(eng.debug_layer_fused(li)) for li in range(nb)], grads=grads, argmax=argmax)


# ---- gates and report ------------------------------------------------------------------------------------------------

class Report:
    def __init__(self):
        self.rows: Dict[str, Dict[str, float]] = {}
        self.failures: List[str] = []
        self.excluded = 0
        self.elements = 0
        self.times: Dict[str, float] = {}

    def note(self, layer, key, value):
        r = self.rows.setdefault(layer, {})
        r[key] = max(r.get(key, 0.0), float(value))

    def fail(self, msg):
        self.failures.append(msg)

    def table(self):
        keys = []
        for r in self.rows.values():
            keys += [k for k in r if k not in keys]
        lines = ["layer         " + " ".join(f"{k:>11s}" for k in keys)]
        for name, r in self.rows.items():
            lines.append(f"{name:13s} " + " ".join(f"{r[k]:11.3e}" if k in r else f"{'-':>11s}" for k in keys))
        lines.append(f"excluded (mask / route decided within fp32 rounding): {self.excluded} of {self.elements} elements")
        if self.times:
            lines.append("model time: " + ", ".join(f"{k} {v:.1f} s" for k, v in self.times.items()))
        return "\n".join(lines)


def _first(mask):
    idx = torch.nonzero(mask)[0].tolist()
    return idx


class ElementGate:
    """Per-element gate of one tensor of one layer, fed chunk by chunk."""

    def __init__(self, rep, layer, what, mode, excl_ok=False, rel_l2=REL_L2):
        self.rep, self.layer, self.what, self.mode, self.rel_l2 = rep, layer, what, mode, rel_l2
        self.sq_err = self.sq_ref = 0.0
        self.worst = 0.0
        self.failed = False
        self.excl_ok = excl_ok

    def _fail(self, msg):
        if not self.failed:
            self.rep.fail(f"{self.layer} {self.what}: {msg}")
            self.failed = True

    def f32(self, lo, got, ref, bound, excl=None):
        err = (got - ref).abs()
        if excl is not None:
            n = int(excl.sum())
            self.rep.excluded += n
            err = torch.where(excl, torch.zeros_like(err), err)
        self.rep.elements += err.numel()
        ratio = err / bound.clamp_min(TINY)
        self.worst = max(self.worst, float(ratio.max()))
        self.sq_err += float((err * err).sum()); self.sq_ref += float((ref * ref).sum())
        bad = err > bound
        if bool(bad.any()):
            b, y, x, c = _first(bad)
            self._fail(f"image {lo + b} at (y={y}, x={x}, c={c}): stored {float(got[b, y, x, c]):.9e}, fp64 "
                       f"{float(ref[b, y, x, c]):.9e}, err {float(err[b, y, x, c]):.3e} > bound {float(bound[b, y, x, c]):.3e}")

    def bf16(self, lo, got, ref_rounded, bound, hard):
        """The one-rounding gates per image: (err <= bound) on > 99.9 %, err <= hard everywhere, err == 0 on > 99 %."""
        err = (got - ref_rounded).abs()
        self.rep.elements += err.numel()
        self.worst = max(self.worst, float((err / bound.clamp_min(TINY)).max()))
        self.sq_err += float((err * err).sum()); self.sq_ref += float((ref_rounded * ref_rounded).sum())
        per = err.reshape(err.shape[0], -1)
        within = (per <= bound.reshape(err.shape[0], -1)).double().mean(1)
        exact = (per == 0).double().mean(1)
        self.rep.note(self.layer, f"{self.what}!=0", float((1 - exact).max()))
        for b in range(err.shape[0]):
            over = err[b] > hard[b]
            if bool(over.any()):
                y, x, c = _first(over)
                self._fail(f"image {lo + b} at (y={y}, x={x}, c={c}): err {float(err[b, y, x, c]):.3e} > "
                           f"{float(hard[b, y, x, c]):.3e} (stored {float(got[b, y, x, c]):.6e}, fp64 rounded "
                           f"{float(ref_rounded[b, y, x, c]):.6e})")
            elif within[b] <= 0.999:
                y, x, c = _first(err[b] > bound[b])
                self._fail(f"image {lo + b}: only {float(within[b]):.5f} of the elements within one rounding; first "
                           f"beyond at (y={y}, x={x}, c={c}) err {float(err[b, y, x, c]):.3e}")
            elif exact[b] <= 0.99:
                y, x, c = _first(err[b] != 0)
                self._fail(f"image {lo + b}: only {float(exact[b]):.5f} of the elements identical to the fp64 value "
                           f"rounded once; first different at (y={y}, x={x}, c={c}): stored {float(got[b, y, x, c]):.6e}, "
                           f"fp64 rounded {float(ref_rounded[b, y, x, c]):.6e}")

    def close(self):
        self.rep.note(self.layer, self.what, self.worst)
        if self.mode == "f32" and self.sq_ref > 0:
            rel = (self.sq_err / self.sq_ref) ** 0.5
            self.rep.note(self.layer, f"{self.what}.L2", rel)
            if rel > self.rel_l2:
                self.rep.fail(f"{self.layer} {self.what}: relative L2 {rel:.3e} > {self.rel_l2:.3g}")


def _vec_gate(rep, layer, what, got, ref, bound, labels=None):
    """Gate on a small (per channel / per tap) tensor: got, ref, bound numpy arrays of one shape."""
    err = np.abs(np.asarray(got, np.float64) - ref)
    ratio = err / np.maximum(bound, TINY)
    rep.note(layer, what, float(ratio.max()) if ratio.size else 0.0)
    bad = err > bound
    if bad.any():
        i = tuple(int(v) for v in np.argwhere(bad)[0])
        where = ", ".join(f"{n}={v}" for n, v in zip(labels or ("c",) * len(i), i))
        rep.fail(f"{layer} {what} at ({where}): stored {float(np.asarray(got)[i]):.9e}, fp64 {float(ref[i]):.9e}, "
                 f"err {float(err[i]):.3e} > bound {float(np.asarray(bound)[i]):.3e}")


# ---- the model -------------------------------------------------------------------------------------------------------

class LayerLocal:
    """fp64 layer-local recomputation of one step of the engine.

    cfg, params (fp64 numpy dicts as ``oracle.unet_numpy.init_params``), state (BN moving statistics; used in inference
    only), stored (``Stored``), images (B,H,W,Cin) uint8, labels (B,H,W) (training), dropout_mask (the {0,1} keep-mask;
    training), mode "f32" | "bf16", mfma_mode (bf16 operand rules), macro / loss_scale (the Dice gradient of the step).
    ``keep=True`` keeps every recomputed tensor in ``self.kept`` (small shapes: the CPU tests compare it with the oracle).
    ``wide_rel_l2=True`` lets the fp32 relative L2 gate of a tensor follow its accumulation length (``rel_l2_gate``:
    REL_L2 itself for every K <= 1152, i.e. for every layer of start_neurons <= 16 at four pool levels)."""

    def __init__(self, cfg, params, stored, images, *, training=True, state=None, labels=None, dropout_mask=None,
                 mode="f32", mfma_mode=1, macro=True, loss_scale=1.0, device="cpu", chunk=8, keep=False, wide_rel_l2=False):
        assert mode in ("f32", "bf16") and 1 <= chunk <= 8
        self.cfg, self.plan, self.S = cfg, on.build_plan(cfg), stored
        self.nb = len(self.plan) - 1
        self.training, self.mode, self.mm, self.macro, self.loss_scale = training, mode, mfma_mode, macro, loss_scale
        self.dev, self.chunk, self.keep, self.wide_rel_l2 = torch.device(device), chunk, keep, wide_rel_l2
        self.B = int(images.shape[0])
        self.images = torch.as_tensor(np.asarray(images)).to(self.dev)
        self.labels = None if labels is None else torch.as_tensor(np.asarray(labels)).reshape(self.B, images.shape[1], images.shape[2]).to(self.dev)
        self.mask = None if dropout_mask is None else torch.as_tensor(dropout_mask).to(self.dev, torch.float64)
        self.lut = torch.as_tensor((np.arange(256) / 255.0).astype(np.float32).astype(np.float64), device=self.dev)
        T = lambda a: torch.as_tensor(np.asarray(a, np.float64), device=self.dev)
        self.P = [{k: T(v) for k, v in p.items()} for p in params]
        self.rep = Report()
        self.kept: Dict[str, dict] = {}
        if training:
            self.rec = [T(torch.as_tensor(r).double().cpu().numpy()) for r in stored.rec]
            self.coef = [(r[0], r[1]) for r in self.rec]
        else:
            bi, self.coef = 0, []
            for li in range(self.nb):
                st = state[bi]; bi += 1
                a = self.P[li]["gamma"] / torch.sqrt(T(st["moving_var"]) + cfg.bn_eps)
                self.coef.append((a, self.P[li]["beta"] - a * T(st["moving_mean"])))

    # -- access ---------------------------------------------------------------------------------------------------------
    def _get(self, t, lo, hi):
        return torch.as_tensor(t)[lo:hi].to(self.dev, torch.float64)

    def _chunks(self):
        return [(lo, min(lo + self.chunk, self.B)) for lo in range(0, self.B, self.chunk)]

    def _keep(self, li, key, lo, t):
        if self.keep:
            self.kept.setdefault(self.plan[li].name, {}).setdefault(key, {})[lo] = t.cpu().numpy()

    def kept_tensor(self, name, key):
        d = self.kept[name][key]
        return np.concatenate([d[k] for k in sorted(d)])

    def _rel_l2(self, li, backward):
        """Relative L2 gate of layer li's z (its own K = kh kw cin) or of its g' / dz (the longest backward-data sum of
        its consumers: kh kw cout of the consumer)."""
        if not self.wide_rel_l2:
            return REL_L2
        if not backward:
            sp = self.plan[li]
            return rel_l2_gate(sp.kh * sp.kw * sp.cin)
        cons = [li + 1] + [j for j, s in enumerate(self.plan) if s.src == "concat" and s.skip_from == li]
        return rel_l2_gate(max(self.plan[c].kh * self.plan[c].kw * self.plan[c].cout for c in cons))

    def _drop_layer(self, li):
        return self.training and self.cfg.dropout_rate > 0 and self.plan[li].name == f"mid.conv{self.cfg.conv_layers - 1}"

    def act(self, li, lo, hi):
        """What a consumer forms from layer li's stored z: (relu(a z + b) [x dropout], operand magnitude, alive,
        unsure) -- unsure: the fp32 affine lies within its own rounding of the ReLU kink."""
        a, b = self.coef[li]
        z = self._get(self.S.z[li], lo, hi)
        pre = a * z + b
        mag = (a * z).abs() + b.abs()
        alive = pre > 0
        unsure = pre.abs() <= 2 * U32 * mag
        y = torch.where(alive, pre, torch.zeros_like(pre))
        yabs = torch.where(alive | unsure, mag, torch.zeros_like(mag))
        if self._drop_layer(li):
            d = self.mask[lo:hi] / (1.0 - self.cfg.dropout_rate)
            y, yabs = y * d, yabs * d
        return y, yabs, alive, unsure

    def layer_input(self, li, lo, hi):
        """(input, magnitude) of layer li, recomputed from the stored tensors of its producers."""
        sp = self.plan[li]
        if sp.src == "input":
            x = self.lut[self.images[lo:hi].long()]
            return x, x
        y, yabs, _, _ = self.act(li - 1, lo, hi)
        if sp.src in ("prev", "head"):
            return y, yabs
        if sp.src == "pool":
            p = t_maxpool(y)
            return (t_bf16(p) if self.mode == "bf16" else p), t_maxpool(yabs)
        if sp.src == "up":
            return t_upsample(y), t_upsample(yabs)
        s, sabs, _, _ = self.act(sp.skip_from, lo, hi)
        return torch.cat([y, s], -1), torch.cat([yabs, sabs], -1)

    # -- forward --------------------------------------------------------------------------------------------------------
    def check_forward(self):
        bf = self.mode == "bf16"
        self._zsums = {}
        for li, sp in enumerate(self.plan):
            p = self.P[li]
            rnd = bf and bf16_fwd_operands(self.plan, li, self.cfg, self.mm, self.training)
            w = t_bf16(p["kernel"]) if rnd else p["kernel"]
            if sp.has_bn:
                gate = ElementGate(self.rep, sp.name, "z", self.mode, rel_l2=self._rel_l2(li, False))
                zmax = float(torch.as_tensor(self.S.z[li][:self.B]).abs().max())
            for lo, hi in self._chunks():
                x, xabs = self.layer_input(li, lo, hi)
                z = t_conv(t_bf16(x) if rnd else x, w) + p["bias"]
                self._keep(li, "x", lo, x); self._keep(li, "z", lo, z)
                if sp.has_bn:
                    got = self._get(self.S.z[li], lo, hi)
                    if bf and self.training:   # the engine takes the batch statistics of z BEFORE it rounds z for the store
                        zs = self._zsums.setdefault(li, [0.0, 0.0, 0])
                        zs[0] = zs[0] + z.sum((0, 1, 2)); zs[1] = zs[1] + (z * z).sum((0, 1, 2)); zs[2] += z[..., 0].numel()
                    if bf:
                        bound = 1.001 * t_bf16_ulp(z) + 5e-5 * zmax
                        loose = bound + 2.0 ** -7 * float(xabs.abs().max()) * float(p["kernel"].abs().max())
                        gate.bf16(lo, got, t_bf16(z), bound, loose)
                    else:
                        bound = GAMMA * (t_conv(xabs, p["kernel"].abs()) + p["bias"].abs()) + TINY
                        gate.f32(lo, got, z, bound)
                else:
                    self._check_probs(li, lo, hi, x, xabs, z)
            if sp.has_bn:
                gate.close()

    def _check_probs(self, li, lo, hi, x, xabs, z):
        name = self.plan[li].name
        probs = torch.softmax(z, -1)
        self._keep(li, "probs", lo, probs)
        got = self._get(self.S.probs, lo, hi)
        # the head is fp32 VALU arithmetic in both modes (its input formed from the stored z, its weights unrounded): a
        # logit error within zb moves p_i by at most p_i (|dz_i| + max_j |dz_j|), plus the softmax's own few roundings
        zb = GAMMA * (t_conv(xabs, self.P[li]["kernel"].abs()) + self.P[li]["bias"].abs())
        bound = probs * (2 * zb.amax(-1, keepdim=True) + GAMMA) + 1e-12
        g = getattr(self, "_pgate", None)
        if g is None or g.layer != name:
            g = self._pgate = ElementGate(self.rep, name, "probs", "f32")
        g.f32(lo, got, probs, bound)
        if hi == self.B:
            g.close()
        if self.S.argmax is not None:
            top = probs.topk(2, dim=-1).values
            clear = (top[..., 0] - top[..., 1]) > 2 * float(bound.max()) + 1e-6
            am = torch.as_tensor(self.S.argmax)[lo:hi].to(self.dev).long()
            bad = clear & (am != probs.argmax(-1))
            self.rep.note(name, "argmax_ties", float((~clear).double().mean()))
            if bool(bad.any()):
                b, y, xx = _first(bad)
                self.rep.fail(f"{name} argmax: image {lo + b} at (y={y}, x={xx}): stored {int(am[b, y, xx])}, fp64 "
                              f"{int(probs[b, y, xx].argmax())}")

    # -- records --------------------------------------------------------------------------------------------------------
    def check_records(self):
        for li in range(self.nb):
            sp, r = self.plan[li], self.rec[li]
            s1 = s2 = 0.0
            n = 0
            for lo, hi in self._chunks():
                z = self._get(self.S.z[li], lo, hi)
                s1 = s1 + z.sum((0, 1, 2)); n += z[..., 0].numel()
            mean = s1 / n
            for lo, hi in self._chunks():
                z = self._get(self.S.z[li], lo, hi)
                s2 = s2 + ((z - mean) ** 2).sum((0, 1, 2))
            var = s2 / n
            if self.mode == "bf16" and li in getattr(self, "_zsums", {}):
                # bf16 storage: the record holds the statistics of the UNROUNDED z (fp32 accumulators, rounded only at the
                # store); check_forward recomputed exactly that tensor in fp64 -- its sums, not those of the stored
                # roundings (which differ by the mean of n rounding errors: visible in a 4 x 8 bottleneck)
                zs = self._zsums[li]
                mean = zs[0] / zs[2]
                var = (zs[1] / zs[2] - mean * mean).clamp_min(0.0)
            rstd = 1.0 / torch.sqrt(var + self.cfg.bn_eps)
            g, bt = self.P[li]["gamma"], self.P[li]["beta"]
            if self.keep:
                self.kept.setdefault(sp.name, {})["stats"] = {0: torch.stack([mean, var, rstd]).cpu().numpy()}
            N = lambda t: t.cpu().numpy()
            if self.mode == "bf16":       # statistics of the unrounded z: the tolerances of the small-shape test
                zmax = float(torch.as_tensor(self.S.z[li][:self.B]).abs().max())
                _vec_gate(self.rep, sp.name, "rec.mean", N(r[2]), N(mean), np.full(sp.cout, 2e-4 * zmax))
                _vec_gate(self.rep, sp.name, "rec.rstd", N(r[3]), N(rstd), 2e-3 * N(rstd))
                _vec_gate(self.rep, sp.name, "rec.a", N(r[0]), N(g * r[3]), 1e-5 * N((g * r[3]).abs()) + 1e-7)
                _vec_gate(self.rep, sp.name, "rec.b", N(r[1]), N(bt - r[0] * r[2]), 1e-5 * N((bt - r[0] * r[2]).abs()) + 1e-6)
            else:
                std = torch.sqrt(var + self.cfg.bn_eps)
                _vec_gate(self.rep, sp.name, "rec.mean", N(r[2]), N(mean), REC_RTOL * N(std))
                _vec_gate(self.rep, sp.name, "rec.rstd", N(r[3]), N(rstd), REC_RTOL * N(rstd))
                a = g * rstd
                _vec_gate(self.rep, sp.name, "rec.a", N(r[0]), N(a), REC_RTOL * N(a.abs()) + TINY)
                _vec_gate(self.rep, sp.name, "rec.b", N(r[1]), N(bt - a * mean), REC_RTOL * N(bt.abs() + (a * mean).abs()) + TINY)
            self._stats = getattr(self, "_stats", {})
            self._stats[li] = (mean, rstd)

    # -- backward -------------------------------------------------------------------------------------------------------
    def _dz(self, li, lo, hi):
        """(dz, magnitude, flip) of layer li as its consumers read it: the stored buffer, or -- fused layers -- the
        transform ga g' + gb z + gd of the stored g' and z with the record's rows, rounded to bf16 in bf16 mode.  flip:
        where the consumer's fp32 two-fma value may round to the other bf16 neighbour than this fp64 one (its distance to
        a rounding midpoint is within 4 fp32 roundings of the terms), one bf16 ulp, else 0."""
        if li == self.nb:
            return (*self._head_dz(lo, hi), None)
        g = self._get(self.S.gbuf[li], lo, hi)
        if not self.S.fused[li]:
            return g, g.abs(), None
        r = self.rec[li]
        z = self._get(self.S.z[li], lo, hi)
        dz = r[6] * g + (r[7] * z + r[8])
        mag = (r[6] * g).abs() + (r[7] * z).abs() + r[8].abs()
        flip = None
        if self.mode == "bf16":
            q = t_bf16(dz)
            ulp = t_bf16_ulp(q)
            flip = torch.where((0.5 * ulp - (dz - q).abs()).abs() <= 4 * U32 * mag, ulp, torch.zeros_like(ulp))
            dz = q
        return dz, mag, flip

    def _head_sums(self):
        if getattr(self, "_hs", None) is None:
            I = T = Pp = 0.0
            for lo, hi in self._chunks():
                p = self._get(self.S.probs, lo, hi)
                y = F.one_hot(self.labels[lo:hi].long(), p.shape[-1]).double()
                I = I + (y * p).sum(); T = T + y.sum(); Pp = Pp + p.sum()
            self._hs = (I, T, Pp)
        return self._hs

    def _head_dz(self, lo, hi):
        """Softmax Jacobian times the Dice gradient, both from the STORED probabilities."""
        p = self._get(self.S.probs, lo, hi)
        y = F.one_hot(self.labels[lo:hi].long(), p.shape[-1]).double()
        sm = 1e-5
        if self.macro:
            I = (y * p).sum((1, 2), keepdim=True)
            D = y.sum((1, 2), keepdim=True) + p.sum((1, 2), keepdim=True) + sm
            dp = -(2.0 * y * D - (2.0 * I + sm)) / (D * D) / (self.B * p.shape[-1])
        else:
            I, T, Pp = self._head_sums()
            D = T + Pp + sm
            dp = -(2.0 * y * D - (2.0 * I + sm)) / (D * D)
        dp = dp * self.loss_scale
        dz = p * (dp - (p * dp).sum(-1, keepdim=True))
        return dz, p * (dp.abs() + (p * dp).abs().sum(-1, keepdim=True))

    def _consumer_dx(self, c, lo, hi):
        """Backward-data of consumer layer c from its dz: (gx, magnitude) over c's whole input (low resolution for up)."""
        sp, k = self.plan[c], self.P[c]["kernel"]
        dz, dzabs, flip = self._dz(c, lo, hi)
        wq = self.mode == "bf16" and bf16_dx_weights(self.plan, c, self.mm)
        if sp.src == "up":
            wabs = t_upconv_weff(k.abs(), False)
            return (t_upconv_dx(dz, t_upconv_weff(k, wq)), t_upconv_dx(dzabs, wabs),
                    None if flip is None else t_upconv_dx(flip, wabs))
        return (t_conv_dx(dz, t_bf16(k) if wq else k), t_conv_dx(dzabs, k.abs()),
                None if flip is None else t_conv_dx(flip, k.abs()))

    def masked_grad(self, li, lo, hi):
        """(g' recomputed in fp64, magnitude, excluded, flip, g' before its storage rounding) of BN layer li from the dz of
        its consumers; flip: what the bf16 dz operands that may round the other way (``_dz``) can move it by, through |w|."""
        bf = self.mode == "bf16"
        R = t_bf16 if bf else (lambda t: t)
        c = li + 1
        y, _, alive, unsure = self.act(li, lo, hi)
        gx, gabs, gfl = self._consumer_dx(c, lo, hi)
        gfl = torch.zeros_like(gabs) if gfl is None else gfl
        excl = unsure.clone()
        csp = self.plan[c]
        if csp.src == "concat":
            gx, gabs, gfl = gx[..., :self.plan[li].cout], gabs[..., :self.plan[li].cout], gfl[..., :self.plan[li].cout]
        if csp.src == "pool":
            a, b = self.coef[li]
            z = self._get(self.S.z[li], lo, hi)
            act = torch.where(alive, a * z + b, torch.zeros_like(z))
            mag = (a * z).abs() + b.abs()
            routed = t_pool_route(act, R(gx))
            rabs = t_pool_route(act, gabs)
            # (the pooled gradient is itself stored in bf16: it may round the other way where a dz operand may, or where
            #  its own fp32 accumulation sits on a rounding midpoint -- one ulp of IT, which is many of g' where the routed
            #  and the skip half cancel)
            gfl = t_pool_route(act, gfl + t_bf16_ulp(gx) * ((gfl > 0) | t_bf16_may_flip(gx, gabs)) if bf else gfl)
            excl |= t_pool_near_tie(act, mag, 4)
            gx, gabs = routed, rabs
        if self._drop_layer(li):
            d = self.mask[lo:hi] / (1.0 - self.cfg.dropout_rate)
            gx, gabs, gfl = gx * d, gabs * d, gfl * d
        skips = [j for j, s in enumerate(self.plan) if s.src == "concat" and s.skip_from == li]
        for j in skips:
            sx, sabs, sfl = self._consumer_dx(j, lo, hi)
            C0 = self.plan[j - 1].cout
            gx, gabs = gx + R(sx[..., C0:]), gabs + sabs[..., C0:]
            if bf:         # (the raw skip half is stored in bf16 too)
                sfl = torch.zeros_like(sabs) if sfl is None else sfl
                gfl = gfl + sfl[..., C0:] + t_bf16_ulp(sx[..., C0:]) * ((sfl[..., C0:] > 0) | t_bf16_may_flip(sx[..., C0:], sabs[..., C0:]))
        zero = torch.zeros_like(gx)
        gun = torch.where(alive, gx, zero)
        return R(gun), torch.where(alive | unsure, gabs, zero), (excl & (gabs > 0)), torch.where(alive, gfl, zero), gun

    def check_backward(self):
        bf = self.mode == "bf16"
        if not hasattr(self, "_stats"):
            self.check_records()
        self._gsums = {}
        for li in range(self.nb - 1, -1, -1):
            sp, r = self.plan[li], self.rec[li]
            fused = self.S.fused[li]
            gate = ElementGate(self.rep, sp.name, "g'" if fused else "dz", self.mode, rel_l2=self._rel_l2(li, True))
            s_g = s_gx = a_g = a_gx = 0.0
            gmax = float(torch.as_tensor(self.S.gbuf[li][:self.B]).abs().max()) if bf else 0.0
            mean_r, rstd_r = r[2], r[3]
            for lo, hi in self._chunks():
                g, gabs, excl, gfl, gun = self.masked_grad(li, lo, hi)
                self._keep(li, "gmask", lo, g)
                z = self._get(self.S.z[li], lo, hi)
                xhat = (z - mean_r) * rstd_r
                # (the sums behind c1, c2, beta and gamma are taken of g' BEFORE its storage rounding, as the engine
                #  takes them of its fp32 accumulators; fp32 mode stores unrounded: gun is g)
                s_g = s_g + gun.sum((0, 1, 2)); s_gx = s_gx + (gun * xhat).sum((0, 1, 2))
                a_g = a_g + gun.abs().sum((0, 1, 2)); a_gx = a_gx + (gun * xhat).abs().sum((0, 1, 2))
                got = self._get(self.S.gbuf[li], lo, hi)
                if fused:
                    if bf:
                        bound = 1.001 * t_bf16_ulp(g) + 5e-5 * gmax
                        # (+ the operands that may round the other way, then one more rounding of the sum)
                        gate.bf16(lo, got, g, bound, 4 * bound + gfl + t_bf16_ulp(g) * (gfl > 0))
                    else:
                        gate.f32(lo, got, g, GAMMA * gabs + TINY, excl)
                else:
                    gr = self.P[li]["gamma"] * rstd_r
                    pred = gr * (g - r[4] - xhat * r[5])
                    self._keep(li, "dz", lo, pred)
                    if bf:
                        bound = 1.001 * t_bf16_ulp(pred) + gr.abs() * t_bf16_ulp(g) * (g != 0) + 5e-5 * gmax
                        gate.bf16(lo, got, t_bf16(pred), bound, 4 * bound + gr.abs() * (gfl + t_bf16_ulp(g) * (gfl > 0)))
                    else:
                        # (the stand-alone pass forms ga g' + gb z + gd from the fp32 rows: their magnitudes count too)
                        mag = gr.abs() * (gabs + r[4].abs() + (xhat * r[5]).abs()) + (r[7] * z).abs() + r[8].abs()
                        bound = GAMMA * mag + TINY
                        gate.f32(lo, got, pred, bound, excl)
            gate.close()
            self._gsums[li] = (s_g, s_gx, a_g, a_gx)
            n = self.B * self.S.z[li].shape[1] * self.S.z[li].shape[2]
            c1, c2 = s_g / n, s_gx / n
            if self.keep:
                self.kept[sp.name]["c12"] = {0: torch.stack([c1, c2]).cpu().numpy()}
            self._check_bwd_record(li, c1, c2, a_g / n, a_gx / n)

    def _check_bwd_record(self, li, c1, c2, sc1, sc2):
        sp, r = self.plan[li], self.rec[li]
        N = lambda t: t.cpu().numpy()
        tol = REC_RTOL if self.mode == "f32" else 1e-3      # bf16: g' is rounded at the store, the means are not
        mean, rstd = self._stats[li]
        ga = self.P[li]["gamma"] * rstd
        gb = -ga * rstd * c2
        gd = -ga * c1 - gb * mean
        _vec_gate(self.rep, sp.name, "rec.c1", N(r[4]), N(c1), tol * N(sc1) + TINY)
        _vec_gate(self.rep, sp.name, "rec.c2", N(r[5]), N(c2), tol * N(sc2) + TINY)
        if self.mode == "bf16":       # (the statistics themselves carry the bf16 tolerances: ga, gb, gd on the record's own rows)
            ga, gb = r[0], -r[0] * r[3] * r[5]
            gd = -ga * r[4] - gb * r[2]
        _vec_gate(self.rep, sp.name, "rec.ga", N(r[6]), N(ga), tol * N(ga.abs()) + TINY)
        gbs = (ga * rstd).abs() * sc2
        _vec_gate(self.rep, sp.name, "rec.gb", N(r[7]), N(gb), tol * N(gbs) + TINY)
        _vec_gate(self.rep, sp.name, "rec.gd", N(r[8]), N(gd), tol * N(ga.abs() * sc1 + gbs * mean.abs()) + TINY)

    def check_param_grads(self, only=None):
        """dW and bias of every layer (or of the layers named in ``only``), gamma and beta of every BN layer, summed in
        fp64 over the whole batch from the layer's recomputed input and its dz as read by the backward kernels."""
        bf = self.mode == "bf16"
        for li, sp in enumerate(self.plan):
            if only is not None and sp.name not in only:
                continue
            rnd = bf and bf16_dw_operands(self.plan, li, self.mm)
            dk = db = dabs = sg = sgx = 0.0
            for lo, hi in self._chunks():
                x, _ = self.layer_input(li, lo, hi)
                dz = self._dz(li, lo, hi)[0]
                dk = dk + t_conv_dw(t_bf16(x) if rnd else x, dz, sp.kh, sp.kw)
                db = db + dz.sum((0, 1, 2)); dabs = dabs + dz.abs().sum((0, 1, 2))
            dk, db, dabs = dk.cpu().numpy(), db.cpu().numpy(), dabs.cpu().numpy()
            if self.keep:
                self.kept.setdefault(sp.name, {})["grads"] = {0: {"kernel": dk, "bias": db}}
            G = self.S.grads[li]
            kscale = np.abs(dk).max()
            tap = ("ky", "kx", "ci", "co")
            if bf:     # the small-shape test's dW gate: fp32 accumulation of exact bf16 products, relative L2
                rel = np.linalg.norm(G["kernel"] - dk) / max(np.linalg.norm(dk), 1e-30)
                self.rep.note(sp.name, "dW", rel / 1e-4)
                if rel > 1e-4:
                    i = tuple(int(v) for v in np.unravel_index(np.abs(G["kernel"] - dk).argmax(), dk.shape))
                    self.rep.fail(f"{sp.name} dW: relative L2 {rel:.3e} > 1e-4; worst tap at "
                                  f"(ky={i[0]}, kx={i[1]}, ci={i[2]}, co={i[3]}): stored {G['kernel'][i]:.9e}, fp64 {dk[i]:.9e}")
            else:
                _vec_gate(self.rep, sp.name, "dW", G["kernel"], dk, np.full(dk.shape, PARAM_RTOL * kscale), tap)
            if sp.has_bn:    # analytically zero (bias ahead of a BN): judged on the scale of its accumulation
                btol = (1e-5 if bf else PARAM_RTOL) * dabs.max() + (1e-7 if bf else 0.0)
                _vec_gate(self.rep, sp.name, "bias", G["bias"], db, np.full(db.shape, btol))
                sg, sgx, ag, agx = (t.cpu().numpy() for t in self._gsums[li])
                if bf:
                    # the small-shape test's rule: the gradients are the record's means times the count ...
                    n = self.B * self.S.z[li].shape[1] * self.S.z[li].shape[2]
                    r = self.rec[li].cpu().numpy()
                    _vec_gate(self.rep, sp.name, "beta=c1*N", G["beta"], r[4] * n, 1e-4 * np.abs(r[4] * n) + 1e-6)
                    _vec_gate(self.rep, sp.name, "gamma=c2*N", G["gamma"], r[5] * n, 1e-4 * np.abs(r[5] * n) + 1e-6)
                    # ... and, vs the fp64 sums of the recomputed g' before its storage rounding, on the scale of the
                    # accumulation (the device sums the unrounded fp32 g' in fp32 partial rows of up to ~1e5 elements:
                    # ~u sqrt(1e5) = 2e-5 of sum |g'|, and these sums cancel to ~1e-5 of it at the full-resolution layers)
                    _vec_gate(self.rep, sp.name, "beta", G["beta"], sg, 2e-4 * ag)
                    _vec_gate(self.rep, sp.name, "gamma", G["gamma"], sgx, 2e-4 * agx)
                else:
                    _vec_gate(self.rep, sp.name, "beta", G["beta"], sg, np.full(sg.shape, PARAM_RTOL * max(np.abs(sg).max(), 1e-30)))
                    _vec_gate(self.rep, sp.name, "gamma", G["gamma"], sgx, np.full(sgx.shape, PARAM_RTOL * max(np.abs(sgx).max(), 1e-30)))
            else:
                _vec_gate(self.rep, sp.name, "bias", G["bias"], db, np.full(db.shape, PARAM_RTOL * max(np.abs(db).max(), 1e-30)))

    def run(self):
        import time
        phases = [self.check_forward] + ([self.check_records, self.check_backward, self.check_param_grads] if self.training else [])
        for f in phases:
            t0 = time.time()
            f()
            if self.dev.type == "cuda":
                torch.cuda.synchronize(self.dev)
            self.rep.times[f.__name__] = time.time() - t0
        if self.mode == "f32" and self.rep.elements and self.rep.excluded > EXCLUDE_MAX * self.rep.elements:
            self.rep.fail(f"{self.rep.excluded} of {self.rep.elements} elements excluded (mask / route within fp32 "
                          f"rounding): more than {EXCLUDE_MAX:.0e}")
        return self.rep
