"""Calibration of the class probabilities: reliability counts, ECE / MCE / NLL / Brier, and the
temperature that minimises the NLL (Guo et al. 2017).

The device side is ``oct_calibration_counts`` / ``oct_temperature_apply`` / ``oct_temperature_nll`` (include/oct_unet.h,
csrc/kernels_calibration.hpp), reached through ``UNetEngine.calibration_counts`` / ``.temperature_apply`` /
``.temperature_nll`` and, in the inference pipeline, through ``CalibrationCounts``.  This module holds their numpy
restatements -- the definitions of the header, element by element, in ``dtype`` arithmetic (``np.float32``: the operations
of the kernels; ``np.float64``: the yardstick of the tests) -- and the host arithmetic behind them: the metrics of a count
table (``calibration_from_counts``) and THE fit rule (``fit_beta``), which is used with device sums and with reference sums
alike."""
from __future__ import annotations

import json
import math
from types import SimpleNamespace
from typing import Callable, Optional, Tuple

import numpy as np

from ..common.custom_losses import FOCAL_EPS

MAX_BINS, MAX_BETAS, MAX_CLASSES = 64, 8, 32
CONF_BITS = 28                                   # confidences in fixed point: k = floor(conf * 2^28)
BETA_LO, BETA_HI = 1.0 / 16.0, 16.0              # the bracket of the fit, and the range of the public `temperature`
FIT_STEPS, FIT_RTOL, BOUND_RTOL = 20, 1e-4, 1e-3
CALIBRATION_METRICS = ("ece", "mce", "nll", "brier")
TEMPERATURE_FILENAME = "temperature.json"


def check_bins(calibration_bins) -> int:
    """The public ``calibration_bins``, validated: an int in 0..64 (0: off)."""
    if isinstance(calibration_bins, (bool, np.bool_)) or not isinstance(calibration_bins, (int, np.integer)) \
            or not 0 <= int(calibration_bins) <= MAX_BINS:
        raise ValueError(f"calibration_bins must be an int in 0..{MAX_BINS}, not {calibration_bins!r}")
    return int(calibration_bins)


def check_temperature(temperature) -> float:
    """The public ``temperature``, validated: a float in [1/16, 16] (1.0: off)."""
    if isinstance(temperature, (bool, np.bool_)) or not isinstance(temperature, (int, float, np.integer, np.floating)) \
            or not BETA_LO <= float(temperature) <= BETA_HI:
        raise ValueError(f"temperature must be a number in [1/16, 16], not {temperature!r}")
    return float(temperature)


def _ignore(ignore_label) -> int:
    if ignore_label is None:
        return -1
    if isinstance(ignore_label, (bool, np.bool_)) or int(ignore_label) != ignore_label or not -1 <= int(ignore_label) <= 255:
        raise ValueError(f"ignore_label must be None or an int in 0..255, not {ignore_label!r}")
    return int(ignore_label)


def _inputs(probs, labels) -> Tuple[np.ndarray, np.ndarray]:
    """(B, ..., C) float32 probabilities and (B, ...) labels -> (B, npix, C) float32 and (B, npix) int64."""
    p = np.asarray(probs)
    if p.dtype != np.float32 or p.ndim < 3 or not 2 <= p.shape[-1] <= MAX_CLASSES:
        raise ValueError(f"probs must be float32 (B, ..., C) with 2 <= C <= {MAX_CLASSES}")
    y = np.asarray(labels)
    if y.shape == p.shape[:-1] + (1,):
        y = y[..., 0]
    if y.shape != p.shape[:-1]:
        raise ValueError(f"labels of shape {y.shape} do not match probs of shape {p.shape}")
    B, Cn = p.shape[0], p.shape[-1]
    return p.reshape(B, -1, Cn), y.reshape(B, -1).astype(np.int64)


def _logs(p: np.ndarray, dtype) -> np.ndarray:
    """l_c = log(max(p_c, EPS)) in ``dtype``; the input is the float32 array either way."""
    return np.log(np.maximum(p.astype(dtype), dtype(np.float32(FOCAL_EPS))))


def _softmax_terms(l: np.ndarray, beta, dtype):
    """With l (..., C): L, e (..., C), S, q (..., C) of the header -- the sum in class order, one operation per step."""
    b = dtype(np.float32(beta))
    L = l.max(axis=-1)
    e = np.exp(b * (l - L[..., None]))
    S = e[..., 0].copy()
    for c in range(1, l.shape[-1]):
        S = S + e[..., c]
    return L, e, S, e / S[..., None]


def calibration_counts_reference(probs, labels, n_bins: int, ignore_label: Optional[int] = None, dtype=np.float32,
                                 terms: bool = False):
    """``oct_calibration_counts`` restated: (B, ..., C) float32 probabilities and (B, ...) labels -> ``counts`` (B, M, 3)
    uint64 = [pixels, correct pixels, sum of k] and ``sums`` (B, 4) float64 = [sum nll, sum brier, counted, labels >= C
    that are not the ignore label].  The integer words do not depend on ``dtype``; nll and brier are formed per pixel in
    ``dtype`` and summed in float64.  ``terms``: also return the per-pixel ``(nll, brier)`` (B, npix) arrays in ``dtype``,
    zero where a pixel is not counted."""
    M = int(n_bins)
    if not 1 <= M <= MAX_BINS:
        raise ValueError(f"n_bins must be in 1..{MAX_BINS}")
    p, y = _inputs(probs, labels)
    B, npix, Cn = p.shape
    ig = _ignore(ignore_label)
    counted = (y >= 0) & (y < Cn) & (y != ig)
    bad = ~counted & (y != ig)
    m = p.argmax(axis=-1)                                            # the lowest index of the maximum
    conf = np.minimum(np.maximum(np.take_along_axis(p, m[..., None], -1)[..., 0], np.float32(0)), np.float32(1))
    k = np.floor(conf * np.float32(2.0 ** CONF_BITS)).astype(np.uint64)            # the product is exact
    bins = np.minimum(np.uint64(M - 1), (k * np.uint64(M)) >> np.uint64(CONF_BITS)).astype(np.int64)
    ys = np.where(counted, y, 0)
    eps = dtype(np.float32(FOCAL_EPS))
    pd = p.astype(dtype)
    py = np.take_along_axis(pd, ys[..., None], -1)[..., 0]
    nll = -np.log(np.minimum(np.maximum(py, eps), dtype(1) - eps))
    brier = None
    for c in range(Cn):
        d = pd[..., c] - (ys == c).astype(dtype)
        t = d * d
        brier = t if brier is None else brier + t
    nll, brier = np.where(counted, nll, dtype(0)), np.where(counted, brier, dtype(0))
    counts, sums = np.zeros((B, M, 3), np.uint64), np.zeros((B, 4), np.float64)
    for b in range(B):
        w = counted[b]
        counts[b, :, 0] = np.bincount(bins[b][w], minlength=M).astype(np.uint64)
        counts[b, :, 1] = np.bincount(bins[b][w & (m[b] == y[b])], minlength=M).astype(np.uint64)
        for j in range(M):                                           # (uint64 sums: bincount's weights would go through float64)
            counts[b, j, 2] = k[b][w & (bins[b] == j)].sum(dtype=np.uint64)
        sums[b] = (nll[b].sum(dtype=np.float64), brier[b].sum(dtype=np.float64), float(w.sum()), float(bad[b].sum()))
    return (counts, sums, (nll, brier)) if terms else (counts, sums)


def temperature_apply_reference(probs, beta: float, dtype=np.float64) -> np.ndarray:
    """``oct_temperature_apply`` restated: q = softmax(beta * log(max(p, EPS))) over the last axis, in ``dtype``."""
    p = np.asarray(probs)
    if p.dtype != np.float32:
        raise ValueError("probs must be float32")
    return _softmax_terms(_logs(p, dtype), beta, dtype)[3]


def temperature_nll_reference(probs, labels, betas, ignore_label: Optional[int] = None, dtype=np.float64, terms: bool = False):
    """``oct_temperature_nll`` restated: ``sums`` (B, K, 3) float64 = the sums over an image's counted pixels of nll, g, h
    at each beta, and ``counted`` (B) float64.  ``terms``: also the per-pixel (B, K, 3, npix) array in ``dtype``, zero where
    a pixel is not counted."""
    betas = [float(b) for b in np.atleast_1d(betas)]
    if not 1 <= len(betas) <= MAX_BETAS:
        raise ValueError(f"1..{MAX_BETAS} betas")
    p, y = _inputs(probs, labels)
    B, npix, Cn = p.shape
    ig = _ignore(ignore_label)
    counted = (y >= 0) & (y < Cn) & (y != ig)
    ys = np.where(counted, y, 0)
    l = _logs(p, dtype)
    ly = np.take_along_axis(l, ys[..., None], -1)[..., 0]
    per = np.zeros((B, len(betas), 3, npix), dtype)
    for i, beta in enumerate(betas):
        L, _, S, q = _softmax_terms(l, beta, dtype)
        mu = v = None
        for c in range(Cn):
            t = q[..., c] * l[..., c]
            mu = t if mu is None else mu + t
        for c in range(Cn):
            r = l[..., c] - mu
            t = q[..., c] * (r * r)
            v = t if v is None else v + t
        nll = np.log(S) - dtype(np.float32(beta)) * (ly - L)
        for j, t in enumerate((nll, mu - ly, v)):
            per[:, i, j] = np.where(counted, t, dtype(0))
    sums = per.sum(axis=-1, dtype=np.float64)
    cnt = counted.sum(axis=-1).astype(np.float64)
    return (sums, cnt, per) if terms else (sums, cnt)


def calibration_from_counts(counts, sums) -> dict:
    """One count table (M, 3) = [n, correct, sum of k] (uint64 words, or the float64 rows of the result files, whose third
    column is the sum of the confidences) and one row of sums (4,) -> ``ece`` = sum_b (n_b / N) |acc_b - conf_b|, ``mce`` =
    the largest |acc_b - conf_b| over the non-empty bins, ``nll`` and ``brier`` = the means over the counted pixels.  All
    four are NaN when nothing is counted."""
    c = np.asarray(counts)
    if c.ndim != 2 or c.shape[1] != 3:
        raise ValueError("counts must be one (M, 3) table")
    conf_sum = c[:, 2].astype(np.float64) / (2.0 ** CONF_BITS if c.dtype.kind in "ui" else 1.0)
    n, ok = c[:, 0].astype(np.float64), c[:, 1].astype(np.float64)
    s = np.asarray(sums, np.float64).reshape(-1)
    N = n.sum()
    if N == 0:
        return dict.fromkeys(CALIBRATION_METRICS, float("nan"))
    full = n > 0
    gap = np.abs(ok[full] / n[full] - conf_sum[full] / n[full])
    return {"ece": float(np.sum(n[full] / N * gap)), "mce": float(gap.max()),
            "nll": float(s[0] / s[2]) if s[2] > 0 else float("nan"), "brier": float(s[1] / s[2]) if s[2] > 0 else float("nan")}


def counts_as_float(counts) -> np.ndarray:
    """(..., M, 3) uint64 words -> the float64 rows [n, correct, sum of the confidences] of the result files."""
    c = np.asarray(counts).astype(np.float64)
    c[..., 2] /= 2.0 ** CONF_BITS
    return c


def pooled_calibration(tables, nll, brier) -> Tuple[np.ndarray, dict]:
    """The per-image datasets of the result files -- ``tables`` (n, M, 3) float64 ``calibration_counts``, ``nll`` and ``brier``
    (n) means, NaN for an image without a counted pixel -- -> the summed table (M, 3) and ``calibration_from_counts`` of it:
    an image's sums are its means times its counted pixels, added in image order."""
    tables = np.asarray(tables, np.float64)
    total, s = np.zeros(tables.shape[1:], np.float64), np.zeros(4, np.float64)
    for t, a, b in zip(tables, np.asarray(nll, np.float64), np.asarray(brier, np.float64)):
        n = t[:, 0].sum()
        total = total + t
        if n > 0:
            s = s + np.array([a * n, b * n, n, 0.0])
    return total, calibration_from_counts(total, s)


def fit_beta(stats: Callable[[float], Tuple[float, float]]):
    """THE fit rule.  ``stats(beta) -> (sum g, sum h)``, the first and second derivative in beta of the summed NLL (convex).
    Start at beta = 1 with the bracket lo = 1/16, hi = 16; per step: g > 0 moves hi to beta, else lo; the next beta is the
    Newton step beta - g / h if h > 0, else sqrt(lo * hi), and sqrt(lo * hi) as well when that is not strictly inside
    (lo, hi); stop when it moved by <= 1e-4 beta, after at most 20 steps.  Returns ``(beta, steps, at_bound)`` --
    ``at_bound``: the result is within 1e-3 relative of an end of the bracket (the optimum lies outside it)."""
    beta, lo, hi = 1.0, BETA_LO, BETA_HI
    steps = 0
    for steps in range(1, FIT_STEPS + 1):
        g, h = (float(v) for v in stats(beta))
        if g > 0:
            hi = beta
        else:
            lo = beta
        nxt = beta - g / h if h > 0 else math.sqrt(lo * hi)
        if not lo < nxt < hi:
            nxt = math.sqrt(lo * hi)
        done = abs(nxt - beta) <= FIT_RTOL * beta
        beta = nxt
        if done:
            break
    at_bound = abs(beta - BETA_LO) <= BOUND_RTOL * BETA_LO or abs(beta - BETA_HI) <= BOUND_RTOL * BETA_HI
    return beta, steps, at_bound


def fit_record(beta: float, steps: int, at_bound: bool, nll_before: float, nll_after: float, counted: float) -> SimpleNamespace:
    """The record ``Model.fit_temperature`` and ``fit_temperature_reference`` return."""
    return SimpleNamespace(temperature=1.0 / beta, beta=float(beta), nll_before=float(nll_before), nll_after=float(nll_after),
                           steps=int(steps), counted=int(counted), at_bound=bool(at_bound))


def fit_with(sums_at: Callable[[float], Tuple[np.ndarray, float]]) -> SimpleNamespace:
    """``fit_beta`` over ``sums_at(beta) -> ((sum nll, sum g, sum h), counted)``, one pass over the data per call, and the
    record of the result: the mean NLL at beta = 1 comes from the first step, that at the result from one more pass.  Where
    nothing is counted there is nothing to fit: the record then has beta = 1, no steps and NaN for both means."""
    first, n = sums_at(1.0)
    n = float(n)
    if n == 0:
        return fit_record(1.0, 0, False, float("nan"), float("nan"), 0)

    def stats(beta):
        s = first if beta == 1.0 else sums_at(beta)[0]
        return float(s[1]), float(s[2])

    beta, steps, at_bound = fit_beta(stats)
    nll1 = float(first[0])
    s, _ = sums_at(beta)
    mean = lambda v: v / n if n > 0 else float("nan")      # noqa: E731
    return fit_record(beta, steps, at_bound, mean(nll1), mean(float(s[0])), n)


def fit_temperature_reference(probs, labels, ignore_label: Optional[int] = None, dtype=np.float64) -> SimpleNamespace:
    """The fit on host arrays: ``fit_beta`` over ``temperature_nll_reference``, per-image sums added in image order."""
    def sums_at(beta):
        s, n = temperature_nll_reference(probs, labels, [np.float32(beta)], ignore_label, dtype)
        tot = np.zeros(3)
        for b in range(s.shape[0]):
            tot = tot + s[b, 0]
        return tot, float(n.sum())
    return fit_with(sums_at)


def write_temperature(path, record) -> None:
    with open(path, "w") as fh:
        json.dump({k: getattr(record, k) for k in ("temperature", "beta", "nll_before", "nll_after", "steps", "counted", "at_bound")},
                  fh, indent=1)


def read_temperature(path) -> SimpleNamespace:
    """The record of a ``temperature.json`` (``train_model(fit_temperature=True)``); its ``temperature`` is validated."""
    with open(path, "r") as fh:
        d = json.load(fh)
    check_temperature(d["temperature"])
    return SimpleNamespace(**d)


class CalibrationCounts:
    """``oct_calibration_counts`` for up to ``batch`` images of one shape: ``(probs, gt)`` -- (n,H,W,C) float32 class
    probabilities and (n,H,W) uint8 ground truth on the device -> ``counts`` (n, M, 3) int64 (the bits are the uint64 words)
    and ``sums`` (n, 4) float64 on the device, queued on the current stream.  The workspace is the object's own.
    ``ignore_label``: None or an int in C..255, as ``ConfusionCounts``."""

    def __init__(self, batch: int, H: int, W: int, num_classes: int, device, n_bins: int, ignore_label: Optional[int] = None):
        import torch
        from .. import _hip
        from .dice_device import check_ignore_label
        self.B, self.H, self.W, self.C = int(batch), int(H), int(W), int(num_classes)
        self.M = check_bins(n_bins)
        self.ignore_label = check_ignore_label(ignore_label, self.C)
        nbytes = int(_hip.lib().oct_calibration_workspace_bytes(self.B, self.H * self.W, self.C, self.M)) if self.M else 0
        if not nbytes:
            raise _hip.OctError(f"oct_calibration_counts does not support B={batch}, {H}x{W}, {num_classes} classes, {n_bins} bins")
        self.device = torch.device(device)
        self.counts = torch.empty((self.B, self.M, 3), dtype=torch.int64, device=self.device)
        self.sums = torch.empty((self.B, 4), dtype=torch.float64, device=self.device)
        self.ws = torch.empty((nbytes,), dtype=torch.uint8, device=self.device)
        self.outs, self.geometry = (self.counts, self.sums), (self.B, self.H, self.W, self.C)

    def __call__(self, probs, gt, counts=None, sums=None):
        import torch
        from .. import _hip
        _hip.expect(probs, "probs", device=self.device, dtype=torch.float32, shape=(None, self.H, self.W, self.C))
        n = probs.shape[0]
        _hip.expect(gt, "gt", device=self.device, dtype=torch.uint8, shape=(n, self.H, self.W))
        if not 1 <= n <= self.B:
            raise _hip.OctError(f"probs and gt need a count n in 1..{self.B}, not {n}")
        counts, sums = _hip.out_view(counts, self.counts, n, "counts"), _hip.out_view(sums, self.sums, n, "sums")
        _hip.call("oct_calibration_counts", self.device, probs.data_ptr(), gt.data_ptr(), n, self.H * self.W, self.C,
                  -1 if self.ignore_label is None else self.ignore_label, self.M, counts.data_ptr(), sums.data_ptr(),
                  self.ws.data_ptr(), self.ws.numel(), _hip.stream_ptr(self.device))
        return counts, sums

    def to_host(self, counts, sums, first_image: int = 0) -> Tuple[np.ndarray, np.ndarray]:
        """Device rows -> ``(counts (n, M, 3) uint64, sums (n, 4) float64)`` on the host (waits for the stream); a label
        outside 0..C-1 that is not the ignore label raises with the image index."""
        c, s = counts.cpu().numpy().view(np.uint64), sums.cpu().numpy()
        bad = np.nonzero(s[:, 3])[0]
        if bad.size:
            i = int(bad[0])
            raise ValueError(f"image {first_image + i}: {int(s[i, 3])} pixels carry a label outside 0..{self.C - 1}")
        return c.copy(), s.copy()
