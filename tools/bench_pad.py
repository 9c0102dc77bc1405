"""Times pad and crop on the device at B = 32, one channel, 500x760 scans padded to 512x768, 3 classes, fp32:

* ``oct_pad_batch`` (uint8 input, the three modes) and ``oct_crop_batch`` of each output (arg-max maps, 1 B/px; entropy /
  mutual information, 4 B/px; probabilities, 12 B/px): ms per call and achieved bytes/s over the bytes the call must move
  (source bytes read + destination bytes written), next to a device-to-device ``copy_`` of a tensor of the destination's size
  timed in the same run -- that copy is the yardstick; the ratio of the two rates is reported;
* ``Model.predict_labels`` ms per scan on the 500x760 scans with ``pad_mode="edge"`` against the same model on native
  512x768 scans, alternated in the same run (both include the upload of the batch and the download of the labels).

Every shape is warmed up before it is timed, a timed window is ``--reps`` repetitions between two device events (a host
clock around a synchronised call for ``predict_labels``), and the median of ``--windows`` windows is reported with the
spread.  Prints one JSON line.
Usage: python tools/bench_pad.py [--reps 5] [--windows 5] [--kernel-reps 200]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oct_image_segmentation_models_amd.common.synthetic import make_scans  # noqa: E402
from oct_image_segmentation_models_amd.common.utils import padded_geometry  # noqa: E402
from oct_image_segmentation_models_amd.models.engine_model import Model  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--kernel-reps", type=int, default=200)
    a = ap.parse_args()
    B, H, W, C, P = 32, 500, 760, 3, 4
    Hp, Wp, top, left = padded_geometry(H, W, P)
    model = Model("unet", dict(input_channels=1, num_classes=C, image_height=Hp, image_width=Wp, pool_layers=P, seed=1))
    eng = model._ensure_engine(B, False)
    dev = eng.device
    native8, _ = make_scans(8, Hp, Wp, C, seed=1234)
    native = np.tile(native8, (B // 8, 1, 1, 1))
    scans = np.ascontiguousarray(native[:, top:top + H, left:left + W])

    def window(call, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            call()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps

    def stats(v, digits=4):
        v = sorted(v)
        return {"median": round(v[len(v) // 2], digits), "min": round(v[0], digits), "max": round(v[-1], digits)}

    def timed(call, reps):
        for _ in range(5):
            call()
        torch.cuda.synchronize()
        return stats([window(call, reps) for _ in range(a.windows)])

    res = {"what": f"pad and crop on the device, B={B}, {H}x{W}x1 -> {Hp}x{Wp} at ({top}, {left}), {C} classes, fp32",
           "reps": a.reps, "windows": a.windows, "kernel_reps": a.kernel_reps}

    # ---- the kernels, each next to a same-size device-to-device copy ----
    x = torch.from_numpy(scans).to(dev)
    x_pad = torch.empty((B, Hp, Wp, 1), dtype=torch.uint8, device=dev)
    probs, am = eng.forward(eng.pad(x, Hp, Wp, top, left, "edge", out=x_pad), training=False, want_probs=True, want_argmax=True)
    ent = probs[..., 0].contiguous()
    kernels = {}

    def against_copy(name, call, dst, moved):
        twin = torch.empty_like(dst)
        k, c = timed(call, a.kernel_reps), timed(lambda: twin.copy_(dst), a.kernel_reps)
        copied = 2 * dst.numel() * dst.element_size()
        k_rate, c_rate = moved / (k["median"] * 1e-3) / 1e9, copied / (c["median"] * 1e-3) / 1e9
        kernels[name] = {"ms_per_call": k, "bytes_moved": int(moved), "GBps": round(k_rate, 1),
                         "copy_ms_per_call": c, "copy_bytes_moved": int(copied), "copy_GBps": round(c_rate, 1),
                         "rate_over_copy": round(k_rate / c_rate, 3), "time_over_copy": round(k["median"] / c["median"], 3)}

    for mode in ("edge", "reflect", "constant"):
        against_copy(f"pad_u8_{mode}", lambda mode=mode: eng.pad(x, Hp, Wp, top, left, mode, 0, out=x_pad), x_pad,
                     x.numel() + x_pad.numel())
    for name, t in (("crop_argmax_1B", am), ("crop_entropy_4B", ent), ("crop_probs_12B", probs)):
        out = eng.crop(t, H, W, top, left)
        against_copy(name, lambda t=t, out=out: eng.crop(t, H, W, top, left, out=out), out, 2 * out.numel() * out.element_size())
    res["kernels"] = kernels

    # ---- predict_labels: padded 500x760 against native 512x768, alternated ----
    def host_timed(images, **kw):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.reps):
            model.predict_labels(images, batch_size=B, **kw)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / a.reps / B * 1e3

    for _ in range(2):
        model.predict_labels(scans, batch_size=B, pad_mode="edge"); model.predict_labels(native, batch_size=B)
    t_pad, t_nat = [], []
    for _ in range(a.windows):
        t_pad.append(host_timed(scans, pad_mode="edge"))
        t_nat.append(host_timed(native))
    res["predict_labels_ms_per_scan"] = {"padded_500x760": stats(t_pad), "native_512x768": stats(t_nat),
                                         "padded_over_native": round(stats(t_pad)["median"] / stats(t_nat)["median"], 4)}
    # the forward alone, on device tensors, for the share the three launches take of it
    fwd = timed(lambda: eng.forward(x_pad, training=False, want_probs=False, want_argmax=True), a.reps)
    res["forward_argmax_ms_per_batch"] = fwd
    three = kernels["pad_u8_edge"]["ms_per_call"]["median"] + kernels["crop_argmax_1B"]["ms_per_call"]["median"]
    res["pad_plus_argmax_crop_over_forward"] = round(three / fwd["median"], 4)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
