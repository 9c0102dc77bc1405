"""Times the contrast stage on the device, 256x512x1 scans, fp32 model, 3 classes:

* ``oct_contrast_batch`` at batch 32 and 128 with (8,8), (1,1) and (16,16) tiles, CLAHE with clip 2 and the (1,99) stretch, on
  clean synthetic scans and on constant images: ms per call between two device events, next to a device-to-device ``copy_``
  of the same bytes timed in the same run -- that copy is the yardstick --, and the time of each of the call's three
  launches from the library's per-launch profiler (event pairs around each launch; they add the events' own cost);
* the replayed inference pipeline (``BatchedPredictor``, batch 32) ms per scan with the stage off and on, in alternating
  windows of one run, with the spread of the off windows;
* ``contrast_images`` over ``--scans`` scans through the kernel against the numpy path (``contrast_reference``, timed on
  ``--numpy-scans`` scans).

Every shape is warmed up before it is timed; the median of ``--windows`` windows is reported with the spread.  No hardware
counters are read.  Prints one JSON line.
Usage: python tools/bench_contrast.py [--windows 5] [--kernel-reps 200] [--scans 2048] [--numpy-scans 64] [--pipeline-scans 2048]"""
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
from oct_image_segmentation_models_amd.common.utils import contrast_images, contrast_reference  # noqa: E402
from oct_image_segmentation_models_amd.evaluation.pipeline import BatchedPredictor  # noqa: E402
from oct_image_segmentation_models_amd.models.engine_model import Model  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--kernel-reps", type=int, default=200)
    ap.add_argument("--scans", type=int, default=2048)
    ap.add_argument("--numpy-scans", type=int, default=64)
    ap.add_argument("--pipeline-scans", type=int, default=2048)
    a = ap.parse_args()
    H, W, C = 256, 512, 3
    model = Model("unet", dict(input_channels=1, num_classes=C, image_height=H, image_width=W, seed=1))
    eng = model._ensure_engine(32, False)
    dev = eng.device
    clean8, _ = make_scans(8, H, W, C, seed=1234)

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

    res = {"what": f"contrast stage on the device, {H}x{W}x1 uint8", "windows": a.windows, "kernel_reps": a.kernel_reps}
    specs = {"clahe2": {"method": "clahe", "clip": 2.0}, "stretch": {"method": "stretch", "percentiles": (1, 99)}}
    eng.forward(torch.from_numpy(clean8).to(dev), training=False)        # the engine's profiler becomes this thread's
    kernels = {}
    for B in (32, 128):
        contents = {"clean": np.tile(clean8, (B // 8, 1, 1, 1)), "constant": np.full((B, H, W, 1), 37, np.uint8)}
        for cname, host in contents.items():
            x = torch.from_numpy(host).to(dev)
            out, twin = torch.empty_like(x), torch.empty_like(x)
            copy = timed(lambda: twin.copy_(x), a.kernel_reps)
            for tiles in ((8, 8), (1, 1), (16, 16)):
                for sname, spec in specs.items():
                    if sname == "stretch" and tiles != (8, 8):
                        continue
                    s = dict(spec, tiles=tiles)
                    call = lambda: eng.contrast(x, s, out=out)      # noqa: E731
                    t = timed(call, a.kernel_reps)
                    eng.profile_begin()
                    for _ in range(20):
                        call()
                    per = {e["kernel"]: round(e["total_ms"] / e["launches"], 4) for e in eng.profile_end() if e["layer"] == "contrast"}
                    kernels[f"B{B}_{cname}_{sname}_{tiles[0]}x{tiles[1]}"] = {
                        "ms_per_call": t, "copy_ms": copy, "time_over_copy": round(t["median"] / copy["median"], 2),
                        "GBps_in_plus_out": round(2 * x.numel() / (t["median"] * 1e-3) / 1e9, 1), "profiled_ms_per_launch": per}
    res["kernels"] = kernels

    # ---- the replayed pipeline, stage off and on, alternated ----
    images = np.tile(clean8, (a.pipeline_scans // 8, 1, 1, 1))
    spec = dict(specs["clahe2"], tiles=(8, 8))

    def pipeline(**kw):
        pred = BatchedPredictor(eng, 32, **kw)
        for _ in pred.run(images[:64]):
            pass
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in pred.run(images):
            pass
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / images.shape[0] * 1e3
    off, on = [], []
    for _ in range(a.windows):
        off.append(pipeline())
        on.append(pipeline(contrast=spec))
    res["pipeline_ms_per_scan"] = {"off": stats(off), "on": stats(on), "on_over_off": round(stats(on)["median"] / stats(off)["median"], 4),
                                   "off_spread": round((max(off) - min(off)) / stats(off)["median"], 4), "scans": int(images.shape[0])}

    # ---- a dataset array through contrast_images: kernel against numpy ----
    data = np.tile(clean8, (a.scans // 8, 1, 1, 1))
    contrast_images(data[:128], spec, device=dev)
    t0 = time.perf_counter()
    got = contrast_images(data, spec, device=dev)
    t_dev = time.perf_counter() - t0
    t0 = time.perf_counter()
    want = contrast_reference(data[:a.numpy_scans], spec)
    t_np = time.perf_counter() - t0
    res["contrast_images"] = {"scans": int(data.shape[0]), "device_s": round(t_dev, 3), "device_ms_per_scan": round(t_dev / data.shape[0] * 1e3, 4),
                              "numpy_scans": a.numpy_scans, "numpy_ms_per_scan": round(t_np / a.numpy_scans * 1e3, 2),
                              "numpy_over_device": round((t_np / a.numpy_scans) / (t_dev / data.shape[0]), 1),
                              "equal_bytes": bool(np.array_equal(got[:a.numpy_scans], want))}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
