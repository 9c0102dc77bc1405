#!/usr/bin/env python3
"""Times the photometric augmentation stage (runs on the GPU box; prints one JSON line).

* kernel: ``oct_photo_batch`` at B = 32, 256x512x1, one case per flag combination -- table only, shadows only (4 per sample),
  blur at R = 2 and R = 8, and all three at R = 8 -- and kind 0 (the copy inside the kernel): HIP events around every launch,
  median of ``--reps`` launches after warm-up, microseconds and GB/s over the bytes moved (u8 images in and out).  Beside them,
  in the same run and measured the same way: ``oct_elastic_batch`` (S = 32, 8 px, images only) and a device copy of the same
  bytes.  The cases are timed in ``--rounds`` alternating windows; every window's median is listed and the best is the
  headline.  Event pairs around a ~10 us launch include the launch gap: upper bounds.  For the kernel's own time run one
  case under the profiler:
  rocprofv3 --kernel-trace --stats --output-format csv -d out -- python tools/bench_photo.py --legs "" --kinds photo_all_r8
* fit: ``Model.fit`` scans/s for (a) ``aug_mode "none"``, (p) mode "one" over a flip list with the photometric stage (every
  part on, p = 1) on the device, (f) the same list on the device without it, (h) the (p) configuration on the host (over
  ``--host-scans`` scans: the numpy path is slow).

Usage: tools/bench_photo.py [--reps 50] [--rounds 3] [--scans 2048] [--host-scans 128] [--legs apfapfh] [--no-kernel]
                            [--kinds photo_all_r8,copy]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oct_image_segmentation_models_amd import optimizers  # noqa: E402
from oct_image_segmentation_models_amd.common import augmentation as A  # noqa: E402
from oct_image_segmentation_models_amd.common import custom_losses, custom_metrics  # noqa: E402
from oct_image_segmentation_models_amd.common.data_generator import DataGenerator  # noqa: E402
from oct_image_segmentation_models_amd.common.synthetic import make_scans  # noqa: E402
from oct_image_segmentation_models_amd.models import get_model_class  # noqa: E402

H, W, C, P, B = 256, 512, 3, 4, 32
FLIPS = [(A.flip_aug, {"flip_type": "left-right"}), (A.flip_aug, {"flip_type": "up-down"}), (A.no_aug, {})]
PROBS = (0.4, 0.4, 0.2)
PHOTO = {"p": 1.0, "gamma": (0.6, 1.6), "brightness": 0.1, "contrast": (0.8, 1.25), "blur": {"p": 1.0, "sigma": (0.5, 8.0 / 3.0)},
         "shadows": {"p": 1.0, "max_count": 4, "width": (4, 24), "strength": (0.3, 0.9), "top": (0.2, 0.6)}}


def photo_ops(kind, sigma):
    ops = np.zeros(B, dtype=A.PHOTO_OP_DTYPE)
    rng = np.random.default_rng(kind)
    for b in range(B):
        ops[b]["kind"] = kind
        ops[b]["lut"] = A.photo_lut(0.6 + b / 32.0, 0.05, 1.1)
        if kind & A.PHOTO_BLUR:
            ops[b]["radius"], ops[b]["w"] = A.blur_weights(sigma)
        if kind & A.PHOTO_SHADOW:
            ops[b]["n_shadows"] = 4
            ops[b]["cx"], ops[b]["hw"] = rng.integers(0, W, 4), rng.integers(4, 25, 4)
            ops[b]["y0"], ops[b]["strength"] = rng.integers(50, 150, 4), rng.integers(77, 231, 4)
    A.check_photo_ops(ops, H, W)
    return ops


def kernel_times(reps, rounds, only=None):
    from oct_image_segmentation_models_amd.engine import UNetEngine
    eng = UNetEngine(device="cuda:0", input_channels=1, num_classes=C, image_height=32, image_width=64, pool_layers=2,
                     max_batch=1, training=False)
    images, _ = make_scans(B, H, W, C, seed=3)
    x = torch.from_numpy(images).cuda()
    out = torch.empty_like(x)
    nbytes = x.numel() * 2
    cases = {}
    for name, kind, sigma in (("photo_none", 0, 0), ("photo_lut", 4, 0), ("photo_shadows", 2, 0), ("photo_blur_r2", 1, 2.0 / 3.0),
                              ("photo_blur_r8", 1, 8.0 / 3.0), ("photo_all_r2", 7, 2.0 / 3.0), ("photo_all_r8", 7, 8.0 / 3.0)):
        dev_ops = torch.from_numpy(photo_ops(kind, sigma).view(np.uint8).copy()).cuda()
        cases[name] = lambda o=dev_ops: eng.photometric(x, o, out=out)
    eops = np.zeros(B, dtype=A.ELASTIC_OP_DTYPE)
    eops["kind"], eops["spacing"], eops["amp_x"], eops["amp_y"] = 1, 32, 2048, 2048
    eops["seed_lo"], eops["seed_hi"] = np.arange(B), 7
    A.check_elastic_ops(eops, H, W)
    dev_eops = torch.from_numpy(eops.view(np.uint8).copy()).cuda()
    cases["elastic_s32_images"] = lambda: eng.elastic(x, None, dev_eops, out=(out, None))
    cases["copy"] = lambda: out.copy_(x)
    if only:
        cases = {k: v for k, v in cases.items() if k in only}
    res = {"bytes": nbytes}
    for _ in range(rounds):         # alternating windows: every case once per round
        for name, run in cases.items():
            for _ in range(5):
                run()
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
            for e0, e1 in ev:
                e0.record(); run(); e1.record()
            torch.cuda.synchronize()
            us = sorted(e0.elapsed_time(e1) * 1e3 for e0, e1 in ev)[reps // 2]
            res.setdefault(name, {"us_windows": []})["us_windows"].append(round(us, 2))
    for name in cases:
        best = min(res[name]["us_windows"])
        res[name].update(us=best, GB_per_s=round(nbytes / best * 1e-3, 0))
    return res


def fit_rate(images, labels, mode, device_aug, photometric):
    mc = get_model_class("unet")(input_channels=1, num_classes=C, image_height=H, image_width=W, pool_layers=P)
    model = mc.build_model()
    loss_fn = custom_losses.custom_loss_objects["dice_loss_macro"]["function"](num_classes=C, is_y_true_sparse=False)
    metric_fn = custom_metrics.training_monitor_metric_objects["dice_coef_macro"](False, C)
    model.compile(optimizer=optimizers.Adam(learning_rate=1e-3), loss=loss_fn, metrics=[metric_fn])
    args = ([], "none", ()) if mode == "none" else (FLIPS, "one", PROBS)
    kw = dict(seed=5, device_aug=device_aug, photometric=photometric)
    warm = DataGenerator(images[:4 * B], labels[:4 * B], B, *args, True, mc.get_preprocess_input_fn(), **kw)
    model.fit(x=warm, epochs=1, verbose=0)
    gen = DataGenerator(images, labels, B, *args, True, mc.get_preprocess_input_fn(), **kw)
    assert gen.oct_device_aug == (device_aug and mode != "none")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    model.fit(x=gen, epochs=1, verbose=0)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    res = {"scans_per_s": round(len(gen) * B / dt, 1), "ms_per_step": round(dt / len(gen) * 1e3, 3), "steps": len(gen)}
    if mode == "none" or device_aug:    # what the host spends assembling a batch (gather + descriptors), no GPU involved
        nxt = gen.next_batch_aug if gen.oct_device_aug else gen.next_batch_u8
        t0 = time.perf_counter()
        for _ in range(16):
            nxt()
        res["host_assembly_ms_per_batch"] = round((time.perf_counter() - t0) / 16 * 1e3, 3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--scans", type=int, default=2048)
    ap.add_argument("--host-scans", type=int, default=128)
    ap.add_argument("--legs", default="apfapfh")
    ap.add_argument("--no-kernel", action="store_true")
    ap.add_argument("--kinds", default="", help="comma-separated subset of the kernel cases (one case per profiler run)")
    a = ap.parse_args()
    res = {"what": f"photometric stage, B={B}, {H}x{W}x1, fit: every part on, p=1, over a flip list"}
    base_i, base_l = make_scans(64, H, W, C, seed=77)
    legs = {"a": ("fit_none", "none", False, None, a.scans), "p": ("fit_device_photo", "one", True, PHOTO, a.scans),
            "f": ("fit_device_flips", "one", True, None, a.scans), "h": ("fit_host_photo", "one", False, PHOTO, a.host_scans)}
    for leg in a.legs:      # a leg named twice runs twice ("apap": alternating, for the spread); every run is listed
        name, mode, dev, photometric, scans = legs[leg]
        reps = max(scans // 64, 1)
        run = fit_rate(np.tile(base_i, (reps, 1, 1, 1))[:scans], np.tile(base_l, (reps, 1, 1, 1))[:scans], mode, dev, photometric)
        res.setdefault(name, []).append(run)
    # (the kernel cases come last, as in tools/bench_warp.py)
    if not a.no_kernel:
        res["kernel"] = kernel_times(a.reps, a.rounds, set(filter(None, a.kinds.split(","))))
    best = lambda name: max(r["scans_per_s"] for r in res[name])     # noqa: E731
    if "fit_none" in res and len(res["fit_none"]) > 1:
        rates = [r["scans_per_s"] for r in res["fit_none"]]
        res["none_spread"] = round(min(rates) / max(rates), 3)
    if "fit_device_photo" in res and "fit_none" in res:
        res["device_over_none"] = round(best("fit_device_photo") / best("fit_none"), 3)
    if "fit_device_photo" in res and "fit_host_photo" in res:
        res["device_over_host"] = round(best("fit_device_photo") / best("fit_host_photo"), 1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
