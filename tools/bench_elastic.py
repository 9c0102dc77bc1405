#!/usr/bin/env python3
"""Times the elastic deformation stage (runs on the GPU box; prints one JSON line).

* kernel: ``oct_elastic_batch`` at B = 32, 256x512x1, images + labels, spacing 8 / 32 / 128, both axes (8 px) and axial only
  (amp_x = 0): HIP events around every launch, median of ``--reps`` launches after warm-up, microseconds and GB/s over the
  bytes moved (u8 images and labels, in and out).  Beside them, in the same run and measured the same way: ``oct_warp_batch``'s
  affine kind and a device copy of the same bytes.  The cases are timed in ``--rounds`` alternating windows; every window's
  median is listed and the best is the headline.  Event pairs around a ~10 us launch include the launch gap: upper bounds.
  For the kernel's own time run one case under the profiler:
  rocprofv3 --kernel-trace --stats --output-format csv -d out -- python tools/bench_elastic.py --legs "" --kinds elastic_s32
* fit: ``Model.fit`` scans/s for (a) ``aug_mode "none"``, (e) mode "one" over a flip list with elastic (p = 1, S = 32, 8 px) on
  the device, (f) the same list on the device without elastic, (h) the (e) configuration on the host (over ``--host-scans``
  scans: the numpy path is slow).

Usage: tools/bench_elastic.py [--reps 50] [--rounds 3] [--scans 2048] [--host-scans 128] [--legs aefaefh] [--no-kernel]
                              [--kinds elastic_s32,copy]"""
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
ELASTIC = {"p": 1.0, "spacing": 32, "max_displacement": 8}


def kernel_times(reps, rounds, only=None):
    from oct_image_segmentation_models_amd.engine import UNetEngine
    eng = UNetEngine(device="cuda:0", input_channels=1, num_classes=C, image_height=32, image_width=64, pool_layers=2,
                     max_batch=1, training=False)
    images, labels = make_scans(B, H, W, C, seed=3)
    x = torch.from_numpy(images).cuda()
    lab = torch.from_numpy(np.ascontiguousarray(labels[..., 0])).cuda()
    out = (torch.empty_like(x), torch.empty_like(lab))
    nbytes = x.numel() * 2 + lab.numel() * 2
    cases = {}
    for S in (8, 32, 128):
        for name, amp_x in ((f"elastic_s{S}", 2048), (f"elastic_s{S}_axial", 0)):
            ops = np.zeros(B, dtype=A.ELASTIC_OP_DTYPE)
            ops["kind"], ops["spacing"], ops["amp_x"], ops["amp_y"] = 1, S, amp_x, 2048
            ops["seed_lo"], ops["seed_hi"] = np.arange(B), 7
            A.check_elastic_ops(ops, H, W)
            dev_ops = torch.from_numpy(ops.view(np.uint8).copy()).cuda()
            cases[name] = lambda o=dev_ops: eng.elastic(x, lab, o, out=out)
    none = torch.zeros(B * A.ELASTIC_OP_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    cases["elastic_none"] = lambda: eng.elastic(x, lab, none, out=out)
    th = np.radians(10.0)
    wops = np.zeros(B, dtype=A.WARP_OP_DTYPE)
    wops["kind"] = A.WARP_AFFINE
    wops["p"] = [int(v) for v in np.rint(65536 / 1.05 * np.array([np.cos(th), np.sin(th), -np.sin(th), np.cos(th)]))] + [65536 * 9, -65536 * 5]
    A.check_warp_ops(wops, H, W)
    dev_wops = torch.from_numpy(wops.view(np.uint8).copy()).cuda()
    cases["warp_affine_replicate"] = lambda: eng.warp(x, lab, dev_wops, out=out)
    cases["copy"] = lambda: (out[0].copy_(x), out[1].copy_(lab))
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


def fit_rate(images, labels, mode, device_aug, elastic):
    mc = get_model_class("unet")(input_channels=1, num_classes=C, image_height=H, image_width=W, pool_layers=P)
    model = mc.build_model()
    loss_fn = custom_losses.custom_loss_objects["dice_loss_macro"]["function"](num_classes=C, is_y_true_sparse=False)
    metric_fn = custom_metrics.training_monitor_metric_objects["dice_coef_macro"](False, C)
    model.compile(optimizer=optimizers.Adam(learning_rate=1e-3), loss=loss_fn, metrics=[metric_fn])
    args = ([], "none", ()) if mode == "none" else (FLIPS, "one", PROBS)
    kw = dict(seed=5, device_aug=device_aug, elastic=elastic)
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
    ap.add_argument("--legs", default="aefaefh")
    ap.add_argument("--no-kernel", action="store_true")
    ap.add_argument("--kinds", default="", help="comma-separated subset of the kernel cases (one case per profiler run)")
    a = ap.parse_args()
    res = {"what": f"elastic deformation stage, B={B}, {H}x{W}x1, fit: p=1, S=32, 8 px over a flip list"}
    base_i, base_l = make_scans(64, H, W, C, seed=77)
    legs = {"a": ("fit_none", "none", False, None, a.scans), "e": ("fit_device_elastic", "one", True, ELASTIC, a.scans),
            "f": ("fit_device_flips", "one", True, None, a.scans), "h": ("fit_host_elastic", "one", False, ELASTIC, a.host_scans)}
    for leg in a.legs:      # a leg named twice runs twice ("aeae": alternating, for the spread); every run is listed
        name, mode, dev, elastic, scans = legs[leg]
        reps = max(scans // 64, 1)
        run = fit_rate(np.tile(base_i, (reps, 1, 1, 1))[:scans], np.tile(base_l, (reps, 1, 1, 1))[:scans], mode, dev, elastic)
        res.setdefault(name, []).append(run)
    # (the kernel cases come last, as in tools/bench_warp.py)
    if not a.no_kernel:
        res["kernel"] = kernel_times(a.reps, a.rounds, set(filter(None, a.kinds.split(","))))
    best = lambda name: max(r["scans_per_s"] for r in res[name])     # noqa: E731
    if "fit_device_elastic" in res and "fit_none" in res:
        res["device_over_none"] = round(best("fit_device_elastic") / best("fit_none"), 3)
    if "fit_device_elastic" in res and "fit_host_elastic" in res:
        res["device_over_host"] = round(best("fit_device_elastic") / best("fit_host_elastic"), 1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
