#!/usr/bin/env python3
"""Times the geometric training augmentations (runs on the GPU box; prints one JSON line).

* kernel: ``oct_warp_batch`` per kind at B = 32, 256x512x1, images + labels: HIP events around every launch, median of
  ``--reps`` launches after warm-up, microseconds and GB/s over the bytes moved (u8 images and labels, in and out).  The
  column shift is timed flat (every 4-byte group shares its shift: the word load) and tilted + curved (byte gathers where
  the shift changes inside a group).  Event pairs around a ~10 us launch include the launch gap: upper bounds.  For the
  kernel's own time run one case under the profiler:
  rocprofv3 --kernel-trace --stats --output-format csv -d out -- python tools/bench_warp.py --legs "" --kinds affine_replicate
* fit: ``Model.fit`` scans/s for (a) ``aug_mode "none"``, (b) mode "one" with [column_shift, affine, no_augmentation] applied
  on the host (over ``--host-scans`` scans: the numpy path is slow), (c) the same applied on the device
  (``device_aug=True``: ``oct_warp_batch`` then ``oct_augment_batch``), (d) the flip and noise list of
  tools/bench_augment.py on the device (``oct_augment_batch`` alone).  The device legs and (a) also report what the host
  spends assembling one batch (gather and descriptors, no GPU involved).

Usage: tools/bench_warp.py [--reps 50] [--scans 2048] [--host-scans 256] [--legs adcadcb] [--no-kernel] [--kinds none,affine_replicate]"""
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
AUGS = [(A.column_shift_aug, {"max_shift": 24, "max_tilt": 16, "max_curvature": 8}),
        (A.affine_aug, {"max_rotation": 10, "scale_range": (0.9, 1.1), "max_translate": (16, 8)}), (A.no_aug, {})]
PROBS = (0.4, 0.4, 0.2)
# the list tools/bench_augment.py times: what the flip and noise stage alone costs, in the same run
STAGE_AUGS = [(A.add_noise_aug, {"mode": "gaussian", "variance": 0.01}), (A.flip_aug, {"flip_type": "left-right"}),
              (A.add_noise_aug, {"mode": "speckle"})]


def kernel_times(reps, only=None):
    from oct_image_segmentation_models_amd.engine import UNetEngine
    eng = UNetEngine(device="cuda:0", input_channels=1, num_classes=C, image_height=32, image_width=64, pool_layers=2,
                     max_batch=1, training=False)
    images, labels = make_scans(B, H, W, C, seed=3)
    x = torch.from_numpy(images).cuda()
    lab = torch.from_numpy(np.ascontiguousarray(labels[..., 0])).cuda()
    out = (torch.empty_like(x), torch.empty_like(lab))
    nbytes = x.numel() * 2 + lab.numel() * 2
    th = np.radians(10.0)
    rot = [int(v) for v in np.rint(65536 / 1.05 * np.array([np.cos(th), np.sin(th), -np.sin(th), np.cos(th)]))] + [65536 * 9, -65536 * 5]
    kinds = {"none": (0, 0, [0] * 6), "column_shift_flat": (1, 1, [256 * 17, 0, 0, 0, 0, 0]),
             "column_shift_tilted_curved": (1, 1, [256 * 17 + 40, 256 * 16, -256 * 8, 0, 0, 0]),
             "affine_replicate": (2, 0, rot), "affine_constant": (2, 2, rot)}
    res = {"bytes": nbytes}
    for name, (kind, border, p) in kinds.items():
        if only and name not in only:
            continue
        ops = np.zeros(B, dtype=A.WARP_OP_DTYPE)
        ops["kind"], ops["border"], ops["p"] = kind, border, p
        A.check_warp_ops(ops, H, W)
        dev_ops = torch.from_numpy(ops.view(np.uint8).copy()).cuda()
        for _ in range(5):
            eng.warp(x, lab, dev_ops, out=out)
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
        for e0, e1 in ev:
            e0.record(); eng.warp(x, lab, dev_ops, out=out); e1.record()
        torch.cuda.synchronize()
        us = sorted(e0.elapsed_time(e1) * 1e3 for e0, e1 in ev)[reps // 2]
        res[name] = {"us": round(us, 2), "GB_per_s": round(nbytes / us * 1e-3, 0)}
    return res


def fit_rate(images, labels, mode, device_aug, augs=None):
    mc = get_model_class("unet")(input_channels=1, num_classes=C, image_height=H, image_width=W, pool_layers=P)
    model = mc.build_model()
    loss_fn = custom_losses.custom_loss_objects["dice_loss_macro"]["function"](num_classes=C, is_y_true_sparse=False)
    metric_fn = custom_metrics.training_monitor_metric_objects["dice_coef_macro"](False, C)
    model.compile(optimizer=optimizers.Adam(learning_rate=1e-3), loss=loss_fn, metrics=[metric_fn])
    args = ([], "none", ()) if mode == "none" else (augs or AUGS, "one", PROBS)
    warm = DataGenerator(images[:4 * B], labels[:4 * B], B, *args, True, mc.get_preprocess_input_fn(), seed=5, device_aug=device_aug)
    model.fit(x=warm, epochs=1, verbose=0)
    gen = DataGenerator(images, labels, B, *args, True, mc.get_preprocess_input_fn(), seed=5, device_aug=device_aug)
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
    ap.add_argument("--scans", type=int, default=2048)
    ap.add_argument("--host-scans", type=int, default=256)
    ap.add_argument("--legs", default="adcadcb")
    ap.add_argument("--no-kernel", action="store_true")
    ap.add_argument("--kinds", default="", help="comma-separated subset of the kernel cases (one case per profiler run)")
    a = ap.parse_args()
    res = {"what": f"geometric training augmentations, B={B}, {H}x{W}x1"}
    base_i, base_l = make_scans(64, H, W, C, seed=77)
    legs = {"a": ("fit_none", "none", False, a.scans), "b": ("fit_host_warp", "one", False, a.host_scans),
            "c": ("fit_device_warp", "one", True, a.scans), "d": ("fit_device_flip_noise", "one", True, a.scans)}
    for leg in a.legs:      # a leg named twice runs twice ("acac": alternating, for the spread); every run is listed
        name, mode, dev, scans = legs[leg]
        reps = max(scans // 64, 1)
        run = fit_rate(np.tile(base_i, (reps, 1, 1, 1))[:scans], np.tile(base_l, (reps, 1, 1, 1))[:scans], mode, dev,
                       STAGE_AUGS if leg == "d" else None)
        res.setdefault(name, []).append(run)
    # (the kernel cases come LAST: with an engine of their own built before the fit legs, every third or fourth Model of the
    # process -- un-augmented ones too -- ran at 6.2-6.4 ms per step instead of 3.8; without it none did.  Not understood.)
    if not a.no_kernel:
        res["kernel"] = kernel_times(a.reps, set(filter(None, a.kinds.split(","))))
    best = lambda name: max(r["scans_per_s"] for r in res[name])
    if "fit_device_warp" in res and "fit_none" in res:
        res["device_over_none"] = round(best("fit_device_warp") / best("fit_none"), 3)
    if "fit_device_warp" in res and "fit_host_warp" in res:
        res["device_over_host"] = round(best("fit_device_warp") / best("fit_host_warp"), 1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
