#!/usr/bin/env python3
"""Times the training augmentations (runs on the GPU box; prints one JSON line).

* kernel: ``oct_augment_batch`` per kind at B = 32, 256x512x1, images + labels: HIP events around every launch, median
  of ``--reps`` launches after warm-up, microseconds and GB/s over the bytes moved (u8 in + f32 out + labels in and out).
* fit: ``Model.fit`` scans/s over ``--scans`` scans for (a) ``aug_mode "none"``, (b) mode "one" with [gaussian
  variance 0.01, flip left-right, speckle] applied on the host, (c) the same applied on the device (``device_aug=True``).

A tree without the device path (no ``device_aug`` keyword) runs legs (a) and (b) only, so the same file measures the
commit before the feature.  Event pairs around a ~10 us launch include the launch gap; for the kernel's own time run one
kind under the profiler: rocprofv3 --kernel-trace --stats -d out -- python tools/bench_augment.py --legs "" --kinds gaussian
Usage: tools/bench_augment.py [--reps 50] [--scans 2048] [--legs abc] [--no-kernel] [--kinds none,gaussian]"""
import argparse
import inspect
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
AUGS = [(A.add_noise_aug, {"mode": "gaussian", "variance": 0.01}), (A.flip_aug, {"flip_type": "left-right"}),
        (A.add_noise_aug, {"mode": "speckle"})]
HAS_DEVICE_AUG = "device_aug" in inspect.signature(DataGenerator.__init__).parameters


def kernel_times(reps, only=None):
    from oct_image_segmentation_models_amd.engine import UNetEngine
    eng = UNetEngine(device="cuda:0", input_channels=1, num_classes=C, image_height=32, image_width=64, pool_layers=2,
                     max_batch=1, training=False)
    images, labels = make_scans(B, H, W, C, seed=3)
    x = torch.from_numpy(images).cuda()
    lab = torch.from_numpy(np.ascontiguousarray(labels[..., 0])).cuda()
    out = (torch.empty(x.shape, dtype=torch.float32, device="cuda"), torch.empty_like(lab))
    nbytes = x.numel() * 5 + lab.numel() * 2
    kinds = {"none": (0, 0, 0), "flip_up_down": (1, 0, 0), "flip_left_right": (2, 0, 0), "gaussian": (3, 0.0, 0.1),
             "speckle": (4, 0.0, 0.1), "salt_and_pepper": (5, 0.05, 0.5)}
    res = {"bytes": nbytes}
    for name, (kind, p0, p1) in kinds.items():
        if only and name not in only:
            continue
        ops = np.zeros(B, dtype=A.AUG_OP_DTYPE)
        ops["kind"], ops["p0"], ops["p1"], ops["noise_id"] = kind, p0, p1, np.arange(B)
        dev_ops = torch.from_numpy(ops.view(np.uint8).copy()).cuda()
        for _ in range(5):
            eng.augment(x, lab, dev_ops, 7, out=out)
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
        for e0, e1 in ev:
            e0.record(); eng.augment(x, lab, dev_ops, 7, out=out); e1.record()
        torch.cuda.synchronize()
        us = sorted(e0.elapsed_time(e1) * 1e3 for e0, e1 in ev)[reps // 2]
        res[name] = {"us": round(us, 2), "GB_per_s": round(nbytes / us * 1e-3, 0)}
    return res


def fit_rate(images, labels, mode, device_aug):
    mc = get_model_class("unet")(input_channels=1, num_classes=C, image_height=H, image_width=W, pool_layers=P)
    model = mc.build_model()
    loss_fn = custom_losses.custom_loss_objects["dice_loss_macro"]["function"](num_classes=C, is_y_true_sparse=False)
    metric_fn = custom_metrics.training_monitor_metric_objects["dice_coef_macro"](False, C)
    model.compile(optimizer=optimizers.Adam(learning_rate=1e-3), loss=loss_fn, metrics=[metric_fn])
    kw = {"device_aug": True} if device_aug else {}
    args = ([], "none", ()) if mode == "none" else (AUGS, "one", (0.4, 0.2, 0.4))
    warm = DataGenerator(images[:4 * B], labels[:4 * B], B, *args, True, mc.get_preprocess_input_fn(), seed=5, **kw)
    model.fit(x=warm, epochs=1, verbose=0)
    gen = DataGenerator(images, labels, B, *args, True, mc.get_preprocess_input_fn(), seed=5, **kw)
    assert not device_aug or gen.oct_device_aug
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    model.fit(x=gen, epochs=1, verbose=0)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return {"scans_per_s": round(len(gen) * B / dt, 1), "ms_per_step": round(dt / len(gen) * 1e3, 3), "steps": len(gen)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--scans", type=int, default=2048)
    ap.add_argument("--legs", default="abc")
    ap.add_argument("--no-kernel", action="store_true")
    ap.add_argument("--kinds", default="", help="comma-separated subset of the kernel kinds (one kind per profiler run)")
    a = ap.parse_args()
    res = {"what": f"training augmentations, B={B}, {H}x{W}x1", "device_path": HAS_DEVICE_AUG}
    if HAS_DEVICE_AUG and not a.no_kernel:
        res["kernel"] = kernel_times(a.reps, set(filter(None, a.kinds.split(","))))
    base_i, base_l = make_scans(64, H, W, C, seed=77)
    images = np.tile(base_i, (a.scans // 64, 1, 1, 1)); labels = np.tile(base_l, (a.scans // 64, 1, 1, 1))
    legs = {"a": ("fit_none", "none", False), "b": ("fit_host_aug", "one", False), "c": ("fit_device_aug", "one", True)}
    for leg in a.legs:
        name, mode, dev = legs[leg]
        if dev and not HAS_DEVICE_AUG:
            continue
        res[name] = fit_rate(images, labels, mode, dev)
    if "fit_device_aug" in res and "fit_none" in res:
        res["device_over_none"] = round(res["fit_device_aug"]["scans_per_s"] / res["fit_none"]["scans_per_s"], 3)
    if "fit_device_aug" in res and "fit_host_aug" in res:
        res["device_over_host"] = round(res["fit_device_aug"]["scans_per_s"] / res["fit_host_aug"]["scans_per_s"], 1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
