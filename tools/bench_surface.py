"""Times the device surface-distance metrics (oct_surface_distances via evaluation/surface.py) at B = 32, 256x512,
3 classes on clean, 5 %-noise and uniformly random predicted maps (us per scan, CUDA events around repeated calls),
with the numpy host restatement (common/custom_metrics.py) on a few scans beside it.  Prints one JSON line.
Usage: python tools/bench_surface.py [--reps 20] [--host-scans 2]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oct_image_segmentation_models_amd.common import custom_metrics as cm  # noqa: E402
from oct_image_segmentation_models_amd.evaluation.surface import SPACING, SurfaceDistances  # noqa: E402
from oracle import unet_numpy as on  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-scans", type=int, default=2)
    a = ap.parse_args()
    B, H, W, C = 32, 256, 512, 3
    _, lab = on.synth_scans(B, H, W, C, seed=1)
    gt = lab[..., 0]
    rng = np.random.default_rng(0)
    noisy = gt.copy()
    flip = rng.random(gt.shape) < 0.05
    noisy[flip] = rng.integers(0, C, int(flip.sum()))
    cases = {"clean": np.roll(gt, 1, axis=1), "noise5": noisy, "random": rng.integers(0, C, gt.shape).astype(np.uint8)}
    sd = SurfaceDistances(B, H, W, C, "cuda:0")
    g = torch.from_numpy(gt).cuda()
    res = {"what": f"oct_surface_distances, B={B}, {H}x{W}, {C} classes, both directions, ASD + percentile 95",
           "workspace_MiB": round(sd.workspace.numel() / 2**20, 1)}
    for name, pred in cases.items():
        p = torch.from_numpy(pred).cuda()
        for _ in range(3):
            rows = sd(p, g)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.reps):
            sd(p, g)
        e1.record()
        torch.cuda.synchronize()
        dev_us = e0.elapsed_time(e1) * 1e3 / a.reps / B
        t0 = time.perf_counter()
        for b in range(a.host_scans):
            for c in range(1, C):
                cm.compute_surface_distances(gt[b] == c, pred[b] == c, SPACING)
        host_us = (time.perf_counter() - t0) * 1e6 / a.host_scans
        res[name] = {"device_us_per_scan": round(dev_us, 2), "host_numpy_us_per_scan": round(host_us, 1),
                     "surfels_per_class_gt": int(rows[..., 4].float().mean().item()),
                     "surfels_per_class_pred": int(rows[..., 5].float().mean().item())}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
