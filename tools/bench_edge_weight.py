#!/usr/bin/env python3
"""Times the boundary-weighted pixel loss (runs on the GPU box; prints one JSON line).

* kernel: ``oct_edge_weight_map`` at B = 32, 256x512, R = 3 and R = 15, on clean layered labels and on labels with 0.5 % of
  the pixels relabelled at random: HIP events around every launch, median of ``--reps`` launches after warm-up, microseconds
  and GB/s over the bytes it must move (1 read + 4 written per pixel).  Beside them, in the same run and measured the same way:
  a device copy that moves the same number of bytes (2.5 read + 2.5 written per pixel).  The cases are timed in ``--rounds``
  alternating windows; every window's median is listed and the best is the headline.  Event pairs around a short launch
  include the launch gap: upper bounds.
* head: per-launch times of the benched head pair (head_fwd_k / head_bwd_k<3,8,float>, focal_dice_loss) from the engine's own
  profiler, without and with a map, in ``--rounds`` alternating windows of ``--steps`` training steps.
* fit: ``Model.fit`` scans/s with focal_dice_loss, without and with ``edge_weight`` (gauss, R = 3), legs alternated.

Usage: tools/bench_edge_weight.py [--reps 50] [--rounds 3] [--steps 10] [--scans 1024] [--legs pepe] [--no-kernel] [--no-head]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oct_image_segmentation_models_amd import optimizers  # noqa: E402
from oct_image_segmentation_models_amd.common import custom_losses, custom_metrics  # noqa: E402
from oct_image_segmentation_models_amd.common.data_generator import DataGenerator  # noqa: E402
from oct_image_segmentation_models_amd.common.synthetic import make_scans  # noqa: E402
from oct_image_segmentation_models_amd.common.utils import edge_weight_lut  # noqa: E402
from oct_image_segmentation_models_amd.models import get_model_class  # noqa: E402

H, W, C, P, B = 256, 512, 3, 4, 32
SPEC = {"radius": 3, "weight": 10.0, "profile": "gauss", "sigma": 1.5}


def _median_windows(cases, reps, rounds):
    res = {}
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
    return res


def kernel_times(eng, reps, rounds):
    _, labels = make_scans(B, H, W, C, seed=3)
    clean = np.ascontiguousarray(labels[..., 0])
    rng = np.random.default_rng(1)
    noisy = clean.copy()
    flip = rng.random(noisy.shape) < 0.005
    noisy[flip] = rng.integers(0, C, int(flip.sum()))
    n = clean.size
    out = torch.empty((B, H, W), dtype=torch.float32, device="cuda")
    cases = {}
    for tag, lab in (("clean", clean), ("noise", noisy)):
        dev = torch.from_numpy(lab).cuda()
        for R in (3, 15):
            lut = torch.from_numpy(edge_weight_lut(R, "gauss", 10.0, R / 2.0)).cuda()
            cases[f"map_r{R}_{tag}"] = lambda d=dev, r=R, t=lut: eng.edge_weight_map(d, r, t, out=out)
    src = torch.zeros(5 * n // 2, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    cases["copy"] = lambda: dst.copy_(src)
    res = _median_windows(cases, reps, rounds)
    for name in cases:
        best = min(res[name]["us_windows"])
        res[name].update(us=best, GB_per_s=round(5 * n / best * 1e-3, 0))
    res["bytes"] = 5 * n
    return res


def head_times(steps, rounds):
    from oct_image_segmentation_models_amd.engine import UNetEngine
    eng = UNetEngine(device="cuda:0", input_channels=1, num_classes=C, image_height=H, image_width=W, pool_layers=P,
                     max_batch=B, training=True)
    images, labels = make_scans(B, H, W, C, seed=5)
    x = torch.from_numpy(images).cuda()
    lab = torch.from_numpy(np.ascontiguousarray(labels[..., 0])).cuda()
    eng.set_focal_dice(0.5, 2.0)
    wmap = eng.edge_weight_map(lab, SPEC["radius"], edge_weight_lut(**SPEC))
    res = {"off": [], "map": []}
    for _ in range(rounds):
        for name, w in (("off", None), ("map", wmap)):
            eng.set_pixel_weights(w)
            for _ in range(2):
                eng.forward(x, training=True, labels=lab, want_probs=False); eng.loss_focal_dice(); eng.backward(lab)
            eng.profile_begin()
            for _ in range(steps):
                eng.forward(x, training=True, labels=lab, want_probs=False); eng.loss_focal_dice(); eng.backward(lab)
            torch.cuda.synchronize()
            t = {e["kernel"]: e["total_ms"] / e["launches"] * 1e3 for e in eng.profile_end() if e["kernel"].startswith("head_")}
            res[name].append({k: round(v, 2) for k, v in sorted(t.items())})
    return res


def fit_rate(images, labels, edge_weight):
    mc = get_model_class("unet")(input_channels=1, num_classes=C, image_height=H, image_width=W, pool_layers=P)
    model = mc.build_model()
    kw = {"edge_weight": edge_weight} if edge_weight else {}
    loss_fn = custom_losses.custom_loss_objects["focal_dice_loss"]["function"](num_classes=C, is_y_true_sparse=True, **kw)
    metric_fn = custom_metrics.training_monitor_metric_objects["dice_coef_macro"](True, C)
    model.compile(optimizer=optimizers.Adam(learning_rate=1e-3), loss=loss_fn, metrics=[metric_fn])
    warm = DataGenerator(images[:4 * B], labels[:4 * B], B, [], "none", (), True, mc.get_preprocess_input_fn(), seed=5)
    model.fit(x=warm, epochs=1, verbose=0)
    gen = DataGenerator(images, labels, B, [], "none", (), True, mc.get_preprocess_input_fn(), seed=5)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    model.fit(x=gen, epochs=1, verbose=0)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return {"scans_per_s": round(len(gen) * B / dt, 1), "ms_per_step": round(dt / len(gen) * 1e3, 3), "steps": len(gen)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--scans", type=int, default=1024)
    ap.add_argument("--legs", default="pepe", help="p: plain focal_dice_loss, e: with edge_weight; a leg named twice runs twice")
    ap.add_argument("--no-kernel", action="store_true")
    ap.add_argument("--no-head", action="store_true")
    a = ap.parse_args()
    res = {"what": f"edge weight map + weighted head, B={B}, {H}x{W}, fit: focal_dice_loss, edge_weight {SPEC}"}
    if not a.no_kernel:
        from oct_image_segmentation_models_amd.engine import UNetEngine
        small = UNetEngine(device="cuda:0", input_channels=1, num_classes=C, image_height=32, image_width=64, pool_layers=2,
                           max_batch=1, training=False)
        res["kernel"] = kernel_times(small, a.reps, a.rounds)
    if not a.no_head:
        res["head_us_per_launch"] = head_times(a.steps, a.rounds)
    if a.legs:
        base_i, base_l = make_scans(64, H, W, C, seed=77)
        reps = max(a.scans // 64, 1)
        images, labels = np.tile(base_i, (reps, 1, 1, 1))[:a.scans], np.tile(base_l, (reps, 1, 1, 1))[:a.scans]
        for leg in a.legs:
            res.setdefault({"p": "fit_plain", "e": "fit_edge_weight"}[leg], []).append(fit_rate(images, labels, SPEC if leg == "e" else None))
        if "fit_plain" in res and "fit_edge_weight" in res:
            best = lambda k: max(r["scans_per_s"] for r in res[k])     # noqa: E731
            res["edge_over_plain"] = round(best("fit_edge_weight") / best("fit_plain"), 4)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
