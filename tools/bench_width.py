"""Times a training step (forward, Dice-macro loss, backward, Adam) at start_neurons 32 and 64 on one MI355X: fp32, 256x512x1,
3 classes, pool_layers 4, batch 8.

* start_neurons 32 with the register head kernels (``head_wide`` 0) and with the channel-streaming ones (``head_wide`` 1) on
  the same handle and inputs, alternated;
* start_neurons 64, which always runs the channel-streaming head.

For each: B-scans/s over the timed steps, and from the per-launch profiler (a few further untimed steps, launches
serialised) the two head kernels' ms per step and bytes/s by the profiler's own byte model (backward: px * (cin * 4 * 2 + 1)).
At start_neurons 64 also the share of the profiled step taken by the three layers whose K = 1024 input channels exceed what
the bf16-pipe kernels place (mid.conv1, dec0.up, dec0.conv0: fp32-pipe forward, and for the first two an fp32-pipe
backward-data launch with a separate bn_bwd_apply pass), with the kernels that ran them.

Prints one JSON line.  Usage: python tools/bench_width.py [--steps 100] [--warmup 10] [--reps 3] [--profile-steps 3]"""
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
from oct_image_segmentation_models_amd.engine import UNetEngine  # noqa: E402

FALLBACK_LAYERS = ("mid.conv1", "dec0.up", "dec0.conv0")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--profile-steps", type=int, default=3)
    a = ap.parse_args()
    B, H, W, C, P = 8, 256, 512, 3, 4
    images, labels = make_scans(B, H, W, C, seed=1234)
    x = torch.from_numpy(images).cuda()
    lab = torch.from_numpy(labels[..., 0].copy()).cuda()

    def engine(sn):
        return UNetEngine(device="cuda:0", input_channels=1, num_classes=C, image_height=H, image_width=W, max_batch=B,
                          training=True, seed=1000, init_seed=0, pool_layers=P, start_neurons=sn)

    def step(eng):
        eng.forward(x, training=True, labels=lab, want_probs=False)
        v = eng.loss_dice()
        eng.backward(lab, macro=True, loss_scale=1.0)
        eng.adam_step(lr=1e-3)
        return v

    def scans_per_s(eng):
        for _ in range(a.warmup):
            step(eng)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            v = step(eng)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        assert np.isfinite(v.cpu().numpy()).all()
        return B * a.steps / dt

    def stats(v, digits=1):
        v = sorted(v)
        return {"median": round(v[len(v) // 2], digits), "min": round(v[0], digits), "max": round(v[-1], digits)}

    def profile(eng, sn):
        for _ in range(3):
            step(eng)
        eng.profile_begin()
        for _ in range(a.profile_steps):
            eng.forward(x, training=True, labels=lab, want_probs=False)
            eng.loss_dice(); eng.backward(lab, macro=True, loss_scale=1.0)
        ents = eng.profile_end()
        total = sum(e["total_ms"] for e in ents)
        out = {"profiled_step_ms": round(total / a.profile_steps, 4)}
        for e in ents:
            if e["layer"] == "head" and e["kernel"].startswith(("head_fwd", "head_bwd")):
                out[e["kernel"]] = {"ms_per_step": round(e["total_ms"] / a.profile_steps, 4),
                                    "GBps": round(e["bytes"] / (e["total_ms"] * 1e-3) / 1e9, 1)}
        if sn == 64:
            fb = {}
            for e in ents:
                if e["layer"] in FALLBACK_LAYERS:
                    d = fb.setdefault(e["layer"], {"ms_per_step": 0.0, "kernels": []})
                    d["ms_per_step"] += e["total_ms"] / a.profile_steps
                    d["kernels"].append(e["kernel"])
            for d in fb.values():
                d["ms_per_step"] = round(d["ms_per_step"], 4); d["kernels"] = sorted(set(d["kernels"]))
            out["fp32_fallback_layers"] = fb
            out["fp32_fallback_share_of_step"] = round(sum(d["ms_per_step"] for d in fb.values()) * a.profile_steps / total, 4)
        return out

    res = {"what": f"train step, fp32, {H}x{W}x1, {C} classes, pool_layers {P}, batch {B}", "steps": a.steps, "warmup": a.warmup,
           "reps": a.reps, "profile_steps": a.profile_steps}
    eng = engine(32)
    rates = {0: [], 1: []}
    for _ in range(a.reps):                      # alternated: both settings see the same clock and thermal state
        for hw in (0, 1):
            eng.set_option("head_wide", hw)
            rates[hw].append(scans_per_s(eng))
    for hw in (0, 1):
        eng.set_option("head_wide", hw)
        res[f"start_neurons_32_head_wide_{hw}"] = dict(scans_per_s=stats(rates[hw]), **profile(eng, 32))
    del eng
    torch.cuda.empty_cache()
    eng = engine(64)
    res["start_neurons_64"] = dict(scans_per_s=stats([scans_per_s(eng) for _ in range(a.reps)]), **profile(eng, 64))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
