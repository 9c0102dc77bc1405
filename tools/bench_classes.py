"""Times the head kernels and a whole training step (forward with probabilities and arg-max, Dice-macro loss, backward, Adam)
across class counts on one MI355X: fp32, 256x512x1, start_neurons 8, pool_layers 4, batch 32.

* 8 classes with the register head kernels (``head_wide`` 0) and with the channel-streaming ones (``head_wide`` 1): the
  yardstick pair of the same run;
* 9, 12, 13 and 16 classes, which always run the class-streaming kernels (kernels_head_cls.hpp); 12 is the last count
  with Dice rows of 64 floats, 13 the first with rows of 96;
* 8 classes (``head_wide`` 1) and 16 classes once more under ``bce_dice_loss``: the O(C^2) complement and Jacobian loops.

Per configuration: B-scans/s over the timed steps (the configurations are alternated inside every repetition, each on an
engine of its own that lives for that measurement only), and from the per-launch profiler -- further untimed steps, launches
serialised, ``--windows`` windows of ``--profile-steps`` steps per repetition --
the sum of a step's launch times (``profiled_step_ms``; forward, loss, backward, no optimizer) and each head kernel's time
per launch with the bytes it has to move per second:
    forward   px * (4 CIN + 4 C + 1 + 1)     z read, probabilities and arg-max written, labels read
    backward  px * (8 CIN + 1)               z read, g written, labels read
(the second read of z in the streaming backward kernels comes from L2 and is not counted).  Median, min and max are over the
windows; the spread of the yardstick pair is the bound the other rows are read against.

Prints one JSON line.  Usage: python tools/bench_classes.py [--steps 40] [--warmup 5] [--reps 3] [--windows 2] [--profile-steps 4]
                                                [--configs C8_register,C16,...]"""
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

B, H, W, SN, P = 32, 256, 512, 8, 4
# name -> (classes, head_wide, loss)
CONFIGS = {"C8_register": (8, 0, "dice"), "C8_head_wide": (8, 1, "dice"), "C9": (9, 0, "dice"), "C12": (12, 0, "dice"),
           "C13": (13, 0, "dice"), "C16": (16, 0, "dice"), "C8_head_wide_bce": (8, 1, "bce"), "C16_bce": (16, 0, "bce")}


def head_bytes(kernel: str, C: int) -> float:
    px = float(B * H * W)
    return px * (4 * SN + 4 * C + 1 + 1) if kernel.startswith("head_fwd") else px * (8 * SN + 1)


def stats(v, digits):
    v = sorted(v)
    return {"median": round(v[len(v) // 2], digits), "min": round(v[0], digits), "max": round(v[-1], digits)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--windows", type=int, default=2)
    ap.add_argument("--profile-steps", type=int, default=4)
    ap.add_argument("--configs", default=",".join(CONFIGS), help="comma-separated names out of " + ", ".join(CONFIGS) +
                    ": which configurations run, in this order")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_classes.py needs the GPU: nothing is measured without one")

    names = a.configs.split(",")
    rates = {name: [] for name in names}
    per = {name: {} for name in names}           # name -> kernel -> [us per launch of each window]
    whole = {name: [] for name in names}         # name -> [ms of all launches of a step, serialised, of each window]

    def measure(name):
        """One engine, alive for this call only: a handle owns a side stream, and with several handles alive the streams
        of the later ones share hardware queues -- their steps lose the overlap (measured: the fourth engine of a process
        steps at 0.6 of its rate alone)."""
        C, wide, loss = CONFIGS[name]
        images, labels = make_scans(B, H, W, C, seed=1234)
        eng = UNetEngine(device="cuda:0", input_channels=1, num_classes=C, image_height=H, image_width=W, max_batch=B,
                         training=True, seed=1000, init_seed=0, pool_layers=P, start_neurons=SN, max_classes=16)
        eng.set_option("head_wide", wide)
        if loss == "bce":
            eng.set_bce_dice(True)
        x, lab = torch.from_numpy(images).cuda(), torch.from_numpy(labels[..., 0].copy()).cuda()
        # the step's outputs go into fixed buffers, as a training loop keeps them
        probs = torch.empty((B, H, W, C), dtype=torch.float32, device="cuda:0")
        am = torch.empty((B, H, W), dtype=torch.uint8, device="cuda:0")

        def step(adam=True):
            eng.forward(x, training=True, labels=lab, want_probs=True, want_argmax=True, probs_out=probs, argmax_out=am)
            v = eng.loss_bce_dice() if loss == "bce" else eng.loss_dice()
            eng.backward(lab, macro=loss != "bce", loss_scale=1.0)
            if adam:
                eng.adam_step(lr=1e-3)
            return v

        for _ in range(a.warmup):
            step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            v = step()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        assert np.isfinite(v.cpu().numpy()).all()
        rates[name].append(B * a.steps / dt)
        for _ in range(a.windows):
            step(adam=False)
            eng.profile_begin()
            for _ in range(a.profile_steps):
                step(adam=False)
            ents = eng.profile_end()
            whole[name].append(sum(e["total_ms"] for e in ents) / a.profile_steps)
            for e in ents:
                if e["layer"] == "head" and e["kernel"].startswith(("head_fwd", "head_bwd")):
                    per[name].setdefault(e["kernel"], []).append(e["total_ms"] * 1e3 / e["launches"])
        torch.cuda.synchronize()
        del eng
        torch.cuda.empty_cache()

    for _ in range(a.reps):                      # alternated: every configuration sees the same clock and thermal state
        for name in names:
            measure(name)

    res = {"what": f"train step, fp32, {H}x{W}x1, start_neurons {SN}, pool_layers {P}, batch {B}", "steps": a.steps,
           "warmup": a.warmup, "reps": a.reps, "windows": a.windows, "profile_steps": a.profile_steps, "configs": {}}
    for name in names:
        C, _, loss = CONFIGS[name]
        out = {"classes": C, "loss": loss, "scans_per_s": stats(rates[name], 1), "profiled_step_ms": stats(whole[name], 3),
               "kernels": {}}
        for k, us in per[name].items():
            by = head_bytes(k, C)
            out["kernels"][k] = {"us_per_launch": stats(us, 1), "bytes": by,
                                 "GBps": stats([by / (u * 1e-6) / 1e9 for u in us], 1)}
        res["configs"][name] = out
    print(json.dumps(res))


if __name__ == "__main__":
    main()
