"""What a shape of the Dice term costs at B = 32, 256x512, 3 classes, fp32, four pool levels:

* ``--leg kernels``: dice_shape_finalize_k against dice_finalize_k, per-launch time from the engine's per-launch profiler, shape
  off and on alternated on one engine; a window is ``--steps`` training steps;
* ``--leg steps`` (default): the train-step rate (forward + loss + backward + Adam, not profiled) in scans/s with the shape off
  and on, alternated on one engine; a window is ``--steps`` steps between two synchronisations.

The shape is Tversky 0.3 / 0.7, g = 0.75 with "volume" weights (every pass of the kernel runs); ``--shape tversky`` drops the
exponent and the weights.  The median of ``--windows`` windows is reported with the spread; the spread of the off windows is
the run-to-run noise the on / off ratio is read against.  One leg per run; prints one JSON line.
Usage: python tools/bench_dice_shape.py [--leg steps|kernels] [--windows 7] [--steps 100] [--shape full|tversky] [--first off|on]"""
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

B, H, W, C, P = 32, 256, 512, 3, 4
SHAPES = {"full": dict(alpha=0.3, beta=0.7, gamma=0.75, class_weight="volume"), "tversky": dict(alpha=0.3, beta=0.7)}
FIN = {False: "dice_finalize_k", True: "dice_shape_finalize_k"}


def stats(v, digits=4):
    v = sorted(v)
    return {"median": round(v[len(v) // 2], digits), "min": round(v[0], digits), "max": round(v[-1], digits)}


def setup():
    eng = UNetEngine(device="cuda:0", input_channels=1, num_classes=C, image_height=H, image_width=W, max_batch=B,
                     training=True, seed=1000, init_seed=0, pool_layers=P)
    images, labels = make_scans(8, H, W, C, seed=1234)
    x = torch.from_numpy(np.tile(images, (B // 8, 1, 1, 1))).to(eng.device)
    lab = torch.from_numpy(np.tile(labels, (B // 8, 1, 1, 1))).to(eng.device)
    return eng, x, lab


def run_steps(eng, x, lab, n, adam):
    for _ in range(n):
        eng.forward(x, training=True, labels=lab, want_probs=False)
        eng.loss_dice()
        eng.backward(lab, macro=True, loss_scale=1.0)
        if adam:
            eng.adam_step(lr=1e-4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--leg", choices=["steps", "kernels"], default="steps")
    ap.add_argument("--shape", choices=sorted(SHAPES), default="full")
    ap.add_argument("--first", choices=["off", "on"], default="off", help="which setting goes first in every window pair")
    a = ap.parse_args()
    eng, x, lab = setup()
    order = (False, True) if a.first == "off" else (True, False)
    select = lambda on: eng.set_dice_shape(**SHAPES[a.shape]) if on else eng.set_dice_shape(None)      # noqa: E731
    res = {"what": f"shape of the Dice term ({a.shape}: {SHAPES[a.shape]}), B={B}, {H}x{W}, {C} classes, fp32", "leg": a.leg,
           "windows": a.windows, "steps_per_window": a.steps, "first": a.first}
    for on in order:                                          # warm both settings
        select(on); run_steps(eng, x, lab, 3, a.leg == "steps")
    torch.cuda.synchronize()
    got = {False: [], True: []}
    for _ in range(a.windows):
        for on in order:
            select(on)
            if a.leg == "kernels":
                eng.profile_begin()
                run_steps(eng, x, lab, a.steps, False)
                torch.cuda.synchronize()
                ent = {e["kernel"]: e for e in eng.profile_end()}
                assert FIN[on] in ent and FIN[not on] not in ent, sorted(ent)
                got[on].append(ent[FIN[on]]["total_ms"] / ent[FIN[on]]["launches"] * 1e3)
            else:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run_steps(eng, x, lab, a.steps, True)
                torch.cuda.synchronize()
                got[on].append(a.steps * B / (time.perf_counter() - t0))
    off, on = stats(got[False], 2), stats(got[True], 2)
    key = "finalize_us_per_launch" if a.leg == "kernels" else "train_step_scans_per_s"
    res[key] = {"shape_off": off, "shape_on": on, "on_over_off": round(on["median"] / off["median"], 4),
                "off_spread": round((off["max"] - off["min"]) / off["median"], 4)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
