"""Times the Monte-Carlo dropout prediction at B = 32, 256x512x1, 3 classes, fp32:

* ``oct_mc_update`` per call -- a middle sample (reads p and S, writes S; reads and writes E) and the last one (reads p,
  S and E, writes the maps) -- and its achieved bytes/s against the bytes that call must move;
* ``forward_mc`` for T = 1, 8, 16, 32, with a plain non-graph ``forward(training=False)`` of the same batch alternated with
  them in the same run.  T stochastic predictions cost one encoder pass plus T decoder passes, so for T >= 8
  ``forward_mc(T)`` must take less than T plain forwards: the tool checks it and exits non-zero otherwise.

Every shape is warmed up before it is timed, a timed window is ``--reps`` repetitions between two device events, and the
median of ``--windows`` windows is reported with the spread.  Prints one JSON line.
Usage: python tools/bench_mc.py [--reps 10] [--windows 5] [--kernel-reps 50]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oct_image_segmentation_models_amd import _hip  # noqa: E402
from oct_image_segmentation_models_amd.common.synthetic import make_scans  # noqa: E402
from oct_image_segmentation_models_amd.engine import UNetEngine  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--kernel-reps", type=int, default=50)
    a = ap.parse_args()
    B, H, W, C = 32, 256, 512, 3
    eng = UNetEngine(device="cuda:0", input_channels=1, num_classes=C, image_height=H, image_width=W, max_batch=B,
                     training=False, seed=1000, init_seed=0)
    images, _ = make_scans(8, H, W, C, seed=1234)
    x = torch.from_numpy(np.tile(images, (B // 8, 1, 1, 1))).to(eng.device)

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

    res = {"what": f"Monte-Carlo dropout prediction, B={B}, {H}x{W}x1, {C} classes, fp32", "reps": a.reps, "windows": a.windows,
           "kernel_reps": a.kernel_reps}

    # ---- the reduction kernel on the net's own softmax output ----
    probs, _ = eng.forward(x, training=False)
    bufs = eng._mc_buffers(B)
    outs = {k: bufs[k] for k in ("mean_probs", "argmax", "entropy", "mutual_info")}
    eng.mc_update(probs, 0, 3, bufs["ws"])
    npix = B * H * W
    kernel = {}
    for name, t, kw, nbytes in (("middle_sample", 1, {}, npix * (3 * C + 2) * 4),
                                ("last_sample_all_maps", 2, outs, npix * ((2 * C + 1) * 4 + C * 4 + 1 + 8))):
        call = lambda: eng.mc_update(probs, t, 3, bufs["ws"], **kw)      # noqa: E731
        for _ in range(5):
            call()
        torch.cuda.synchronize()
        ms = stats([window(call, a.kernel_reps) for _ in range(a.windows)])
        kernel[name] = {"ms_per_call": ms, "bytes_moved": int(nbytes), "GBps": round(nbytes / (ms["median"] * 1e-3) / 1e9, 1)}
    res["oct_mc_update"] = kernel

    # ---- forward_mc against the plain forward, alternated ----
    Ts = (1, 8, 16, 32)
    plain = lambda: eng.forward(x, training=False, probs_out=probs)       # noqa: E731
    calls = {T: (lambda T=T: eng.forward_mc(x, T, step0=0)) for T in Ts}
    for f in (plain, *calls.values()):
        f(); f()
    torch.cuda.synchronize()
    t_plain, t_mc = [], {T: [] for T in Ts}
    for _ in range(a.windows):
        t_plain.append(window(plain, a.reps))
        for T in Ts:
            t_mc[T].append(window(calls[T], max(1, a.reps // max(1, T // 4))))
    p = stats(t_plain)
    res["forward_plain_ms"] = p
    res["forward_mc_ms"] = {str(T): stats(t_mc[T]) for T in Ts}
    res["forward_mc_over_T_plain"] = {str(T): round(stats(t_mc[T])["median"] / (T * p["median"]), 3) for T in Ts}
    res["encoder_reused"] = all(stats(t_mc[T])["median"] < T * p["median"] for T in Ts if T >= 8)
    print(json.dumps(res))
    if not res["encoder_reused"]:
        sys.exit("forward_mc(T) took at least T plain forwards for some T >= 8: the encoder is not being reused")


if __name__ == "__main__":
    main()
