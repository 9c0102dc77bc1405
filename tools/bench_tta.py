"""Times test-time augmentation at B = 32, 256x512x1 uint8 scans, 3 classes, fp32:

* ``oct_flip_batch`` of the uint8 input batch per view, and its achieved bytes/s (read + write);
* ``oct_tta_update`` per sample -- a middle sample and the last one with all maps, per view -- with ``oct_mc_update`` at the
  same shape ALTERNATED with it in the same windows: the two move the same bytes, so ``oct_mc_update`` is the yardstick and
  its own spread over the windows is the noise floor;
* the replayed TTA graph for T = 2 and T = 4, alternated with T replays of the plain inference graph (a second engine
  with the same weights: an engine holds one captured graph);
* ``Model.predict_labels`` per scan over 64 scans, without and with ``tta`` (host time, upload and download included).

Every shape is warmed up before it is timed, a timed window is a number of repetitions between two device events, and the
median of ``--windows`` windows is reported with the spread.  Prints one JSON line.
Usage: python tools/bench_tta.py [--reps 10] [--windows 7] [--kernel-reps 50]"""
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
from oct_image_segmentation_models_amd.common.utils import TTA_VIEW_NAMES  # noqa: E402
from oct_image_segmentation_models_amd.engine import UNetEngine  # noqa: E402
from oct_image_segmentation_models_amd.models.engine_model import Model  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--kernel-reps", type=int, default=50)
    a = ap.parse_args()
    B, H, W, C = 32, 256, 512, 3
    kw = dict(device="cuda:0", input_channels=1, num_classes=C, image_height=H, image_width=W, max_batch=B, training=False,
              seed=1000, init_seed=0)
    eng, eng_plain = UNetEngine(**kw), UNetEngine(**kw)
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

    def alternated(calls, reps):
        """{name: call} -> {name: stats}: every window times each call once, in turn, after a warm-up of each."""
        for f in calls.values():
            f(); f()
        torch.cuda.synchronize()
        t = {k: [] for k in calls}
        for _ in range(a.windows):
            for k, f in calls.items():
                t[k].append(window(f, reps))
        return {k: stats(v) for k, v in t.items()}

    res = {"what": f"test-time augmentation, B={B}, {H}x{W}x1 uint8, {C} classes, fp32", "reps": a.reps, "windows": a.windows,
           "kernel_reps": a.kernel_reps}

    # ---- the flip of the input batch ----
    x_view = torch.empty_like(x)
    flips = alternated({name: (lambda v=v: eng.flip(x, v, out=x_view)) for v, name in enumerate(TTA_VIEW_NAMES)}, a.kernel_reps)
    nbytes = 2 * x.numel()
    res["oct_flip_batch"] = {k: {"ms_per_call": s, "bytes_moved": nbytes, "GBps": round(nbytes / (s["median"] * 1e-3) / 1e9, 1)}
                             for k, s in flips.items()}

    # ---- the mirrored fold beside oct_mc_update, on the net's own softmax output ----
    probs, _ = eng.forward(x, training=False)
    bufs = eng._mc_buffers(B)
    outs = {k: bufs[k] for k in ("mean_probs", "argmax", "entropy", "mutual_info")}
    eng.mc_update(probs, 0, 3, bufs["ws"])
    npix = B * H * W
    fold = {}
    for name, t, okw, nb in (("middle_sample", 1, {}, npix * (3 * C + 2) * 4),
                             ("last_sample_all_maps", 2, outs, npix * ((2 * C + 1) * 4 + C * 4 + 1 + 8))):
        calls = {"oct_mc_update": lambda: eng.mc_update(probs, t, 3, bufs["ws"], **okw)}
        calls.update({f"oct_tta_update[{n}]": (lambda v=v: eng.tta_update(probs, v, t, 3, bufs["ws"], **okw))
                      for v, n in enumerate(TTA_VIEW_NAMES)})
        st = alternated(calls, a.kernel_reps)
        mc = st["oct_mc_update"]
        fold[name] = {"bytes_moved": int(nb), "ms_per_call": st,
                      "GBps": {k: round(nb / (s["median"] * 1e-3) / 1e9, 1) for k, s in st.items()},
                      "median_over_mc_update": {k: round(s["median"] / mc["median"], 3) for k, s in st.items()},
                      "mc_update_spread": round((mc["max"] - mc["min"]) / mc["median"], 3),
                      "inside_mc_update_spread": {k: bool(mc["min"] <= s["median"] <= mc["max"]) for k, s in st.items()}}
    res["fold"] = fold

    # ---- the replayed graphs ----
    x_fix = x.clone()
    eng_plain.graph_capture(x_fix, want_probs=False, want_argmax=True)
    graphs = {}
    for T in (2, 4):
        eng.graph_capture_tta(x_fix, TTA_VIEW_NAMES[:T])

        def t_plain(T=T):
            for _ in range(T):
                eng_plain.graph_launch()
        st = alternated({"tta_graph": eng.graph_launch, "T_plain_graphs": t_plain}, a.reps)
        graphs[str(T)] = dict(st, tta_over_T_plain=round(st["tta_graph"]["median"] / st["T_plain_graphs"]["median"], 3))
    res["graph_ms"] = graphs

    # ---- the public path, per scan ----
    n = 64
    model = Model(name="unet", config=dict(input_channels=1, num_classes=C, image_height=H, image_width=W, start_neurons=8,
                                           pool_layers=4))
    scans = np.tile(images, (n // 8, 1, 1, 1))
    per_scan = {}
    for name, kw2 in (("plain", {}), ("tta2", dict(tta=TTA_VIEW_NAMES[:2])), ("tta4", dict(tta=TTA_VIEW_NAMES))):
        model.predict_labels(scans, batch_size=B, **kw2)
        t = []
        for _ in range(a.windows):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            model.predict_labels(scans, batch_size=B, **kw2)
            t.append((time.perf_counter() - t0) / n * 1e3)
        per_scan[name] = stats(t)
    res["predict_labels_ms_per_scan"] = per_scan
    print(json.dumps(res))


if __name__ == "__main__":
    main()
