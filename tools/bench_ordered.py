"""Times the ordered layer decode, fp32, in ONE run with alternating windows:

* ``oct_ordered_decode`` at B = 32, 256x512 with 3 and 9 classes beside a device-to-device copy of the same probabilities,
  with the achieved bytes/s against the bytes the call must move (probabilities in; decision words out and in; labels, rows
  and score out) and the ratio to the copy.  Up to 8 classes the four-column form (option "ordered_float4": float4 loads) runs
  on the same data.  At 3 classes two more forms place the time: the score alone (no decision words, no back-trace) and an input whose columns are already
  ordered (nothing for the back-trace to step through but the C-1 boundaries);
* larger shapes at 3 classes: B = 32 at 512x1024 (twice the columns, twice the rows), and many short columns (B = 128 at
  64x2048, B = 256 at 32x4096), where even a quarter of the threads fills the device;
* the replayed inference pipeline (``BatchedPredictor``: upload, graph, boundary maps, download) per scan, switch off and on;
* ``evaluate_model`` end to end over ``--eval-scans`` scans, switch off and on.

Every form is warmed up before it is timed; a timed window is ``--kernel-reps`` repetitions between two device events, the
windows of the forms of one shape alternate (copy, decode, ..., copy, decode, ...), and the median of ``--windows`` windows is
reported with the spread.  Prints one JSON line.
Usage: python tools/bench_ordered.py [--windows 5] [--kernel-reps 30] [--eval-scans 32]"""
import argparse
import json
import os
import sys
import tempfile
import time
from pathlib import Path

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oct_image_segmentation_models_amd import _hip  # noqa: E402
from oct_image_segmentation_models_amd.common import h5io  # noqa: E402
from oct_image_segmentation_models_amd.common.synthetic import make_scans  # noqa: E402
from oct_image_segmentation_models_amd.engine import UNetEngine  # noqa: E402
from oct_image_segmentation_models_amd.evaluation.ordered import OrderedDecode  # noqa: E402
from oct_image_segmentation_models_amd.evaluation.pipeline import BatchedPredictor  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--kernel-reps", type=int, default=30)
    ap.add_argument("--eval-scans", type=int, default=32)
    a = ap.parse_args()
    B, H, W = 32, 256, 512
    eng = UNetEngine(device="cuda:0", input_channels=1, num_classes=3, image_height=H, image_width=W, max_batch=B,
                     training=False, seed=1000, init_seed=0)
    dev = eng.device
    lib = _hip.lib()

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

    def alternating(forms):
        """forms: name -> (call, bytes moved).  Windows alternate between the forms."""
        for call, _ in forms.values():
            for _ in range(3):
                call()
        torch.cuda.synchronize()
        ts = {k: [] for k in forms}
        for _ in range(a.windows):
            for k, (call, _) in forms.items():
                ts[k].append(window(call, a.kernel_reps))
        out = {}
        for k, (_, nbytes) in forms.items():
            ms = stats(ts[k])
            out[k] = {"ms_per_call": ms, "bytes_moved": int(nbytes), "GBps": round(nbytes / (ms["median"] * 1e-3) / 1e9, 1),
                      "over_copy": round(ms["median"] / stats(ts["copy"])["median"], 3)}
        return out

    def raw(p, shape, ws, labels, rows, score):
        ptr = lambda t: None if t is None else t.data_ptr()      # noqa: E731
        _hip.call("oct_ordered_decode", dev, p.data_ptr(), *shape, ws.data_ptr(), ws.numel(), ptr(labels), ptr(rows), ptr(score),
                  _hip.stream_ptr(dev))

    def kernel_forms(shape, extra: bool):
        Bs, Hs, Ws, C = shape
        npix = Bs * Hs * Ws
        g = torch.Generator(device=dev).manual_seed(C)
        probs = torch.softmax(torch.randn(shape, generator=g, device=dev) * 2.0, dim=-1).contiguous()
        out = torch.empty_like(probs)
        ws = torch.empty(int(lib.oct_ordered_workspace_bytes(*shape)), dtype=torch.uint8, device=dev)
        labels, rows, score = eng.ordered_decode(probs, ws=ws)
        n_in, n_out = npix * C * 4, npix + Bs * (C - 1) * Ws * 2 + Bs * Ws * 4
        full = n_in + 2 * ws.numel() + n_out
        forms = {"copy": (lambda: out.copy_(probs), 2 * n_in),
                 "oct_ordered_decode": (lambda: raw(probs, shape, ws, labels, rows, score), full)}
        res = alternating(forms)
        if C <= 8:                                                # the four-column form on the same data
            _hip.set_option("ordered_float4", 1)
            try:
                res["float4_form"] = alternating({"copy": forms["copy"], "float4_form": forms["oct_ordered_decode"]})["float4_form"]
            finally:
                _hip.set_option("ordered_float4", 0)
        if extra:
            ordered = torch.empty_like(probs)
            cuts = torch.sort(torch.randint(1, Hs, (Bs, 1, Ws, C - 1), generator=g, device=dev), dim=-1).values
            lab = (torch.arange(Hs, device=dev).view(1, Hs, 1, 1) >= cuts).sum(dim=-1)
            ordered.copy_(torch.nn.functional.one_hot(lab, C).float() * 0.9 + 0.1 / C)
            more = {"copy": forms["copy"],
                    "score_only": (lambda: raw(probs, shape, ws, None, None, score), n_in + Bs * Ws * 4),
                    "ordered_input": (lambda: raw(ordered, shape, ws, labels, rows, score), full)}
            res.update({k: v for k, v in alternating(more).items() if k != "copy"})
        return res

    res = {"what": "ordered decode, fp32", "windows": a.windows, "kernel_reps": a.kernel_reps,
           "kernels": {"B32_256x512_C3": kernel_forms((B, H, W, 3), True), "B32_256x512_C9": kernel_forms((B, H, W, 9), False),
                       "B32_512x1024_C3": kernel_forms((B, 512, 1024, 3), False),
                       # many short columns: where the four-column form has enough threads of its own
                       "B128_64x2048_C3": kernel_forms((128, 64, 2048, 3), False),
                       "B256_32x4096_C3": kernel_forms((256, 32, 4096, 3), False)}}

    # ---- the replayed pipeline, per scan ----
    images, labels = make_scans(8, H, W, 3, seed=1234)
    n_batches = 6
    imgs = np.tile(images, (B * n_batches // 8, 1, 1, 1))
    ts = {"off": [], "on": []}
    for _ in range(a.windows):
        for name in ("off", "on"):
            # (a predictor captures the engine's graph when it is built: each window builds its own, untimed, and warms it up)
            pred = BatchedPredictor(eng, B, want_maps=True, ordered=OrderedDecode(B, H, W, 3, dev) if name == "on" else None)
            for _ in pred.run(imgs[:2 * B]):
                pass
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in pred.run(imgs):
                pass
            ts[name].append((time.perf_counter() - t0) / imgs.shape[0] * 1e3)
    res["pipeline_ms_per_scan"] = {k: stats(v) for k, v in ts.items()}

    # ---- evaluate_model end to end ----
    from oct_image_segmentation_models_amd.evaluation import eval_model
    from oct_image_segmentation_models_amd.evaluation.evaluation_parameters import EvaluationParameters, EvaluationSaveParams
    from oct_image_segmentation_models_amd.models import get_model_class
    model = get_model_class("unet")(input_channels=1, num_classes=3, image_height=H, image_width=W).build_model()
    n = a.eval_scans
    x, y = np.tile(images, (n // 8 + 1, 1, 1, 1))[:n], np.tile(labels, (n // 8 + 1, 1, 1, 1))[:n]
    with tempfile.TemporaryDirectory() as tmp:
        tmp = Path(tmp)
        model.save(tmp / "model" / "model.npz")
        with open(tmp / "model" / "model_config.json", "w") as fh:
            json.dump(model.config, fh)
        h5io.save(tmp / "data.hdf5", {"test_images": x, "test_labels": y})
        ev = {}
        for rep in range(2):                                             # the first round warms both up
            for name, on in (("off", False), ("on", True)):
                ep = EvaluationParameters(model_path=tmp / "model" / "model.npz", mlflow_tracking_uri=None, mlflow_run_uuid=None,
                                          test_dataset_path=tmp / "data.hdf5", save_foldername=tmp / f"{name}{rep}",
                                          save_params=EvaluationSaveParams(), graph_search=False,
                                          metrics=["dice_coef_classes", "dice_coef_macro", "dice_coef_micro"], batch_size=B,
                                          ordered_decode=on)
                t0 = time.perf_counter()
                eval_model(ep)
                ev[name] = round((time.perf_counter() - t0) / n * 1e3, 3)
        res["evaluate_model_ms_per_scan"] = dict(ev, scans=n)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
