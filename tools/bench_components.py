"""Times the connected components in ONE run with alternating windows:

* ``oct_components`` (roots, sizes, statistics) and ``oct_component_filter`` (min_pixels and keep_largest together, column fill)
  at B = 32, 256x512 with 3 and 9 classes on three inputs -- a clean layered map, the layered map with 0.5 % of the pixels
  replaced by random classes, uniformly random labels -- each beside a device copy of the bytes the call must move: 1 B read
  and 8 B (roots and sizes) or 1 B (the cleaned map; it also reads 8 B) written per pixel;
* ``scipy.ndimage.label`` per class and image over the same batch on the host (where scipy is installed);
* the replayed inference pipeline (``BatchedPredictor``: upload, graph, boundary maps, download) per scan, stage off and on;
* ``evaluate_model`` end to end over ``--eval-scans`` scans, stage off and on.

Every form is warmed up before it is timed; a timed window is ``--kernel-reps`` repetitions between two device events, the
windows of the forms of one input alternate, and the median of ``--windows`` windows is reported with the spread.  Prints one
JSON line.
Usage: python tools/bench_components.py [--windows 5] [--kernel-reps 30] [--eval-scans 32]"""
import argparse
import ctypes
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
from oct_image_segmentation_models_amd.evaluation.components import ComponentRule, Components  # noqa: E402
from oct_image_segmentation_models_amd.evaluation.pipeline import BatchedPredictor  # noqa: E402


def layered(B, H, W, C, noise, seed):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    out = np.empty((B, H, W), np.uint8)
    for b in range(B):
        cuts = [H * (k + 1) / C + 0.04 * H * np.sin((x[0] + 11 * b) / (7.0 + 3 * k)) for k in range(C - 1)]
        out[b] = sum((y >= c[None, :]).astype(np.uint8) for c in cuts)
        hit = rng.random((H, W)) < noise
        out[b][hit] = rng.integers(0, C, size=int(hit.sum()), dtype=np.uint8)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--kernel-reps", type=int, default=30)
    ap.add_argument("--eval-scans", type=int, default=32)
    a = ap.parse_args()
    B, H, W = 32, 256, 512
    dev = torch.device("cuda:0")
    lib = _hip.lib()
    npx = B * H * W

    def window(call, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            call()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps * 1e3                      # microseconds

    def stats(v, digits=2):
        v = sorted(v)
        return {"median": round(v[len(v) // 2], digits), "min": round(v[0], digits), "max": round(v[-1], digits)}

    def alternating(forms):
        for call in forms.values():
            for _ in range(3):
                call()
        torch.cuda.synchronize()
        ts = {k: [] for k in forms}
        for _ in range(a.windows):
            for k, call in forms.items():
                ts[k].append(window(call, a.kernel_reps))
        return {k: stats(v) for k, v in ts.items()}

    ws = torch.empty(int(lib.oct_components_workspace_bytes(B, H, W)), dtype=torch.uint8, device=dev)
    root = torch.empty((B, H, W), dtype=torch.int32, device=dev)
    size = torch.empty_like(root)
    clean = torch.empty((B, H, W), dtype=torch.uint8, device=dev)
    src9, dst9 = (torch.empty(npx * 9 // 2, dtype=torch.uint8, device=dev) for _ in range(2))      # a copy that moves 9 B/px
    src10, dst10 = (torch.empty(npx * 5, dtype=torch.uint8, device=dev) for _ in range(2))         # ... 10 B/px
    st = _hip.stream_ptr(dev)

    def kernel_forms(C, labels_np):
        labels = torch.from_numpy(labels_np).to(dev)
        stat = torch.empty((B, C, 2), dtype=torch.int32, device=dev)
        removed = torch.empty((B, C), dtype=torch.int32, device=dev)
        rule = ComponentRule(connectivity=8, min_pixels=16, keep_largest="all", fill="column").pack(C)

        def label():
            _hip.call("oct_components", dev, labels.data_ptr(), B, H, W, C, 8, ws.data_ptr(), ws.numel(), root.data_ptr(),
                      size.data_ptr(), stat.data_ptr(), st)

        def filt():
            _hip.call("oct_component_filter", dev, labels.data_ptr(), root.data_ptr(), size.data_ptr(), B, H, W, C,
                      ctypes.byref(rule), ws.data_ptr(), ws.numel(), clean.data_ptr(), removed.data_ptr(), st)
        label()
        t = alternating({"copy_9B": lambda: dst9.copy_(src9), "oct_components": label,
                         "copy_10B": lambda: dst10.copy_(src10), "oct_component_filter": filt})
        t["components_over_copy"] = round(t["oct_components"]["median"] / t["copy_9B"]["median"], 2)
        t["filter_over_copy"] = round(t["oct_component_filter"]["median"] / t["copy_10B"]["median"], 2)
        t["components"] = int(stat.cpu().numpy().view(np.uint32)[..., 0].sum())
        t["removed_pixels"] = int(removed.cpu().numpy().view(np.uint32).sum())
        try:
            from scipy import ndimage
            t0 = time.perf_counter()
            for b in range(B):
                for c in range(C):
                    ndimage.label(labels_np[b] == c, structure=np.ones((3, 3), int))
            t["scipy_label_ms_per_batch"] = round((time.perf_counter() - t0) * 1e3, 1)
        except ImportError:
            t["scipy_label_ms_per_batch"] = None
        return t

    res = {"what": "connected components, us per call at B=32, 256x512", "windows": a.windows, "kernel_reps": a.kernel_reps,
           "kernels": {}}
    for C in (3, 9):
        inputs = {"layered": layered(B, H, W, C, 0.0, C), "layered_noise": layered(B, H, W, C, 0.005, C),
                  "random": np.random.default_rng(C).integers(0, C, size=(B, H, W), dtype=np.uint8)}
        for name, lab in inputs.items():
            res["kernels"][f"C{C}_{name}"] = kernel_forms(C, lab)

    # ---- the replayed pipeline, per scan ----
    eng = UNetEngine(device="cuda:0", input_channels=1, num_classes=3, image_height=H, image_width=W, max_batch=B,
                     training=False, seed=1000, init_seed=0)
    images, labels = make_scans(8, H, W, 3, seed=1234)
    n_batches = 6
    imgs = np.tile(images, (B * n_batches // 8, 1, 1, 1))
    rule = ComponentRule(connectivity=8, min_pixels=16, keep_largest="all", fill="column")
    ts = {"off": [], "on": []}
    for _ in range(a.windows):
        for name in ("off", "on"):
            # (a predictor captures the engine's graph when it is built: each window builds its own, untimed, and warms it up)
            more = {"components": Components(B, H, W, 3, rule, dev)} if name == "on" else {}
            pred = BatchedPredictor(eng, B, want_maps=True, **more)
            for _ in pred.run(imgs[:2 * B]):
                pass
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in pred.run(imgs):
                pass
            ts[name].append((time.perf_counter() - t0) / imgs.shape[0] * 1e3)
    res["pipeline_ms_per_scan"] = {k: stats(v, 4) for k, v in ts.items()}

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
            for name, on in (("off", None), ("on", rule)):
                ep = EvaluationParameters(model_path=tmp / "model" / "model.npz", mlflow_tracking_uri=None, mlflow_run_uuid=None,
                                          test_dataset_path=tmp / "data.hdf5", save_foldername=tmp / f"{name}{rep}",
                                          save_params=EvaluationSaveParams(), graph_search=False,
                                          metrics=["dice_coef_classes", "dice_coef_macro", "dice_coef_micro"], batch_size=B,
                                          components=on)
                t0 = time.perf_counter()
                eval_model(ep)
                ev[name] = round((time.perf_counter() - t0) / n * 1e3, 3)
        res["evaluate_model_ms_per_scan"] = dict(ev, scans=n)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
