"""Times the min-path boundary search on the device (oct_minpath_device via min_path_processing/device_search.py) at
B = 128, 256x512, 3 classes, on the two inputs evaluation/pipeline.py::bench_fields uses: the boundary maps of the
synthetic ground-truth class maps (what a trained model emits) and the untrained net's own maps (noise).  Reports the
kernel's ms per batch (CUDA events around repeated calls), the share of tied maps, and end-to-end ms per scan through
``BatchedPredictor`` -- upload, hipGraph forward, boundary maps, search, download, merge -- with the device search in both
tie modes and, in the same process, with the pooled host search (what ``inference_e2e_ms_per_scan`` of bench.py measures).
Prints one JSON line.  Usage: python tools/bench_minpath.py [--batches 6] [--reps 3] [--kernel-reps 20]"""
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
from oct_image_segmentation_models_amd.evaluation.pipeline import BatchedPredictor  # noqa: E402
from oct_image_segmentation_models_amd.min_path_processing.device_search import DeviceMinPath, merge_ties_async  # noqa: E402
from oct_image_segmentation_models_amd.min_path_processing.pool import SegmentPool, default_workers  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=6)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--kernel-reps", type=int, default=20)
    a = ap.parse_args()
    B, H, W, C = 128, 256, 512, 3
    workers = default_workers()
    with SegmentPool((H, W), gsgrad=1, workers=workers) as pool:
        eng = UNetEngine(device="cuda:0", input_channels=1, num_classes=C, image_height=H, image_width=W, max_batch=B,
                         training=False, seed=1000, init_seed=0)
        images, labels = make_scans(8, H, W, C, seed=1234)
        imgs = np.tile(images, (B * a.batches // 8 + 1, 1, 1, 1))[:B * a.batches]
        lab = np.ascontiguousarray(np.tile(labels[..., 0], (B // 8 + 1, 1, 1))[:B].astype(np.uint8))
        clean_dev = eng.boundary_maps(torch.from_numpy(lab).to(eng.device))
        mp = DeviceMinPath(B, C - 1, H, W, 1, eng.device)
        pred = BatchedPredictor(eng, B, want_maps=True, minpath=mp)
        noise = next(iter(pred.run(imgs[:B]))).maps                 # warm-up: graph, pinned buffers, the kernel's LDS limit
        noise_dev = torch.from_numpy(noise).to(eng.device)
        pool.segment(noise[:min(B, 2 * workers)])                   # worker start-up
        res = {"what": f"oct_minpath_device, B={B}, {H}x{W}, {C} classes ({C - 1} maps per scan), max_grad 1",
               "pool_workers": workers, "scans_per_run": int(imgs.shape[0]), "reps": a.reps,
               "workspace_bytes": int(mp.workspace.numel())}

        real_maps = eng.boundary_maps

        def clean_maps(am, **kw):            # the real kernel still runs; the search sees the clean maps instead
            real_maps(am, **kw)
            return clean_dev

        def e2e_device(ties):
            pred.minpath = mp
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            jobs = [merge_ties_async(b.maps, b.minpath[0], b.minpath[2], None, pool.segment_async, ties)
                    for b in pred.run(imgs)]
            for j in jobs:
                j.get()
            return (time.perf_counter() - t0) / imgs.shape[0] * 1e3

        def e2e_host():
            pred.minpath = None
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            jobs = [pool.segment_async(b.maps) for b in pred.run(imgs)]
            for j in jobs:
                j.get()
            return (time.perf_counter() - t0) / imgs.shape[0] * 1e3

        def gpu_only():
            pred.minpath = mp
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in pred.run(imgs):
                pass
            return (time.perf_counter() - t0) / imgs.shape[0] * 1e3

        def stats(f):
            v = sorted(f() for _ in range(a.reps))
            return {"median": round(v[len(v) // 2], 4), "min": round(v[0], 4), "max": round(v[-1], 4)}

        for kind, maps_dev in (("clean_maps", clean_dev), ("untrained_maps", noise_dev)):
            for _ in range(3):
                _, _, tied = mp(maps_dev)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.kernel_reps):
                mp(maps_dev)
            e1.record()
            torch.cuda.synchronize()
            eng.boundary_maps = clean_maps if kind == "clean_maps" else real_maps
            try:
                res[kind] = {"kernel_ms_per_batch": round(e0.elapsed_time(e1) / a.kernel_reps, 4),
                             "tied_share": round(float(tied.float().mean().item()), 4),
                             "e2e_ms_per_scan_device_ties_host": stats(lambda: e2e_device("host")),
                             "e2e_ms_per_scan_device_ties_device": stats(lambda: e2e_device("device")),
                             "e2e_ms_per_scan_host_pool": stats(e2e_host),
                             "gpu_pipeline_with_search_ms_per_scan": stats(gpu_only)}
            finally:
                eng.boundary_maps = real_maps
    print(json.dumps(res))


if __name__ == "__main__":
    main()
