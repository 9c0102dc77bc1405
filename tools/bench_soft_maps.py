"""Times the soft boundary maps (oct_boundary_maps_soft, ``soft_maps`` / ``binarize=False``) at B = 128, 256x512, 3 classes:

* the kernel's ms per batch and its achieved bytes/s against the bytes it must move (one read of the probability channels
  the maps use + C-1 bytes per pixel written), with ``boundary_maps_k`` on the arg-max of the same batch beside it;
* the pipeline's GPU-side ms per B-scan through ``BatchedPredictor`` (upload, hipGraph forward, maps, download) with
  ``soft_maps`` off and on, alternated in one process;
* on the two inputs tools/bench_minpath.py uses -- the untrained net's own output, and the synthetic ground truth
  (softened into probabilities by a sigmoid ramp across each boundary for the soft maps) -- the share of maps whose
  minimum-cost path is tied, binary against soft, and the end-to-end ms per B-scan of the device search with host ties.

Prints one JSON line.  Usage: python tools/bench_soft_maps.py [--batches 4] [--reps 3] [--kernel-reps 20]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oct_image_segmentation_models_amd import _hip  # noqa: E402
from oct_image_segmentation_models_amd.common.synthetic import make_scans  # noqa: E402
from oct_image_segmentation_models_amd.engine import UNetEngine  # noqa: E402
from oct_image_segmentation_models_amd.evaluation.pipeline import BatchedPredictor  # noqa: E402
from oct_image_segmentation_models_amd.min_path_processing.device_search import DeviceMinPath, merge_ties_async  # noqa: E402
from oct_image_segmentation_models_amd.min_path_processing.pool import SegmentPool, default_workers  # noqa: E402


def ramp_probs(lab: np.ndarray, C: int, width: float = 1.5) -> np.ndarray:
    """(n,H,W) layered class maps -> (n,H,W,C) float32 probabilities with a sigmoid ramp of ``width`` rows across each
    boundary (boundary k of a column = its number of pixels with a class below k)."""
    n, H, W = lab.shape
    r = np.arange(H, dtype=np.float64)[None, :, None]
    below = [np.ones((n, H, W))]
    for k in range(1, C):
        bnd = (lab < k).sum(axis=1, dtype=np.float64)[:, None, :]
        below.append(1.0 / (1.0 + np.exp(-(r - bnd + 0.5) / width)))
    below.append(np.zeros((n, H, W)))
    return np.ascontiguousarray(np.stack([below[k] - below[k + 1] for k in range(C)], axis=-1).astype(np.float32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=4)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--kernel-reps", type=int, default=20)
    a = ap.parse_args()
    B, H, W, C = 128, 256, 512, 3
    workers = default_workers()
    lib = _hip.lib()

    def stats(f, reps=a.reps, digits=4):
        v = sorted(f() for _ in range(reps))
        return {"median": round(v[len(v) // 2], digits), "min": round(v[0], digits), "max": round(v[-1], digits)}

    with SegmentPool((H, W), gsgrad=1, workers=workers) as pool:
        eng = UNetEngine(device="cuda:0", input_channels=1, num_classes=C, image_height=H, image_width=W, max_batch=B,
                         training=False, seed=1000, init_seed=0)
        images, labels = make_scans(8, H, W, C, seed=1234)
        imgs = np.tile(images, (B * a.batches // 8 + 1, 1, 1, 1))[:B * a.batches]
        lab = np.ascontiguousarray(np.tile(labels[..., 0], (B // 8 + 1, 1, 1))[:B].astype(np.uint8))
        stream = torch.cuda.current_stream(eng.device).cuda_stream
        res = {"what": f"oct_boundary_maps_soft, B={B}, {H}x{W}, {C} classes", "pool_workers": workers,
               "scans_per_run": int(imgs.shape[0]), "reps": a.reps, "kernel_reps": a.kernel_reps}

        # ---- the kernels, on the untrained net's forward of one batch ----
        probs, am = eng.forward(torch.from_numpy(imgs[:B]).to(eng.device), training=False, want_probs=True, want_argmax=True)
        out = torch.empty((B, C - 1, H, W), dtype=torch.uint8, device=eng.device)

        def soft_call():
            _hip.check(lib.oct_boundary_maps_soft(probs.data_ptr(), B, H, W, C, 1, 0, out.data_ptr(), stream))

        def binary_call():
            _hip.check(lib.oct_boundary_maps(am.data_ptr(), B, H, W, C, 1, 0, out.data_ptr(), stream))

        def kernel_ms(call):
            def once():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.kernel_reps):
                    call()
                e1.record()
                torch.cuda.synchronize()
                return e0.elapsed_time(e1) / a.kernel_reps
            for _ in range(5):
                call()
            torch.cuda.synchronize()
            return stats(once, reps=max(a.reps, 5))

        npix = B * H * W
        channels = len({(m - 1 if m == 1 else m) for m in range(1, C)})          # bg_ilm: map 1 reads class 0
        must = npix * (4 * channels + (C - 1))
        soft_ms, bin_ms = kernel_ms(soft_call), kernel_ms(binary_call)
        res["kernel"] = {"soft_maps_k_ms_per_batch": soft_ms, "boundary_maps_k_ms_per_batch": bin_ms,
                         "soft_must_move_bytes": int(must), "soft_probs_bytes": int(npix * 4 * C),
                         "soft_GBps_of_must_move": round(must / (soft_ms["median"] * 1e-3) / 1e9, 1),
                         "binary_GBps": round(npix * C / (bin_ms["median"] * 1e-3) / 1e9, 1)}

        # ---- the pipeline's GPU side, soft_maps off and on, alternated ----
        # (one engine holds one captured graph: each predictor is rebuilt, and warmed up, before its turn)

        def gpu_side(soft):
            pred = BatchedPredictor(eng, B, want_maps=True, soft_maps=soft)
            next(iter(pred.run(imgs[:B])))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in pred.run(imgs):
                pass
            return (time.perf_counter() - t0) / imgs.shape[0] * 1e3

        off, on = [], []
        for _ in range(max(a.reps, 3)):
            off.append(gpu_side(False))
            on.append(gpu_side(True))
        res["gpu_pipeline_ms_per_scan"] = {k: {"median": round(sorted(v)[len(v) // 2], 4), "min": round(min(v), 4),
                                               "max": round(max(v), 4)} for k, v in (("soft_maps_off", off), ("soft_maps_on", on))}

        # ---- ties and end-to-end with the device search, host ties ----
        mp = DeviceMinPath(B, C - 1, H, W, 1, eng.device)
        clean_binary = eng.boundary_maps(torch.from_numpy(lab).to(eng.device))
        clean_soft = eng.boundary_maps_soft(torch.from_numpy(ramp_probs(lab, C)).to(eng.device))
        real_binary, real_soft = eng.boundary_maps, eng.boundary_maps_soft

        def replaced(real, maps):            # the real kernel still runs; the search sees the clean maps instead
            def f(x, **kw):
                real(x, **kw)
                return maps
            return f

        pool.segment(clean_binary.cpu().numpy()[:min(B, 2 * workers)])           # worker start-up
        for kind in ("clean", "untrained"):
            for soft in (False, True):
                if kind == "clean":
                    eng.boundary_maps, eng.boundary_maps_soft = replaced(real_binary, clean_binary), replaced(real_soft, clean_soft)
                try:
                    pred = BatchedPredictor(eng, B, want_maps=True, minpath=mp, soft_maps=soft)
                    first = next(iter(pred.run(imgs[:B])))

                    def e2e():
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        jobs = [merge_ties_async(b.maps, b.minpath[0], b.minpath[2], None, pool.segment_async, "host")
                                for b in pred.run(imgs)]
                        for j in jobs:
                            j.get()
                        return (time.perf_counter() - t0) / imgs.shape[0] * 1e3

                    res[f"{kind}_{'soft' if soft else 'binary'}"] = {
                        "tied_share": round(float(first.minpath[2].mean()), 4),
                        "distinct_map_values": int(len(np.unique(first.maps))),
                        "e2e_ms_per_scan_device_ties_host": stats(e2e)}
                finally:
                    eng.boundary_maps, eng.boundary_maps_soft = real_binary, real_soft
    print(json.dumps(res))


if __name__ == "__main__":
    main()
