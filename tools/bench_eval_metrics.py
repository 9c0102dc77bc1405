"""Times the metric stage of evaluate_model with ``metrics_device`` off and on, at B = 128, 256x512, 3 classes and at
B = 32, 512x1024, 8 classes, on synthetic class maps (a shifted copy as the prediction, the ground truth's own boundaries
as the delineations).

  host_ms_per_image.off   what the host path spends per image on the steps the switch replaces: _dice_metrics on the arg-max
                          map, labels_from_delineations, _dice_metrics on the graph-search map (a few images, one thread)
  host_ms_per_image.on    what the host spends per image with the switch on: DelineationLabels for the whole batch (upload
                          of delineations and ground truth, both kernels, download of the class maps, the wait) and
                          dice_from_counts twice per image
  kernel_us_per_batch     oct_confusion_counts and oct_area_labels alone, CUDA events around repeated calls; beside them
                          oct_confusion_counts_masked on the same maps with about 10 % of the ground truth set to the ignore
                          label 255 (a column strip and a rectangle per image), and the whole oct_surface_distances /
                          oct_surface_distances_masked calls (three launches and one stream wait each) on the two ground truths

With ``--e2e N`` it also runs evaluate_model itself over N synthetic 256x512 scans (an untrained 3-class net, the three
Dice metrics, graph search on the device with "device" ties, batch 32, result files into a temporary directory) with the
switch off and on, alternating, twice each: ``evaluate_model_s_per_image``, wall seconds per image, files included; and with
all five metrics and ``metrics_device`` on, the fully labelled scans without ``ignore_label`` against the same scans with about
10 % of the labels set to 255 and ``ignore_label=255``: ``evaluate_model_ignore_s_per_image``.

``--kernels-only`` runs nothing but the four metric calls of the first case, ``--reps`` times each, for a kernel trace: the
column pass of the surface distances has no entry point of its own, and its time is read from
``rocprofv3 --kernel-trace --stats -d out -- python tools/bench_eval_metrics.py --kernels-only`` (``surf_col_k<false>`` and
``surf_col_k<true>`` are the unmasked and the masked instantiation).

Prints one JSON line.  Usage: python tools/bench_eval_metrics.py [--reps 20] [--host-images 4] [--e2e N] [--kernels-only]"""
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

from oct_image_segmentation_models_amd.common import utils  # noqa: E402
from oct_image_segmentation_models_amd.evaluation import dice_device as dd  # noqa: E402
from oct_image_segmentation_models_amd.evaluation.surface import SurfaceDistances  # noqa: E402
from oct_image_segmentation_models_amd.evaluation.evaluation import _dice_metrics  # noqa: E402
from oct_image_segmentation_models_amd.min_path_processing.utils import generate_boundary  # noqa: E402
from oracle import unet_numpy as on  # noqa: E402

METRICS = list(dd.DICE_METRICS)
ALL_METRICS = METRICS + ["average_surface_distance", "hausdorff_distance"]
IGNORE = 255


def with_ignored(labels):
    """A copy of (n,H,W[,1]) label maps with about 10 % of every image set to IGNORE: a strip of W/16 columns (an optic-nerve
    head) and a rectangle of H/4 x W/6 whose place depends on the image."""
    out = labels.copy()
    n, H, W = out.shape[:3]
    out[:, :, W // 2:W // 2 + W // 16] = IGNORE
    for i in range(n):
        r, c = (37 * i) % (H - H // 4), (53 * i) % (W - W // 6)
        out[i, r:r + H // 4, c:c + W // 6] = IGNORE
    return out


def metric_calls(B, H, W, C, pred, gt):
    """The metric calls on device maps, unmasked and masked: {name: thunk}."""
    p, g, gi = torch.from_numpy(pred).cuda(), torch.from_numpy(gt).cuda(), torch.from_numpy(with_ignored(gt)).cuda()
    cc, ccm = dd.ConfusionCounts(B, H, W, C, "cuda:0"), dd.ConfusionCounts(B, H, W, C, "cuda:0", ignore_label=IGNORE)
    sd, sdm = SurfaceDistances(B, H, W, C, "cuda:0"), SurfaceDistances(B, H, W, C, "cuda:0", ignore_label=IGNORE)
    return {"confusion_counts": lambda: cc(p, g), "confusion_counts_masked": lambda: ccm(p, gi),
            "surface_distances": lambda: sd(p, g), "surface_distances_masked": lambda: sdm(p, gi),
            "surface_distances_masked_nothing_ignored": lambda: sdm(p, g)}


def _events(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def case(B, H, W, C, reps, host_images):
    _, lab = on.synth_scans(min(B, 16), H, W, C, seed=1)
    gt = np.ascontiguousarray(np.tile(lab[..., 0].astype(np.uint8), ((B + 15) // 16, 1, 1))[:B])
    pred = np.ascontiguousarray(np.roll(gt, 2, axis=1))
    segs = np.ascontiguousarray(np.swapaxes(generate_boundary(gt, axis=1), 0, 1).astype(np.uint16))     # (B, C-1, W)
    assert segs.shape == (B, C - 1, W)
    # switch off: the host steps, per image (the one-hot arrays feed the saved files with the switch on as well: timed apart)
    onehot = off = 0.0
    for i in range(host_images):
        a = time.perf_counter()
        label = utils.to_categorical(gt[i][..., None], C)
        cat = utils.labels_to_categorical(pred[i:i + 1].astype(np.int64), C)
        b = time.perf_counter()
        _dice_metrics(METRICS, C, label, cat)
        gs_label, rec = utils.labels_from_delineations((W, H, 1), segs[i], C)
        _dice_metrics(METRICS, C, label, rec, transposed=True)
        c = time.perf_counter()
        onehot, off = onehot + (b - a), off + (c - b)
    # switch on: the batch stage and the count-to-Dice step
    stage = dd.DelineationLabels(B, H, W, C, "cuda:0")
    stage(segs, gt)
    torch.cuda.synchronize()
    best = None
    for _ in range(5):
        a = time.perf_counter()
        labels, counts = stage(segs, gt)
        b = time.perf_counter()
        best = b - a if best is None else min(best, b - a)
    a = time.perf_counter()
    for i in range(B):
        dice_from = dd.dice_from_counts(counts[i], METRICS)
        dice_from = dd.dice_from_counts(counts[i], METRICS)
    dice_s = (time.perf_counter() - a) / B
    assert np.array_equal(labels[host_images - 1], gs_label.astype(np.uint8)) and dice_from[0].shape == (1, C)
    cc, al = dd.ConfusionCounts(B, H, W, C, "cuda:0"), dd.AreaLabels(B, H, W, C, "cuda:0")
    p, g, s = torch.from_numpy(pred).cuda(), torch.from_numpy(gt).cuda(), torch.from_numpy(segs.view(np.int16)).cuda()
    rnd = torch.randint(0, C, (B, H, W), dtype=torch.uint8, device="cuda")
    calls = metric_calls(B, H, W, C, pred, gt)
    ignored_share = float((with_ignored(gt) == IGNORE).mean())
    windows = {k: [] for k in calls}                       # five windows per call, the calls alternating: [median, min, max]
    for _ in range(5):
        for k, f in calls.items():
            windows[k].append(_events(f, reps))
    spread = {k: [round(float(np.median(v)), 2), round(min(v), 2), round(max(v), 2)] for k, v in windows.items()}
    return {"shape": f"B={B}, {H}x{W}, {C} classes",
            "host_ms_per_image": {"off": round(off / host_images * 1e3, 3),
                                  "on": round((best / B + dice_s) * 1e3, 4),
                                  "on_batch_stage": round(best / B * 1e3, 4), "on_dice_from_counts_x2": round(dice_s * 1e3, 4),
                                  "one_hot_arrays_kept_by_both": round(onehot / host_images * 1e3, 3)},
            "kernel_us_per_batch": {"confusion_counts": round(_events(lambda: cc(p, g), reps), 2),
                                    "confusion_counts_random_maps": round(_events(lambda: cc(rnd, g), reps), 2),
                                    "area_labels": round(_events(lambda: al(s), reps), 2),
                                    "ignored_share_of_the_masked_calls": round(ignored_share, 4),
                                    "median_min_max_of_5_alternated_windows": spread}}


def write_model_and_data(root: Path, n: int, H: int, W: int, C: int):
    """An untrained model saved by ``Model.save`` plus its config, and a test set of ``n`` synthetic scans; beside it the
    same set with about 10 % of the labels ignored (test_ignored.hdf5)."""
    from oct_image_segmentation_models_amd.common import h5io
    from oct_image_segmentation_models_amd.models.engine_model import Model
    config = dict(input_channels=1, num_classes=C, image_height=H, image_width=W, start_neurons=8, pool_layers=4)
    cfg = on.UNetConfig(num_classes=C, start_neurons=8, pool_layers=4)
    params, state = on.init_params(cfg, seed=3, dtype=np.float32, randomize_bn=True)
    m = Model(name="unet", config=config)
    m.set_weights(on.keras_weight_list(params, state))
    (root / "model").mkdir()
    m.save(root / "model" / "model.npz")
    with open(root / "model" / "model_config.json", "w") as fh:
        json.dump(config, fh)
    images, labels = on.synth_scans(n, H, W, C, seed=5)
    h5io.save(root / "test.hdf5", {"test_images": images, "test_labels": labels})
    h5io.save(root / "test_ignored.hdf5", {"test_images": images, "test_labels": with_ignored(labels)})
    return root / "model" / "model.npz", root / "test.hdf5"


def end_to_end(n):
    from oct_image_segmentation_models_amd.evaluation import eval_model
    from oct_image_segmentation_models_amd.evaluation.evaluation_parameters import EvaluationParameters, EvaluationSaveParams
    H, W, C = 256, 512, 3
    out = {"what": f"evaluate_model over {n} scans, {H}x{W}, {C} classes, batch 32, gs_device with device ties, files included",
           "off": [], "on": []}
    with tempfile.TemporaryDirectory() as tmp:
        root = Path(tmp)
        model_path, data = write_model_and_data(root, n, H, W, C)
        for rep in range(3):                                       # (the first pass warms both settings up: not reported)
            for name, switch in (("off", False), ("on", True)):
                ep = EvaluationParameters(model_path=model_path, mlflow_tracking_uri=None, mlflow_run_uuid=None,
                                          test_dataset_path=data, save_foldername=root / f"{name}{rep}",
                                          save_params=EvaluationSaveParams(), graph_search=True, metrics=METRICS,
                                          batch_size=32, gs_device=True, gs_device_ties="device", metrics_device=switch)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                eval_model(ep)
                dt = (time.perf_counter() - t0) / n
                if rep:
                    out[name].append(round(dt, 4))
        # the ignore label: all five metrics on the device, fully labelled scans against partially labelled ones
        ign = {"what": "as above with all five metrics and metrics_device: fully labelled scans without ignore_label / the same "
                       "scans with about 10 % of the labels 255 and ignore_label=255", "labelled": [], "ignore_label": []}
        for rep in range(3):
            for name, file, label in (("labelled", "test.hdf5", None), ("ignore_label", "test_ignored.hdf5", IGNORE)):
                ep = EvaluationParameters(model_path=model_path, mlflow_tracking_uri=None, mlflow_run_uuid=None,
                                          test_dataset_path=root / file, save_foldername=root / f"{name}{rep}",
                                          save_params=EvaluationSaveParams(), graph_search=True, metrics=ALL_METRICS,
                                          batch_size=32, gs_device=True, gs_device_ties="device", metrics_device=True,
                                          ignore_label=label)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                eval_model(ep)
                dt = (time.perf_counter() - t0) / n
                if rep:
                    ign[name].append(round(dt, 4))
    return out, ign


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-images", type=int, default=4)
    ap.add_argument("--e2e", type=int, default=0, help="also time evaluate_model over this many scans, switch off / on")
    ap.add_argument("--kernels-only", action="store_true", help="only the metric calls of the first case (for a kernel trace)")
    a = ap.parse_args()
    if a.kernels_only:
        B, H, W, C = 128, 256, 512, 3
        _, lab = on.synth_scans(16, H, W, C, seed=1)
        gt = np.ascontiguousarray(np.tile(lab[..., 0].astype(np.uint8), (B // 16, 1, 1)))
        for name, f in metric_calls(B, H, W, C, np.ascontiguousarray(np.roll(gt, 2, axis=1)), gt).items():
            if name.endswith("nothing_ignored"):          # (would mix into the masked instantiation's figures)
                continue
            for _ in range(a.reps):
                f()
        torch.cuda.synchronize()
        return
    res = {"what": "metric stage of evaluate_model, metrics_device off / on (tools/bench_eval_metrics.py)",
           "cases": [case(128, 256, 512, 3, a.reps, a.host_images), case(32, 512, 1024, 8, a.reps, a.host_images)]}
    if a.e2e:
        res["evaluate_model_s_per_image"], res["evaluate_model_ignore_s_per_image"] = end_to_end(a.e2e)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
