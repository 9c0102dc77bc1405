"""Times the metric stage of evaluate_model with ``metrics_device`` off and on, at B = 128, 256x512, 3 classes and at
B = 32, 512x1024, 8 classes, on synthetic class maps (a shifted copy as the prediction, the ground truth's own boundaries
as the delineations).

  host_ms_per_image.off   what the host path spends per image on the steps the switch replaces: _dice_metrics on the arg-max
                          map, labels_from_delineations, _dice_metrics on the graph-search map (a few images, one thread)
  host_ms_per_image.on    what the host spends per image with the switch on: DelineationLabels for the whole batch (upload
                          of delineations and ground truth, both kernels, download of the class maps, the wait) and
                          dice_from_counts twice per image
  kernel_us_per_batch     oct_confusion_counts and oct_area_labels alone, CUDA events around repeated calls

With ``--e2e N`` it also runs evaluate_model itself over N synthetic 256x512 scans (an untrained 3-class net, the three
Dice metrics, graph search on the device with "device" ties, batch 32, result files into a temporary directory) with the
switch off and on, alternating, twice each: ``evaluate_model_s_per_image``, wall seconds per image, files included.

Prints one JSON line.  Usage: python tools/bench_eval_metrics.py [--reps 20] [--host-images 4] [--e2e N]"""
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
from oct_image_segmentation_models_amd.evaluation.evaluation import _dice_metrics  # noqa: E402
from oct_image_segmentation_models_amd.min_path_processing.utils import generate_boundary  # noqa: E402
from oracle import unet_numpy as on  # noqa: E402

METRICS = list(dd.DICE_METRICS)


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
    return {"shape": f"B={B}, {H}x{W}, {C} classes",
            "host_ms_per_image": {"off": round(off / host_images * 1e3, 3),
                                  "on": round((best / B + dice_s) * 1e3, 4),
                                  "on_batch_stage": round(best / B * 1e3, 4), "on_dice_from_counts_x2": round(dice_s * 1e3, 4),
                                  "one_hot_arrays_kept_by_both": round(onehot / host_images * 1e3, 3)},
            "kernel_us_per_batch": {"confusion_counts": round(_events(lambda: cc(p, g), reps), 2),
                                    "confusion_counts_random_maps": round(_events(lambda: cc(rnd, g), reps), 2),
                                    "area_labels": round(_events(lambda: al(s), reps), 2)}}


def write_model_and_data(root: Path, n: int, H: int, W: int, C: int):
    """An untrained model saved by ``Model.save`` plus its config, and a test set of ``n`` synthetic scans."""
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
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-images", type=int, default=4)
    ap.add_argument("--e2e", type=int, default=0, help="also time evaluate_model over this many scans, switch off / on")
    a = ap.parse_args()
    res = {"what": "metric stage of evaluate_model, metrics_device off / on (tools/bench_eval_metrics.py)",
           "cases": [case(128, 256, 512, 3, a.reps, a.host_images), case(32, 512, 1024, 8, a.reps, a.host_images)]}
    if a.e2e:
        res["evaluate_model_s_per_image"] = end_to_end(a.e2e)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
