"""What the ignore label and padded training cost at B = 32, 3 classes, fp32, four pool levels:

* ``--leg kernels``: the four head kernels (register pair, and the channel-streaming pair under option "head_wide") at 256x512: per-launch
  time from the engine's per-launch profiler with the mask off and with it on -- labels that carry the 255 frame of a
  250x500 scan padded to 256x512 --, alternated; a window is ``--steps`` training steps;
* ``--leg fit`` (default): ``Model.fit`` scans/s on 250x500 scans with ``pad_mode="edge"`` (padded on the device to 256x512, label frame 255)
  against the same model class on native 256x512 scans, alternated in the same run; a window is one epoch of ``--scans``
  uint8 scans through ``DataGenerator``.

The median of ``--windows`` windows is reported with the spread.  One leg per run; prints one JSON line.
Usage: python tools/bench_masked_fit.py [--leg fit|kernels] [--windows 5] [--steps 10] [--scans 1024] [--first padded|native]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oct_image_segmentation_models_amd import _hip, optimizers  # noqa: E402
from oct_image_segmentation_models_amd.common import custom_losses, custom_metrics  # noqa: E402
from oct_image_segmentation_models_amd.common.data_generator import DataGenerator  # noqa: E402
from oct_image_segmentation_models_amd.common.synthetic import make_scans  # noqa: E402
from oct_image_segmentation_models_amd.common.utils import pad_reference, padded_geometry  # noqa: E402
from oct_image_segmentation_models_amd.engine import UNetEngine  # noqa: E402
from oct_image_segmentation_models_amd.models import get_model_class  # noqa: E402

B, H, W, C, P = 32, 250, 500, 3, 4
HEAD = ("head_fwd_k<", "head_bwd_k<", "head_fwd_wide_k<", "head_bwd_wide_k<")


def stats(v, digits=4):
    v = sorted(v)
    return {"median": round(v[len(v) // 2], digits), "min": round(v[0], digits), "max": round(v[-1], digits)}


def head_kernel_times(a, wide):
    Hp, Wp, top, left = padded_geometry(H, W, P)
    old = _hip.get_option("head_wide")
    try:
        _hip.set_option("head_wide", int(wide))
        eng = UNetEngine(device="cuda:0", input_channels=1, num_classes=C, image_height=Hp, image_width=Wp, max_batch=B,
                         training=True, seed=1000, init_seed=0, pool_layers=P)
    finally:
        _hip.set_option("head_wide", old)
    images, labels = make_scans(8, Hp, Wp, C, seed=1234)
    x = torch.from_numpy(np.tile(images, (B // 8, 1, 1, 1))).to(eng.device)
    plain = np.tile(labels, (B // 8, 1, 1, 1))
    framed = pad_reference(plain[:, top:top + H, left:left + W], Hp, Wp, top, left, "constant", 255)
    lab = {False: torch.from_numpy(plain).to(eng.device), True: torch.from_numpy(framed).to(eng.device)}

    def window(masked):
        eng.set_ignore_label(255 if masked else None)
        eng.profile_begin()
        for _ in range(a.steps):
            eng.forward(x, training=True, labels=lab[masked], want_probs=False)
            eng.loss_dice()
            eng.backward(lab[masked], macro=True, loss_scale=1.0)
        torch.cuda.synchronize()
        return {e["kernel"]: e["total_ms"] / e["launches"] for e in eng.profile_end() if e["kernel"].startswith(HEAD)}

    for masked in (False, True):
        window(masked)
    got = {False: [], True: []}
    for _ in range(a.windows):
        for masked in (False, True):
            got[masked].append(window(masked))
    out = {}
    for k in got[False][0]:
        off, on = stats([w[k] for w in got[False]]), stats([w[k] for w in got[True]])
        out[k] = {"mask_off_ms": off, "mask_on_ms": on, "on_over_off": round(on["median"] / off["median"], 4)}
    return out


def fit_rates(a):
    Hp, Wp, top, left = padded_geometry(H, W, P)
    base_i, base_l = make_scans(64, Hp, Wp, C, seed=77)
    reps = a.scans // 64
    native = (np.tile(base_i, (reps, 1, 1, 1)), np.tile(base_l, (reps, 1, 1, 1)))
    crop = lambda t: np.ascontiguousarray(t[:, top:top + H, left:left + W])     # noqa: E731
    small = (crop(native[0]), crop(native[1]))

    def compiled(h, w, pad_mode):
        mc = get_model_class("unet")(input_channels=1, num_classes=C, image_height=h, image_width=w, pool_layers=P)
        model = mc.build_model()
        model.compile(optimizer=optimizers.Adam(learning_rate=1e-3),
                      loss=custom_losses.custom_loss_objects["dice_loss_macro"]["function"](num_classes=C, is_y_true_sparse=False),
                      metrics=[custom_metrics.training_monitor_metric_objects["dice_coef_macro"](False, C)], pad_mode=pad_mode)
        return model, mc.get_preprocess_input_fn()

    runs = {}
    legs = [("padded_250x500", small, "edge"), ("native_256x512", native, None)]
    for name, (im, lb), pad_mode in (legs[::-1] if a.first == "native" else legs):
        model, pre = compiled(Hp, Wp, pad_mode)
        gen = DataGenerator(im, lb, B, [], "none", (), False, pre, seed=5)
        warm = DataGenerator(im[:4 * B], lb[:4 * B], B, [], "none", (), False, pre, seed=5)
        model.fit(x=warm, epochs=1, verbose=0)
        torch.cuda.synchronize()
        runs[name] = (model, gen, [])
    for _ in range(a.windows):
        for name, (model, gen, rates) in runs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            model.fit(x=gen, epochs=1, verbose=0)
            torch.cuda.synchronize()
            rates.append(len(gen) * B / (time.perf_counter() - t0))
    out = {name: stats(r[2], 1) for name, r in runs.items()}
    out["padded_over_native"] = round(out["padded_250x500"]["median"] / out["native_256x512"]["median"], 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--scans", type=int, default=1024)
    ap.add_argument("--leg", choices=["fit", "kernels"], default="fit",
                    help="one leg per process: with the profiled engines of the kernel leg alive in the same process the "
                         "native fit leg that followed ran at 0.62 of its rate")
    ap.add_argument("--first", choices=["padded", "native"], default="padded",
                    help="which leg's model is built, warmed and timed first in every window")
    a = ap.parse_args()
    Hp, Wp, top, left = padded_geometry(H, W, P)
    res = {"what": f"ignore label and padded training, B={B}, {H}x{W} -> {Hp}x{Wp} at ({top}, {left}), {C} classes, fp32",
           "windows": a.windows, "steps_per_window": a.steps, "scans_per_epoch": a.scans,
           "first": a.first}
    if a.leg == "kernels":
        res["head_kernels_ms_per_launch"] = {**head_kernel_times(a, False), **head_kernel_times(a, True)}
    else:
        res["fit_scans_per_s"] = fit_rates(a)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
