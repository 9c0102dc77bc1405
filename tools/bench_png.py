"""Times the PNG pictures (``png_plots``) at 256x512:

* ``oct_render_rgba`` per chunk of 128 images -- the chunk a ``PngRenderer`` takes at this size -- with the base layer
  alone, with 2 lines (3 classes) and with 14 lines (8 classes: 7 solid truths + 7 dotted predictions), by device events,
  and the bytes each call moves (base + line rows read, picture written);
* the PNG stage per image: render and download (``PngRenderer.render`` of an overlay over 128 scans), encode
  (``common.png.encode_rgba``) for every filter type the writer emits at zlib levels 1, 3, 6 and 9, with the file size, on
  an overlay and on a class map, and the write of the encoded bytes;
* with ``--e2e N``: ``evaluate_model`` over N synthetic scans (untrained 3-class net, ``gs_device`` with device ties,
  ``metrics_device``, files included) with ``png_plots`` off and on, alternated, wall seconds per image.

Prints one JSON line.  Usage: python tools/bench_png.py [--reps 5] [--kernel-reps 20] [--e2e 64]"""
import argparse
import ctypes as C
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
from oct_image_segmentation_models_amd.common import plotting, png  # noqa: E402
from oct_image_segmentation_models_amd.common.synthetic import make_scans  # noqa: E402
from oct_image_segmentation_models_amd.evaluation.render import PngRenderer  # noqa: E402
from oct_image_segmentation_models_amd.min_path_processing import utils as mp_utils  # noqa: E402
from oracle import unet_numpy as on  # noqa: E402

B, H, W = 128, 256, 512
METRICS = ["dice_coef_classes", "dice_coef_macro", "dice_coef_micro"]


def stats(values, digits=4):
    v = sorted(values)
    return {"median": round(v[len(v) // 2], digits), "min": round(v[0], digits), "max": round(v[-1], digits)}


def scans_and_truths(Cc):
    images, labels = make_scans(8, H, W, Cc, seed=1234)
    lab = labels[..., 0]
    truths = np.swapaxes(mp_utils.generate_boundary(lab, axis=1), 0, 1).astype(np.uint16)      # (8, Cc-1, W)
    reps = B // 8
    return (np.ascontiguousarray(np.tile(images, (reps, 1, 1, 1))), np.ascontiguousarray(np.tile(lab, (reps, 1, 1)).astype(np.uint8)),
            np.ascontiguousarray(np.tile(truths, (reps, 1, 1))))


def kernel_case(renderer, name, base, lines, colours, styles, palette, reps, kernel_reps):
    """ms per call of ``oct_render_rgba`` alone, over inputs already on the device."""
    dev = renderer.device
    base_dev = torch.from_numpy(base).to(dev)
    rows_dev = None if lines is None else torch.from_numpy(lines.view(np.int16)).to(dev)
    K = 0 if lines is None else lines.shape[1]
    st = _hip.RenderStyle()
    st.n_cls, st.n_lines, st.col_lo, st.col_hi, st.half_width = (len(palette) if palette is not None else 1), K, 0, W - 1, 22
    for i, v in enumerate(np.asarray(palette if palette is not None else [], np.uint8).reshape(-1)):
        st.palette[i] = int(v)
    for i, v in enumerate(np.asarray(colours, np.uint8).reshape(-1)):
        st.line_rgb[i] = int(v)
    for i, v in enumerate(styles):
        st.line_style[i] = int(v)
    mode = _hip.RENDER_BASE_LABELS if palette is not None else _hip.RENDER_BASE_IMAGE
    ic = 1 if base.ndim == 3 else base.shape[3]
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    lib = _hip.lib()

    def call():
        _hip.check(lib.oct_render_rgba(mode, base_dev.data_ptr(), ic, None if rows_dev is None else rows_dev.data_ptr(),
                                       C.byref(st), B, H, W, renderer.out_dev.data_ptr(), stream), "oct_render_rgba")

    def once():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(kernel_reps):
            call()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / kernel_reps
    for _ in range(5):
        call()
    torch.cuda.synchronize()
    ms = stats([once() for _ in range(reps)])
    moved = base.size + (0 if lines is None else lines.size * 2) + B * H * W * 4
    return {"case": name, "lines": K, "ms_per_chunk": ms, "bytes_moved": int(moved),
            "GBps": round(moved / (ms["median"] * 1e-3) / 1e9, 1)}


def write_model_and_data(root: Path, n: int, Cc: int):
    from oct_image_segmentation_models_amd.common import h5io
    from oct_image_segmentation_models_amd.models.engine_model import Model
    config = dict(input_channels=1, num_classes=Cc, image_height=H, image_width=W, start_neurons=8, pool_layers=4)
    cfg = on.UNetConfig(num_classes=Cc, start_neurons=8, pool_layers=4)
    params, state = on.init_params(cfg, seed=3, dtype=np.float32, randomize_bn=True)
    m = Model(name="unet", config=config)
    m.set_weights(on.keras_weight_list(params, state))
    (root / "model").mkdir()
    m.save(root / "model" / "model.npz")
    with open(root / "model" / "model_config.json", "w") as fh:
        json.dump(config, fh)
    images, labels = on.synth_scans(n, H, W, Cc, seed=5)
    h5io.save(root / "test.hdf5", {"test_images": images, "test_labels": labels})
    return root / "model" / "model.npz", root / "test.hdf5"


def end_to_end(n):
    from oct_image_segmentation_models_amd.evaluation import eval_model
    from oct_image_segmentation_models_amd.evaluation.evaluation_parameters import EvaluationParameters, EvaluationSaveParams
    out = {"what": f"evaluate_model over {n} scans, {H}x{W}, 3 classes, batch 32, gs_device with device ties, metrics_device, "
                   "files included", "off": [], "on": []}
    with tempfile.TemporaryDirectory() as tmp:
        root = Path(tmp)
        model_path, data = write_model_and_data(root, n, 3)
        for rep in range(3):                                       # (the first pass warms both settings up: not reported)
            for name, switch in (("off", False), ("on", True)):
                ep = EvaluationParameters(model_path=model_path, mlflow_tracking_uri=None, mlflow_run_uuid=None,
                                          test_dataset_path=data, save_foldername=root / f"{name}{rep}",
                                          save_params=EvaluationSaveParams(), graph_search=True, metrics=METRICS,
                                          batch_size=32, gs_device=True, gs_device_ties="device", metrics_device=True,
                                          png_plots=switch)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                eval_model(ep)
                dt = (time.perf_counter() - t0) / n
                if rep:
                    out[name].append(round(dt, 4))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--kernel-reps", type=int, default=20)
    ap.add_argument("--e2e", type=int, default=0, help="also time evaluate_model over this many scans, png_plots off / on")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_png.py measures on the GPU: none is visible")
    renderer = PngRenderer(B, H, W, "cuda:0")
    res = {"what": f"PNG pictures, chunk of {renderer.chunk} images of {H}x{W} (tools/bench_png.py)", "reps": a.reps,
           "kernel_reps": a.kernel_reps, "default_filter": png.FILTER, "default_level": png.LEVEL}
    img3, lab3, tr3 = scans_and_truths(3)
    img8, lab8, tr8 = scans_and_truths(8)
    pred8 = np.ascontiguousarray(np.where(tr8 > 0, np.minimum(tr8 + 3, H - 1), 0).astype(np.uint16))
    res["kernel"] = [
        kernel_case(renderer, "scan, base only", img3, None, [], [], None, a.reps, a.kernel_reps),
        kernel_case(renderer, "class map, base only", lab3, None, [], [], plotting.region_palette(3), a.reps, a.kernel_reps),
        kernel_case(renderer, "scan + 2 solid lines", img3, tr3, plotting.TRUTH_COLOURS[:2], [0, 0], None, a.reps, a.kernel_reps),
        kernel_case(renderer, "scan + 7 solid + 7 dotted lines", img8, np.ascontiguousarray(np.concatenate([tr8, pred8], axis=1)),
                    plotting.TRUTH_COLOURS[:7] + plotting.PREDICT_COLOURS[:7], [0] * 7 + [1] * 7, None, a.reps, a.kernel_reps),
    ]

    # ---- the PNG stage per image: render + download, encode, write ----
    overlay_kw = dict(lines=tr3, colours=plotting.TRUTH_COLOURS[:2])
    renderer.render(img3, **overlay_kw)

    def render_once():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        renderer.render(img3, **overlay_kw)
        return (time.perf_counter() - t0) / B * 1e3
    overlays = renderer.render(img3[:8], lines=tr3[:8], colours=plotting.TRUTH_COLOURS[:2])
    maps = renderer.render(lab3[:8], palette=plotting.region_palette(3))
    stage = {"render_and_download_ms_per_image": stats([render_once() for _ in range(a.reps)]), "encode": []}
    for kind, pics in (("overlay", overlays), ("class map", maps)):
        for f in (png.FILTER_NONE, png.FILTER_SUB, png.FILTER_UP):
            for level in (1, 3, 6, 9):
                t0 = time.perf_counter()
                sizes = [len(png.encode_rgba(p, f, level)) for p in pics]
                ms = (time.perf_counter() - t0) / len(pics) * 1e3
                stage["encode"].append({"picture": kind, "filter": f, "level": level, "ms_per_image": round(ms, 3),
                                        "bytes": int(np.mean(sizes))})
    with tempfile.TemporaryDirectory() as tmp:
        blobs = [png.encode_rgba(p) for p in list(overlays) + list(maps)]
        t0 = time.perf_counter()
        for rep in range(8):
            for i, blob in enumerate(blobs):
                with open(os.path.join(tmp, f"{rep}_{i}.png"), "wb") as fh:
                    fh.write(blob)
        stage["write_ms_per_image"] = round((time.perf_counter() - t0) / (8 * len(blobs)) * 1e3, 4)
    res["png_stage"] = stage
    if a.e2e:
        res["evaluate_model_s_per_image"] = end_to_end(a.e2e)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
