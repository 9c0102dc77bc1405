"""Generates tests/golden/png_reference_golden.npz: inputs and the RGBA pixels that the REAL reference's
``common/plotting.py::save_image_plot`` writes for them under matplotlib (Agg).  The reference's file is imported by path,
with a stub for ``typeguard`` (its only import beyond matplotlib and numpy); only inputs and recorded pixels travel.

    python tests/golden/make_png_golden.py <path of the reference's common/plotting.py>

Cases: a 64x256 one-channel ramp holding all 256 levels, a random 36x68x1 and a random 36x68x3 scan (``cm.gray`` /
``None`` with vmin=0, vmax=255, as evaluation.py:514-520 calls it), label maps 36x68 with C = 3 and C = 8, each containing
class 0 and class C-1 (``ListedColormap(region_colours, N=C)``)."""
import importlib.util
import os
import sys
import tempfile
import types
from pathlib import Path

import numpy as np


def load_reference(path):
    stub = types.ModuleType("typeguard")
    stub.typechecked = lambda f=None, **kw: f if f is not None else (lambda g: g)
    sys.modules["typeguard"] = stub
    import matplotlib
    matplotlib.use("Agg")
    spec = importlib.util.spec_from_file_location("reference_plotting", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    ref = load_reference(sys.argv[1])
    from matplotlib import cm
    from PIL import Image
    rng = np.random.default_rng(77)
    ramp = np.tile(np.arange(256, dtype=np.uint8)[None, :], (64, 1))[:, :, None]
    scan1 = rng.integers(0, 256, (36, 68, 1), dtype=np.uint8)
    scan3 = rng.integers(0, 256, (36, 68, 3), dtype=np.uint8)
    labels = {}
    for C in (3, 8):
        lab = rng.integers(0, C, (36, 68)).astype(np.uint8)
        lab[:6] = (np.arange(68) * C // 68)[None, :]            # broad bands, so class 0 and class C-1 are surely there
        assert lab.min() == 0 and lab.max() == C - 1
        labels[C] = lab
    out = {"ramp_in": ramp, "scan1_in": scan1, "scan3_in": scan3}
    with tempfile.TemporaryDirectory() as tmp:
        def shoot(name, image, cmap, **kw):
            path = Path(tmp) / f"{name}.png"
            ref.save_image_plot(image, path, cmap=cmap, **kw)
            rgba = np.array(Image.open(path).convert("RGBA"))
            assert rgba.shape == image.shape[:2] + (4,), (name, rgba.shape)
            out[f"{name}_out"] = rgba
        shoot("ramp", ramp, cm.gray, vmin=0, vmax=255)
        shoot("scan1", scan1, cm.gray, vmin=0, vmax=255)
        shoot("scan3", scan3, None, vmin=0, vmax=255)
        for C, lab in labels.items():
            out[f"labels{C}_in"] = lab
            shoot(f"labels{C}", lab, ref.colors.ListedColormap(ref.region_colours, N=C))
    dst = os.path.join(os.path.dirname(os.path.abspath(__file__)), "png_reference_golden.npz")
    np.savez_compressed(dst, **out)
    print(dst, os.path.getsize(dst), "bytes")


if __name__ == "__main__":
    main()
