"""Generates tests/golden/minpath_device_golden.npz by running the REAL reference implementation of the host
post-process (``oct_image_segmentation_models.min_path_processing.graph_search.segment_maps``, numpy + heapq only) on
seeded small boundary maps, as make_min_path_golden.py does.  The reference itself never travels; only the vectors do.

    PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=<reference checkout> python tests/golden/make_minpath_device_golden.py

Per shape tag ``s`` (H x W): ``s_maps`` (n, H, W) uint8, ``s_family`` (n,) index into ``families``, and per max_grad g
``s_g{g}_rows`` (n, W) uint16 (the reference delineations) and ``s_g{g}_cost`` (n,) float64 (the reference's final
distance of the end vertex, read from what its ``run_dijkstras`` returns)."""
import os
import sys

import numpy as np

from oct_image_segmentation_models.min_path_processing import graph_search as gs  # noqa: E402  (reference)

FAMILIES = ["noise", "ridge_noise", "ridge_clean", "ridge_jump3", "ridge_salt", "zeros", "full"]
SHAPES = [(16, 24), (12, 40), (70, 33), (3, 9), (2, 9), (1, 5)]          # H x W
PER_FAMILY = 4                                                           # seeded maps per random family and shape
BASE_SEED = 20260


def max_grads(H):
    return [1, 2, 3, min(16, H + 3)]        # the last one: larger than H where the host library's limit of 16 allows


def ridge(rng, H, W, max_step, force_jump=0):
    """Row of a one-pixel ridge per column: a random walk with steps in -max_step..max_step, kept inside the image; with
    ``force_jump`` at least one step of exactly that size (where the height allows it)."""
    r = np.zeros(W, np.int64)
    r[0] = rng.integers(0, H)
    for j in range(1, W):
        r[j] = np.clip(r[j - 1] + rng.integers(-max_step, max_step + 1), 0, H - 1)
    if force_jump and H > force_jump:
        j = int(rng.integers(1, W))
        base = int(rng.integers(0, H - force_jump))
        r[:j] = np.clip(r[:j] - r[j - 1] + base, 0, H - 1)
        r[j:] = np.clip(r[j:] - r[j] + base + force_jump, 0, H - 1)
    return r


def make_maps(H, W, seed):
    maps, fam = [], []
    for f, name in enumerate(FAMILIES):
        if name == "zeros":
            maps.append(np.zeros((H, W), np.uint8)); fam.append(f); continue
        if name == "full":
            maps.append(np.full((H, W), 255, np.uint8)); fam.append(f); continue
        for k in range(PER_FAMILY):
            rng = np.random.default_rng([seed, H, W, f, k])
            if name == "noise":
                m = rng.integers(0, 256, (H, W)).astype(np.uint8)
            else:
                m = np.zeros((H, W), np.uint8)
                if name == "ridge_noise":
                    m = rng.integers(0, 200, (H, W)).astype(np.uint8)
                r = ridge(rng, H, W, 3 if name == "ridge_jump3" else 1, force_jump=3 if name == "ridge_jump3" else 0)
                m[r, np.arange(W)] = 255
                if name == "ridge_salt":
                    salt = rng.uniform(size=m.shape) < 0.02
                    m[salt] = rng.integers(0, 256, int(salt.sum())).astype(np.uint8)
            maps.append(m); fam.append(f)
    return np.stack(maps), np.array(fam, np.uint8)


def main():
    end_distance = []
    run = gs.run_dijkstras

    def recording(prob_map, start_ind, graph_structure):
        paths = run(prob_map, start_ind, graph_structure)
        end_distance.append(float(paths[-1][0]))
        return paths
    gs.run_dijkstras = recording

    out = {"families": np.array(FAMILIES), "shapes": np.array(SHAPES, np.int32)}
    for H, W in SHAPES:
        tag = f"s{H}x{W}"
        maps, fam = make_maps(H, W, BASE_SEED)
        out[f"{tag}_maps"], out[f"{tag}_family"] = maps, fam
        out[f"{tag}_max_grads"] = np.array(max_grads(H), np.int32)
        maps_t = np.ascontiguousarray(np.transpose(maps, (0, 2, 1)))      # (n, W, H)  evaluation.py:292
        for g in max_grads(H):
            graph = gs.create_graph_structure((W, H), max_grad=g)
            del end_distance[:]
            preds, _, _ = gs.segment_maps(maps_t, None, graph)
            assert len(end_distance) == maps.shape[0]
            out[f"{tag}_g{g}_rows"] = preds.astype(np.uint16)
            out[f"{tag}_g{g}_cost"] = np.array(end_distance, np.float64)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "minpath_device_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    sys.exit(main())
