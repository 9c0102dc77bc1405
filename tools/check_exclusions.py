#!/usr/bin/env python3
"""CPU pre-check of the scan seeds of tests/test_gpu_layer_local.py's non-power-of-two tests: the layer-local fp64 model
(tests/layer_local.py) on the tensors of a defect-free engine (tests/test_layer_local.perfect_engine: the oracle's
primitives, the tests' weights, scans, rolls and dropout bits) must report no failure and exclude fewer than EXCLUDE_MAX
of the elements -- then what a device run excludes beyond that is the device's.  No GPU.
usage: check_exclusions.py [H W P B mode seed step]     (no arguments: the four training inputs of the tests, full batch)"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402

from oracle import unet_numpy as on  # noqa: E402
from tests import layer_local as ll  # noqa: E402
from tests.helpers import dropout_keep_mask  # noqa: E402
from tests.test_gpu_layer_local import SCAN_SEED, ragged_scans  # noqa: E402
from tests.test_layer_local import perfect_engine  # noqa: E402


def run(H, W, P, B, mode, seed, step):
    t0 = time.time()
    cfg = on.UNetConfig(num_classes=3, start_neurons=8, pool_layers=P)
    params, _ = on.init_params(cfg, seed=7, dtype=np.float32, randomize_bn=True)
    p64 = [{k: v.astype(np.float64) for k, v in p.items()} for p in params]
    img, lab = ragged_scans(B, H, W, seed, step)
    mask = dropout_keep_mask(5, 3, (B, H >> P, W >> P, 8 << P)).astype(np.float64)      # engine seed 5, dropout step 3
    fused = [True] * (len(on.build_plan(cfg)) - 1)
    S, _, _, _ = perfect_engine(cfg, p64, img, lab[..., 0], mask, mode, fused)
    rep = ll.LayerLocal(cfg, p64, S, img, labels=lab[..., 0], dropout_mask=mask, mode=mode, chunk=1).run()
    share = rep.excluded / max(rep.elements, 1)
    print(f"{H}x{W} P={P} B={B} {mode} scan seed {seed} roll {step}: {len(rep.failures)} failures, excluded {rep.excluded} of "
          f"{rep.elements} = {share:.2e} (cap {ll.EXCLUDE_MAX:.0e}), {time.time() - t0:.0f} s", flush=True)
    for f in rep.failures[:5]:
        print("   ", f)
    return not rep.failures and share <= ll.EXCLUDE_MAX


if __name__ == "__main__":
    if len(sys.argv) > 1:
        a = sys.argv[1:8]
        jobs = [(int(a[0]), int(a[1]), int(a[2]), int(a[3]), a[4], int(a[5]), int(a[6]))]
    else:
        jobs = [(272, 432, 4, 8, "f32", SCAN_SEED[272, 432], 5), (272, 432, 4, 3, "f32", SCAN_SEED[272, 432, "partial"], 11),
                (496, 768, 4, 8, "f32", SCAN_SEED[496, 768], 5), (480, 736, 5, 8, "bf16", SCAN_SEED[480, 736], 5)]
    sys.exit(0 if all([run(*j) for j in jobs]) else 1)
