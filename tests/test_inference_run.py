"""CPU tests of ``evaluation/pipeline.py::InferenceRun`` with an injected batch source: ``graph_search`` in the three
search modes on ALL maps of tests/golden/minpath_device_golden.npz (tied and untied; the kernel is stood in for by its
numpy restatement ``delineate_dp``, which tests/test_gpu_minpath.py holds it to), and the closing of the worker pools
on the normal and on the exceptional way out of the ``with`` block."""
import glob
import os
from pathlib import Path

import numpy as np
import pytest

import __graft_entry__ as ge

ROOT = Path(__file__).resolve().parent.parent
G = np.load(ROOT / "tests" / "golden" / "minpath_device_golden.npz")
M, B = 2, 8                   # maps per image; 22 fixture maps = 11 images = a batch of 8 and a ragged one of 3


def _cases():
    for h, w in G["shapes"]:
        tag = f"s{int(h)}x{int(w)}"
        for g in G[f"{tag}_max_grads"]:
            yield tag, int(h), int(w), int(g)


def _batches(maps, g, device):
    from oct_image_segmentation_models_amd.evaluation.pipeline import Batch
    from oct_image_segmentation_models_amd.min_path_processing.device_search import delineate_dp
    n = maps.shape[0]
    return [Batch(lo, min(lo + B, n), np.zeros((min(lo + B, n) - lo,) + maps.shape[2:], np.uint8), maps[lo:lo + B],
                  None, delineate_dp(maps[lo:lo + B], g) if device else None) for lo in range(0, n, B)]


def _run(maps, g, truths, **kw):
    """Every batch of ``maps`` through ``graph_search`` of an InferenceRun over the injected records -> (per-image
    results, the run after its ``with`` block)."""
    from oct_image_segmentation_models_amd.evaluation.pipeline import InferenceRun
    images = np.empty(maps.shape[:1] + maps.shape[2:] + (1,), np.uint8)
    out = []
    with InferenceRun(None, images, B, M + 1, graph_search=True, gsgrad=g, gs_workers=1,
                      batches=_batches(maps, g, kw.get("gs_device", False)), **kw) as run:
        spans = []
        for b in run:
            spans.append((b.lo, b.hi))
            out += run.graph_search(b, None if truths is None else truths[b.lo:b.hi])
    assert spans == [(0, 8), (8, 11)]
    return out, run


@pytest.fixture(scope="module")
def fixture_runs():
    """Per (shape, max_grad): the maps as 11 images of 2, seeded truths, the tie flags and the pool-mode results."""
    ge.build()
    from oct_image_segmentation_models_amd.min_path_processing import graph_search
    from oct_image_segmentation_models_amd.min_path_processing.device_search import delineate_dp
    assert graph_search._native() is not None, "liboct_minpath.so was not built"
    rng = np.random.default_rng(11)
    runs = {}
    for tag, H, W, g in _cases():
        maps = np.ascontiguousarray(G[f"{tag}_maps"].reshape(-1, M, H, W))
        assert maps.shape[0] == 11 and maps.size == G[f"{tag}_maps"].size          # no map left out
        truths = rng.integers(0, H + 1, (11, M, W)).astype(np.float64)             # zeros exercise calc_errors' invalid rows
        runs[tag, g] = (maps, truths, delineate_dp(maps, g)[2], _run(maps, g, truths)[0])
    return runs


def test_pool_mode_equals_segment_maps_per_image(fixture_runs):
    from oct_image_segmentation_models_amd.min_path_processing import graph_search
    for (tag, g), (maps, truths, _, got) in fixture_runs.items():
        H, W = maps.shape[2:]
        graph = graph_search.create_graph_structure((W, H), g)
        assert len(got) == 11
        for i in range(11):
            pred, err, _ = graph_search.segment_maps(np.transpose(maps[i], (0, 2, 1)), truths[i], graph)
            assert got[i][0].dtype == np.uint16 and np.array_equal(got[i][0], pred), (tag, g, i)
            assert np.array_equal(got[i][1], err, equal_nan=True), (tag, g, i)


def test_device_mode_with_host_ties_equals_pool_mode_and_starts_the_pool_per_tied_batch(fixture_runs):
    n_tied = n_untied = 0
    for (tag, g), (maps, truths, tied, want) in fixture_runs.items():
        got, run = _run(maps, g, truths, gs_device=True, gs_device_ties="host")
        assert run.pool is None
        for i in range(11):
            assert np.array_equal(got[i][0], want[i][0]), (tag, g, i)
            assert np.array_equal(got[i][1], want[i][1], equal_nan=True), (tag, g, i)
        assert run.host_ties.calls == int(tied[:B].any()) + int(tied[B:].any()), (tag, g)
        n_tied, n_untied = n_tied + int(tied.sum()), n_untied + int((~tied).sum())
    assert n_tied > 0 and n_untied > 0                             # the fixture holds both kinds


def test_device_mode_with_device_ties_never_starts_the_pool(fixture_runs):
    for (tag, g), (maps, truths, tied, want) in fixture_runs.items():
        got, run = _run(maps, g, truths, gs_device=True, gs_device_ties="device")
        assert run.pool is None and run.host_ties.calls == 0
        for i in range(11):
            for m in np.nonzero(~tied[i])[0]:
                assert np.array_equal(got[i][0][m], want[i][0][m]), (tag, g, i, m)
                assert np.array_equal(got[i][1][m], want[i][1][m], equal_nan=True), (tag, g, i, m)


@pytest.mark.parametrize("mode", ["pool", "device"])
@pytest.mark.parametrize("fail", [False, True])
def test_leaving_the_block_closes_the_pools(mode, fail):
    """Spawned workers and a batch large enough (>= 1 MiB) to travel as a /dev/shm file: after the ``with`` block, left
    normally or by an exception of the consumer, no worker lives and no file of this process remains.  Map 0 of every
    image is a clean ridge, map 1 is all zeros (every path ties: the device mode starts its lazy pool)."""
    ge.build()
    from oct_image_segmentation_models_amd.evaluation.pipeline import Batch, InferenceRun
    from oct_image_segmentation_models_amd.min_path_processing.device_search import delineate_dp
    n, H, W = 8, 256, 512
    maps = np.zeros((n, M, H, W), np.uint8)
    maps[:, 0, H // 2, :] = 255
    device = mode == "device"
    found = delineate_dp(maps, 1) if device else None
    assert maps[:, 1:].nbytes >= 1 << 20 and (not device or (found[2][:, 1].all() and not found[2][:, 0].any()))
    mine = os.path.join("/dev/shm", f"oct_gs_{os.getpid()}_*.u8")
    assert glob.glob(mine) == []
    workers = []

    class ConsumerError(Exception):
        pass

    def consume():
        with InferenceRun(None, np.empty((n, H, W, 1), np.uint8), n, M + 1, graph_search=True, gs_workers=2,
                          gs_device=device, batches=[Batch(0, n, np.zeros((n, H, W), np.uint8), maps, None, found)]) as run:
            runs.append(run)
            for b in run:
                res = run.graph_search(b)
                assert len(res) == n and all((r[0][0] == H // 2).all() for r in res)
                pool = run.pool if run.pool is not None else run.host_ties._pool
                assert pool is not None
                if pool._pool is not None:                         # (None where worker processes cannot start: inline)
                    workers.extend(pool._pool._pool)
                    assert len(workers) == 2 and all(w.is_alive() for w in workers)
                if fail:
                    raise ConsumerError("the per-image loop failed")

    runs = []
    if fail:
        with pytest.raises(ConsumerError):
            consume()
    else:
        consume()
    run, = runs
    inner = run.pool if run.pool is not None else run.host_ties
    assert inner._pool is None                                     # SegmentPool.close() / LazyPool.close() ran
    assert not any(w.is_alive() for w in workers)
    assert glob.glob(mine) == []


def test_a_failing_construction_leaves_no_pool():
    """Ground-truth labels outside 0..C-1 are refused before any pool exists."""
    import multiprocessing as mp
    from oct_image_segmentation_models_amd.evaluation.pipeline import InferenceRun
    before = set(mp.active_children())
    with pytest.raises(ValueError):
        InferenceRun(None, np.empty((2, 8, 8, 1), np.uint8), 2, 3, gt=np.full((2, 8, 8), 3), graph_search=True,
                     gs_workers=2, batches=[])
    assert set(mp.active_children()) == before
