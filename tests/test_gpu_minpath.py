"""GPU tests of the min-path boundary search on the device (oct_minpath_device, min_path_processing/device_search.py)
against its numpy restatement ``delineate_dp`` (rows, tie flags and fp64 costs all exact), against the native host
search on untied maps, through ``BatchedPredictor(minpath=...)`` and through ``evaluate_model`` / ``predict``."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest
import torch

from oracle import unet_numpy as on
from tests.helpers import datasets_equal, save_untrained_model

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
G = np.load(ROOT / "tests" / "golden" / "minpath_device_golden.npz")
SHAPES = [(int(h), int(w)) for h, w in G["shapes"]]


def _device(maps, max_grad, batch=None):
    """maps (n, M, H, W) uint8 numpy -> (rows uint16, cost, tied bool) numpy through DeviceMinPath."""
    from oct_image_segmentation_models_amd.min_path_processing.device_search import DeviceMinPath
    n, M, H, W = maps.shape
    mp = DeviceMinPath(batch or n, M, H, W, max_grad, "cuda:0")
    out = mp.to_host(*mp(torch.from_numpy(np.ascontiguousarray(maps)).cuda()))
    torch.cuda.synchronize()
    return out


def _assert_equals_dp(maps, max_grad, what):
    from oct_image_segmentation_models_amd.min_path_processing.device_search import delineate_dp
    rows, cost, tied = _device(maps, max_grad)
    e_rows, e_cost, e_tied = delineate_dp(maps, max_grad)
    assert rows.dtype == np.uint16 and np.array_equal(rows, e_rows), what
    assert np.array_equal(cost, e_cost), what                      # fp64, bit for bit
    assert np.array_equal(tied, e_tied), what
    return rows, cost, tied


@pytest.mark.parametrize("H,W", SHAPES)
def test_device_equals_restatement_on_fixture_maps(H, W):
    """Every fixture map and max_grad, batched as (B, M) = (3, 1) and (5, 3) -- B*M odd --, with M = 1 and with M = 7."""
    tag = f"s{H}x{W}"
    maps = G[f"{tag}_maps"]
    n = maps.shape[0]
    assert n >= 21
    for g in (int(x) for x in G[f"{tag}_max_grads"]):
        for B, M, first in ((3, 1, 0), (5, 3, n - 15), (n, 1, 0), (3, 7, 0)):
            batch = maps[first:first + B * M].reshape(B, M, H, W)
            _assert_equals_dp(batch, g, (tag, g, B, M))


def _seeded_maps(H, W, seed, n_noise=3, n_ridge=3):
    rng = np.random.default_rng([seed, H, W])
    maps = [rng.integers(0, 256, (H, W)).astype(np.uint8) for _ in range(n_noise)]
    for _ in range(n_ridge):                                       # a 255 ridge with steps <= 1 under noise below 200
        m = rng.integers(0, 200, (H, W)).astype(np.uint8)
        r = np.clip(np.cumsum(rng.integers(-1, 2, W)) + H // 2, 0, H - 1)
        m[r, np.arange(W)] = 255
        maps.append(m)
    return np.stack(maps)


# more rows than a 256-thread block; a row count and a width that divide neither a wave nor the staging tile; tiny;
# and a map whose W*H predecessor bytes do not fit LDS (they go through the workspace)
@pytest.mark.parametrize("H,W", [(300, 20), (65, 130), (5, 7), (260, 520)])
def test_launch_geometry_shapes(H, W):
    from oct_image_segmentation_models_amd.min_path_processing import graph_search
    assert graph_search._native() is not None
    maps = _seeded_maps(H, W, 77).reshape(3, 2, H, W)
    for g in (1, 2):
        rows, cost, tied = _assert_equals_dp(maps, g, (H, W, g))
        assert not tied.reshape(-1)[3:].any()                      # the ridge maps: a unique zero-cost path
        graph = graph_search.create_graph_structure((W, H), g)
        flat = maps.reshape(-1, H, W)
        for k in np.nonzero(~tied.reshape(-1))[0]:
            host = graph_search.delineate_boundary(np.transpose(flat[k]) / 255, graph)
            assert np.array_equal(rows.reshape(-1, W)[k], host.astype(np.uint16)), (H, W, g, k)


def test_real_size_equals_host_path():
    """256x512, B = 4, M = 2: boundary maps of synthetic ground-truth labels and the same with 2 % salt; with "host"
    ties the merged rows equal the host search on every map."""
    from oct_image_segmentation_models_amd.engine import UNetEngine
    from oct_image_segmentation_models_amd.min_path_processing import graph_search
    from oct_image_segmentation_models_amd.min_path_processing.device_search import delineate_dp, merge_ties
    from oct_image_segmentation_models_amd.min_path_processing.pool import SegmentPool
    H, W, Cc, B = 256, 512, 3, 4
    eng = UNetEngine(device="cuda:0", input_channels=1, num_classes=Cc, image_height=H, image_width=W, max_batch=B,
                     training=False, seed=2, init_seed=4)
    _, labels = on.synth_scans(B, H, W, Cc, seed=5)
    clean = eng.boundary_maps(torch.from_numpy(np.ascontiguousarray(labels[..., 0].astype(np.uint8))).cuda()).cpu().numpy()
    rng = np.random.default_rng(8)
    salted = clean.copy()
    salt = rng.uniform(size=salted.shape) < 0.02
    salted[salt] = rng.integers(0, 256, int(salt.sum())).astype(np.uint8)
    graph = graph_search.create_graph_structure((W, H), 1)
    with SegmentPool((H, W), 1, workers=1) as pool:
        for name, maps in (("clean", clean), ("salted", salted)):
            rows, cost, tied = _device(maps, 1)
            e_rows, e_cost, e_tied = delineate_dp(maps, 1)
            assert np.array_equal(rows, e_rows) and np.array_equal(cost, e_cost) and np.array_equal(tied, e_tied), name
            got = merge_ties(maps, rows, tied, None, pool.segment, "host")
            for i in range(B):
                host, _, _ = graph_search.segment_maps(np.transpose(maps[i], (0, 2, 1)), None, graph)
                assert np.array_equal(got[i][0], host), (name, i)
                assert np.array_equal(rows[i][~tied[i]], host[~tied[i]]), (name, i)


@pytest.mark.parametrize("H,W", [(16, 24), (256, 512)])          # default LDS size, and the raised limit (128 KiB of bytes)
def test_call_is_graph_capturable(H, W):
    """One launch, no allocation, no host wait: the call records into a stream capture and the replay serves new maps."""
    from oct_image_segmentation_models_amd.min_path_processing.device_search import DeviceMinPath, delineate_dp
    first, second = _seeded_maps(H, W, 5, 2, 2).reshape(2, 2, H, W), _seeded_maps(H, W, 6, 2, 2).reshape(2, 2, H, W)
    mp = DeviceMinPath(2, 2, H, W, 1, "cuda:0")
    d = torch.from_numpy(first).cuda()
    mp(d)                                                         # outside the capture first: raises the LDS limit
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = mp(d)
    d.copy_(torch.from_numpy(second).cuda())
    graph.replay()
    torch.cuda.synchronize()
    rows, cost, tied = mp.to_host(*outs)
    e = delineate_dp(second, 1)
    assert np.array_equal(rows, e[0]) and np.array_equal(cost, e[1]) and np.array_equal(tied, e[2])


def test_abi_errors_launch_nothing():
    from oct_image_segmentation_models_amd import _hip
    lib = _hip.lib()
    B, M, H, W, g = 2, 3, 9, 11, 1
    need = lib.oct_minpath_workspace_bytes(B, M, H, W, g)
    assert need > 0
    for bad in ((B, M, 65536, W, g), (B, M, H, 65536, g), (B, M, H, W, 0), (B, M, H, W, 17), (0, M, H, W, g),
                (B, 0, H, W, g), (B, M, 0, W, g), (B, M, 40000, W, g)):
        assert lib.oct_minpath_workspace_bytes(*bad) == 0, bad
    maps = torch.randint(0, 256, (B, M, H, W), dtype=torch.uint8, device="cuda")
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    rows = torch.full((B, M, W), 7, dtype=torch.int16, device="cuda")
    cost = torch.full((B, M), 7.0, dtype=torch.float64, device="cuda")
    tied = torch.full((B, M), 7, dtype=torch.uint8, device="cuda")

    def call(maps_p=maps.data_ptr(), g_=g, ws_p=ws.data_ptr(), ws_n=need, rows_p=rows.data_ptr(), cost_p=cost.data_ptr(),
             tied_p=tied.data_ptr(), H_=H, W_=W):
        return lib.oct_minpath_device(maps_p, B, M, H_, W_, g_, ws_p, ws_n, rows_p, cost_p, tied_p,
                                      C.c_void_p(torch.cuda.current_stream().cuda_stream))

    for kw, msg in ((dict(maps_p=None), b"null"), (dict(ws_p=None), b"null"), (dict(rows_p=None), b"null"),
                    (dict(cost_p=None), b"null"), (dict(tied_p=None), b"null"), (dict(g_=0), b"max_grad"),
                    (dict(g_=17), b"max_grad"), (dict(ws_n=need - 1), b"workspace too small"), (dict(H_=65536), b"uint16"),
                    (dict(W_=65536), b"uint16")):
        assert call(**kw) < 0, kw
        assert msg in lib.oct_last_error(), (kw, lib.oct_last_error())
    torch.cuda.synchronize()
    assert (rows == 7).all() and (cost == 7.0).all() and (tied == 7).all()          # nothing was written
    assert call() == 0
    torch.cuda.synchronize()
    assert (tied <= 1).all() and (rows.cpu().numpy().view(np.uint16) < H).all() and (cost >= 0).all()


def test_batched_predictor_minpath_double_buffers():
    """2 1/2 batches, then 5 batches (each pinned / device buffer pair is reused): rows, costs and tie flags per image equal
    a direct DeviceMinPath call on the maps the predictor yields; without minpath the records are what they were."""
    from oct_image_segmentation_models_amd.engine import UNetEngine
    from oct_image_segmentation_models_amd.evaluation.pipeline import BatchedPredictor
    from oct_image_segmentation_models_amd.min_path_processing.device_search import DeviceMinPath
    H, W, Cc, B = 32, 64, 4, 4
    eng = UNetEngine(device="cuda:0", input_channels=1, num_classes=Cc, image_height=H, image_width=W, start_neurons=8,
                     pool_layers=2, max_batch=B, training=False, seed=2, init_seed=4)
    images, _ = on.synth_scans(20, H, W, Cc, seed=21)
    mp = DeviceMinPath(B, Cc - 1, H, W, 1, "cuda:0")
    direct = DeviceMinPath(B, Cc - 1, H, W, 1, "cuda:0")
    # (a predictor captures the engine's one forward graph over its own input buffer: the plain one runs first)
    plain = list(BatchedPredictor(eng, B, want_maps=True).run(images[:10]))
    assert all(b.surface is None and b.minpath is None for b in plain)
    pred = BatchedPredictor(eng, B, want_maps=True, minpath=mp)
    for n, spans in ((10, [(0, 4), (4, 8), (8, 10)]), (20, [(4 * i, 4 * i + 4) for i in range(5)])):
        got = list(pred.run(images[:n]))
        assert [(b[0], b[1]) for b in got] == spans
        for b in got:
            lo, hi, maps, (rows, cost, tied) = b.lo, b.hi, b.maps, b.minpath
            assert rows.dtype == np.uint16 and rows.shape == (hi - lo, Cc - 1, W) and tied.dtype == bool
            e = direct.to_host(*direct(torch.from_numpy(maps).cuda()))
            assert np.array_equal(rows, e[0]) and np.array_equal(cost, e[1]) and np.array_equal(tied, e[2]), (n, lo)
    again = list(pred.run(images[:10]))
    assert all(np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3]) for a, b in zip(plain, again))


def _path_cost(map_hw, rows):
    """Cost of a delineation, summed along the path in the search's order and with its edge expression."""
    p = map_hw / 255
    d, prev = 0.0, 1.0
    for j, r in enumerate(rows):
        d = d + (2.0 - (prev + p[r, j]))
        prev = p[r, j]
    return d + (2.0 - (prev + 1.0))


@pytest.mark.parametrize("dtype", ["u8", "f32"])
def test_evaluate_and_predict_with_gs_device(tmp_path, dtype):
    """The small golden dataset (noise images: an untrained net's maps, tied and untied) through evaluate_model and
    predict: "host" ties reproduce the gs_device=False outputs and files; "device" ties give the same path cost on every
    map and the same rows on every untied map, and never start the host pool."""
    from oct_image_segmentation_models_amd.common import dataset_loader as dl, h5io
    from oct_image_segmentation_models_amd.common.dataset import Dataset
    from oct_image_segmentation_models_amd.evaluation import eval_model
    from oct_image_segmentation_models_amd.evaluation.evaluation_parameters import EvaluationParameters, EvaluationSaveParams
    from oct_image_segmentation_models_amd.min_path_processing import device_search
    from oct_image_segmentation_models_amd.prediction import predict
    from oct_image_segmentation_models_amd.prediction.prediction_parameters import PredictionParams, PredictionSaveParams
    data = ROOT / "tests" / "golden" / "dataset_small.hdf5"
    images, labels, _ = dl.load_testing_data(dl.open_dataset(data))
    n, H, W = images.shape[:3]
    Cc = 3
    if dtype == "f32":                                               # the non-uint8 path of both workflows
        data = tmp_path / "f32.hdf5"
        images = images.astype(np.float32)
        h5io.save(data, {"test_images": images, "test_labels": labels})
    save_untrained_model(tmp_path, H, W, Cc, 8, 2)
    metrics = ["dice_coef_classes", "dice_coef_macro", "dice_coef_micro"]

    def evaluate(name, **kw):
        ep = EvaluationParameters(model_path=tmp_path / "model" / "model.npz", mlflow_tracking_uri=None, mlflow_run_uuid=None,
                                  test_dataset_path=data, save_foldername=tmp_path / name, save_params=EvaluationSaveParams(),
                                  graph_search=True, metrics=metrics, batch_size=2, **kw)
        ep.gs_workers = 1
        return eval_model(ep)

    started = []
    real_call = device_search.LazyPool.__call__

    def counting(self, maps, truths=None):
        started.append(maps.shape[0])
        return real_call(self, maps, truths)
    device_search.LazyPool.__call__ = counting
    try:
        host = evaluate("eval_host")
        dev_host = evaluate("eval_dev_host", gs_device=True, gs_device_ties="host")
        n_host_calls = len(started)
        dev_dev = evaluate("eval_dev_dev", gs_device=True, gs_device_ties="device")
        assert len(started) == n_host_calls                          # "device" ties never reach the host search
    finally:
        device_search.LazyPool.__call__ = real_call
    assert len(host) == len(dev_host) == len(dev_dev) == n
    n_tied = 0
    for i in range(n):
        assert np.array_equal(host[i].gs_pred_segs, dev_host[i].gs_pred_segs)
        assert np.array_equal(host[i].errors, dev_host[i].errors, equal_nan=True)
        datasets_equal(h5io.load(host[i].image_output_dir / "gs_evaluation_results.hdf5"),
                       h5io.load(dev_host[i].image_output_dir / "gs_evaluation_results.hdf5"))
        maps = host[i].boundary_maps
        assert np.array_equal(maps, dev_dev[i].boundary_maps)
        _, _, tied = device_search.delineate_dp(maps[None], 1)
        for m in range(Cc - 1):
            assert _path_cost(maps[m], dev_dev[i].gs_pred_segs[m]) == _path_cost(maps[m], host[i].gs_pred_segs[m]), (i, m)
            if not tied[0, m]:
                assert np.array_equal(dev_dev[i].gs_pred_segs[m], host[i].gs_pred_segs[m]), (i, m)
            n_tied += int(tied[0, m])
    assert sum(started) == n_tied                                    # the tied maps, and only those, went to the host
    datasets_equal(h5io.load(tmp_path / "eval_host" / "overall_evaluation_results.hdf5"),
                   h5io.load(tmp_path / "eval_dev_host" / "overall_evaluation_results.hdf5"))

    def run_predict(name, **kw):
        ds = Dataset(images, [Path(f"volume_{i}.tiff") for i in range(n)], [tmp_path / name / f"image_{i}" for i in range(n)])
        pp = PredictionParams(model_path=tmp_path / "model" / "model.npz", mlflow_tracking_uri=None, mlflow_run_uuid=None,
                              dataset=ds, config_output_dir=tmp_path / name, save_params=PredictionSaveParams(),
                              graph_search=True, batch_size=2, **kw)
        pp.gs_workers = 1
        return predict(pp)

    p_host = run_predict("pred_host")
    p_dev = run_predict("pred_dev_host", gs_device=True)
    p_dd = run_predict("pred_dev_dev", gs_device=True, gs_device_ties="device")
    for i in range(n):
        assert np.array_equal(p_host[i].gs_pred_segs, host[i].gs_pred_segs)
        assert np.array_equal(p_dev[i].gs_pred_segs, p_host[i].gs_pred_segs)
        datasets_equal(h5io.load(p_host[i].image_output_dir / "graph_search_prediction_info.hdf5"),
                       h5io.load(p_dev[i].image_output_dir / "graph_search_prediction_info.hdf5"))
        assert np.array_equal(p_dd[i].gs_pred_segs, dev_dev[i].gs_pred_segs)
