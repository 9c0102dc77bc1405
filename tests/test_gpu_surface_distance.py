"""GPU tests of the device surface-distance metrics (oct_surface_distances, evaluation/surface.py) against the host
restatement in common/custom_metrics.py, and of evaluate_model with all five metrics on both of its paths."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest
import torch

from oracle import unet_numpy as on
from tests.helpers import save_untrained_model

pytestmark = pytest.mark.gpu

SPACING = (0.01111111, 0.01111111)


def _host_rows(pred, gt, C_, spacing=SPACING, percent=95.0):
    from oct_image_segmentation_models_amd.common import custom_metrics as cm
    rows = np.zeros((pred.shape[0], C_ - 1, 6))
    for b in range(pred.shape[0]):
        for c in range(1, C_):
            sd = cm.compute_surface_distances(gt[b] == c, pred[b] == c, spacing)
            a = cm.compute_average_surface_distance(sd)
            L = sd["surfel_lengths"]
            rows[b, c - 1] = (a[0], a[1],
                              cm._robust_percentile(sd["distances_gt_to_pred"], sd["surfel_kinds_gt"], L, percent),
                              cm._robust_percentile(sd["distances_pred_to_gt"], sd["surfel_kinds_pred"], L, percent),
                              sd["distances_gt_to_pred"].size, sd["distances_pred_to_gt"].size)
    return rows


def _assert_rows(dev, host):
    assert dev.shape == host.shape
    np.testing.assert_array_equal(dev[..., 4:], host[..., 4:])                        # surfel counts
    for cols, rel in (((0, 1), 1e-10), ((2, 3), 1e-12)):
        d, h = dev[..., cols], host[..., cols]
        assert np.array_equal(np.isnan(d), np.isnan(h)) and np.array_equal(np.isinf(d), np.isinf(h))
        fin = np.isfinite(h)
        assert np.array_equal(d[~fin & ~np.isnan(h)], h[~fin & ~np.isnan(h)])
        np.testing.assert_allclose(d[fin], h[fin], rtol=rel, atol=0)


def _device(pred, gt, C_, spacing=SPACING, percent=95.0):
    from oct_image_segmentation_models_amd.evaluation.surface import SurfaceDistances
    B, H, W = pred.shape
    sd = SurfaceDistances(B, H, W, C_, "cuda:0", spacing=spacing, percent=percent)
    out = sd(torch.from_numpy(np.ascontiguousarray(pred)).cuda(), torch.from_numpy(np.ascontiguousarray(gt)).cuda())
    return out.cpu().numpy()


def _cases(B, H, W, C_, seed):
    _, lab = on.synth_scans(B, H, W, C_, seed=seed)
    gt = lab[..., 0]
    rng = np.random.default_rng(seed)
    noisy = gt.copy()
    flip = rng.random(gt.shape) < 0.05
    noisy[flip] = rng.integers(0, C_, int(flip.sum()))
    rand = rng.integers(0, C_, gt.shape).astype(np.uint8)
    return gt, {"clean": gt.copy(), "shifted": np.roll(gt, 2, axis=1), "noisy": noisy, "random": rand}


@pytest.mark.parametrize("kind", ["clean", "shifted", "noisy", "random"])
def test_device_matches_host_b32_256x512(kind):
    gt, preds = _cases(32, 256, 512, 3, seed=21)
    pred = preds[kind]
    dev = _device(pred, gt, 3)
    idx = np.arange(0, 32, 4) if kind in ("noisy", "random") else np.arange(32)      # host cost: a subset of the batch
    _assert_rows(dev[idx], _host_rows(pred[idx], gt[idx], 3))
    if kind == "random":
        assert dev[..., 4:].max() > 9e4                                          # ~104 k surfels per class


def test_device_empty_class_and_one_mask_empty():
    gt, preds = _cases(6, 256, 512, 3, seed=5)
    pred = preds["noisy"]
    gt[0][gt[0] == 2] = 1            # class 2 absent from gt: asd gt->pred NaN, hausdorff inf
    pred[1][pred[1] == 1] = 0        # class 1 absent from pred: asd gt->pred inf
    gt[2][:] = 0; pred[2][:] = 0     # both empty for every class
    pred[3][:] = 2                   # pred all class 2 (border only at the image edge), no class 1
    dev = _device(pred, gt, 3)
    _assert_rows(dev, _host_rows(pred, gt, 3))
    assert np.isnan(dev[0, 1, 0]) and dev[0, 1, 2] == np.inf
    assert dev[1, 0, 0] == np.inf and np.isnan(dev[1, 0, 1]) and dev[1, 0, 3] == np.inf
    assert np.isnan(dev[2, :, :2]).all() and (dev[2, :, 2:4] == np.inf).all() and (dev[2, :, 4:] == 0).all()


def test_device_eight_classes_and_anisotropic_percentiles():
    gt, preds = _cases(4, 128, 256, 8, seed=8)
    for percent in (0.0, 50.0, 100.0):
        dev = _device(preds["noisy"], gt, 8, spacing=(0.0039, 0.0111), percent=percent)
        _assert_rows(dev, _host_rows(preds["noisy"], gt, 8, spacing=(0.0039, 0.0111), percent=percent))
    dev = _device(preds["shifted"], gt, 8)
    _assert_rows(dev, _host_rows(preds["shifted"], gt, 8))


def test_device_512x1024_b8():
    gt, preds = _cases(8, 512, 1024, 3, seed=13)
    for kind in ("clean", "noisy"):
        dev = _device(preds[kind], gt, 3)
        idx = [0, 5]
        _assert_rows(dev[idx], _host_rows(preds[kind][idx], gt[idx], 3))


@pytest.mark.parametrize("shape", [(1, 37, 101, 3), (3, 1, 9, 2), (2, 11, 1, 4), (1, 64, 65, 5)])
def test_device_odd_sizes(shape):
    B, H, W, C_ = shape
    rng = np.random.default_rng(H * W)
    gt = rng.integers(0, C_, (B, H, W)).astype(np.uint8)
    gt[:, : H // 2] = 0
    pred = np.where(rng.random((B, H, W)) < 0.1, rng.integers(0, C_, (B, H, W)), gt).astype(np.uint8)
    _assert_rows(_device(pred, gt, C_), _host_rows(pred, gt, C_))


def test_repeated_calls_bit_identical():
    from oct_image_segmentation_models_amd.evaluation.surface import SurfaceDistances
    gt, preds = _cases(8, 256, 512, 3, seed=2)
    sd = SurfaceDistances(8, 256, 512, 3, "cuda:0")
    p, g = torch.from_numpy(preds["random"]).cuda(), torch.from_numpy(gt).cuda()
    a = sd(p, g).clone()
    b = sd(p, g).clone()
    sd.workspace.fill_(0x5A)                             # workspace contents between calls do not matter
    c = sd(p, g).clone()
    torch.cuda.synchronize()
    assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes() == c.cpu().numpy().tobytes()


def test_bad_arguments_rejected_without_launch():
    from oct_image_segmentation_models_amd import _hip
    lib = _hip.lib()
    B, H, W, C_ = 2, 16, 24, 3
    nbytes = lib.oct_surface_workspace_bytes(B, H, W, C_)
    assert nbytes > 0 and lib.oct_surface_workspace_bytes(0, H, W, C_) == 0 and lib.oct_surface_workspace_bytes(B, H, W, 1) == 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda:0")
    good = torch.ones((B, H, W), dtype=torch.uint8, device="cuda:0")
    sentinel = torch.full((B, C_ - 1, 6), 7.0, dtype=torch.float64, device="cuda:0")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(pred=good, gt=good, sr=0.01, sc=0.01, pc=95.0, nb=nbytes):
        return lib.oct_surface_distances(pred.data_ptr(), gt.data_ptr(), B, H, W, C_, sr, sc, pc, ws.data_ptr(), nb,
                                         sentinel.data_ptr(), stream)

    for kw in (dict(pc=-1.0), dict(pc=100.5), dict(pc=float("nan")), dict(sr=0.0), dict(sc=-0.01),
               dict(sr=float("inf")), dict(nb=nbytes - 1)):
        assert call(**kw) != 0, kw
        assert lib.oct_last_error()
    bad = good.clone(); bad[1, 3, 5] = C_
    assert call(gt=bad) != 0 and b"n_cls" in lib.oct_last_error()
    assert call(pred=bad) != 0
    torch.cuda.synchronize()
    assert (sentinel == 7.0).all()                       # nothing was written
    assert call() == 0
    torch.cuda.synchronize()
    r = sentinel.cpu().numpy()
    assert (r[:, 0, 4:] > 0).all() and (r[:, 0, :4] == 0).all()             # class 1: identical maps, distance 0
    assert (r[:, 1, 4:] == 0).all() and np.isnan(r[:, 1, :2]).all() and (r[:, 1, 2:4] == np.inf).all()  # class 2: absent


def _evaluate(root, data, name, metrics):
    from oct_image_segmentation_models_amd.evaluation import eval_model
    from oct_image_segmentation_models_amd.evaluation.evaluation_parameters import EvaluationParameters, EvaluationSaveParams
    ep = EvaluationParameters(model_path=root / "model" / "model.npz", mlflow_tracking_uri=None, mlflow_run_uuid=None,
                              test_dataset_path=data, save_foldername=root / name,
                              save_params=EvaluationSaveParams(), graph_search=False, metrics=metrics, batch_size=3)
    return eval_model(ep)


def test_evaluate_model_all_five_metrics(tmp_path):
    from oct_image_segmentation_models_amd.common import custom_metrics as cm, h5io
    H, W, C_, n = 64, 128, 3, 5
    save_untrained_model(tmp_path, H, W, C_, 8, 2)
    te_i, te_l = on.synth_scans(n, H, W, C_, seed=3)
    te_l[1][te_l[1] == 2] = 1                                  # a class absent from one ground truth
    h5io.save(tmp_path / "u8.hdf5", {"test_images": te_i, "test_labels": te_l})
    h5io.save(tmp_path / "f32.hdf5", {"test_images": te_i.astype(np.float32), "test_labels": te_l})
    metrics = ["dice_coef_classes", "dice_coef_macro", "dice_coef_micro", "average_surface_distance", "hausdorff_distance"]
    names = ["average_surface_distances", "average_surface_distances_gt_to_pred", "average_surface_distances_pred_to_gt",
             "hausdorff_distances"]
    per_path = {}
    for tag in ("u8", "f32"):
        outs = _evaluate(tmp_path, tmp_path / f"{tag}.hdf5", f"eval_{tag}", metrics)
        assert len(outs) == n
        got = []
        for i, o in enumerate(outs):
            f = h5io.load(o.image_output_dir / "evaluation_results.hdf5")
            pred, gt = f["predicted_segmentation_map"], f["eval_labels"]
            exp = {k: [] for k in names}
            for c in range(1, C_):
                a, b = cm.average_surface_distance(gt == c, pred == c, SPACING)
                exp[names[0]].append((a + b) / 2.0); exp[names[1]].append(a); exp[names[2]].append(b)
                exp[names[3]].append(cm.hausdorff_distance(gt == c, pred == c, SPACING, 95))
            for k in names:
                assert f[k].dtype == np.float64 and f[k].shape == (C_ - 1,)
                e = np.array(exp[k])
                assert np.array_equal(np.isnan(f[k]), np.isnan(e)) and np.array_equal(np.isinf(f[k]), np.isinf(e))
                fin = np.isfinite(e)
                np.testing.assert_allclose(f[k][fin], e[fin], rtol=1e-10 if k != "hausdorff_distances" else 1e-12)
                np.testing.assert_array_equal(getattr(o, k), f[k])
            got.append([f[k] for k in names])
        assert np.isnan(got[1][1][1]) and got[1][3][1] == np.inf        # the absent class: NaN mean, inf Hausdorff
        overall = h5io.load(tmp_path / f"eval_{tag}" / "overall_evaluation_results.hdf5")
        csv = (tmp_path / f"eval_{tag}" / "overall_evaluation_results.csv").read_text()
        for j, k in enumerate(names):
            stack = np.array([g[j] for g in got])
            np.testing.assert_array_equal(overall[k], stack)
            st = stack.copy(); st[st == np.inf] = np.nan
            with np.errstate(all="ignore"):
                np.testing.assert_allclose(overall[f"mean_{k}"], np.nanmean(st, axis=0), rtol=1e-12)
                np.testing.assert_allclose(overall[f"sd_{k}"], np.nanstd(st, axis=0), rtol=1e-12)
            assert f"Mean {k}," in csv and f"SD {k}," in csv
        lines = [l.split(",")[0] for l in csv.splitlines()]
        assert lines.index("Mean dice_coef_micro") < lines.index("Mean average_surface_distances") \
            < lines.index("Mean hausdorff_distances")
        per_path[tag] = np.array(got)
    np.testing.assert_array_equal(per_path["u8"], per_path["f32"])       # batched uint8 path == float host_batches path
