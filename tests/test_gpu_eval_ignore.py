"""GPU tests of the evaluation's ignore label: ``oct_confusion_counts_masked`` and
``oct_surface_distances_masked`` against their numpy restatements, at the smallest shapes at which the kernels can go wrong
-- odd sizes, W + 1 cell columns, H + 1 no multiple of the column pass's 8-row unroll, more than one image -- and
``evaluate_model`` on a partially labelled synthetic dataset, on both metric paths.  The surface rows are held to the
comparison of tests/test_gpu_surface_distance.py (``_assert_rows``: counts equal, 1e-10 / 1e-12 relative)."""
import numpy as np
import pytest
import torch

from oracle import unet_numpy as on
from tests.helpers import save_untrained_model, tree_equal
from tests.test_gpu_surface_distance import SPACING, _assert_rows

pytestmark = pytest.mark.gpu

SHAPES = [(3, 9, 13, 3), (2, 20, 34, 4), (1, 33, 70, 8)]
METRICS = ["dice_coef_classes", "dice_coef_macro", "dice_coef_micro", "average_surface_distance", "hausdorff_distance"]
SURFACE_NAMES = ["average_surface_distances", "average_surface_distances_gt_to_pred", "average_surface_distances_pred_to_gt",
                 "hausdorff_distances"]


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---- oct_confusion_counts_masked ----

@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("ignore_at", ["255", "C"])
def test_confusion_counts_masked_equals_restatement(shape, ignore_at):
    from oct_image_segmentation_models_amd.evaluation import dice_device as dd
    B, H, W, C_ = shape
    ignore = 255 if ignore_at == "255" else C_
    rng = np.random.default_rng(B * H * W)
    gt = rng.integers(0, C_, (B, H, W)).astype(np.uint8)
    pred = rng.integers(0, C_, (B, H, W)).astype(np.uint8)
    gt[rng.random((B, H, W)) < 0.15] = ignore
    cc = dd.ConfusionCounts(B + 1, H, W, C_, "cuda:0", ignore_label=ignore)          # a batch shorter than the constructed one
    assert cc.out.shape == (B + 1, C_ * C_ + 2)
    rows = cc(_cuda(pred), _cuda(gt)).cpu().numpy().view(np.uint32)
    ref = dd.confusion_counts_reference(pred, gt, C_, ignore)
    assert rows.shape == ref.shape == (B, C_ * C_ + 2) and np.array_equal(rows, ref)
    assert (rows[:, -1] > 0).all() and (rows[:, -2] == 0).all() and (rows.sum(axis=1) == H * W).all()
    assert np.array_equal(cc.to_host(cc(_cuda(pred), _cuda(gt))), ref[:, :C_ * C_].reshape(B, C_, C_))
    # another value that is no class, and an out-of-range prediction on a counted pixel: word C*C, reported per image
    gt2, pred2 = gt.copy(), pred.copy()
    gt2[B - 1, 0, 0], gt2[B - 1, H - 1, W - 1] = C_ + 1 if ignore == 255 else 255, 0
    pred2[B - 1, H - 1, W - 1] = 200
    rows2 = cc(_cuda(pred2), _cuda(gt2))
    assert np.array_equal(rows2.cpu().numpy().view(np.uint32), dd.confusion_counts_reference(pred2, gt2, C_, ignore))
    with pytest.raises(ValueError, match=f"image {7 + B - 1}: 2 pixels"):
        cc.to_host(rows2, first_image=7)
    # unaligned maps (the kernel's byte path): views one byte into a larger buffer
    pbuf, gbuf = torch.zeros(B * H * W + 3, dtype=torch.uint8, device="cuda"), torch.zeros(B * H * W + 2, dtype=torch.uint8, device="cuda")
    pbuf[3:].copy_(_cuda(pred).view(-1)); gbuf[2:].copy_(_cuda(gt).view(-1))
    rows3 = cc(pbuf[3:].view(B, H, W), gbuf[2:].view(B, H, W)).cpu().numpy().view(np.uint32)
    assert np.array_equal(rows3, ref)


def test_confusion_counts_masked_rejects_bad_arguments():
    import ctypes as C
    from oct_image_segmentation_models_amd import _hip
    from oct_image_segmentation_models_amd.evaluation import dice_device as dd
    lib = _hip.lib()
    B, H, W = 2, 9, 13
    p = torch.zeros((B, H, W), dtype=torch.uint8, device="cuda:0")
    out = torch.full((B, 3 * 3 + 2), 7, dtype=torch.int32, device="cuda:0")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for ignore in (2, 0, -1, 256):
        assert lib.oct_confusion_counts_masked(p.data_ptr(), p.data_ptr(), B, H, W, 3, ignore, out.data_ptr(), st) < 0
        assert b"ignore_label" in lib.oct_last_error()
    for args in ((0, H, W, 3, 255), (B, 0, W, 3, 255), (B, H, W, 1, 255), (B, H, W, 33, 255)):
        assert lib.oct_confusion_counts_masked(p.data_ptr(), p.data_ptr(), *args, out.data_ptr(), st) < 0, args
    assert lib.oct_confusion_counts_masked(p.data_ptr(), p.data_ptr(), B, H, W, 3, 255, None, st) < 0
    torch.cuda.synchronize()
    assert (out == 7).all()                                  # nothing was written
    for bad in (2, 256, 3.0):
        with pytest.raises(ValueError, match="ignore_label"):
            dd.ConfusionCounts(B, H, W, 3, "cuda:0", ignore_label=bad)


# ---- oct_surface_distances_masked ----

def _host_rows_masked(pred, gt, C_, ignore, spacing=SPACING, percent=95.0):
    """The rows of tests/test_gpu_surface_distance.py::_host_rows with ``valid = gt != ignore``."""
    from oct_image_segmentation_models_amd.common import custom_metrics as cm
    rows = np.zeros((pred.shape[0], C_ - 1, 6))
    for b in range(pred.shape[0]):
        for c in range(1, C_):
            sd = cm.compute_surface_distances(gt[b] == c, pred[b] == c, spacing, valid=gt[b] != ignore)
            a = cm.compute_average_surface_distance(sd)
            L = sd["surfel_lengths"]
            rows[b, c - 1] = (a[0], a[1],
                              cm._robust_percentile(sd["distances_gt_to_pred"], sd["surfel_kinds_gt"], L, percent),
                              cm._robust_percentile(sd["distances_pred_to_gt"], sd["surfel_kinds_pred"], L, percent),
                              sd["distances_gt_to_pred"].size, sd["distances_pred_to_gt"].size)
    return rows


def _surface_maps(B, H, W, C_):
    _, lab = on.synth_scans(B, H, W, C_, seed=H + W)
    gt = np.ascontiguousarray(lab[..., 0])
    rng = np.random.default_rng(H * W)
    pred = np.roll(gt, 1, axis=1)
    flip = rng.random(gt.shape) < 0.08
    pred[flip] = rng.integers(0, C_, int(flip.sum()))
    return pred.astype(np.uint8), gt


def _device_masked(pred, gt, C_, ignore, batch=None):
    from oct_image_segmentation_models_amd.evaluation.surface import SurfaceDistances
    B, H, W = pred.shape
    sd = SurfaceDistances(batch or B, H, W, C_, "cuda:0", ignore_label=ignore)
    return sd(_cuda(pred), _cuda(gt)).cpu().numpy()


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("ignore_at", ["255", "C"])
def test_surface_distances_masked_equals_restatement(shape, ignore_at):
    from oct_image_segmentation_models_amd.evaluation.surface import SurfaceDistances
    B, H, W, C_ = shape
    ignore = 255 if ignore_at == "255" else C_
    pred, clean = _surface_maps(B, H, W, C_)
    # no ignored pixel: the restatement, and oct_surface_distances on the same maps bit for bit
    dev = _device_masked(pred, clean, C_, ignore, batch=B + 1)
    _assert_rows(dev, _host_rows_masked(pred, clean, C_, ignore))
    plain = SurfaceDistances(B, H, W, C_, "cuda:0")(_cuda(pred), _cuda(clean)).cpu().numpy()
    assert dev.tobytes() == plain.tobytes()
    assert (dev[..., 4:] > 0).any()
    regions = {"rectangle": (slice(H // 4, H - H // 4), slice(W // 3, W // 3 + max(2, W // 5))),     # crosses the class surfaces
               "left_strip": (slice(None), slice(0, 2)),
               "last_row": (slice(H - 1, H), slice(None)),
               "everything": (slice(None), slice(None))}
    for name, (rs, cs) in regions.items():
        gt = clean.copy()
        gt[:, rs, cs] = ignore
        dev = _device_masked(pred, gt, C_, ignore)
        host = _host_rows_masked(pred, gt, C_, ignore)
        _assert_rows(dev, host)
        if name == "everything":                             # no surfels: NaN / inf / count 0
            assert np.isnan(dev[..., :2]).all() and (dev[..., 2:4] == np.inf).all() and (dev[..., 4:] == 0).all()
        else:
            assert dev[..., 4:].sum() < plain[..., 4:].sum() and dev[..., 4:].sum() > 0, name


def test_surface_distances_masked_label_errors():
    from oct_image_segmentation_models_amd._hip import OctError
    from oct_image_segmentation_models_amd.evaluation.surface import SurfaceDistances
    B, H, W, C_ = 2, 20, 34, 4
    pred, gt = _surface_maps(B, H, W, C_)
    gt[:, 3:9, 5:11] = 255
    sd = SurfaceDistances(B, H, W, C_, "cuda:0", ignore_label=255)
    sd(_cuda(pred), _cuda(gt))
    bad_gt = gt.copy(); bad_gt[1, H - 1, W - 1] = 200        # a value that is neither a class nor the ignore label
    with pytest.raises(OctError, match="n_cls=4 and not the ignore label 255"):
        sd(_cuda(pred), _cuda(bad_gt))
    bad_pred = pred.copy(); bad_pred[0, 0, 0] = C_
    with pytest.raises(OctError, match="n_cls=4"):
        sd(_cuda(bad_pred), _cuda(gt))
    bad_pred = pred.copy(); bad_pred[1, 4, 6] = 255          # the ignore value is no prediction, on an ignored pixel either
    with pytest.raises(OctError, match="n_cls=4"):
        sd(_cuda(bad_pred), _cuda(gt))
    with pytest.raises(OctError, match="n_cls=4"):           # the unmasked entry point refuses the ignore label, as before
        SurfaceDistances(B, H, W, C_, "cuda:0")(_cuda(pred), _cuda(gt))
    for bad in (3, 256):
        with pytest.raises(ValueError, match="ignore_label"):
            SurfaceDistances(B, H, W, C_, "cuda:0", ignore_label=bad)
    out = sd(_cuda(pred), _cuda(gt)).cpu().numpy()           # and the wrapper still works after the refusals
    _assert_rows(out, _host_rows_masked(pred, gt, C_, 255))


# ---- evaluate_model ----

def _evaluate(root, data, name, **kw):
    from oct_image_segmentation_models_amd.evaluation import eval_model
    from oct_image_segmentation_models_amd.evaluation.evaluation_parameters import EvaluationParameters, EvaluationSaveParams
    ep = EvaluationParameters(model_path=root / "model" / "model.npz", mlflow_tracking_uri=None, mlflow_run_uuid=None,
                              test_dataset_path=data, save_foldername=root / name, save_params=EvaluationSaveParams(),
                              graph_search=True, metrics=METRICS, batch_size=3, gs_workers=1, png_plots=True, **kw)
    return eval_model(ep)


def _close_to(got, exp, rel):
    got, exp = np.asarray(got, np.float64), np.asarray(exp, np.float64)
    assert got.shape == exp.shape
    assert np.array_equal(np.isnan(got), np.isnan(exp)) and np.array_equal(np.isinf(got), np.isinf(exp))
    fin = np.isfinite(exp)
    np.testing.assert_allclose(got[fin], exp[fin], rtol=rel, atol=0)


def test_evaluate_model_with_ignore_label(tmp_path):
    from oct_image_segmentation_models_amd.common import custom_metrics as cm, h5io, plotting, png
    from oct_image_segmentation_models_amd.evaluation import dice_device as dd
    from oct_image_segmentation_models_amd.min_path_processing.graph_search import calc_errors
    from oct_image_segmentation_models_amd.min_path_processing.utils import generate_boundary_masked
    H, W, C_, n, IGN = 32, 64, 3, 4, 255
    save_untrained_model(tmp_path, H, W, C_, 4, 2)
    images, clean = on.synth_scans(n, H, W, C_, seed=3)
    labels = clean.copy()
    for i in range(n):                                       # one ignored rectangle per scan, across the class surfaces
        labels[i, 4 + 2 * i:22 + 2 * i, 8 + 9 * i:20 + 9 * i] = IGN
    labels[2, :, 3:6] = IGN                                  # a few fully ignored columns in one scan
    replaced = np.where(labels == IGN, 0, labels).astype(labels.dtype)
    h5io.save(tmp_path / "partial.hdf5", {"test_images": images, "test_labels": labels})
    h5io.save(tmp_path / "replaced.hdf5", {"test_images": images, "test_labels": replaced})

    with pytest.raises((ValueError, IndexError)):            # without the switch the value is no label
        _evaluate(tmp_path, tmp_path / "partial.hdf5", "refused")
    outs = _evaluate(tmp_path, tmp_path / "partial.hdf5", "host", ignore_label=IGN)
    _evaluate(tmp_path, tmp_path / "partial.hdf5", "device", ignore_label=IGN, metrics_device=True)
    _evaluate(tmp_path, tmp_path / "replaced.hdf5", "replaced_off")
    _evaluate(tmp_path, tmp_path / "replaced.hdf5", "replaced_on", ignore_label=IGN)

    # both metric paths write the same files; an ignore-free dataset gives the files of a run without the switch, apart from
    # the attribute of eval_params.hdf5 (tree_equal: datasets, CSV, text and PNG files equal; the second tree may carry attributes)
    names = ("evaluation_results.hdf5", "gs_evaluation_results.hdf5", "overall_evaluation_results.hdf5", "eval_params.hdf5")
    tree_equal(tmp_path / "host", tmp_path / "device", names)
    tree_equal(tmp_path / "replaced_off", tmp_path / "replaced_on", names)
    assert int(h5io.load(tmp_path / "host" / "eval_params.hdf5")["attr:ignore_label"]) == IGN
    assert int(h5io.load(tmp_path / "replaced_on" / "eval_params.hdf5")["attr:ignore_label"]) == IGN
    assert "attr:ignore_label" not in h5io.load(tmp_path / "replaced_off" / "eval_params.hdf5")

    assert len(outs) == n
    some_nan = some_kept = False
    for i, o in enumerate(outs):
        f = h5io.load(o.image_output_dir / "evaluation_results.hdf5")
        g = h5io.load(o.image_output_dir / "gs_evaluation_results.hdf5")
        pred, gt = f["predicted_segmentation_map"], f["eval_labels"]
        assert np.array_equal(gt, labels[i, :, :, 0]) and (gt == IGN).any()           # the ground truth as given
        csv = np.loadtxt(o.image_output_dir / "ground_truth_segmentation_map.csv", delimiter=",")
        assert np.array_equal(csv, gt)
        # rule 4: truth boundaries, and the errors that follow them
        segs = generate_boundary_masked(gt, C_, IGN, axis=0)
        assert f["raw_segs"].dtype == np.uint16 and np.array_equal(f["raw_segs"], segs)
        errors = np.stack([calc_errors(g["gs_pred_segs"][k], segs[k]) for k in range(C_ - 1)])
        assert np.array_equal(g["errors"], errors, equal_nan=True)
        assert np.array_equal(np.isnan(g["errors"]), f["raw_segs"] == 0)
        some_nan |= bool((f["raw_segs"] == 0).any()); some_kept |= bool((f["raw_segs"] > 0).any())
        with np.errstate(all="ignore"):
            _close_to(g["mean_abs_err"], np.nanmean(np.abs(errors), axis=1), 1e-15)
        # rule 2: Dice of the counted pixels, arg-max maps and graph-search maps
        for file, p in ((f, pred), (g, g["gs_predicted_labels"])):
            counts = dd.counts_matrix(dd.confusion_counts_reference(p[None], gt[None], C_, IGN), C_, ignored=True)[0]
            assert counts.sum() == int((gt != IGN).sum())
            dc, dm, dmi = dd.dice_from_counts(counts, METRICS)
            assert np.array_equal(file["dice_coef_classes"], np.squeeze(dc).astype(np.float64))
            assert np.array_equal(file["dice_coef_macro"], np.expand_dims(dm, 0).astype(np.float64))
            assert np.array_equal(file["dice_coef_micro"], np.expand_dims(dmi, 0).astype(np.float64))
        # rule 3: surface distances inside the labelled region
        exp = {k: [] for k in SURFACE_NAMES}
        for c in range(1, C_):
            sd = cm.compute_surface_distances(gt == c, pred == c, SPACING, valid=gt != IGN)
            a, b = cm.compute_average_surface_distance(sd)
            exp[SURFACE_NAMES[0]].append((a + b) / 2.0); exp[SURFACE_NAMES[1]].append(a); exp[SURFACE_NAMES[2]].append(b)
            exp[SURFACE_NAMES[3]].append(cm.compute_robust_hausdorff(sd, 95))
        for k in SURFACE_NAMES:
            assert f[k].dtype == np.float64
            _close_to(f[k], exp[k], 1e-10 if k != "hausdorff_distances" else 1e-12)
        # rule 6: mid-grey exactly on the ignored pixels, the picture of the replaced labels elsewhere
        pic = png.read_rgba(o.image_output_dir / "ground_truth_segmentation_map.png")
        ref = png.read_rgba(tmp_path / "replaced_off" / f"image_{i}" / "ground_truth_segmentation_map.png")
        ign = gt == IGN
        assert (pic[ign] == (128, 128, 128, 255)).all() and np.array_equal(pic[~ign], ref[~ign])
        assert not (ref == (128, 128, 128, 255)).all(axis=-1).any()
        # the scan under the truth overlay is grey there too: the picture is the renderer's restatement of that base under
        # the truth lines, which skip the columns whose boundary is 0
        overlay = png.read_rgba(o.image_output_dir / "truth_plot.png")
        base = images[i:i + 1].copy()
        base[0][ign] = 128
        expect = plotting.render_reference(base, lines=f["raw_segs"][None], colours=plotting.TRUTH_COLOURS[:C_ - 1])
        assert np.array_equal(overlay, expect[0]) and (overlay[ign] == (128, 128, 128, 255)).all(axis=-1).any()
        assert np.array_equal(png.read_rgba(o.image_output_dir / "raw_image.png")[..., 0], images[i, :, :, 0])
    assert some_nan and some_kept
    assert (h5io.load(outs[2].image_output_dir / "evaluation_results.hdf5")["raw_segs"][:, 3:6] == 0).all()
