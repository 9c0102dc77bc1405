"""GPU tests of the device Dice stage: oct_confusion_counts and oct_area_labels (evaluation/dice_device.py) against their
numpy restatements -- exact equality everywhere -- the ``Batch.confusion`` field of both batch sources, and
evaluate_model / predict with the ``metrics_device`` / ``gs_labels_device`` switches against the host path, file by file."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest
import torch

from oracle import unet_numpy as on
from tests.dice_cases import SEG_FAMILIES, host_area_labels, map_pairs, seg_family
from tests.helpers import save_untrained_model, tree_equal

pytestmark = pytest.mark.gpu

COUNT_SHAPES = [(1, 16, 16, 2), (3, 20, 34, 5), (2, 36, 68, 8), (5, 48, 80, 3)]       # 20x34: image bases off the 16-byte grid
AREA_SHAPES = [(16, 16, 2), (20, 34, 5), (36, 68, 8), (48, 80, 3)]
METRICS = ["dice_coef_classes", "dice_coef_macro", "dice_coef_micro"]


def _dd():
    from oct_image_segmentation_models_amd.evaluation import dice_device
    return dice_device


def _counts(pred, gt, C_, cc=None, out=None):
    """Device rows (n, C*C + 1) as uint32 on the host."""
    B, H, W = pred.shape
    cc = cc or _dd().ConfusionCounts(B, H, W, C_, "cuda:0")
    rows = cc(torch.from_numpy(np.ascontiguousarray(pred)).cuda(), torch.from_numpy(np.ascontiguousarray(gt)).cuda(), out=out)
    return rows.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("B,H,W,C_", COUNT_SHAPES)
def test_confusion_counts_equal_restatement(B, H, W, C_):
    ref = _dd().confusion_counts_reference
    for name, (pred, gt) in map_pairs(B, H, W, C_, seed=B + C_).items():
        got = _counts(pred, gt, C_)
        assert got.shape == (B, C_ * C_ + 1)
        assert np.array_equal(got, ref(pred, gt, C_)), name
        assert not got[:, -1].any() and (got.sum(axis=1) == H * W).all()
        if name == "constant":
            assert (got[:, 1 * C_ + C_ - 1] == H * W).all()                    # one counter holds the whole image


@pytest.mark.parametrize("B,H,W,C_", COUNT_SHAPES)
def test_confusion_counts_out_of_range_word_small_n_and_second_call(B, H, W, C_):
    dd = _dd()
    pred, gt = (a.copy() for a in map_pairs(B, H, W, C_, seed=7)["shifted"])
    pred[0, 0, 0] = C_                                                          # first pixel of image 0
    gt[B - 1, H - 1, W - 1] = 255                                               # last pixel of the last image
    want = dd.confusion_counts_reference(pred, gt, C_)
    assert want[0, -1] >= 1 and want[B - 1, -1] >= 1 and want[:, -1].sum() == 2
    # a buffer for more images than the call is given: the rows behind n stay as they were
    cc = dd.ConfusionCounts(B + 2, H, W, C_, "cuda:0")
    cc.out.fill_(-7)
    got = _counts(pred, gt, C_, cc)
    assert np.array_equal(got, want)
    assert (cc.out[B:] == -7).all()
    with pytest.raises(ValueError, match=f"image {10 + 0}"):
        cc.to_host(cc.out[:B], first_image=10)
    # a second call into the same rows overwrites them (zeroing is part of the call)
    pred2, gt2 = map_pairs(B, H, W, C_, seed=8)["random"]
    assert np.array_equal(_counts(pred2, gt2, C_, cc), dd.confusion_counts_reference(pred2, gt2, C_))
    assert np.array_equal(_counts(pred2, gt2, C_, cc), dd.confusion_counts_reference(pred2, gt2, C_))
    clean = cc.to_host(cc.out[:B])
    assert clean.shape == (B, C_, C_) and clean.dtype == np.uint32


def test_confusion_counts_maps_at_different_offsets_from_16_bytes():
    """pred starts one byte past a 16-byte boundary, gt on one: the byte path of the kernel."""
    dd = _dd()
    B, H, W, C_ = 3, 20, 34, 5
    pred, gt = map_pairs(B, H, W, C_, seed=3)["shifted"]
    buf = torch.zeros(B * H * W + 16, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    p = buf[1:1 + B * H * W].view(B, H, W)
    p.copy_(torch.from_numpy(pred))
    cc = dd.ConfusionCounts(B, H, W, C_, "cuda:0")
    got = cc(p, torch.from_numpy(gt).cuda()).cpu().numpy().view(np.uint32)
    assert np.array_equal(got, dd.confusion_counts_reference(pred, gt, C_))


def test_confusion_counts_single_counter_512x1024():
    H, W = 512, 1024
    pred, gt = np.full((1, H, W), 2, np.uint8), np.full((1, H, W), 1, np.uint8)
    got = _counts(pred, gt, 3)
    want = np.zeros((1, 10), np.uint32)
    want[0, 1 * 3 + 2] = 524288
    assert np.array_equal(got, want)


def test_confusion_counts_32_classes_and_refusals():
    dd = _dd()
    from oct_image_segmentation_models_amd import _hip
    B, H, W = 2, 36, 68
    rng = np.random.default_rng(1)
    pred, gt = rng.integers(0, 33, (B, H, W)).astype(np.uint8), rng.integers(0, 32, (B, H, W)).astype(np.uint8)
    got = _counts(pred, gt, 32)
    assert got.shape == (B, 1025) and np.array_equal(got, dd.confusion_counts_reference(pred, gt, 32))
    assert got[:, -1].all()                                                     # pred holds label 32
    with pytest.raises(_hip.OctError):
        dd.ConfusionCounts(B, H, W, 33, "cuda:0")
    # the C ABI itself: argument errors return a negative code, name the reason and launch nothing
    lib = _hip.lib()
    p, g = torch.from_numpy(pred).cuda(), torch.from_numpy(gt).cuda()
    out = torch.full((B, 33 * 33 + 1), -7, dtype=torch.int32, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for args in ((p.data_ptr(), g.data_ptr(), B, H, W, 33), (p.data_ptr(), g.data_ptr(), B, H, W, 1),
                 (p.data_ptr(), g.data_ptr(), 0, H, W, 3), (p.data_ptr(), g.data_ptr(), 65536, H, W, 3),
                 (p.data_ptr(), g.data_ptr(), B, 65536, 65536, 3), (None, g.data_ptr(), B, H, W, 3),
                 (p.data_ptr(), None, B, H, W, 3)):
        assert lib.oct_confusion_counts(*args, out.data_ptr(), st) < 0, args
        assert b"confusion_counts" in lib.oct_last_error()
    assert lib.oct_confusion_counts(p.data_ptr(), g.data_ptr(), B, H, W, 3, None, st) < 0
    s = torch.zeros((B, 2, W), dtype=torch.int16, device="cuda")
    lab = torch.full((B, H, W), 7, dtype=torch.uint8, device="cuda")
    for args in ((s.data_ptr(), B, H, W, 34), (s.data_ptr(), B, H, W, 1), (s.data_ptr(), 0, H, W, 3),
                 (s.data_ptr(), B, 65536, W, 3), (None, B, H, W, 3)):
        assert lib.oct_area_labels(*args, lab.data_ptr(), st) < 0, args
        assert b"area_labels" in lib.oct_last_error()
    assert lib.oct_area_labels(s.data_ptr(), B, H, W, 3, None, st) < 0
    torch.cuda.synchronize()
    assert (out == -7).all() and (lab == 7).all()                               # nothing was written


@pytest.mark.parametrize("H,W,C_", AREA_SHAPES)
def test_area_labels_equal_restatement(H, W, C_):
    dd = _dd()
    B = 3
    al = dd.AreaLabels(B + 1, H, W, C_, "cuda:0")
    for f, kind in enumerate(SEG_FAMILIES):
        segs = seg_family(kind, B, H, W, C_, seed=10 * C_ + f)
        al.out.fill_(99)
        got = al(torch.from_numpy(segs.view(np.int16)).cuda())
        assert got.shape == (B, H, W) and got.dtype == torch.uint8
        want = dd.area_labels_reference(segs, H, W)
        assert np.array_equal(got.cpu().numpy(), want), kind
        assert (al.out[B:] == 99).all()                                         # n smaller than the buffer's batch
        if kind in ("zeros40", "beyond"):
            assert np.array_equal(want, host_area_labels(segs, H, W)), kind     # and the host loop itself


def test_both_calls_record_into_a_graph():
    """No allocation and no host wait: the two calls record into a stream capture, and the replay serves new inputs."""
    dd = _dd()
    B, H, W, C_ = 3, 20, 34, 5
    al, cc = dd.AreaLabels(B, H, W, C_, "cuda:0"), dd.ConfusionCounts(B, H, W, C_, "cuda:0")
    first, second = seg_family("crossing", B, H, W, C_, 1), seg_family("zeros40", B, H, W, C_, 2)
    _, gt = map_pairs(B, H, W, C_, seed=5)["shifted"]
    segs_dev, gt_dev = torch.from_numpy(first.view(np.int16)).cuda(), torch.from_numpy(gt).cuda()
    cc(al(segs_dev), gt_dev)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        rows = cc(al(segs_dev), gt_dev)
    segs_dev.copy_(torch.from_numpy(second.view(np.int16)).cuda())
    graph.replay()
    torch.cuda.synchronize()
    want = dd.area_labels_reference(second, H, W)
    assert np.array_equal(al.out.cpu().numpy(), want)
    assert np.array_equal(rows.cpu().numpy().view(np.uint32), dd.confusion_counts_reference(want, gt, C_))


# ---- pipeline and workflows: an untrained start_neurons=4, pool_layers=2 net at 32x64, 4 classes; 6 images at batch 4 ----
H_, W_, CC, SN, P_, N_IMG, BATCH = 32, 64, 4, 4, 2, 6, 4


def _scans():
    images, labels = on.synth_scans(N_IMG, H_, W_, CC, seed=31)
    return images, labels


def test_batch_confusion_from_both_sources(tmp_path):
    dd = _dd()
    from oct_image_segmentation_models_amd.engine import UNetEngine
    from oct_image_segmentation_models_amd.evaluation.pipeline import BatchedPredictor, host_batches
    from oct_image_segmentation_models_amd.models.engine_model import load_model
    images, labels = _scans()
    gt = np.ascontiguousarray(labels[..., 0].astype(np.uint8))
    eng = UNetEngine(device="cuda:0", input_channels=1, num_classes=CC, image_height=H_, image_width=W_, start_neurons=SN,
                     pool_layers=P_, max_batch=BATCH, training=False, seed=2, init_seed=4)
    pred = BatchedPredictor(eng, BATCH, want_maps=True, confusion=dd.ConfusionCounts(BATCH, H_, W_, CC, "cuda:0"))
    for _ in range(2):                                                          # the second run reuses every buffer pair
        got = list(pred.run(images, gt))
        assert [(b.lo, b.hi) for b in got] == [(0, 4), (4, 6)]                  # the last batch is ragged
        for b in got:
            assert b.surface is None and b.confusion.dtype == np.uint32 and b.confusion.shape == (b.hi - b.lo, CC, CC)
            want = dd.confusion_counts_reference(b.labels, gt[b.lo:b.hi], CC)
            assert np.array_equal(b.confusion, want[:, :-1].reshape(-1, CC, CC))
    assert all(b.confusion is None for b in pred.run(images))                   # no ground truth, no counts
    bad = gt.copy()
    bad[5, 3, 3] = CC
    with pytest.raises(ValueError, match="image 5"):
        list(pred.run(images, bad))
    torch.cuda.synchronize()
    model = load_model(save_untrained_model(tmp_path, H_, W_, CC, SN, P_))
    got = list(host_batches(model, images.astype(np.float32), BATCH, gt_u8=gt,
                            confusion=dd.ConfusionCounts(BATCH, H_, W_, CC, "cuda:0")))
    assert [(b.lo, b.hi) for b in got] == [(0, 4), (4, 6)]
    for b in got:
        want = dd.confusion_counts_reference(b.labels, gt[b.lo:b.hi], CC)
        assert b.confusion.dtype == np.uint32 and np.array_equal(b.confusion, want[:, :-1].reshape(-1, CC, CC))


@pytest.mark.parametrize("mode", ["pool", "device_host_ties", "device_device_ties"])
def test_workflows_with_the_switches_equal_the_host_path(tmp_path, mode):
    from oct_image_segmentation_models_amd.common import h5io
    from oct_image_segmentation_models_amd.common.dataset import Dataset
    from oct_image_segmentation_models_amd.evaluation import dice_device, eval_model
    from oct_image_segmentation_models_amd.evaluation.evaluation_parameters import EvaluationParameters, EvaluationSaveParams
    from oct_image_segmentation_models_amd.prediction import predict
    from oct_image_segmentation_models_amd.prediction.prediction_parameters import PredictionParams, PredictionSaveParams
    images, labels = _scans()
    data = tmp_path / "test.hdf5"
    h5io.save(data, {"test_images": images, "test_labels": labels})
    save_untrained_model(tmp_path, H_, W_, CC, SN, P_)
    search = {"pool": {}, "device_host_ties": dict(gs_device=True, gs_device_ties="host"),
              "device_device_ties": dict(gs_device=True, gs_device_ties="device")}[mode]
    calls = {"area": 0, "counts": 0}
    real_area, real_counts = dice_device.AreaLabels.__call__, dice_device.ConfusionCounts.__call__

    def area(self, *a, **k):
        calls["area"] += 1
        return real_area(self, *a, **k)

    def counts(self, *a, **k):
        calls["counts"] += 1
        return real_counts(self, *a, **k)

    def evaluate(name, **kw):
        ep = EvaluationParameters(model_path=tmp_path / "model" / "model.npz", mlflow_tracking_uri=None, mlflow_run_uuid=None,
                                  test_dataset_path=data, save_foldername=tmp_path / name, save_params=EvaluationSaveParams(),
                                  graph_search=True, metrics=METRICS, batch_size=BATCH, **search, **kw)
        ep.gs_workers = 1
        return eval_model(ep)

    def run_predict(name, **kw):
        ds = Dataset(images, [Path(f"volume_{i}.tiff") for i in range(N_IMG)],
                     [tmp_path / name / f"image_{i}" for i in range(N_IMG)])
        pp = PredictionParams(model_path=tmp_path / "model" / "model.npz", mlflow_tracking_uri=None, mlflow_run_uuid=None,
                              dataset=ds, config_output_dir=tmp_path / name, save_params=PredictionSaveParams(),
                              graph_search=True, batch_size=BATCH, **search, **kw)
        pp.gs_workers = 1
        return predict(pp)

    dice_device.AreaLabels.__call__, dice_device.ConfusionCounts.__call__ = area, counts
    try:
        host = evaluate("eval_host")
        p_host = run_predict("pred_host")
        assert calls == {"area": 0, "counts": 0}                                # switches off: the kernels are not used
        dev = evaluate("eval_dev", metrics_device=True)
        assert calls == {"area": 2, "counts": 4}                                # 2 batches: arg-max maps and search maps
        p_dev = run_predict("pred_dev", gs_labels_device=True)
        assert calls == {"area": 4, "counts": 4}
    finally:
        dice_device.AreaLabels.__call__, dice_device.ConfusionCounts.__call__ = real_area, real_counts
    tree_equal(tmp_path / "eval_host", tmp_path / "eval_dev",
               ["evaluation_results.hdf5", "gs_evaluation_results.hdf5", "overall_evaluation_results.hdf5"])
    tree_equal(tmp_path / "pred_host", tmp_path / "pred_dev", ["prediction_info.hdf5", "graph_search_prediction_info.hdf5"])
    assert len(host) == len(dev) == len(p_host) == len(p_dev) == N_IMG
    for h, d in zip(host, dev):
        for field in ("predicted_labels", "categorical_pred", "boundary_maps", "gs_pred_segs", "errors", "mean_abs_err",
                      "mean_err", "abs_err_sd", "err_sd", "dice_classes", "dice_macro", "dice_micro"):
            u, v = np.asarray(getattr(h, field)), np.asarray(getattr(d, field))
            assert u.dtype == v.dtype and u.shape == v.shape and np.array_equal(u, v, equal_nan=u.dtype.kind == "f"), field
    for h, d in zip(p_host, p_dev):
        for field in ("predicted_labels", "categorical_pred", "boundary_maps", "gs_pred_segs"):
            assert np.array_equal(getattr(h, field), getattr(d, field)), field
