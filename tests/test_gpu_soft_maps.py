"""GPU tests of the soft boundary maps (``binarize=False``): ``oct_boundary_maps_soft`` against its numpy restatement --
exact equality everywhere -- on odd shapes, misaligned buffers, a strided grid and in a stream capture; the ``soft_maps``
switch of both batch sources; ``evaluate_model`` / ``predict`` with ``binarize=False`` against a host composition
(probabilities -> perform_argmax(bin=False) -> convert_predictions_to_maps_semantic -> the host search), file by file."""
from pathlib import Path

import numpy as np
import pytest
import torch

from oracle import unet_numpy as on
from tests.helpers import save_untrained_model, tree_equal
from tests.soft_maps_cases import BG, FAMILIES, class_map, family

pytestmark = pytest.mark.gpu

# H = 2: both rows are edge rows and wrap; H = 3: one interior row; W = 5, 34: the byte path; 20x34: image and map bases
# off the 16-byte grid
SHAPES = [(1, 2, 5, 2), (1, 3, 4, 4), (1, 16, 16, 2), (3, 20, 34, 5), (2, 36, 68, 8), (5, 48, 80, 3)]
FILL = 0xAB


def _lib():
    from oct_image_segmentation_models_amd import _hip
    return _hip.lib()


def _ref(p, bg_ilm, bg_csi):
    from oct_image_segmentation_models_amd.common.utils import soft_boundary_maps_reference
    return soft_boundary_maps_reference(p, bg_ilm, bg_csi)


def _call(probs_dev, shape, bg_ilm, bg_csi, maps_dev):
    B, H, W, C_ = shape
    return _lib().oct_boundary_maps_soft(probs_dev.data_ptr() if probs_dev is not None else None, B, H, W, C_, int(bg_ilm),
                                         int(bg_csi), maps_dev.data_ptr() if maps_dev is not None else None,
                                         torch.cuda.current_stream().cuda_stream)


def _soft(p, bg_ilm, bg_csi):
    B, H, W, C_ = p.shape
    out = torch.full((B, C_ - 1, H, W), FILL, dtype=torch.uint8, device="cuda")
    assert _call(torch.from_numpy(p).cuda(), p.shape, bg_ilm, bg_csi, out) == 0, _lib().oct_last_error()
    return out.cpu().numpy()


@pytest.mark.parametrize("fam", FAMILIES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_equals_restatement(shape, fam):
    p = family(fam, shape)
    for bg_ilm, bg_csi in BG:
        assert np.array_equal(_soft(p, bg_ilm, bg_csi), _ref(p, bg_ilm, bg_csi)), (bg_ilm, bg_csi)


@pytest.mark.parametrize("p_off,m_off", [(1, 1), (0, 1), (1, 0)])
@pytest.mark.parametrize("shape", [(3, 20, 34, 5), (2, 12, 16, 3)], ids=lambda s: "x".join(map(str, s)))
def test_buffers_off_the_16_byte_grid(shape, p_off, m_off):
    """probs 4 bytes past a 16-byte boundary and / or maps 1 byte past one (no dword store is possible in any row); at
    12x16x3 an aligned base would take the float4 rows."""
    B, H, W, C_ = shape
    p = family("saturated", shape)
    pbuf = torch.zeros(p.size + 8, dtype=torch.float32, device="cuda")
    mbuf = torch.full((B * (C_ - 1) * H * W + 32,), FILL, dtype=torch.uint8, device="cuda")
    assert pbuf.data_ptr() % 16 == 0 and mbuf.data_ptr() % 16 == 0
    pv = pbuf[p_off:p_off + p.size].view(shape)
    pv.copy_(torch.from_numpy(p))
    mv = mbuf[m_off:m_off + B * (C_ - 1) * H * W].view(B, C_ - 1, H, W)
    assert pv.data_ptr() % 16 == 4 * p_off and mv.data_ptr() % 16 == m_off
    for bg_ilm, bg_csi in BG[:2]:
        assert _call(pv, shape, bg_ilm, bg_csi, mv) == 0
        assert np.array_equal(mv.cpu().numpy(), _ref(p, bg_ilm, bg_csi))
        assert (mbuf[:m_off] == FILL).all() and (mbuf[m_off + mv.numel():] == FILL).all()


def test_sub_batch_write_leaves_the_rows_behind_it():
    shape = B, H, W, C_ = 3, 20, 36, 4
    p = family("layered", shape)
    out = torch.full((B + 2, C_ - 1, H, W), FILL, dtype=torch.uint8, device="cuda")
    assert _call(torch.from_numpy(p).cuda(), shape, True, False, out) == 0
    assert np.array_equal(out[:B].cpu().numpy(), _ref(p, True, False)) and (out[B:] == FILL).all()


def test_grid_stride_at_72_images_of_256x512():
    """72 x 64 x 128 work items (4 rows x 4 columns each) exceed the launch's capped grid (2048 blocks x 256 threads)."""
    base = family("saturated", (8, 256, 512, 3))
    p = np.concatenate([np.roll(base, 7 * k, axis=2) for k in range(9)])
    assert p.shape[0] * (256 // 4) * (512 // 4) > 2048 * 256
    got = _soft(p, True, False)
    want = _ref(p, True, False)
    assert np.array_equal(got, want)
    assert not np.array_equal(want[0], want[71])


@pytest.mark.parametrize("shape", [(3, 20, 34, 5), (2, 36, 68, 8), (5, 48, 80, 3)], ids=lambda s: "x".join(map(str, s)))
def test_on_one_hot_floats_equals_the_binary_kernel(shape):
    B, H, W, C_ = shape
    lab = class_map(shape)
    p = family("onehot", shape)
    for bg_ilm, bg_csi in BG:
        binary = torch.empty((B, C_ - 1, H, W), dtype=torch.uint8, device="cuda")
        assert _lib().oct_boundary_maps(torch.from_numpy(lab).cuda().data_ptr(), B, H, W, C_, int(bg_ilm), int(bg_csi),
                                        binary.data_ptr(), torch.cuda.current_stream().cuda_stream) == 0
        assert np.array_equal(_soft(p, bg_ilm, bg_csi), binary.cpu().numpy())


def test_argument_errors_launch_nothing():
    shape = B, H, W, C_ = 2, 8, 12, 3
    p = torch.from_numpy(family("saturated", shape)).cuda()
    out = torch.full((B, C_ - 1, H, W), FILL, dtype=torch.uint8, device="cuda")
    big = torch.from_numpy(family("saturated", (B, H, W, 33))).cuda()
    bad = [(None, shape, out), (p, shape, None), (p, (0, H, W, C_), out), (p, (B, 0, W, C_), out), (p, (B, H, 0, C_), out),
           (p, (-1, H, W, C_), out), (p, (B, H, W, 1), out), (big, (B, H, W, 33), out)]
    for probs, shp, maps in bad:
        assert _call(probs, shp, True, False, maps) < 0 and b"boundary_maps_soft" in _lib().oct_last_error(), shp
    # an output inside the input, and an input inside the output
    before = p.clone()
    as_bytes = p.view(-1).view(torch.uint8)
    assert _call(p, shape, True, False, as_bytes[16:]) < 0 and b"overlap" in _lib().oct_last_error()
    assert _call(p, shape, True, False, as_bytes[as_bytes.numel() - 1:]) < 0
    wide = torch.full((p.numel() * 4 + 1024,), FILL, dtype=torch.uint8, device="cuda")
    inner = wide[128:128 + p.numel() * 4].view(torch.float32)               # the maps would cover bytes 0..383 of `wide`
    assert _call(inner, shape, True, False, wide[:]) < 0
    torch.cuda.synchronize()
    assert (out == FILL).all() and torch.equal(p, before) and (wide == FILL).all()


def test_call_records_into_a_graph():
    shape = B, H, W, C_ = 3, 20, 34, 5
    first, second = family("saturated", shape), family("layered", shape)
    p = torch.from_numpy(first).cuda()
    out = torch.full((B, C_ - 1, H, W), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        assert _call(p, shape, True, False, out) == 0
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), _ref(first, True, False))
    p.copy_(torch.from_numpy(second))
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), _ref(second, True, False))


def test_engine_method_checks_its_tensor():
    from oct_image_segmentation_models_amd._hip import OctError
    eng = _engine(2)
    p = family("layered", (2, H_, W_, CC))
    got = eng.boundary_maps_soft(torch.from_numpy(p).cuda(), bg_ilm=False, bg_csi=True)
    assert np.array_equal(got.cpu().numpy(), _ref(p, False, True))
    for bad in (torch.from_numpy(p), torch.from_numpy(p).cuda().double(), torch.from_numpy(p).cuda()[:, :, ::2],
                torch.from_numpy(p).cuda()[..., :CC - 1].contiguous(), torch.from_numpy(p).cuda()[0]):
        with pytest.raises(OctError):
            eng.boundary_maps_soft(bad)


# ---- pipeline and workflows: an untrained start_neurons=4, pool_layers=2 net at 36x68, 4 classes; 5 images at batch 2 ----
H_, W_, CC, SN, P_, N_IMG, BATCH = 36, 68, 4, 4, 2, 5, 2
METRICS = ["dice_coef_classes", "dice_coef_macro", "dice_coef_micro"]


def _scans():
    return on.synth_scans(N_IMG, H_, W_, CC, seed=31)


def _engine(max_batch):
    from oct_image_segmentation_models_amd.engine import UNetEngine
    return UNetEngine(device="cuda:0", input_channels=1, num_classes=CC, image_height=H_, image_width=W_, start_neurons=SN,
                      pool_layers=P_, max_batch=max_batch, training=False, seed=2, init_seed=4)


def test_batched_predictor_soft_maps_with_a_ragged_last_batch():
    from oct_image_segmentation_models_amd.evaluation.pipeline import BatchedPredictor
    images, _ = _scans()
    eng = _engine(BATCH)
    hard = list(BatchedPredictor(eng, BATCH, want_maps=True).run(images))
    pred = BatchedPredictor(eng, BATCH, want_maps=True, soft_maps=True)
    for _ in range(2):                                                          # the second run reuses every buffer pair
        soft = list(pred.run(images))
        assert [(b.lo, b.hi) for b in soft] == [(0, 2), (2, 4), (4, 5)]
        stale = None
        for b, h in zip(soft, hard):
            # the graph always runs BATCH images: behind a ragged batch sits what its staging buffer held two batches ago
            x = images[b.lo:b.hi] if b.hi - b.lo == BATCH else np.concatenate([images[b.lo:b.hi], stale[b.hi - b.lo:]])
            probs, _ = eng.forward(torch.from_numpy(np.ascontiguousarray(x)).cuda(), training=False, want_probs=True)
            want = _ref(probs.cpu().numpy(), True, False)[:b.hi - b.lo]
            assert b.maps.dtype == np.uint8 and np.array_equal(b.maps, want), b.lo
            assert np.array_equal(b.labels, h.labels)
            assert not np.array_equal(b.maps, h.maps)                           # the switch is no no-op
            if b.lo == 0:
                stale = x                                                       # batch 2 shares batch 0's staging buffer
    with pytest.raises(ValueError, match="soft_maps"):
        BatchedPredictor(eng, BATCH, want_maps=False, soft_maps=True)


def test_host_batches_soft_maps_with_float_images(tmp_path):
    from oct_image_segmentation_models_amd.evaluation.pipeline import host_batches
    from oct_image_segmentation_models_amd.models.engine_model import load_model
    images, _ = _scans()
    model = load_model(save_untrained_model(tmp_path, H_, W_, CC, SN, P_))
    fimg = images.astype(np.float32)
    soft = list(host_batches(model, fimg, BATCH, soft_maps=True))
    hard = list(host_batches(model, fimg, BATCH))
    assert [(b.lo, b.hi) for b in soft] == [(0, 2), (2, 4), (4, 5)]
    eng = model._ensure_engine(BATCH, False)
    for b, h in zip(soft, hard):
        x = torch.from_numpy(np.ascontiguousarray(fimg[b.lo:b.hi] / np.float32(255.0))).to(eng.device)
        probs, _ = eng.forward(x, training=False, want_probs=True)
        assert np.array_equal(b.maps, _ref(probs.cpu().numpy(), True, False)), b.lo
        assert np.array_equal(b.labels, h.labels) and not np.array_equal(b.maps, h.maps)
    with pytest.raises(ValueError, match="soft_maps"):
        model.predict_labels(images, batch_size=BATCH, want_maps=False, soft_maps=True)


@pytest.mark.parametrize("mode", ["host", "device_host_ties", "metrics_device"])
def test_workflows_with_binarize_false_equal_a_host_composition(tmp_path, mode):
    """The expected files come from the workflows' own binary path, host search and host metrics, with the boundary-map
    kernel replaced by the host composition: the probabilities of a forward over the very batch the pipeline holds
    (same partition, same batch size) -> perform_argmax(bin=False) -> convert_predictions_to_maps_semantic.  From there
    on the binary path IS the host composition: graph_search.segment_maps -> labels_from_delineations -> Dice, files."""
    from oct_image_segmentation_models_amd.common import h5io, utils as cu
    from oct_image_segmentation_models_amd.common.dataset import Dataset
    from oct_image_segmentation_models_amd.engine import UNetEngine
    from oct_image_segmentation_models_amd.evaluation import eval_model
    from oct_image_segmentation_models_amd.evaluation.evaluation_parameters import EvaluationParameters, EvaluationSaveParams
    from oct_image_segmentation_models_amd.min_path_processing import graph_search
    from oct_image_segmentation_models_amd.prediction import predict
    from oct_image_segmentation_models_amd.prediction.prediction_parameters import PredictionParams, PredictionSaveParams
    images, labels = _scans()
    data = tmp_path / "test.hdf5"
    h5io.save(data, {"test_images": images, "test_labels": labels})
    save_untrained_model(tmp_path, H_, W_, CC, SN, P_)
    switches = {"host": ({}, {}), "device_host_ties": (dict(gs_device=True, gs_device_ties="host"),) * 2,
                "metrics_device": (dict(metrics_device=True), dict(gs_labels_device=True))}[mode]

    def evaluate(name, **kw):
        ep = EvaluationParameters(model_path=tmp_path / "model" / "model.npz", mlflow_tracking_uri=None, mlflow_run_uuid=None,
                                  test_dataset_path=data, save_foldername=tmp_path / name,
                                  save_params=EvaluationSaveParams(categorical_pred=True), graph_search=True, metrics=METRICS,
                                  batch_size=BATCH, **kw)
        ep.gs_workers = 1
        return eval_model(ep)

    def run_predict(name, **kw):
        ds = Dataset(images, [Path(f"volume_{i}.tiff") for i in range(N_IMG)],
                     [tmp_path / name / f"image_{i}" for i in range(N_IMG)])
        pp = PredictionParams(model_path=tmp_path / "model" / "model.npz", mlflow_tracking_uri=None, mlflow_run_uuid=None,
                              dataset=ds, config_output_dir=tmp_path / name,
                              save_params=PredictionSaveParams(categorical_pred=True), graph_search=True, batch_size=BATCH, **kw)
        pp.gs_workers = 1
        return predict(pp)

    real_maps = UNetEngine.boundary_maps
    composed = []

    def host_composition(self, am, bg_ilm=True, bg_csi=False):
        x, _, graph_am = self._graph_keep                                       # the batch the captured forward just ran on
        assert am.data_ptr() == graph_am.data_ptr()
        probs, _ = self.forward(x, training=False, want_probs=True)
        _, cat = cu.perform_argmax(probs.cpu().numpy(), bin=False)
        maps = cu.convert_predictions_to_maps_semantic(cat.copy(), bg_ilm, bg_csi)
        composed.append(maps)
        return torch.from_numpy(maps).to(am.device)

    UNetEngine.boundary_maps = host_composition
    try:
        want = evaluate("eval_want")
        n_eval = len(composed)
        p_want = run_predict("pred_want")
    finally:
        UNetEngine.boundary_maps = real_maps
    assert n_eval == 3 and len(composed) == 6
    want_maps = np.concatenate([m[:n] for m, n in zip(composed[:3], (2, 2, 1))])    # (a ragged batch composes BATCH images)
    assert np.array_equal(want_maps, np.concatenate([m[:n] for m, n in zip(composed[3:], (2, 2, 1))]))

    got = evaluate("eval_got", binarize=False, **switches[0])
    p_got = run_predict("pred_got", binarize=False, **switches[1])
    tree_equal(tmp_path / "eval_want", tmp_path / "eval_got",
               ["evaluation_results.hdf5", "gs_evaluation_results.hdf5", "overall_evaluation_results.hdf5"])
    tree_equal(tmp_path / "pred_want", tmp_path / "pred_got", ["prediction_info.hdf5", "graph_search_prediction_info.hdf5"])
    assert not h5io.load(tmp_path / "eval_got" / "eval_params.hdf5")["attr:binarize"]
    assert not h5io.load(tmp_path / "pred_got" / "prediction_params.hdf5")["attr:binarize"]
    assert "attr:binarize" not in h5io.load(tmp_path / "eval_want" / "eval_params.hdf5")
    graph = graph_search.create_graph_structure((W_, H_), 1)
    for i, (w, g, pw, pg) in enumerate(zip(want, got, p_want, p_got)):
        for field in ("predicted_labels", "categorical_pred", "boundary_maps", "gs_pred_segs", "errors", "mean_abs_err",
                      "mean_err", "abs_err_sd", "err_sd", "dice_classes", "dice_macro", "dice_micro"):
            u, v = np.asarray(getattr(w, field)), np.asarray(getattr(g, field))
            assert u.dtype == v.dtype and u.shape == v.shape and np.array_equal(u, v, equal_nan=u.dtype.kind == "f"), field
        for field in ("predicted_labels", "categorical_pred", "boundary_maps", "gs_pred_segs"):
            assert np.array_equal(getattr(pw, field), getattr(pg, field)), field
        # and the composition spelled out for the fields the search produces
        assert np.array_equal(g.boundary_maps, want_maps[i]) and np.array_equal(pg.boundary_maps, want_maps[i])
        seg, err, _ = graph_search.segment_maps(np.transpose(want_maps[i], (0, 2, 1)), g.image_segments, graph)
        assert np.array_equal(g.gs_pred_segs, seg) and np.array_equal(g.errors, err, equal_nan=True)
        assert np.array_equal(pg.gs_pred_segs, seg)
        gs_lab, _ = cu.labels_from_delineations((W_, H_, 1), seg, CC)
        f = h5io.load(g.image_output_dir / "gs_evaluation_results.hdf5")
        assert np.array_equal(f["gs_predicted_labels"], gs_lab)
        assert np.array_equal(g.categorical_pred, cu.labels_to_categorical(g.predicted_labels[None], CC)[0])   # stays one-hot

    if mode == "host":
        # binarize=True, spelled out, is still the binary path -- and the two settings differ on this model
        hard = evaluate("eval_hard", binarize=True)
        p_hard = run_predict("pred_hard", binarize=True)
        plain = evaluate("eval_plain")
        tree_equal(tmp_path / "eval_plain", tmp_path / "eval_hard",
                   ["evaluation_results.hdf5", "gs_evaluation_results.hdf5", "overall_evaluation_results.hdf5"])
        assert "attr:binarize" not in h5io.load(tmp_path / "eval_hard" / "eval_params.hdf5")
        assert "attr:binarize" not in h5io.load(tmp_path / "pred_hard" / "prediction_params.hdf5")
        for hd, ph, g in zip(hard, p_hard, got):
            binary = cu.convert_predictions_to_maps_semantic(cu.labels_to_categorical(hd.predicted_labels[None], CC))[0]
            assert np.array_equal(hd.boundary_maps, binary) and np.array_equal(ph.boundary_maps, binary)
            assert np.array_equal(hd.predicted_labels, g.predicted_labels)
        assert any(not np.array_equal(hd.boundary_maps, g.boundary_maps) for hd, g in zip(hard, got))
