"""GPU tests of the connected components: ``oct_components`` and ``oct_component_filter`` bit for bit
against ``common.utils.components_reference`` / ``component_filter_reference``, their argument errors, a stream capture, and
the switch through ``InferenceRun``, ``Model``, ``evaluate_model`` and ``predict``.  Everything the kernels compute is an
integer, so every comparison is for equality.  The tile is 64x64: 131x133 and 133x131 span two whole tiles and a remainder in
each direction."""
import ctypes
from pathlib import Path

import numpy as np
import pytest
import torch

from oracle import unet_numpy as on
from tests.components_cases import BATCHES, CONNECTIVITIES, N_CLS, PATTERNS, SHAPES, filter_cases, pattern, wanted
from tests.helpers import datasets_equal, save_untrained_model, tree_equal

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
ids = lambda c: "x".join(map(str, c))      # noqa: E731


def _hip():
    from oct_image_segmentation_models_amd import _hip
    return _hip


def _up(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()


def _poison(shape, dtype):
    """A tensor with every byte at 0xFF: an unwritten word shows."""
    return torch.full(shape, -1 if dtype != torch.uint8 else 255, dtype=dtype, device="cuda")


def _ws(B, H, W):
    n = int(_hip().lib().oct_components_workspace_bytes(B, H, W))
    assert n >= B * H * W * 4 and n % 8 == 0
    return _poison((n,), torch.uint8)


def _ptr(t):
    return None if t is None else (t if isinstance(t, int) else t.data_ptr())


def _components(labels, shape, n_cls, conn, ws, nb, root, size, stats):
    """The C call itself, with tensors, addresses or None: returns its code."""
    h = _hip()
    with torch.cuda.device(0):
        return h.lib().oct_components(_ptr(labels), *shape, n_cls, conn, _ptr(ws), nb, _ptr(root), _ptr(size), _ptr(stats),
                                      h.stream_ptr(torch.device("cuda:0")))


def _packed(r):
    p = _hip().ComponentRuleC()
    for c, v in enumerate(r.min_pixels):
        p.min_pixels[c] = v
    p.keep_largest, p.fill_mode, p.fill_label = r.keep_largest, r.fill_mode, r.fill_label
    return p


def _filter(labels, root, size, shape, n_cls, r, ws, nb, out, removed):
    h = _hip()
    with torch.cuda.device(0):
        return h.lib().oct_component_filter(_ptr(labels), _ptr(root), _ptr(size), *shape, n_cls,
                                            None if r is None else ctypes.byref(_packed(r)), _ptr(ws), nb, _ptr(out), _ptr(removed),
                                            h.stream_ptr(torch.device("cuda:0")))


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _same(got, want, note=None):
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), note


# ---- 1. the kernels against the restatements -----------------------------------------------------------------------------------
@pytest.mark.parametrize("connectivity", CONNECTIVITIES)
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_components_equal_the_restatement(shape, B, connectivity):
    H, W = shape
    ws = _ws(B, H, W)
    for name in PATTERNS:
        labels = _up(pattern(name, B, H, W))
        want = wanted(name, B, H, W, connectivity)
        outs = _poison((B, H, W), torch.int32), _poison((B, H, W), torch.int32), _poison((B, N_CLS, 2), torch.int32)
        assert _components(labels, (B, H, W), N_CLS, connectivity, ws, ws.numel(), *outs) == 0
        torch.cuda.synchronize()
        got = tuple(_u32(t) for t in outs)
        _same(got, want, (name, "first"))
        assert _components(labels, (B, H, W), N_CLS, connectivity, ws, ws.numel(), *outs) == 0      # a second call: the same bytes
        torch.cuda.synchronize()
        _same(tuple(_u32(t) for t in outs), got, (name, "again"))
        # without the size and statistics outputs: the same roots, nothing else written
        root = _poison((B, H, W), torch.int32)
        assert _components(labels, (B, H, W), N_CLS, connectivity, ws, ws.numel(), root, None, None) == 0
        torch.cuda.synchronize()
        _same((_u32(root),), want[:1], (name, "root alone"))


def test_more_tile_rows_than_a_grid_dimension_holds():
    """One column of 64 * 65536 + 1 pixels: 65537 tile rows, past what grid.y or grid.z can hold; the fault could show only at
    this size.  Runs of three pixels (the last one shorter), so the answer has a closed form: no restatement over 4 M pixels."""
    H = 64 * 65536 + 1
    y = np.arange(H)
    labels = ((y // 3) % 2).astype(np.uint8).reshape(1, H, 1)
    want_root = (y - y % 3).astype(np.uint32).reshape(1, H, 1)
    want_size = np.where(y % 3 == 0, np.minimum(3, H - y), 0).astype(np.uint32).reshape(1, H, 1)
    runs = (H + 2) // 3
    want_stats = np.array([[[(runs + 1) // 2, 3], [runs // 2, 3]]], np.uint32)
    ws = _ws(1, H, 1)
    for conn in CONNECTIVITIES:
        outs = _poison((1, H, 1), torch.int32), _poison((1, H, 1), torch.int32), _poison((1, 2, 2), torch.int32)
        assert _components(_up(labels), (1, H, 1), 2, conn, ws, ws.numel(), *outs) == 0
        torch.cuda.synchronize()
        _same(tuple(_u32(t) for t in outs), (want_root, want_size, want_stats), conn)


@pytest.mark.parametrize("name", sorted(filter_cases()))
def test_filter_equals_the_restatement(name):
    c = filter_cases()[name]
    shape = B, H, W = c.labels.shape
    ws, labels = _ws(*shape), _up(c.labels)
    root, size, stats = _poison(shape, torch.int32), _poison(shape, torch.int32), _poison((B, c.n_cls, 2), torch.int32)
    assert _components(labels, shape, c.n_cls, c.connectivity, ws, ws.numel(), root, size, stats) == 0
    outs = _poison(shape, torch.uint8), _poison((B, c.n_cls), torch.int32)
    assert _filter(labels, root, size, shape, c.n_cls, c.rule, ws, ws.numel(), *outs) == 0
    torch.cuda.synchronize()
    _same((_u32(root), _u32(size), _u32(stats)), (c.root, c.size, c.stats), name)
    got = outs[0].cpu().numpy(), _u32(outs[1])
    _same(got, (c.clean, c.removed), name)
    assert _filter(labels, root, size, shape, c.n_cls, c.rule, ws, ws.numel(), *outs) == 0
    torch.cuda.synchronize()
    _same((outs[0].cpu().numpy(), _u32(outs[1])), got, (name, "again"))
    clean = _poison(shape, torch.uint8)                              # without the removed counts
    assert _filter(labels, root, size, shape, c.n_cls, c.rule, ws, ws.numel(), clean, None) == 0
    torch.cuda.synchronize()
    assert clean.cpu().numpy().tobytes() == c.clean.tobytes()
    assert torch.equal(labels, _up(c.labels))                        # out of place


def test_calls_record_into_a_graph_and_replay():
    cases = filter_cases()
    first, second = cases["crafted_column"], cases["keep_largest_tie_column"]
    assert first.labels.shape == second.labels.shape and first.n_cls == second.n_cls
    shape = B, H, W = first.labels.shape
    r = first.rule
    from oct_image_segmentation_models_amd.common.utils import component_filter_reference, components_reference
    labels, ws = _up(first.labels), _ws(*shape)
    root, size, stats = _poison(shape, torch.int32), _poison(shape, torch.int32), _poison((B, 3, 2), torch.int32)
    clean, removed = _poison(shape, torch.uint8), _poison((B, 3), torch.int32)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        assert _components(labels, shape, 3, 8, ws, ws.numel(), root, size, stats) == 0
        assert _filter(labels, root, size, shape, 3, r, ws, ws.numel(), clean, removed) == 0
    for case in (first, second, first):
        labels.copy_(_up(case.labels))
        graph.replay()
        torch.cuda.synchronize()
        want = components_reference(case.labels, 3, 8)
        _same((_u32(root), _u32(size), _u32(stats)), want)
        _same((clean.cpu().numpy(), _u32(removed)), component_filter_reference(case.labels, want[0], want[1], 3, r))


def test_argument_errors_return_negative_and_write_nothing():
    from tests.components_cases import rule
    h = _hip()
    c = filter_cases()["both_random_column"]
    shape = B, H, W = c.labels.shape
    C = c.n_cls
    labels, ws = _up(c.labels), _ws(*shape)
    nb = ws.numel()
    root, size, stats = _poison(shape, torch.int32), _poison(shape, torch.int32), _poison((B, C, 2), torch.int32)
    clean, removed = _poison(shape, torch.uint8), _poison((B, C), torch.int32)
    good_root, good_size = _up(c.root.view(np.int32)), _up(c.size.view(np.int32))
    tensors = (labels, ws, root, size, stats, clean, removed, good_root, good_size)
    before = [t.clone() for t in tensors]
    refused_shapes = [(0, H, W), (65536, 1, 1), (B, 0, W), (B, H, -1), (8, 4096, 65536), (-1, H, W)]
    bad = [dict(labels=None), dict(root=None), dict(ws=None)] + [dict(shape=s) for s in refused_shapes] + [
        dict(n_cls=0), dict(n_cls=33), dict(conn=6), dict(conn=0), dict(nb=nb - 1), dict(nb=0), dict(ws=ws.data_ptr() + 4),
        dict(root=root.data_ptr() + 2), dict(size=size.data_ptr() + 1), dict(stats=stats.data_ptr() + 2),
        dict(root=labels), dict(size=ws), dict(stats=root), dict(size=root), dict(root=ws[256:]), dict(stats=labels),
    ]
    for kw in bad:
        a = dict(labels=labels, shape=shape, n_cls=C, conn=8, ws=ws, nb=nb, root=root, size=size, stats=stats)
        a.update(kw)
        rc = _components(a["labels"], a["shape"], a["n_cls"], a["conn"], a["ws"], a["nb"], a["root"], a["size"], a["stats"])
        assert rc < 0 and h.lib().oct_last_error(), kw
    for s in refused_shapes:
        assert int(h.lib().oct_components_workspace_bytes(*s)) == 0, s
    for s in (shape, (1, 1, 1), (65535, 1, 1), (1, 32768, 65535)):
        assert int(h.lib().oct_components_workspace_bytes(*s)) >= 4 * s[0] * s[1] * s[2], s
    ok = rule(C, 2, fill_mode=1)
    bad = [dict(labels=None), dict(root=None), dict(size=None), dict(r=None), dict(ws=None), dict(out=None)] + [
        dict(shape=s) for s in refused_shapes] + [
        dict(n_cls=0), dict(n_cls=33), dict(nb=nb - 1), dict(ws=ws.data_ptr() + 4), dict(root=good_root.data_ptr() + 2),
        dict(size=good_size.data_ptr() + 2), dict(removed=removed.data_ptr() + 1),
        dict(r=rule(C, fill_mode=2)), dict(r=rule(C, fill_mode=-1)), dict(r=rule(C, fill_label=256)), dict(r=rule(C, fill_label=-1)),
        dict(r=rule(C + 1, keep_largest=(C,))), dict(r=rule(32, keep_largest=(31,))),
        dict(out=labels), dict(out=good_root), dict(out=good_size), dict(out=ws), dict(removed=clean), dict(removed=labels),
        dict(removed=ws[64:]), dict(ws=good_root),
    ]
    for kw in bad:
        a = dict(labels=labels, root=good_root, size=good_size, shape=shape, n_cls=C, r=ok, ws=ws, nb=nb, out=clean, removed=removed)
        a.update(kw)
        rc = _filter(a["labels"], a["root"], a["size"], a["shape"], a["n_cls"], a["r"], a["ws"], a["nb"], a["out"], a["removed"])
        assert rc < 0 and h.lib().oct_last_error(), kw
    torch.cuda.synchronize()
    for t, b in zip(tensors, before):
        assert torch.equal(t, b)
    assert _components(labels, shape, C, c.connectivity, ws, nb, root, size, stats) == 0       # and the good calls still work
    assert _filter(labels, root, size, shape, C, c.rule, ws, nb, clean, removed) == 0
    torch.cuda.synchronize()
    _same((_u32(root), _u32(size), _u32(stats), clean.cpu().numpy(), _u32(removed)), (c.root, c.size, c.stats, c.clean, c.removed))


def test_wrapper_sub_batch_on_a_used_object():
    from oct_image_segmentation_models_amd._hip import OctError
    from oct_image_segmentation_models_amd.evaluation.components import ComponentRule, Components, components_host
    labels = pattern("layered_noise", 3, 131, 133)
    r = ComponentRule(connectivity=8, min_pixels=6, keep_largest=[0, 3], fill="column")
    cc = Components(3, 131, 133, 4, r, "cuda:0")
    assert cc.geometry == (3, 131, 133, 4) and [tuple(t.shape) for t in cc.outs] == [(3, 131, 133), (3, 4, 2), (3, 4)]
    _same(cc.to_host(*cc(_up(labels))), components_host(labels, 4, r), "full")
    for t in cc.outs:
        t.view(torch.uint8).fill_(0xFF)
    for n in (2, 1):
        got = cc.to_host(*cc(_up(labels[3 - n:])))
        assert got[0].shape[0] == n
        _same(got, components_host(labels[3 - n:], 4, r), n)
    assert all((t[2:].view(torch.uint8) == 0xFF).all() for t in cc.outs)             # nothing behind the n images is written
    for wrong in (_up(labels)[:, :, :100], _up(labels).to(torch.int32), _up(np.zeros((4, 131, 133), np.uint8)), _up(labels)[:, ::2]):
        with pytest.raises(OctError):
            cc(wrong)
    with pytest.raises(ValueError):
        Components(3, 131, 133, 4, ComponentRule(min_pixels=[1, 2]), "cuda:0")


# ---- 2. the pipeline ------------------------------------------------------------------------------------------------------------
N_IMG, CC, SN, BATCH = 5, 3, 8, 3
RULE = dict(connectivity=8, min_pixels=[6, 6, 6], keep_largest="all", fill="column")


def _rule(**kw):
    from oct_image_segmentation_models_amd.evaluation.components import ComponentRule
    return ComponentRule(**{**RULE, **kw})


def _host(labels, rule):
    from oct_image_segmentation_models_amd.evaluation.components import components_host
    return components_host(labels, CC, rule)


def _model(tmp_path, H, W, pool_layers):
    from oct_image_segmentation_models_amd.models.engine_model import load_model
    return load_model(save_untrained_model(tmp_path, H, W, CC, SN, pool_layers))


def _run(model, imgs, **kw):
    from oct_image_segmentation_models_amd.evaluation.pipeline import InferenceRun
    with InferenceRun(model, imgs, BATCH, CC, **kw) as run:
        return list(run)


def _cleaned(batches):
    assert [(b.lo, b.hi) for b in batches] == [(0, 3), (3, 5)] and all(len(b) == 7 for b in batches)
    return tuple(np.concatenate([b.components[i] for b in batches]) for i in range(3))


def test_model_predict_components(tmp_path):
    imgs, _ = on.synth_scans(N_IMG, 16, 32, CC, seed=21)
    model = _model(tmp_path, 16, 32, 2)
    argmax = model.predict_labels(imgs, batch_size=BATCH)
    for rule in (_rule(), _rule(connectivity=4, fill=2, keep_largest=[1])):
        got = model.predict_components(imgs, rule, batch_size=BATCH)
        _same(got, _host(argmax, rule), rule)
        _same(model.predict_components(imgs, rule.as_dict()), got, "dict, one batch")
    assert got[2].sum() > 0 and (got[0] != argmax).any()                   # the rule removed something
    for bad in (None, dict(min_pixels=[1, 2]), dict(keep_largest=[3])):
        with pytest.raises(ValueError):
            model.predict_components(imgs, bad)


def test_model_predict_components_on_a_padded_size(tmp_path):
    """34x66 scans on the 36x68 engine (pool depth 2, whose arg-max maps have islands to remove): the labelling sees the
    CROPPED arg-max maps."""
    from oct_image_segmentation_models_amd.common.utils import padded_geometry
    assert padded_geometry(34, 66, 2)[:2] == (36, 68)
    imgs, _ = on.synth_scans(N_IMG, 34, 66, CC, seed=21)
    model = _model(tmp_path, 36, 68, 2)
    model.pad_mode = "edge"                                   # predict_components takes the model's attributes
    argmax = model.predict_labels(imgs, batch_size=BATCH, pad_mode="edge")
    assert argmax.shape == (N_IMG, 34, 66)
    got = model.predict_components(imgs, _rule(), batch_size=BATCH)
    _same(got, _host(argmax, _rule()), "padded")
    assert got[2].sum() > 0 and (got[0] != argmax).any()                   # the rule removed something


@pytest.mark.parametrize("kind", ["plain", "tta", "mc", "temperature"])
@pytest.mark.parametrize("size", [(16, 16), (36, 68)], ids=ids)
def test_inference_run_fills_batch_components(tmp_path, size, kind):
    """``Batch.components`` is the restatement of the batch's own arg-max maps -- the MEAN prediction's under tta / mc, the
    cropped ones at 36x68 (a 40x72 forward), the same under a temperature -- and switching it on changes nothing else."""
    H, W = size
    padded = size == (36, 68)
    imgs, gt = on.synth_scans(N_IMG, H, W, CC, seed=21)
    model = _model(tmp_path, 40 if padded else H, 72 if padded else W, 3 if padded else 2)
    pad = dict(pad_mode="edge") if padded else {}
    rule = _rule()
    more = {"plain": {}, "tta": dict(tta=("identity", "flip_lr")), "mc": dict(mc_samples=2, mc_step0=3),
            "temperature": dict(temperature=2.0)}[kind]
    batches, off = _run(model, imgs, components=rule, **pad, **more), _run(model, imgs, **pad, **more)
    labels = np.concatenate([b.labels for b in batches])
    _same(_cleaned(batches), _host(labels, rule), kind)
    assert all(b.components is None for b in off)
    assert all(np.array_equal(a.labels, b.labels) and np.array_equal(a.maps, b.maps) for a, b in zip(batches, off))
    if kind == "tta":
        assert np.array_equal(labels, model.predict_tta(imgs, more["tta"], batch_size=BATCH, **pad)[1]) if not padded else True
    if kind == "temperature":
        _same(_cleaned(batches), _cleaned(_run(model, imgs, components=rule, **pad)), "the arg-max does not depend on it")
    if kind == "plain" and not padded:
        x = imgs.astype(np.float32)                           # another dtype: host_batches, x / 255 on the host
        _same(_cleaned(_run(model, x, components=rule.as_dict())), _host(labels, rule), "host_batches")
        # beside every other stage: their outputs and this one's are what they are alone
        kw = dict(gt=gt[..., 0], confusion=True, ordered_decode=True, calibration_bins=10, soft_maps=True, graph_search=True,
                  gs_device=True, gs_device_ties="device", gs_workers=1)
        both, alone = _run(model, imgs, components=rule, **kw), _run(model, imgs, **kw)
        _same(_cleaned(both), _host(labels, rule), "with the others")
        for a, b in zip(both, alone):
            assert a.surface.tobytes() == b.surface.tobytes() and a.confusion.tobytes() == b.confusion.tobytes()
            assert all(x.tobytes() == y.tobytes() for x, y in zip(a.ordered + a.calibration + a.minpath, b.ordered + b.calibration + b.minpath))
            assert a.maps.tobytes() == b.maps.tobytes() and a.labels.tobytes() == b.labels.tobytes()


def test_switch_off_launches_no_new_kernel(tmp_path):
    """With the switch at its default the engine's launch profiler sees no kernel of this feature; with it on it sees the two
    calls.  (The profiler records eager launches only: the pipeline runs its Monte-Carlo chain, which is eager.)"""
    from oct_image_segmentation_models_amd.evaluation.pipeline import InferenceRun
    imgs, labels = on.synth_scans(3, 16, 32, CC, seed=2)
    model = _model(tmp_path, 16, 32, 2)

    def pipeline(**kw):
        with InferenceRun(model, imgs, BATCH, CC, gt=labels[..., 0], confusion=True, surface=False, mc_samples=2, **kw) as run:
            e = model._ensure_engine(BATCH, False)
            e.profile_begin()
            list(run)
            return {r["kernel"] for r in e.profile_end()}
    off, on_ = pipeline(), pipeline(components=_rule())
    assert off and not {k for k in off if "cc_" in k}
    assert on_ - off == {"cc_tile_k + cc_border_k + cc_flatten_k", "cc_best_k + cc_filter_k + cc_column_fill_k"}


# ---- 3. evaluate_model and predict end to end -----------------------------------------------------------------------------------
SPACING = (0.01111111, 0.01111111)
SURFACE_NAMES = ("average_surface_distances", "average_surface_distances_gt_to_pred", "average_surface_distances_pred_to_gt",
                 "hausdorff_distances")


def _surface_expected(pred, gt, C, ignore=None):
    """The host formula of the four surface data sets of one image (tests/test_gpu_surface_distance.py, and with ``ignore``
    tests/test_gpu_eval_ignore.py): per class 1..C-1, surface elements inside ``gt != ignore``."""
    from oct_image_segmentation_models_amd.common import custom_metrics as cm
    exp = {k: [] for k in SURFACE_NAMES}
    for c in range(1, C):
        if ignore is None:
            a, b = cm.average_surface_distance(gt == c, pred == c, SPACING)
            h = cm.hausdorff_distance(gt == c, pred == c, SPACING, 95)
        else:
            sd = cm.compute_surface_distances(gt == c, pred == c, SPACING, valid=gt != ignore)
            (a, b), h = cm.compute_average_surface_distance(sd), cm.compute_robust_hausdorff(sd, 95)
        for k, v in zip(SURFACE_NAMES, ((a + b) / 2.0, a, b, h)):
            exp[k].append(v)
    return {k: np.array(v, np.float64) for k, v in exp.items()}


def _close_to(got, exp, rel, note=None):
    got, exp = np.asarray(got, np.float64), np.asarray(exp, np.float64)
    assert got.shape == exp.shape, note
    assert np.array_equal(np.isnan(got), np.isnan(exp)) and np.array_equal(np.isinf(got), np.isinf(exp)), note
    fin = np.isfinite(exp)
    np.testing.assert_allclose(got[fin], exp[fin], rtol=rel, atol=0)


def _surface_files_equal_the_formula(files, clean, argmax, gt, C, overall, ignore=None):
    """The four surface data sets of every cc file against the host formula on the CLEANED map (tolerances of
    tests/test_gpu_surface_distance.py), the cc_ aggregates against the files, and a check that the data can tell the cleaned map
    from the arg-max map."""
    tells = False
    for i, f in enumerate(files):
        exp, of_argmax = _surface_expected(clean[i], gt[i], C, ignore), _surface_expected(argmax[i], gt[i], C, ignore)
        for k in SURFACE_NAMES:
            assert f[k].dtype == np.float64 and f[k].shape == (C - 1,)
            _close_to(f[k], exp[k], 1e-10 if k != "hausdorff_distances" else 1e-12, (i, k))
            tells |= not np.array_equal(exp[k], of_argmax[k], equal_nan=True)
    assert tells                                                  # the arg-max map in the cleaned map's place would show
    for k in SURFACE_NAMES:
        stack = np.array([f[k] for f in files])
        np.testing.assert_array_equal(overall[f"cc_{k}"], stack)
        stack[stack == np.inf] = np.nan
        with np.errstate(all="ignore"):
            np.testing.assert_allclose(overall[f"mean_cc_{k}"], np.nanmean(stack, axis=0), rtol=1e-12)
            np.testing.assert_allclose(overall[f"sd_cc_{k}"], np.nanstd(stack, axis=0), rtol=1e-12)


def test_evaluate_model_and_predict_end_to_end(tmp_path):
    from oct_image_segmentation_models_amd.common import dataset_loader as dl, h5io
    from oct_image_segmentation_models_amd.common.dataset import Dataset
    from oct_image_segmentation_models_amd.evaluation import eval_model
    from oct_image_segmentation_models_amd.evaluation.dice_device import confusion_counts_reference, dice_from_counts
    from oct_image_segmentation_models_amd.evaluation.evaluation_parameters import EvaluationParameters, EvaluationSaveParams
    from oct_image_segmentation_models_amd.evaluation.render import CC_PNG_NAMES
    from oct_image_segmentation_models_amd.models.engine_model import load_model
    from oct_image_segmentation_models_amd.prediction import predict
    from oct_image_segmentation_models_amd.prediction.prediction_parameters import PredictionParams, PredictionSaveParams
    data = ROOT / "tests" / "golden" / "dataset_small.hdf5"
    images, labels, _ = dl.load_testing_data(dl.open_dataset(data))
    n, H, W = images.shape[:3]
    C = int(labels.max()) + 1
    save_untrained_model(tmp_path, H, W, C, SN, 2)
    metrics = ["dice_coef_classes", "dice_coef_macro", "dice_coef_micro", "average_surface_distance", "hausdorff_distance"]
    from oct_image_segmentation_models_amd.evaluation.components import ComponentRule, components_host
    rule = ComponentRule(connectivity=8, min_pixels=8, keep_largest="all", fill="column")

    def evaluate(name, **kw):
        ep = EvaluationParameters(model_path=tmp_path / "model" / "model.npz", mlflow_tracking_uri=None, mlflow_run_uuid=None,
                                  test_dataset_path=data, save_foldername=tmp_path / name, save_params=EvaluationSaveParams(),
                                  graph_search=False, metrics=metrics, batch_size=2, **kw)
        eval_model(ep)
        return tmp_path / name

    plain, off = evaluate("plain"), evaluate("off", components=None)
    on_, on_dev = evaluate("on", components=rule), evaluate("on_dev", components=rule.as_dict(), metrics_device=True)
    tree_equal(plain, off, ["evaluation_results.hdf5", "overall_evaluation_results.hdf5", "eval_params.hdf5"])
    # every file that existed before: the same datasets, CSV files byte for byte; the overall files keep what they had
    for rel in sorted(p.relative_to(off) for p in off.rglob("*") if p.is_file()):
        assert (on_ / rel).is_file(), rel
        if rel.name.startswith("overall_evaluation_results") or rel.name.startswith("eval_params"):
            continue
        if ".hdf5" in rel.suffixes:
            datasets_equal(h5io.load(off / rel), h5io.load(on_ / rel), rel)
        else:
            assert (off / rel).read_bytes() == (on_ / rel).read_bytes(), rel
    added = {p.name.replace(".npz", "") for p in on_.rglob("*") if p.is_file() and not (off / p.relative_to(on_)).exists()}
    assert added == {"cc_evaluation_results.hdf5"}
    o, o_off = h5io.load(on_ / "overall_evaluation_results.hdf5"), h5io.load(off / "overall_evaluation_results.hdf5")
    assert all(np.array_equal(o[k], o_off[k], equal_nan=np.asarray(o[k]).dtype.kind == "f") for k in o_off)
    new = {k for k in o if k not in o_off}
    assert new and all("cc_" in k and k.split("_", 1)[0] in ("cc", "mean", "sd") for k in new)
    off_csv, on_csv = ((d / "overall_evaluation_results.csv").read_text() for d in (off, on_))
    assert on_csv.startswith(off_csv) and "Mean cc_removed_pixels" in on_csv[len(off_csv):]

    argmax = load_model(tmp_path / "model" / "model.npz").predict_labels(images, batch_size=2)
    clean, stats, removed = components_host(argmax, C, rule)
    assert removed.sum() > 0
    gt = labels[..., 0]
    files = []
    for i in range(n):
        f, base = h5io.load(on_ / f"image_{i}" / "cc_evaluation_results.hdf5"), h5io.load(on_ / f"image_{i}" / "evaluation_results.hdf5")
        datasets_equal(f, h5io.load(on_dev / f"image_{i}" / "cc_evaluation_results.hdf5"), i)     # device Dice == host Dice
        assert np.array_equal(base["predicted_segmentation_map"], argmax[i])
        assert f["cc_predicted_labels"].dtype == np.uint8 and np.array_equal(f["cc_predicted_labels"], clean[i])
        for key, want in (("component_count", stats[i, :, 0]), ("largest_component_pixels", stats[i, :, 1]), ("removed_pixels", removed[i])):
            assert f[key].shape == (C,) and np.array_equal(f[key], want), key
        assert int(f["changed_pixels"][0]) == int((clean[i] != argmax[i]).sum())
        dc, dm, dmi = dice_from_counts(confusion_counts_reference(clean[i][None], gt[i:i + 1], C)[0, :C * C].reshape(C, C), metrics)
        assert np.array_equal(f["dice_coef_classes"], np.squeeze(dc).astype(np.float64))
        assert f["dice_coef_macro"][0] == np.float64(dm) and f["dice_coef_micro"][0] == np.float64(dmi)
        files.append(f)
    assert (clean != argmax).any()                                # the cleaned maps are not the arg-max maps
    _surface_files_equal_the_formula(files, clean, argmax, gt, C, o)
    assert all(f"Mean cc_{k}," in on_csv and f"SD cc_{k}," in on_csv for k in SURFACE_NAMES)
    assert np.allclose(o["mean_cc_removed_pixels"], np.mean([f["removed_pixels"] for f in files], axis=0), rtol=1e-12, atol=0)
    assert np.array_equal(o["cc_component_count"], stats[:, :, 0])

    # with png_plots: the picture of the cleaned map, and every other picture byte for byte
    pngs = lambda d: {p.relative_to(d) for p in d.rglob("*.png")}      # noqa: E731
    on_png, off_png = evaluate("on_png", components=rule, png_plots=True), evaluate("off_png", png_plots=True)
    assert pngs(off_png) and {p.name for p in pngs(on_png) - pngs(off_png)} == set(CC_PNG_NAMES.values())
    assert len(pngs(on_png) - pngs(off_png)) == n and all((on_png / p).stat().st_size > 0 for p in pngs(on_png))
    assert all((off_png / p).read_bytes() == (on_png / p).read_bytes() for p in pngs(off_png))

    def run_predict(name, **kw):
        ds = Dataset(images, [Path(f"volume_{i}.tiff") for i in range(n)], [tmp_path / name / f"image_{i}" for i in range(n)])
        pp = PredictionParams(model_path=tmp_path / "model" / "model.npz", mlflow_tracking_uri=None, mlflow_run_uuid=None,
                              dataset=ds, config_output_dir=tmp_path / name, save_params=PredictionSaveParams(),
                              graph_search=False, batch_size=2, **kw)
        return predict(pp)
    run_predict("p_plain"), run_predict("p_off", components=None)
    p_on = run_predict("p_on", components=rule)
    tree_equal(tmp_path / "p_plain", tmp_path / "p_off", ["prediction_info.hdf5", "prediction_params.hdf5"])
    for i in range(n):
        f, g = (h5io.load(tmp_path / d / f"image_{i}" / "prediction_info.hdf5") for d in ("p_on", "p_off"))
        names = lambda d: {k for k in d if not k.startswith("attr:")}      # noqa: E731
        assert names(f) - names(g) == {"cc_predicted_labels", "component_count", "largest_component_pixels", "removed_pixels"}
        assert names(g) <= names(f) and all(np.array_equal(f[k], g[k]) for k in names(g))
        assert np.array_equal(f["cc_predicted_labels"], clean[i]) and np.array_equal(f["removed_pixels"], removed[i])
        assert np.array_equal(f["component_count"], stats[i, :, 0]) and np.array_equal(f["largest_component_pixels"], stats[i, :, 1])
        d_on, d_off = (tmp_path / d / f"image_{i}" for d in ("p_on", "p_off"))
        assert {p.name for p in d_on.iterdir()} == {p.name for p in d_off.iterdir()}
        assert (d_on / "segmentation_map.csv").read_bytes() == (d_off / "segmentation_map.csv").read_bytes()
    assert len(p_on) == n
    run_predict("p_on_png", components=rule, png_plots=True), run_predict("p_off_png", png_plots=True)
    assert {p.name for p in pngs(tmp_path / "p_on_png") - pngs(tmp_path / "p_off_png")} == set(CC_PNG_NAMES.values())
    assert all((tmp_path / "p_off_png" / p).read_bytes() == (tmp_path / "p_on_png" / p).read_bytes() for p in pngs(tmp_path / "p_off_png"))


def test_evaluate_model_components_with_ignore_label(tmp_path):
    """``ignore_label`` composes with the stage: the cleaned map itself does not depend on it, and its Dice and surface
    distances skip the ignored ground-truth pixels exactly as those of the arg-max map do -- by the host formulas of
    tests/test_gpu_eval_ignore.py, on the host path and under ``metrics_device`` alike."""
    from oct_image_segmentation_models_amd.common import h5io
    from oct_image_segmentation_models_amd.evaluation import dice_device as dd, eval_model
    from oct_image_segmentation_models_amd.evaluation.components import ComponentRule, components_host
    from oct_image_segmentation_models_amd.evaluation.evaluation_parameters import EvaluationParameters, EvaluationSaveParams
    from oct_image_segmentation_models_amd.models.engine_model import load_model
    from oct_image_segmentation_models_amd.common import dataset_loader as dl
    # the scans and the model of the end-to-end test above (its arg-max maps have islands to remove)
    images, full, _ = dl.load_testing_data(dl.open_dataset(ROOT / "tests" / "golden" / "dataset_small.hdf5"))
    (n, H, W), C, IGN = images.shape[:3], int(full.max()) + 1, 255
    save_untrained_model(tmp_path, H, W, C, SN, 2)
    labels = full.copy()
    for i in range(n):                                       # one ignored rectangle per scan, across the class surfaces
        labels[i, H // 8 + i:H - H // 4 + i, W // 6 + 3 * i:W // 2 + 3 * i] = IGN
    h5io.save(tmp_path / "partial.hdf5", {"test_images": images, "test_labels": labels})
    h5io.save(tmp_path / "full.hdf5", {"test_images": images, "test_labels": full})
    metrics = ["dice_coef_classes", "dice_coef_macro", "dice_coef_micro", "average_surface_distance", "hausdorff_distance"]
    rule = ComponentRule(connectivity=8, min_pixels=8, keep_largest="all", fill="column")

    def evaluate(name, data, **kw):
        ep = EvaluationParameters(model_path=tmp_path / "model" / "model.npz", mlflow_tracking_uri=None, mlflow_run_uuid=None,
                                  test_dataset_path=tmp_path / data, save_foldername=tmp_path / name,
                                  save_params=EvaluationSaveParams(), graph_search=False, metrics=metrics, batch_size=2,
                                  components=rule, **kw)
        eval_model(ep)
        return tmp_path / name
    host, device = evaluate("host", "partial.hdf5", ignore_label=IGN), evaluate("device", "partial.hdf5", ignore_label=IGN, metrics_device=True)
    unmasked = evaluate("unmasked", "full.hdf5")
    tree_equal(host, device, ["cc_evaluation_results.hdf5", "evaluation_results.hdf5", "overall_evaluation_results.hdf5"])
    argmax = load_model(tmp_path / "model" / "model.npz").predict_labels(images, batch_size=2)
    clean, stats, removed = components_host(argmax, C, rule)
    assert (clean != argmax).any()
    gt, files, differs = labels[..., 0], [], False
    for i in range(n):
        f, u = (h5io.load(d / f"image_{i}" / "cc_evaluation_results.hdf5") for d in (host, unmasked))
        assert np.array_equal(f["cc_predicted_labels"], clean[i]) and np.array_equal(u["cc_predicted_labels"], clean[i])
        assert np.array_equal(f["removed_pixels"], removed[i]) and np.array_equal(f["component_count"], stats[i, :, 0])
        counts = dd.counts_matrix(dd.confusion_counts_reference(clean[i][None], gt[i][None], C, IGN), C, ignored=True)[0]
        assert counts.sum() == int((gt[i] != IGN).sum()) < H * W
        dc, dm, dmi = dd.dice_from_counts(counts, metrics)
        assert np.array_equal(f["dice_coef_classes"], np.squeeze(dc).astype(np.float64))
        assert np.array_equal(f["dice_coef_macro"], np.expand_dims(dm, 0).astype(np.float64))
        assert np.array_equal(f["dice_coef_micro"], np.expand_dims(dmi, 0).astype(np.float64))
        differs |= not np.array_equal(f["dice_coef_classes"], u["dice_coef_classes"])
        files.append(f)
    assert differs                                                # the ignored pixels did count in the run without the label
    _surface_files_equal_the_formula(files, clean, argmax, gt, C, h5io.load(host / "overall_evaluation_results.hdf5"), IGN)
