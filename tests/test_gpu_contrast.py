"""GPU tests of the contrast stage: ``oct_contrast_batch`` against ``contrast_luts_reference`` /
``contrast_reference`` byte for byte -- the LUT bytes at the head of the workspace first, so that a failure names the pass,
then the output --, in place, repeated, inside a captured graph, with canaries behind the workspace and the output; the
argument errors; and the layers: ``BatchedPredictor(contrast=)``, ``Model.predict_labels(contrast=)``, the launches with the
stage off, and ``train_model(contrast=)`` against a run on the normalised dataset.

Shapes (tests/contrast_cases.py): 16x16 in (2,2) tiles -- the smallest legal tile, 64 pixels, L = 1 under any clip below 4;
37x53 in (4,6) -- uneven tile edges, an odd row pitch (no vector path) and unaligned image bases from the second image on;
20x34 in (2,1) and (1,4) -- one interpolation axis degenerate; 40x40 in (1,1) -- one tile per image, the multi-block merge;
256x512 in (8,8) and (16,16) -- the workload's geometry and the largest grid; 24x40x3 in (2,3) -- the channel stride."""
import ctypes as C
import json
from pathlib import Path

import numpy as np
import pytest
import torch

import contrast_cases as cc
from tests.test_gpu_any_size import C3, DEV, SENTINEL, _cfg, _engine, _guarded, _guards_untouched, _model, _up, _weights

pytestmark = pytest.mark.gpu


def _U():
    from oct_image_segmentation_models_amd.common import utils
    return utils


def _desc(spec):
    from oct_image_segmentation_models_amd import _hip
    return _hip.ContrastDesc(*_U().contrast_desc(spec))


def _ws_bytes(shape, spec) -> int:
    from oct_image_segmentation_models_amd import _hip
    B, H, W, ch = shape
    return int(_hip.lib().oct_contrast_workspace_bytes(B, H, W, ch, C.byref(_desc(spec))))


def _call(x_dev, spec, ws, out_dev, ws_bytes=None, shape=None):
    """The raw ABI call on the current stream -> its return code."""
    from oct_image_segmentation_models_amd import _hip
    B, H, W, ch = shape or x_dev.shape
    with torch.cuda.device(DEV):
        return _hip.lib().oct_contrast_batch(x_dev.data_ptr(), B, H, W, ch, C.byref(_desc(spec)), ws.data_ptr(),
                                             ws.numel() if ws_bytes is None else ws_bytes, out_dev.data_ptr(), _hip.stream_ptr(torch.device(DEV)))


def device_contrast(x, spec, in_place=False):
    """``(luts, out)`` of the kernel for host batch ``x``, with canaries behind the workspace and the output checked."""
    B, H, W, ch = x.shape
    need = _ws_bytes(x.shape, spec)
    assert need >= B * ch * spec["tiles"][0] * spec["tiles"][1] * 256
    ws_flat, ws = _guarded(need)
    n = x.size
    # an odd offset from the second image on comes from the shape itself; the first image's base is the buffer's + 64
    out_flat, out = _guarded(n)
    out = out.view(B, H, W, ch)
    if in_place:
        out.copy_(_up(np.array(x)))
        src = out
    else:
        src = _up(np.array(x))
    assert _call(src, spec, ws, out) == 0
    torch.cuda.synchronize()
    assert _guards_untouched(ws_flat, need), "bytes behind ws_bytes were written"
    assert _guards_untouched(out_flat, n), "bytes around out were written"
    if not in_place:
        assert np.array_equal(src.cpu().numpy(), x), "the input was written"
    ty, tx = spec["tiles"]
    luts = ws[:B * ch * ty * tx * 256].cpu().numpy().reshape(B, ch, ty, tx, 256)
    return luts, out.cpu().numpy()


_REF = {}


def reference(content, B, H, W, ch, spec):
    """``(x, luts, out)`` of the numpy restatement: computed once per case, shared, never written."""
    key = (content, B, H, W, ch, json.dumps(spec, sort_keys=True))
    if key not in _REF:
        U = _U()
        x = cc.make_images(content, B, H, W, ch)
        luts = U.contrast_luts_reference(x, spec)
        out = U.contrast_reference(x, spec, luts=luts)
        for a in (x, luts, out):
            a.setflags(write=False)
        _REF[key] = (x, luts, out)
    return _REF[key]


# ---- 1. the kernel against the restatement ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("spec", cc.SPECS, ids=cc.spec_id)
@pytest.mark.parametrize("shape", cc.SHAPES, ids=lambda s: "%dx%dx%d-%dx%d" % (s[0], s[1], s[2], s[3][0], s[3][1]))
def test_kernel_equals_the_restatement(shape, spec, B):
    H, W, ch, tiles = shape
    s = _U().check_contrast(cc.with_tiles(spec, tiles), hw=(H, W))
    for content in cc.CONTENTS:
        x, want_luts, want = reference(content, B, H, W, ch, s)
        if content != "constant":
            cc.assert_not_vacuous(x, s, want_luts, want)
        luts, out = device_contrast(x, s)
        assert np.array_equal(luts, want_luts), f"{content}: LUT pass: {int((luts != want_luts).sum())} bytes differ"
        assert np.array_equal(out, want), f"{content}: apply pass: {int((out != want).sum())} bytes differ"


def test_smallest_tile_has_clip_limit_one():
    """16x16 in (2,2): A = 64, so L = max(1, (clip_q8 * 64) >> 16) = 1 for every clip below 4 -- the clips 1 and 2 give the
    same bytes, and not those of clip 40 (L = 10)."""
    x = cc.make_images("noise", 2, 16, 16, 1)
    outs = [device_contrast(x, {"method": "clahe", "tiles": [2, 2], "clip": c})[1] for c in (1.0, 2.0, 3.99, 40.0)]
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], outs[2]) and not np.array_equal(outs[0], outs[3])


# ---- 2. in place, repeated, captured ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(37, 53, 1, (4, 6)), (256, 512, 1, (8, 8)), (24, 40, 3, (2, 3))], ids=["scalar", "vector", "ch3"])
def test_in_place_and_repeats(shape):
    H, W, ch, tiles = shape
    s = _U().check_contrast({"method": "clahe", "clip": 2.0, "tiles": tiles}, hw=(H, W))
    x, want_luts, want = reference("scan", 3, H, W, ch, s)
    luts, out = device_contrast(x, s)
    luts_ip, out_ip = device_contrast(x, s, in_place=True)
    assert np.array_equal(out, want) and np.array_equal(out_ip, out) and np.array_equal(luts_ip, luts)
    luts2, out2 = device_contrast(x, s)
    assert np.array_equal(out2, out) and np.array_equal(luts2, luts)


def test_records_into_a_graph_and_replays():
    H, W, ch, tiles = 37, 53, 1, (4, 6)
    s = _U().check_contrast({"method": "stretch", "percentiles": (1, 99), "tiles": tiles}, hw=(H, W))
    x, want_luts, want = reference("noise", 5, H, W, ch, s)
    x2, _, want2 = reference("scan", 5, H, W, ch, s)
    src, out = _up(np.array(x)), torch.zeros((5, H, W, ch), dtype=torch.uint8, device=DEV)
    ws = torch.empty((_ws_bytes(x.shape, s),), dtype=torch.uint8, device=DEV)
    stream = torch.cuda.Stream(device=DEV)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        assert _call(src, s, ws, out) == 0              # warm: code objects loaded outside the capture
        torch.cuda.synchronize()
        out.zero_()
        with torch.cuda.graph(graph, stream=stream):
            assert _call(src, s, ws, out) == 0
        torch.cuda.synchronize()
        assert (out.cpu().numpy() == 0).all(), "the capture ran the kernels"
        for k in range(2):
            out.zero_()
            graph.replay()
            torch.cuda.synchronize()
            assert np.array_equal(out.cpu().numpy(), want), f"replay {k}"
        src.copy_(_up(np.array(x2)))                              # the graph reads its fixed input: new bytes, the same nodes
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), want2)


# ---- 3. argument errors -----------------------------------------------------------------------------------------------------------
def test_argument_errors():
    from oct_image_segmentation_models_amd import _hip
    lib = _hip.lib()
    B, H, W, ch = 2, 32, 40, 1
    spec = {"method": "clahe", "tiles": [2, 2], "clip": 2.0}
    need = _ws_bytes((B, H, W, ch), spec)
    assert need > 0
    n = B * H * W * ch
    flat = torch.full((need + 2 * n + 64,), SENTINEL, dtype=torch.uint8, device=DEV)
    ws, x, out = flat[:need], flat[need:need + n], flat[need + n:need + 2 * n]
    stream = _hip.stream_ptr(torch.device(DEV))

    def raw(xp, shape, d, wsp, wsb, outp):
        with torch.cuda.device(DEV):
            return lib.oct_contrast_batch(xp, *shape, None if d is None else C.byref(d), wsp, wsb, outp, stream)
    good = _desc(spec)
    shape = (B, H, W, ch)

    def desc(**kw):
        d = _desc(spec)
        for k, v in kw.items():
            setattr(d, k, v)
        return d
    cases = {
        "null x": lambda: raw(None, shape, good, ws.data_ptr(), need, out.data_ptr()),
        "null desc": lambda: raw(x.data_ptr(), shape, None, ws.data_ptr(), need, out.data_ptr()),
        "null ws": lambda: raw(x.data_ptr(), shape, good, None, need, out.data_ptr()),
        "null out": lambda: raw(x.data_ptr(), shape, good, ws.data_ptr(), need, None),
        "ch = 5": lambda: raw(x.data_ptr(), (1, 16, 16, 5), good, ws.data_ptr(), need, out.data_ptr()),
        "ch = 0": lambda: raw(x.data_ptr(), (B, H, W, 0), good, ws.data_ptr(), need, out.data_ptr()),
        "H = 4097": lambda: raw(x.data_ptr(), (1, 4097, 16, 1), good, ws.data_ptr(), need, out.data_ptr()),
        "W = 4097": lambda: raw(x.data_ptr(), (1, 16, 4097, 1), good, ws.data_ptr(), need, out.data_ptr()),
        "B = 0": lambda: raw(x.data_ptr(), (0, H, W, ch), good, ws.data_ptr(), need, out.data_ptr()),
        "B = 65536": lambda: raw(x.data_ptr(), (65536, H, W, ch), good, ws.data_ptr(), need, out.data_ptr()),
        "tiles_y = 17": lambda: raw(x.data_ptr(), shape, desc(tiles_y=17), ws.data_ptr(), need, out.data_ptr()),
        "tiles_x = 0": lambda: raw(x.data_ptr(), shape, desc(tiles_x=0), ws.data_ptr(), need, out.data_ptr()),
        "tiles of 32 // 5 = 6 rows": lambda: raw(x.data_ptr(), shape, desc(tiles_y=5), ws.data_ptr(), need, out.data_ptr()),
        "tiles of 40 // 6 = 6 columns": lambda: raw(x.data_ptr(), shape, desc(tiles_x=6), ws.data_ptr(), need, out.data_ptr()),
        "unknown method": lambda: raw(x.data_ptr(), shape, desc(method=2), ws.data_ptr(), need, out.data_ptr()),
        "clip_q8 = 255": lambda: raw(x.data_ptr(), shape, desc(clip_q8=255), ws.data_ptr(), need, out.data_ptr()),
        "clip_q8 = 65536": lambda: raw(x.data_ptr(), shape, desc(clip_q8=65536), ws.data_ptr(), need, out.data_ptr()),
        "lo_bp = hi_bp": lambda: raw(x.data_ptr(), shape, desc(method=1, lo_bp=500, hi_bp=500), ws.data_ptr(), need, out.data_ptr()),
        "hi_bp = 10001": lambda: raw(x.data_ptr(), shape, desc(method=1, lo_bp=0, hi_bp=10001), ws.data_ptr(), need, out.data_ptr()),
        "workspace too small": lambda: raw(x.data_ptr(), shape, good, ws.data_ptr(), need - 1, out.data_ptr()),
        "workspace not 4-byte aligned": lambda: raw(x.data_ptr(), shape, good, flat[1:].data_ptr(), need, flat[need + 4:].data_ptr()),
        "out overlaps ws": lambda: raw(x.data_ptr(), shape, good, ws.data_ptr(), need, ws[need - 8:].data_ptr()),
        "out inside ws": lambda: raw(out.data_ptr(), shape, good, ws.data_ptr(), need, ws[16:].data_ptr()),
        "x overlaps ws": lambda: raw(ws[need - 8:].data_ptr(), shape, good, ws.data_ptr(), need, out.data_ptr()),
        "out partly overlaps x": lambda: raw(x.data_ptr(), shape, good, ws.data_ptr(), need, x[n // 2:].data_ptr()),
        "out one byte behind x's start": lambda: raw(x.data_ptr(), shape, good, ws.data_ptr(), need, x[1:].data_ptr()),
    }
    for what, call in cases.items():
        lib.oct_set_option(b"no_such_option", 0)          # leaves another message behind: the call must set its own
        rc = call()
        msg = lib.oct_last_error().decode()
        assert rc < 0 and "contrast_batch" in msg, (what, rc, msg)
    torch.cuda.synchronize()
    assert (flat.cpu().numpy() == SENTINEL).all(), "a refused call launched something"
    zero = {"ch = 5": (1, 16, 16, 5, good), "H = 4097": (1, 4097, 16, 1, good), "tiles": (B, H, W, ch, desc(tiles_y=17)),
            "small tiles": (B, H, W, ch, desc(tiles_y=5)), "B": (65536, H, W, ch, good)}
    for what, (b, h, w, c, d) in zero.items():
        assert lib.oct_contrast_workspace_bytes(b, h, w, c, C.byref(d)) == 0, what
    assert lib.oct_contrast_workspace_bytes(B, H, W, ch, None) == 0


def test_engine_method_validates_like_pad_and_crop():
    from oct_image_segmentation_models_amd._hip import OctError
    cfg = _cfg(16, 16, sn=4)
    eng = _engine(cfg, _weights(cfg, 1), 1)
    spec = {"method": "clahe", "tiles": (4, 6), "clip": 2.0}
    x, _, want = reference("scan", 5, 37, 53, 1, _U().check_contrast(spec))
    xd = _up(np.array(x))
    got = eng.contrast(xd, spec)                              # any size, any batch: the stage does not depend on the engine's
    assert got.data_ptr() != xd.data_ptr() and np.array_equal(got.cpu().numpy(), want)
    assert eng.contrast(xd, spec, out=xd) is xd and np.array_equal(xd.cpu().numpy(), want)
    for bad in (lambda: eng.contrast(_up(x.astype(np.float32)), spec), lambda: eng.contrast(_up(x[:, :, :, 0]), spec),
                lambda: eng.contrast(_up(np.array(x)), None), lambda: eng.contrast(_up(np.array(x)), dict(spec, tiles=(8, 8))),
                lambda: eng.contrast(_up(np.array(x)), spec, out=torch.empty((5, 37, 53), dtype=torch.uint8, device=DEV)),
                lambda: eng.contrast(_up(np.array(x)), spec, ws=torch.empty((16,), dtype=torch.uint8, device=DEV)),
                lambda: eng.contrast(torch.from_numpy(np.array(x)), spec)):
        with pytest.raises(OctError):
            bad()


def test_contrast_images_equals_the_restatement():
    U = _U()
    spec = {"method": "clahe", "tiles": (2, 4), "clip": 3.0}
    x = cc.make_images("scan", 11, 32, 64, 1)
    want = U.contrast_reference(x, spec)
    for chunk in (4, 11, 64):                                 # a partial last chunk, one chunk, a chunk beyond the array
        assert np.array_equal(U.contrast_images(x, spec, device=DEV, chunk=chunk), want), chunk
    assert U.contrast_images(x, None) is x


# ---- 4. the layers ------------------------------------------------------------------------------------------------------------------
def _run(eng, images, batch, **kw):
    from oct_image_segmentation_models_amd.evaluation.pipeline import BatchedPredictor
    pred = BatchedPredictor(eng, batch, **kw)
    got = list(pred.run(images))
    return pred, got


@pytest.mark.parametrize("kind", ["plain", "padded", "tta"])
def test_batched_predictor_equals_a_run_on_the_normalised_images(kind):
    """``BatchedPredictor(contrast=spec).run(images)`` against ``BatchedPredictor().run(contrast_reference(images, spec))``:
    labels and maps byte for byte, with a partial last batch (5 images in batches of 2)."""
    U = _U()
    if kind == "padded":
        (H, W), cfg, more = (37, 70), _cfg(40, 72), dict(hw=(37, 70), pad_mode="edge")       # no multiple of 2^pool_layers
        spec = {"method": "clahe", "tiles": (4, 8), "clip": 2.0}
    else:
        (H, W), cfg, more = (32, 64), _cfg(32, 64), (dict(tta=("identity", "flip_lr")) if kind == "tta" else {})
        spec = {"method": "stretch", "tiles": (2, 4), "percentiles": (2, 98)} if kind == "tta" else \
            {"method": "clahe", "tiles": (2, 4), "clip": 2.0}
    eng = _engine(cfg, _weights(cfg, 5), 2)
    images = cc.make_images("scan", 5, H, W, 1, seed=3)
    normal = U.contrast_reference(images, spec)
    assert (normal != images).any()
    _, want = _run(eng, normal, 2, **more)
    _, plain = _run(eng, images, 2, **more)
    pred, got = _run(eng, images, 2, contrast=spec, **more)
    assert pred.contrast == U.check_contrast(spec)
    assert [(b.lo, b.hi) for b in got] == [(0, 2), (2, 4), (4, 5)]
    for g, w in zip(got, want):
        assert g.labels.shape == (g.hi - g.lo, H, W) and np.array_equal(g.labels, w.labels), (kind, g.lo)
        assert np.array_equal(g.maps, w.maps), (kind, g.lo)
        if kind == "tta":
            assert np.array_equal(g.entropy, w.entropy) and np.array_equal(g.mutual_info, w.mutual_info)
    # the stage does something to the prediction: the labels of the raw scans are others
    assert any(not np.array_equal(g.labels, p.labels) for g, p in zip(got, plain))


def test_predict_and_predict_labels_take_the_keyword():
    U = _U()
    model = _model(_cfg(32, 64))
    spec = {"method": "clahe", "tiles": (4, 8), "clip": 2.0}
    x = cc.make_images("scan", 5, 37, 70, 1, seed=4)
    normal = U.contrast_reference(x, spec)
    want_l, want_m = model.predict_labels(normal, batch_size=2, want_maps=True, pad_mode="edge")
    got_l, got_m = model.predict_labels(x, batch_size=2, want_maps=True, pad_mode="edge", contrast=spec)
    assert np.array_equal(got_l, want_l) and np.array_equal(got_m, want_m)
    assert not np.array_equal(got_l, model.predict_labels(x, batch_size=2, pad_mode="edge"))
    assert np.array_equal(model.predict(x, batch_size=2, pad_mode="edge", contrast=spec),
                          model.predict(normal, batch_size=2, pad_mode="edge"))
    with pytest.raises(ValueError, match="uint8"):
        model.predict(x.astype(np.float32) / 255, pad_mode="edge", contrast=spec)
    with pytest.raises(ValueError, match="uint8"):
        model.predict_labels(x.astype(np.float32), pad_mode="edge", contrast=spec)


def test_nothing_is_launched_with_the_stage_off():
    """The per-launch profiler over ``Model.predict_labels``: with ``contrast=None`` no launch of the stage is listed; with a
    spec the list is the same plus the stage's three kernels, once per batch."""
    model = _model(_cfg(32, 64))
    x = cc.make_images("scan", 4, 32, 64, 1, seed=5)
    spec = {"method": "clahe", "tiles": (2, 4), "clip": 2.0}
    eng = model._ensure_engine(2, False, hw=(32, 64))
    model.predict_labels(x, batch_size=2)                     # warm; the engine's profiler is now this thread's

    def launches(**kw):
        eng.profile_begin()
        model.predict_labels(x, batch_size=2, **kw)
        return {(e["kernel"], e["layer"]): e["launches"] for e in eng.profile_end()}
    off, on = launches(), launches(contrast=spec)
    assert off and not any("contrast" in k or "contrast" in l for k, l in off)
    stage = {k: v for k, v in on.items() if k[1] == "contrast"}
    assert {k: v for k, v in on.items() if k[1] != "contrast"} == off
    assert stage == {("contrast_hist_k", "contrast"): 2, ("contrast_lut_k", "contrast"): 2, ("contrast_apply_k<4>", "contrast"): 2}


def test_train_model_equals_training_on_the_normalised_dataset(tmp_path):
    """Two epochs of ``train_model(contrast=spec)`` against ``train_model`` on a dataset file holding
    ``contrast_reference(images)``, same seed: the weights are bit-equal, and only the first run folder has a contrast.json."""
    from oct_image_segmentation_models_amd import optimizers as O
    from oct_image_segmentation_models_amd.common import h5io
    from oct_image_segmentation_models_amd.common.synthetic import make_scans
    from oct_image_segmentation_models_amd.training.training import train_model
    from oct_image_segmentation_models_amd.training.training_parameters import TrainingParams
    U = _U()
    spec = {"method": "clahe", "tiles": (2, 4), "clip": 2.0}
    tr_i, tr_l = make_scans(8, 32, 64, C3, seed=11)
    va_i, va_l = make_scans(4, 32, 64, C3, seed=12)
    tr_i, va_i = (30 + tr_i.astype(np.int64) * 2 // 3).astype(np.uint8), (30 + va_i.astype(np.int64) * 2 // 3).astype(np.uint8)
    h5io.save(tmp_path / "raw.hdf5", {"train_images": tr_i, "train_labels": tr_l, "val_images": va_i, "val_labels": va_l})
    h5io.save(tmp_path / "normal.hdf5", {"train_images": U.contrast_reference(tr_i, spec), "train_labels": tr_l,
                                         "val_images": U.contrast_reference(va_i, spec), "val_labels": va_l})
    assert (U.contrast_reference(tr_i, spec) != tr_i).any()

    def train(name, data, **kw):
        tp = TrainingParams(model_architecture="unet", training_dataset_path=tmp_path / data, initial_model=None,
                            results_location=tmp_path / name, opt_con=O.Adam, opt_params={"learning_rate": 1e-3},
                            loss="dice_loss_macro", metric="dice_coef_macro", epochs=2, batch_size=2,
                            model_hyperparameters={"pool_layers": 2}, seed=3, **kw)
        return train_model(tp, None)
    on = train("on", "raw.hdf5", contrast=spec)
    ref = train("ref", "normal.hdf5")
    w_on, w_ref = on.model.get_weights(), ref.model.get_weights()
    assert len(w_on) == len(w_ref) and all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(w_on, w_ref))
    with open(Path(on.save_foldername) / "contrast.json") as fh:
        assert json.load(fh) == U.check_contrast(spec)
    assert not (Path(ref.save_foldername) / "contrast.json").exists()
    raw = train("raw", "raw.hdf5")                            # and the stage moved the training: other weights without it
    assert any(not np.array_equal(a, b) for a, b in zip(w_on, raw.model.get_weights()))
