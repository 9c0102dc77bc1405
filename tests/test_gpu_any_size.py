"""GPU tests of "scans of any size": ``oct_pad_batch`` / ``oct_crop_batch`` against their numpy restatements, the model's
engine following the data's geometry with ONE set of weights, padded prediction through ``Model``, ``InferenceRun`` and the
two workflows.  Every comparison is bit for bit: it compares the same kernels on the same geometry with the same weights
(two separately built engines of one geometry repeat each other bit for bit: ``test_two_native_engines_repeat_each_other``)."""
import json
import struct
from pathlib import Path

import numpy as np
import pytest
import torch

from oracle import unet_numpy as on

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
C3 = 3
SENTINEL = 0xA5


def _cfg(H, W, sn=8, **kw):
    return dict(dict(input_channels=1, num_classes=C3, image_height=H, image_width=W, start_neurons=sn, pool_layers=2), **kw)


def _weights(cfg, seed):
    """Keras-order weights with every tensor away from its initial value (BN statistics included)."""
    from oct_image_segmentation_models_amd.engine import layer_table, make_cfg
    rng = np.random.default_rng(seed)
    out = []
    for L in layer_table(make_cfg(**{k: v for k, v in cfg.items() if k != "seed"})):
        kh, kw, cin, cout = L["kh"], L["kw"], L["cin"], L["cout"]
        out += [rng.normal(0, np.sqrt(2.0 / (kh * kw * cin)), (kh, kw, cin, cout)).astype(np.float32),
                rng.normal(0, 0.1, cout).astype(np.float32)]
        if L["has_bn"]:
            out += [rng.uniform(0.5, 1.5, cout).astype(np.float32), rng.normal(0, 0.1, cout).astype(np.float32),
                    rng.normal(0, 0.1, cout).astype(np.float32), rng.uniform(0.5, 1.5, cout).astype(np.float32)]
    return out


def _model(cfg, seed=5):
    from oct_image_segmentation_models_amd.models.engine_model import Model
    m = Model(name="unet", config=dict(cfg, seed=2))
    m.set_weights(_weights(cfg, seed))
    return m


def _engine(cfg, weights, max_batch, seed=2 * 1000003, training=False):
    from oct_image_segmentation_models_amd.engine import UNetEngine
    eng = UNetEngine(device=DEV, max_batch=max_batch, training=training, seed=seed, init_seed=0,
                     **{k: v for k, v in cfg.items() if k != "seed"})
    eng.set_weights(weights)
    return eng


def _up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _scans(n, H, W, seed):
    return on.synth_scans(n, H, W, C3, seed=seed)


@pytest.fixture(scope="module")
def small_engine():
    cfg = _cfg(16, 16, sn=4)
    return _engine(cfg, _weights(cfg, 1), 1)


def _guarded(n_bytes, offset=0):
    """A sentinel-filled flat uint8 device buffer and the ``n_bytes`` view at ``offset`` of it, 64 guard bytes on each side."""
    flat = torch.full((64 + offset + n_bytes + 64,), SENTINEL, dtype=torch.uint8, device=DEV)
    return flat, flat[64 + offset:64 + offset + n_bytes]


def _guards_untouched(flat, n_bytes, offset=0):
    h = flat.cpu().numpy()
    return (h[:64 + offset] == SENTINEL).all() and (h[64 + offset + n_bytes:] == SENTINEL).all()


# ---- 0. what the engine-against-engine comparisons rest on ----------------------------------------------------------------
@pytest.mark.parametrize("sn", [8, 4])
def test_two_native_engines_repeat_each_other(sn):
    cfg = _cfg(48, 80, sn=sn)
    w = _weights(cfg, 5)
    x = _up(_scans(3, 48, 80, 11)[0])
    outs = []
    for _ in range(2):
        eng = _engine(cfg, w, 3)
        p, am = eng.forward(x, training=False, want_probs=True, want_argmax=True)
        outs.append((p.cpu().numpy(), am.cpu().numpy()))
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])


# ---- 1. oct_pad_batch --------------------------------------------------------------------------------------------------
PAD_SHAPES = [((2, 5, 7, 1), (8, 8), (1, 0)), ((1, 33, 70, 3), (36, 72), (1, 1)), ((3, 16, 32, 1), (16, 32), (0, 0)),
              ((1, 3, 3, 1), (4, 4), (0, 0)), ((1, 2, 19, 1), (4, 32), (1, 6)), ((2, 37, 1031, 1), (40, 1032), (1, 0))]


@pytest.mark.parametrize("dtype", [np.uint8, np.float32], ids=["u8", "f32"])
@pytest.mark.parametrize("shape, out, at", PAD_SHAPES, ids=lambda v: "x".join(map(str, v)))
def test_pad_batch_equals_the_numpy_restatement(small_engine, dtype, shape, out, at):
    from oct_image_segmentation_models_amd.common.utils import pad_reference
    x = (np.random.default_rng(7).random(shape) * 255).astype(dtype)
    (Hp, Wp), (top, left) = out, at
    xd = _up(x)
    for mode in ("edge", "reflect", "constant"):
        want = pad_reference(x, Hp, Wp, top, left, mode, 7)
        got = small_engine.pad(xd, Hp, Wp, top, left, mode, 7)
        assert got.dtype == xd.dtype and tuple(got.shape) == want.shape
        assert np.array_equal(got.cpu().numpy().view(np.uint8), want.view(np.uint8)), mode
        # into a caller's buffer that starts 4 bytes off a 16-byte boundary: guard bytes on both sides stay
        flat, view = _guarded(want.nbytes, offset=4)
        out_t = view.view(torch.float32 if dtype == np.float32 else torch.uint8).view(want.shape)
        assert small_engine.pad(xd, Hp, Wp, top, left, mode, 7, out=out_t) is out_t
        assert np.array_equal(out_t.cpu().numpy().view(np.uint8), want.view(np.uint8)) and _guards_untouched(flat, want.nbytes, 4), mode


def test_pad_batch_at_every_source_and_destination_alignment(small_engine):
    """uint8 rows of 100 bytes into rows of 120 at left = 0..7 (the source of a whole chunk is then 0..3 bytes off a dword:
    the 16-byte load, the shifted dwords and, next to the buffer's ends, the byte loads), the destination 0..3 bytes off."""
    from oct_image_segmentation_models_amd.common.utils import pad_reference
    x = (np.random.default_rng(9).random((2, 9, 100, 1)) * 255).astype(np.uint8)
    xd = _up(x)
    for left in range(8):
        for off in range(4):
            want = pad_reference(x, 12, 120, 2, left, "edge")
            flat, view = _guarded(want.nbytes, offset=off)
            small_engine.pad(xd, 12, 120, 2, left, "edge", out=view.view(want.shape))
            assert np.array_equal(view.cpu().numpy().reshape(want.shape), want) and _guards_untouched(flat, want.nbytes, off), (left, off)


# ---- 2. oct_crop_batch -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pb", [1, 4, 8, 12, 32])
@pytest.mark.parametrize("src, out, at", [((2, 8, 8), (5, 7), (1, 0)), ((1, 40, 1032), (37, 1031), (1, 1)), ((3, 16, 32), (16, 32), (0, 0))],
                         ids=lambda v: "x".join(map(str, v)))
def test_crop_batch_equals_the_numpy_restatement(small_engine, pb, src, out, at):
    from oct_image_segmentation_models_amd.common.utils import crop_reference
    t = np.random.default_rng(13).integers(0, 256, src + (pb,), dtype=np.uint8)
    (H, W), (top, left) = out, at
    want = crop_reference(t, H, W, top, left)
    td = _up(t if pb > 1 else t[..., 0])
    got = small_engine.crop(td, H, W, top, left)
    assert np.array_equal(got.cpu().numpy().reshape(want.shape), want)
    for off in (0, 1):                                   # sentinel-filled destination; the bytes past its end stay
        flat, view = _guarded(want.nbytes, offset=off)
        small_engine.crop(td, H, W, top, left, out=view.view(got.shape))
        assert np.array_equal(view.cpu().numpy().reshape(want.shape), want) and _guards_untouched(flat, want.nbytes, off), off
    if pb == 4:                                          # the float32 maps (entropy, mutual information) through the same entry
        f = _up(np.ascontiguousarray(t).view(np.float32)[..., 0])
        assert np.array_equal(small_engine.crop(f, H, W, top, left).cpu().numpy().view(np.uint8).reshape(want.shape), want)


# ---- 3. the engine follows the data ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("sn", [8, 4])
def test_model_runs_at_the_size_of_the_batch_not_of_the_config(sn):
    model = _model(_cfg(32, 64, sn=sn))
    x, _ = _scans(3, 48, 80, 21)
    probs = model.predict(x)
    labels, maps = model.predict_labels(x, want_maps=True)
    assert probs.shape == (3, 48, 80, C3) and labels.shape == (3, 48, 80) and maps.shape == (3, C3 - 1, 48, 80)
    assert (model._engine.cfg.H, model._engine.cfg.W) == (48, 80) and model.config["image_height"] == 32
    native = _engine(_cfg(48, 80, sn=sn), model.get_weights(), 3)
    p, am = native.forward(_up(x), training=False, want_probs=True, want_argmax=True)
    assert np.array_equal(probs, p.cpu().numpy()) and np.array_equal(labels, am.cpu().numpy())
    assert np.array_equal(maps, native.boundary_maps(am).cpu().numpy())
    # back at the config's size, and at a third one: at most two engines are kept, the weights are the same everywhere
    w = model.get_weights()
    x0, _ = _scans(2, 32, 64, 22)
    p0 = model.predict(x0)
    assert np.array_equal(p0, _engine(_cfg(32, 64, sn=sn), w, 2).forward(_up(x0))[0].cpu().numpy())
    model.predict(_scans(1, 16, 96, 23)[0])
    assert len(model._engines) <= 2 and all(np.array_equal(a, b) for a, b in zip(w, model.get_weights()))
    model.release_engines()
    assert model._engine is None and all(np.array_equal(a, b) for a, b in zip(w, model.get_weights()))
    assert np.array_equal(model.predict(x0), p0)


# ---- 4. one set of weights -----------------------------------------------------------------------------------------------------
class _Batches:
    """``keras.utils.Sequence`` duck type over ready (x float32 in [0,1], sparse labels) batches."""

    def __init__(self, images, labels, batch):
        self.items = [(images[i:i + batch].astype(np.float32) / np.float32(255.0), labels[i:i + batch])
                      for i in range(0, len(images), batch)]

    def __len__(self):
        return len(self.items)

    def __getitem__(self, i):
        return self.items[i]


def test_weights_stay_coherent_across_geometries_in_fit():
    from oct_image_segmentation_models_amd import optimizers
    from oct_image_segmentation_models_amd.common import custom_losses, custom_metrics
    model = _model(_cfg(32, 64))
    loss = custom_losses.custom_loss_objects["dice_loss_macro"]["function"](num_classes=C3, is_y_true_sparse=True)
    metric = custom_metrics.training_monitor_metric_objects["dice_coef_macro"](True, C3)
    model.compile(optimizer=optimizers.Adam(learning_rate=2e-3), loss=loss, metrics=[metric])
    w0 = model.get_weights()
    tr, va = _scans(4, 48, 80, 31), _scans(2, 32, 64, 32)
    hist = model.fit(_Batches(*tr, 2), validation_data=_Batches(*va, 2), epochs=1, verbose=0)       # two training steps
    assert np.isfinite(hist.history["loss"][0]) and np.isfinite(hist.history["val_loss"][0])
    eng_train, eng_val = model._engines["train"], model._engines["other"]
    assert (eng_train.cfg.H, eng_train.cfg.W) == (48, 80) and (eng_val.cfg.H, eng_val.cfg.W) == (32, 64)
    assert eng_train.opt_step == 2 and model._engine is eng_val                 # the validation engine ran last
    w = model.get_weights()
    assert any(not np.array_equal(a, b) for a, b in zip(w0, w))                 # training changed them ...
    assert all(np.array_equal(a, b) for a, b in zip(w, eng_train.get_weights()))   # ... and validation saw the trained ones
    x0 = va[0]
    p0 = model.predict(x0)
    assert np.array_equal(p0, _engine(_cfg(32, 64), w, 2).forward(_up(x0))[0].cpu().numpy())
    # get_weights does not depend on which geometry ran last
    model.predict(tr[0][:1])
    assert (model._engine.cfg.H, model._engine.cfg.W) == (48, 80)
    assert all(np.array_equal(a, b) for a, b in zip(w, model.get_weights()))
    # a second epoch goes on from the optimizer state of the first, on the same training engine
    model.fit(_Batches(*tr, 2), validation_data=_Batches(*va, 2), epochs=1, verbose=0)
    assert model._engines["train"] is eng_train and eng_train.opt_step == 4
    assert np.array_equal(model.predict(x0), _engine(_cfg(32, 64), model.get_weights(), 2).forward(_up(x0))[0].cpu().numpy())
    # fit on a size that is no multiple is refused: padding is for inference only
    from oct_image_segmentation_models_amd._hip import OctError
    model.pad_mode = "edge"
    with pytest.raises(OctError, match="pad_mode"):
        model.fit(_Batches(*_scans(2, 37, 70, 33), 2), epochs=1, verbose=0)


# ---- 5. padded prediction ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def padded_case():
    """A 32x64-config model, its native 40x72 engine and a 37x70 batch (padded: top 1, left 1)."""
    model = _model(_cfg(32, 64))
    native = _engine(_cfg(40, 72), model.get_weights(), 3)
    x, _ = _scans(5, 37, 70, 41)
    return model, native, x


def _native_route(native, x, mode, value, soft=False):
    """crop_reference(native.forward(pad_reference(x))): probabilities, arg-max, and the boundary maps of the cropped tensors."""
    from oct_image_segmentation_models_amd.common.utils import crop_reference, pad_reference
    probs, labels, maps = [], [], []
    for lo in range(0, len(x), 3):
        xp = pad_reference(x[lo:lo + 3], 40, 72, 1, 1, mode, value)
        p, am = native.forward(_up(xp), training=False, want_probs=True, want_argmax=True)
        p, am = crop_reference(p.cpu().numpy(), 37, 70, 1, 1), crop_reference(am.cpu().numpy(), 37, 70, 1, 1)
        m = native.boundary_maps_soft(_up(p)) if soft else native.boundary_maps(_up(am))
        probs.append(p); labels.append(am); maps.append(m.cpu().numpy())
    return np.concatenate(probs), np.concatenate(labels), np.concatenate(maps)


@pytest.mark.parametrize("mode, value", [("edge", 0), ("constant", 7)])
def test_padded_prediction_equals_the_native_engine_on_the_padded_batch(padded_case, mode, value):
    from oct_image_segmentation_models_amd.common.utils import crop_reference, pad_reference
    model, native, x = padded_case
    x = x[:3]
    want_p, want_l, want_m = _native_route(native, x, mode, value)
    assert np.array_equal(model.predict(x, pad_mode=mode, pad_value=value), want_p)
    labels, maps = model.predict_labels(x, want_maps=True, pad_mode=mode, pad_value=value)
    assert labels.shape == (3, 37, 70) and np.array_equal(labels, want_l) and np.array_equal(maps, want_m)
    _, soft = model.predict_labels(x, want_maps=True, soft_maps=True, pad_mode=mode, pad_value=value)
    assert np.array_equal(soft, _native_route(native, x, mode, value, soft=True)[2])
    # float input of predict: the constant is in the units of x
    xf = x.astype(np.float32) / np.float32(255.0)
    pf, _ = native.forward(_up(pad_reference(xf, 40, 72, 1, 1, mode, value)), training=False)
    assert np.array_equal(model.predict(xf, pad_mode=mode, pad_value=value), crop_reference(pf.cpu().numpy(), 37, 70, 1, 1))
    # Monte-Carlo dropout, T = 2: predict_mc pads by the model's attributes
    mc = native.forward_mc(_up(pad_reference(x, 40, 72, 1, 1, mode, value)), 2, step0=3, want_mean_probs=True)
    want = [crop_reference(mc[k].cpu().numpy(), 37, 70, 1, 1) for k in ("mean_probs", "entropy", "mutual_info")]
    model.pad_mode, model.pad_value = mode, value
    try:
        got = model.predict_mc(x, 2, step0=3)
        got_l = model.predict_labels(x, mc_samples=2, mc_step0=3)
    finally:
        model.pad_mode, model.pad_value = None, 0
    assert all(g.shape == w.shape and np.array_equal(g, w) for g, w in zip(got, want))
    assert np.array_equal(got_l[0], crop_reference(mc["argmax"].cpu().numpy(), 37, 70, 1, 1)) and np.array_equal(got_l[1], want[1])


def test_a_size_that_is_no_multiple_is_refused_without_pad_mode(padded_case):
    from oct_image_segmentation_models_amd._hip import OctError
    from oct_image_segmentation_models_amd.evaluation.pipeline import InferenceRun
    model, _, x = padded_case
    for call in (lambda: model.predict(x), lambda: model.predict_labels(x), lambda: model.predict_mc(x, 2),
                 lambda: InferenceRun(model, x, 2, C3)):
        with pytest.raises(OctError) as e:
            call()
        assert "37x70" in str(e.value) and "multiple of 4" in str(e.value) and "pad_mode" in str(e.value)


# ---- 6. InferenceRun: the graph replayed with different inputs, a partial last batch ------------------------------------------------
@pytest.mark.parametrize("soft", [False, True], ids=["binary", "soft"])
def test_inference_run_pads_inside_the_graph(padded_case, soft):
    from oct_image_segmentation_models_amd.evaluation.pipeline import InferenceRun
    model, native, x = padded_case
    _, want_l, want_m = _native_route(native, x, "edge", 0, soft=soft)
    for _ in range(2):
        seen = []
        with InferenceRun(model, x, 2, C3, pad_mode="edge", soft_maps=soft) as run:
            for b in run:
                seen.append((b.lo, b.hi))
                assert b.labels.shape == (b.hi - b.lo, 37, 70) and b.maps.shape == (b.hi - b.lo, C3 - 1, 37, 70)
                assert np.array_equal(b.labels, want_l[b.lo:b.hi]) and np.array_equal(b.maps, want_m[b.lo:b.hi]), b.lo
        assert seen == [(0, 2), (2, 4), (4, 5)]
    # float images take host_batches -> Model.predict_labels: the same labels (x / 255 on the host is the device's division)
    with InferenceRun(model, x.astype(np.float32), 2, C3, pad_mode="edge", soft_maps=soft) as run:
        for b in run:
            assert b.labels.shape == (b.hi - b.lo, 37, 70) and b.maps.shape == (b.hi - b.lo, C3 - 1, 37, 70)


def test_inference_run_pads_a_monte_carlo_batch(padded_case):
    from oct_image_segmentation_models_amd.evaluation.pipeline import InferenceRun
    model, _, x = padded_case
    x = x[:4]                      # whole batches: an image's dropout stream depends on its position in its batch
    want = model.predict_labels(x, batch_size=2, want_maps=True, mc_samples=2, mc_step0=1, pad_mode="edge")
    with InferenceRun(model, x, 2, C3, pad_mode="edge", mc_samples=2, mc_step0=1) as run:
        for b in run:
            for got, w in zip((b.labels, b.maps, b.entropy, b.mutual_info), want):
                assert got.shape == w[b.lo:b.hi].shape and np.array_equal(got, w[b.lo:b.hi]), b.lo


# ---- 7. evaluate_model and predict end to end ------------------------------------------------------------------------------------------
def _save_model(folder: Path, cfg, weights):
    from oct_image_segmentation_models_amd.models.engine_model import Model
    folder.mkdir(parents=True)
    m = Model(name="unet", config=dict(cfg, seed=2))
    m.set_weights(weights)
    m.save(folder / "model.npz")
    with open(folder / "model_config.json", "w") as fh:
        json.dump(cfg, fh)
    return folder / "model.npz"


def _dataset(path: Path, n, H, W, seed):
    from oct_image_segmentation_models_amd.common import h5io
    images, labels = _scans(n, H, W, seed)
    h5io.save(path, {"test_images": images, "test_labels": labels,
                     "test_images_source": np.array([f"scan_{i}.tiff".encode() for i in range(n)])})
    return images


METRICS = ["dice_coef_classes", "dice_coef_macro", "dice_coef_micro", "average_surface_distance", "hausdorff_distance"]
VOLATILE = ("time", "timestamp", "model_filename", "test_dataset_path")


def _evaluate(model_path, data, out, **kw):
    from oct_image_segmentation_models_amd.evaluation import eval_model
    from oct_image_segmentation_models_amd.evaluation.evaluation_parameters import EvaluationParameters, EvaluationSaveParams
    ep = EvaluationParameters(model_path=model_path, mlflow_tracking_uri=None, mlflow_run_uuid=None, test_dataset_path=data,
                              save_foldername=out, save_params=EvaluationSaveParams(categorical_pred=True), graph_search=True,
                              metrics=METRICS, batch_size=2, gs_workers=1, **kw)
    return eval_model(ep)


def _predict(model_path, images, out, **kw):
    from oct_image_segmentation_models_amd.common.dataset import Dataset
    from oct_image_segmentation_models_amd.prediction import predict
    from oct_image_segmentation_models_amd.prediction.prediction_parameters import PredictionParams, PredictionSaveParams
    n = len(images)
    ds = Dataset(images, [Path(f"scan_{i}.tiff") for i in range(n)], [out / f"image_{i}" for i in range(n)])
    pp = PredictionParams(model_path=model_path, mlflow_tracking_uri=None, mlflow_run_uuid=None, dataset=ds, config_output_dir=out,
                          save_params=PredictionSaveParams(), graph_search=True, batch_size=2, gs_workers=1, **kw)
    return predict(pp)


def _same_tree(a: Path, b: Path):
    """Every file under ``a`` has a twin under ``b`` with the same content: bytes, or for HDF5 containers every dataset and
    attribute but the timings, the timestamp and the paths."""
    from oct_image_segmentation_models_amd.common import h5io
    fa, fb = (sorted(p.relative_to(r) for p in r.rglob("*") if p.is_file()) for r in (a, b))
    assert fa == fb and fa
    for rel in fa:
        if rel.suffix in (".hdf5", ".npz") or rel.name.endswith(".hdf5.npz"):
            x, y = h5io.load(a / rel), h5io.load(b / rel)
            assert sorted(x) == sorted(y), rel
            for k in x:
                if k.startswith("attr:") and any(v in k for v in VOLATILE):
                    continue
                u, v = np.asarray(x[k]), np.asarray(y[k])
                assert u.dtype == v.dtype and u.shape == v.shape and np.array_equal(u, v, equal_nan=u.dtype.kind == "f"), (rel, k)
        else:
            assert (a / rel).read_bytes() == (b / rel).read_bytes(), rel


def _png_size(path: Path):
    head = path.read_bytes()[:24]
    assert head[:8] == b"\x89PNG\r\n\x1a\n"
    return struct.unpack(">II", head[16:24])           # (width, height)


def test_workflows_follow_the_dataset_size(tmp_path):
    w = _weights(_cfg(32, 64), 5)
    small, native = _save_model(tmp_path / "m32", _cfg(32, 64), w), _save_model(tmp_path / "m40", _cfg(40, 72), w)
    images = _dataset(tmp_path / "data40.hdf5", 3, 40, 72, 51)
    _evaluate(small, tmp_path / "data40.hdf5", tmp_path / "e32")
    _evaluate(native, tmp_path / "data40.hdf5", tmp_path / "e40")
    _same_tree(tmp_path / "e32", tmp_path / "e40")
    _predict(small, images, tmp_path / "p32")
    _predict(native, images, tmp_path / "p40")
    _same_tree(tmp_path / "p32", tmp_path / "p40")


def test_workflows_pad_a_dataset_whose_size_is_no_multiple(tmp_path):
    from oct_image_segmentation_models_amd.common import h5io
    small = _save_model(tmp_path / "m32", _cfg(32, 64), _weights(_cfg(32, 64), 5))
    images = _dataset(tmp_path / "data37.hdf5", 3, 37, 70, 52)
    outs = _evaluate(small, tmp_path / "data37.hdf5", tmp_path / "e", pad_mode="edge", png_plots=True)
    pouts = _predict(small, images, tmp_path / "p", pad_mode="edge", png_plots=True)
    assert len(outs) == len(pouts) == 3
    model = _model(_cfg(32, 64))
    want = model.predict_labels(images, pad_mode="edge")
    for i, (o, p) in enumerate(zip(outs, pouts)):
        assert o.predicted_labels.shape == (37, 70) and np.array_equal(o.predicted_labels, want[i])
        assert np.array_equal(p.predicted_labels, want[i]) and o.boundary_maps.shape == (C3 - 1, 37, 70)
        assert o.gs_pred_segs.shape == (C3 - 1, 70) and np.array_equal(o.gs_pred_segs, p.gs_pred_segs)
        f = h5io.load(tmp_path / "e" / f"image_{i}" / "evaluation_results.hdf5")
        assert f["predicted_segmentation_map"].shape == (37, 70) and f["raw_image"].shape == (37, 70, 1)
        pngs = sorted((tmp_path / "e" / f"image_{i}").glob("*.png")) + sorted((tmp_path / "p" / f"image_{i}").glob("*.png"))
        assert len(pngs) >= 6 and all(_png_size(q) == (70, 37) for q in pngs), pngs
    assert bytes(h5io.load(tmp_path / "e" / "eval_params.hdf5")["attr:pad_mode"]).rstrip(b"\x00") == b"edge"
    assert bytes(h5io.load(tmp_path / "p" / "prediction_params.hdf5")["attr:pad_mode"]).rstrip(b"\x00") == b"edge"


def test_sizes_that_are_multiples_are_never_padded(tmp_path):
    """A config-geometry dataset with the new options at their defaults, and with ``pad_mode`` set: nothing is padded, so
    every result file is the same, and with the options unset the config files record nothing new."""
    from oct_image_segmentation_models_amd.common import h5io
    small = _save_model(tmp_path / "m32", _cfg(32, 64), _weights(_cfg(32, 64), 5))
    images = _dataset(tmp_path / "data32.hdf5", 3, 32, 64, 53)
    _evaluate(small, tmp_path / "data32.hdf5", tmp_path / "e0")
    _evaluate(small, tmp_path / "data32.hdf5", tmp_path / "e1", pad_mode="reflect")
    _predict(small, images, tmp_path / "p0")
    _predict(small, images, tmp_path / "p1", pad_mode="constant", pad_value=9)
    cfg0, cfg1 = h5io.load(tmp_path / "e0" / "eval_params.hdf5"), h5io.load(tmp_path / "e1" / "eval_params.hdf5")
    assert "attr:pad_mode" not in cfg0 and "attr:pad_value" not in cfg0 and "attr:pad_mode" in cfg1
    pc0 = h5io.load(tmp_path / "p0" / "prediction_params.hdf5")
    assert "attr:pad_mode" not in pc0 and "attr:pad_value" not in pc0
    for a, b, name in (("e0", "e1", "eval_params.hdf5"), ("p0", "p1", "prediction_params.hdf5")):
        (tmp_path / a / name).unlink(); (tmp_path / b / name).unlink()       # differ by the recorded option alone (above)
        _same_tree(tmp_path / a, tmp_path / b)


# ---- 9. UNetEngine.infer: the one chain -- every kind padded eagerly, eager against captured, the refusals -------------------------
INFER_KINDS = {"plain": {}, "mc": dict(mc=(2, 3)), "tta": dict(tta=("identity", "flip_both"))}
PAD_37x70 = (1, 1, "edge", 0)


def _kind_on_native(native, xp, kind):
    """The kind's maps of the native-size batch ``xp`` through the public calls of before ``infer``."""
    if kind == "mc":
        return native.forward_mc(xp, 2, step0=3, want_mean_probs=True)
    if kind == "tta":
        return native.forward_tta(xp, ("identity", "flip_both"), want_mean_probs=True)
    probs, am = native.forward(xp, training=False, want_probs=True, want_argmax=True)
    return dict(probs=probs, argmax=am)


@pytest.mark.parametrize("kind", list(INFER_KINDS))
def test_eager_padded_infer_equals_crop_of_the_kind_on_the_padded_batch(padded_case, kind):
    """The pad and the crops issued by the library outside a capture: every map ``infer(x, pad=...)`` returns is byte-equal to
    ``crop(<kind>(pad(x)))`` composed from the public pieces (``crop`` makes new tensors: the next call does not refill them)."""
    _, native, x = padded_case
    x = _up(x[:3])
    want = {k: native.crop(t, 37, 70, 1, 1) for k, t in _kind_on_native(native, native.pad(x, 40, 72, 1, 1, "edge"), kind).items()}
    got = native.infer(x, pad=PAD_37x70, want_probs=True, want_argmax=True, **INFER_KINDS[kind])
    assert set(got) == set(want) == ({"probs", "argmax"} if kind == "plain" else {"mean_probs", "argmax", "entropy", "mutual_info"})
    for k in want:
        assert got[k].shape == want[k].shape and got[k].shape[:3] == (3, 37, 70) and torch.equal(got[k], want[k]), k


@pytest.mark.parametrize("padded", [False, True], ids=["native", "padded"])
@pytest.mark.parametrize("kind", ["plain", "tta"])
def test_captured_infer_equals_eager_infer(padded_case, kind, padded):
    """Two replays of the captured chain, the fixed input refilled in place between them, against the eager chain.  The eager
    call may write the very buffers the graph refills: its maps are cloned and the buffers scrubbed before each replay."""
    _, native, x = padded_case
    pad = PAD_37x70 if padded else None
    batches = [_up(x[:3]), _up(x[2:5])] if padded else [_up(_scans(3, 40, 72, seed)[0]) for seed in (51, 52)]
    ask = dict(pad=pad, want_probs=True, want_argmax=True, **INFER_KINDS[kind])
    x_fix = torch.zeros_like(batches[0])
    outs = native.infer(x_fix, capture=True, **ask)
    for xb in batches:
        want = {k: t.clone() for k, t in native.infer(xb, **ask).items()}
        for t in outs.values():
            t.fill_(SENTINEL if t.dtype == torch.uint8 else -7.0)
        x_fix.copy_(xb)
        native.graph_launch()
        assert set(outs) == set(want)
        for k in want:
            assert torch.equal(outs[k], want[k]), k


def test_infer_refusals_leave_the_engine_usable(padded_case):
    from oct_image_segmentation_models_amd._hip import OctError
    _, native, x = padded_case
    xp = native.pad(_up(x[:3]), 40, 72, 1, 1, "edge")
    before = native.forward(xp, training=False)[0].clone()
    with pytest.raises(OctError, match="dropout step"):             # a Monte-Carlo chain is not captured, and says why
        native.infer(xp, mc=(2, 0), want_probs=True, want_argmax=True, capture=True)
    assert torch.equal(native.forward(xp, training=False)[0], before)
    with pytest.raises(OctError, match="mc and tta"):
        native.infer(xp, mc=(2, 0), tta=("identity",), want_probs=True, want_argmax=True)
    assert torch.equal(native.forward(xp, training=False)[0], before)
