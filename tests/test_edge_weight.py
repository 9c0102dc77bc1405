"""CPU tests of the boundary-weighted pixel loss's host side: the numpy restatement
``edge_weight_reference`` of ``oct_edge_weight_map`` against a brute-force search and against scipy's exact Euclidean
distance transform, the LUT profiles, the spec check, the loss factories' ``edge_weight`` keyword, ``masked_loss_reference``'s
``pixel_weight`` and the attributes ``train_model`` records."""
import re
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent


def _mods():
    from oct_image_segmentation_models_amd.common import custom_losses, utils
    return utils, custom_losses


def layered(B, H, W, n_cls, seed, noise=0.01, frame=(2, 1, 3, 2)):
    """``n_cls`` layers with a wavy border, ``noise`` of the pixels relabelled at random, a 255 frame (top, bottom, left, right)."""
    rng = np.random.default_rng(seed)
    y, x = np.arange(H)[None, :, None], np.arange(W)[None, None, :]
    rows = y + 2.0 * np.sin(x / 5.0 + rng.uniform(0, 6.28, (B, 1, 1)))
    lab = np.clip(np.floor(rows * n_cls / H), 0, n_cls - 1).astype(np.uint8)
    flip = rng.random(lab.shape) < noise
    lab[flip] = rng.integers(0, n_cls, int(flip.sum()))
    t, b, l, r = frame
    lab[:, :t] = 255; lab[:, H - b:] = 255; lab[:, :, :l] = 255; lab[:, :, W - r:] = 255
    return lab


def edge_set(lab, n_cls):
    """By the definition, pixel by pixel."""
    H, W = lab.shape
    L = lab.astype(int)
    e = np.zeros((H, W), bool)
    for y in range(H):
        for x in range(W):
            if L[y, x] >= n_cls:
                continue
            for yy, xx in ((y - 1, x), (y + 1, x), (y, x - 1), (y, x + 1)):
                if 0 <= yy < H and 0 <= xx < W and L[yy, xx] < n_cls and L[yy, xx] != L[y, x]:
                    e[y, x] = True
    return e


def brute_index(labels, n_cls, R):
    out = np.zeros(labels.shape, np.int64)
    for b, lab in enumerate(labels):
        ys, xs = np.nonzero(edge_set(lab, n_cls))
        for y in range(lab.shape[0]):
            for x in range(lab.shape[1]):
                d = int(((ys - y) ** 2 + (xs - x) ** 2).min()) if len(ys) else 1 << 30
                out[b, y, x] = -1 if lab[y, x] >= n_cls else d if d <= R * R else R * R + 1
    return out


CASES = [(16, 16, 3, 32), (20, 34, 4, 3), (36, 68, 3, 7), (24, 40, 2, 1)]


@pytest.mark.parametrize("H, W, n_cls, R", CASES)
def test_reference_equals_brute_force_and_scipy(H, W, n_cls, R):
    utils, _ = _mods()
    labels = layered(2, H, W, n_cls, seed=H + R)
    idx = utils.edge_index_reference(labels, n_cls, R)
    assert np.array_equal(idx, brute_index(labels, n_cls, R))
    assert (idx == 0).any() and (idx == -1).any() and ((idx > 0) & (idx <= R * R)).any()
    assert np.array_equal(idx, utils.edge_index_reference(labels[..., None], n_cls, R))
    ndimage = pytest.importorskip("scipy.ndimage")
    for b in range(2):
        e = edge_set(labels[b], n_cls)
        d2 = np.rint(ndimage.distance_transform_edt(~e) ** 2).astype(np.int64)
        want = np.where(labels[b] >= n_cls, -1, np.where(d2 <= R * R, d2, R * R + 1))
        assert np.array_equal(idx[b], want)
    lut = utils.edge_weight_lut(R, "linear", 3.0)
    w = utils.edge_weight_reference(labels, n_cls, R, lut)
    assert w.dtype == np.float32 and (w[labels == 255] == 0).all() and np.array_equal(w[idx >= 0], lut[idx[idx >= 0]])


def test_reference_edge_cases():
    utils, _ = _mods()
    one = np.full((1, 9, 11), 1, np.uint8)
    assert (utils.edge_index_reference(one, 3, 2) == 5).all()                     # one class: all far
    yy, xx = np.mgrid[0:9, 0:11]
    assert (utils.edge_index_reference(((yy + xx) % 2).astype(np.uint8)[None], 2, 2) == 0).all()
    assert (utils.edge_index_reference(np.full((1, 9, 11), 255, np.uint8), 3, 2) == -1).all()
    two = np.zeros((1, 5, 8), np.uint8); two[0, :, 4:] = 3                       # 3 is a class of n_cls 4, unknown at n_cls 3
    assert (utils.edge_index_reference(two, 4, 1)[0, :, 3:5] == 0).all()
    assert set(np.unique(utils.edge_index_reference(two, 3, 1))) == {-1, 2}      # a border against unknown pixels is none
    with pytest.raises(ValueError):
        utils.edge_index_reference(two.astype(np.int32), 3, 1)
    with pytest.raises(ValueError):
        utils.edge_index_reference(two, 3, 33)
    with pytest.raises(ValueError):
        utils.edge_weight_reference(two, 3, 2, np.ones(5, np.float32))


def test_lut_profiles():
    utils, _ = _mods()
    for R in (1, 3, 32):
        d = np.sqrt(np.arange(R * R + 1, dtype=np.float64))
        box, gauss, lin = (utils.edge_weight_lut(R, p, 10.0, s) for p, s in (("box", None), ("gauss", 2.5), ("linear", None)))
        for t in (box, gauss, lin):
            assert t.dtype == np.float32 and t.shape == (R * R + 2,) and t[-1] == 1.0          # the far entry
        assert (box[:-1] == np.float32(11.0)).all()
        assert np.array_equal(gauss[:-1], (1.0 + 10.0 * np.exp(-d * d / (2 * 2.5 ** 2))).astype(np.float32))
        assert np.array_equal(lin[:-1], (1.0 + 10.0 * (1.0 - d / (R + 1.0))).astype(np.float32))
        assert gauss[0] == 11.0 and lin[0] == 11.0 and (np.diff(lin[:-1]) < 0).all() and lin[-2] > 1.0
    assert np.array_equal(utils.edge_weight_lut(4, "gauss", 2.0), utils.edge_weight_lut(4, "gauss", 2.0, 2.0))   # sigma defaults to R / 2
    assert (utils.edge_weight_lut(3, "box", 0.0) == 1.0).all()


def test_check_edge_weight():
    utils, _ = _mods()
    ok = utils.check_edge_weight({"radius": 3, "weight": 10})
    assert ok == {"radius": 3, "weight": 10.0, "profile": "box", "sigma": None}
    assert utils.check_edge_weight({"radius": 32, "weight": 0, "profile": "gauss", "sigma": 5})["sigma"] == 5.0
    for bad in ({"radius": 0, "weight": 1}, {"radius": 33, "weight": 1}, {"radius": 2.5, "weight": 1}, {"radius": True, "weight": 1},
                {"radius": 3, "weight": -1}, {"radius": 3, "weight": float("inf")}, {"radius": 3, "weight": float("nan")},
                {"radius": 3, "weight": 1, "profile": "gauss", "sigma": 0}, {"radius": 3, "weight": 1, "profile": "gauss", "sigma": -2},
                {"radius": 3, "weight": 1, "profile": "cone"}, {"radius": 3, "weight": 1, "omega": 2}, {"radius": 3}, {"weight": 1},
                {"radius": 3, "weight": 1, "profile": "box", "sigma": 2}, "box", None):
        with pytest.raises(ValueError):
            utils.check_edge_weight(bad)


def test_factories_tag_and_refuse():
    utils, cl = _mods()
    spec = {"radius": 2, "weight": 4.0, "profile": "linear"}
    for name in ("focal_dice_loss", "bce_dice_loss"):
        fac = cl.custom_loss_objects[name]["function"]
        fn = fac(num_classes=3, is_y_true_sparse=True, edge_weight=spec)
        assert fn.oct_loss == name and fn.oct_edge_weight == utils.check_edge_weight(spec)
        assert fac(num_classes=3, is_y_true_sparse=True).oct_edge_weight is None
        with pytest.raises(ValueError):
            fac(num_classes=3, is_y_true_sparse=True, edge_weight={"radius": 99, "weight": 1})
    for name in ("dice_loss_macro", "dice_loss_micro"):
        fac = cl.custom_loss_objects[name]["function"]
        with pytest.raises(ValueError, match="edge_weight"):
            fac(num_classes=3, is_y_true_sparse=True, edge_weight=spec)
        assert fac(num_classes=3, is_y_true_sparse=True, edge_weight=None).oct_loss == name
    assert set(cl.custom_loss_objects) == {"bce_dice_loss", "dice_loss_micro", "dice_loss_macro", "focal_loss", "bce_focal_loss",
                                           "focal_dice_loss"}         # no new registry name


def _probs(labels, C, seed):
    rng = np.random.default_rng(seed)
    z = rng.normal(0, 1, labels.shape + (C,)) + 2.0 * np.eye(C)[np.minimum(labels, C - 1)]
    e = np.exp(z - z.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def test_numpy_callables_apply_the_weights():
    utils, cl = _mods()
    labels = layered(2, 20, 34, 3, seed=4, frame=(0, 0, 0, 0))
    p = _probs(labels, 3, 5)
    spec = {"radius": 2, "weight": 4.0, "profile": "linear", "sigma": None}
    w = utils.edge_weight_reference(labels, 3, 2, utils.edge_weight_lut(2, "linear", 4.0)).astype(np.float64)
    assert w.min() == 1.0 and w.max() == 5.0
    for name, kind, kw in (("focal_dice_loss", "focal", dict(dice_macro=False)), ("bce_dice_loss", "bce", {})):
        fac = cl.custom_loss_objects[name]["function"]
        got = fac(num_classes=3, is_y_true_sparse=True, edge_weight=spec, **kw)(labels, p)
        want = cl.masked_loss_reference(labels, p, 3, None, kind, pixel_weight=w)["loss_micro"]
        plain = fac(num_classes=3, is_y_true_sparse=True, **kw)(labels, p)
        assert abs(got - want) < 1e-12 and got > plain + 1e-3
    dense = np.eye(3)[labels]                                       # bce_dice_loss also takes the one-hot the reference feeds it
    fac = cl.custom_loss_objects["bce_dice_loss"]["function"]
    assert abs(fac(num_classes=3, edge_weight=spec)(dense, p) - fac(num_classes=3, edge_weight=spec)(labels, p)) < 1e-12


@pytest.mark.parametrize("ignore", [None, 255])
@pytest.mark.parametrize("kind", ["dice", "focal", "bce"])
def test_masked_reference_with_ones_is_exact_and_with_twos_doubles(kind, ignore):
    _, cl = _mods()
    labels = layered(2, 20, 34, 3, seed=6)
    if ignore is None:
        labels = np.minimum(labels, 2)
    p = _probs(labels, 3, 7)
    kw = dict(class_weight=[0.5, 1.0, 2.0]) if kind == "focal" else {}
    off = cl.masked_loss_reference(labels, p, 3, ignore, kind, **kw)
    one = cl.masked_loss_reference(labels, p, 3, ignore, kind, pixel_weight=np.ones(labels.shape), **kw)
    assert off == one or all(a == b or (a != a and b != b) for a, b in zip(off.values(), one.values()))
    two = cl.masked_loss_reference(labels, p, 3, ignore, kind, pixel_weight=np.full(labels.shape + (1,), 2.0), **kw)
    assert two["term"] == 2.0 * off["term"]
    for k in ("dice_loss_macro", "dice_loss_micro", "dice_coef_macro", "dice_coef_micro"):
        assert two[k] == off[k]                                     # the Dice term and the metrics never see the map


def test_header_binding_and_kernel_agree():
    hdr = (ROOT / "include" / "oct_unet.h").read_text()
    from oct_image_segmentation_models_amd import _hip
    bound = {n: (r, a) for n, r, a in _hip.SYMBOLS}
    m = re.search(r"\bint\s+oct_edge_weight_map\s*\(([^)]*)\)\s*;", hdr)
    assert m and len(m.group(1).split(",")) == 9 == len(bound["oct_edge_weight_map"][1])
    m = re.search(r"\bint\s+oct_unet_set_pixel_weights\s*\(([^)]*)\)\s*;", hdr)
    assert m and len(m.group(1).split(",")) == 2 == len(bound["oct_unet_set_pixel_weights"][1])
    assert "does NOT divide by the sum of the weights" in hdr
    utils, _ = _mods()
    assert int(re.search(r"#define\s+OCT_EDGE_WEIGHT_MAX_RADIUS\s+(\d+)", hdr).group(1)) == utils.EDGE_WEIGHT_MAX_RADIUS
    k = (ROOT / "oct-image-segmentation-models_amd" / "csrc" / "kernels_edge_weight.hpp").read_text()
    assert re.search(r"EW_TH = 32, EW_TW = 64, EW_MAX_R = 32", k)  # the tile tests/test_gpu_edge_weight.py names


def test_training_params_attributes_round_trip(tmp_path):
    """``save_training_params_file`` writes ``edge_weight_param: <key>`` only when the keyword was given: a run without it
    writes the file it always wrote."""
    from oct_image_segmentation_models_amd import optimizers
    from oct_image_segmentation_models_amd.common import h5io
    from oct_image_segmentation_models_amd.common import custom_losses as cl
    from oct_image_segmentation_models_amd.training import training
    from oct_image_segmentation_models_amd.training.training_parameters import TrainingParams
    spec = {"radius": 3, "weight": 10.0, "profile": "gauss", "sigma": 1.5}
    files = {}
    for tag, kwargs in (("plain", {}), ("edge", {"edge_weight": spec})):
        tp = TrainingParams(model_architecture="unet", training_dataset_path=tmp_path / "data.hdf5", initial_model=None,
                            results_location=tmp_path / "results", opt_con=optimizers.Adam, opt_params={"learning_rate": 1e-3},
                            loss="focal_dice_loss", metric="dice_coef_macro", epochs=1, batch_size=2, loss_fn_kwargs=kwargs)
        loss_fn = cl.custom_loss_objects[tp.loss]["function"](num_classes=3, is_y_true_sparse=True, **training.loss_factory_kwargs(tp, None))
        tp.edge_weight_kwargs = getattr(loss_fn, "oct_edge_weight", None)
        out = tmp_path / tag
        out.mkdir()
        training.save_training_params_file(out, "summary", {"num_classes": 3}, "md5", None, "ts", tp, optimizers.Adam(learning_rate=1e-3))
        files[tag] = h5io.load(out / "training_params.hdf5")
    attrs = {tag: {k[len("attr:"):]: v for k, v in f.items() if k.startswith("attr:")} for tag, f in files.items()}
    edge_keys = {k for k in attrs["edge"] if k.startswith("edge_weight_param: ")}
    assert edge_keys == {f"edge_weight_param: {k}" for k in spec}
    assert int(attrs["edge"]["edge_weight_param: radius"]) == 3 and float(attrs["edge"]["edge_weight_param: weight"]) == 10.0
    assert float(attrs["edge"]["edge_weight_param: sigma"]) == 1.5
    prof = attrs["edge"]["edge_weight_param: profile"][()]
    assert (prof.decode() if isinstance(prof, bytes) else str(prof)) == "gauss"
    assert not [k for k in attrs["plain"] if "edge_weight" in str(k)]
    assert set(attrs["edge"]) - edge_keys == set(attrs["plain"])
