"""GPU tests of ``oct_warp_batch`` (include/oct_unet.h) and of the training path that uses it, against the numpy
restatement ``common.augmentation.warp_reference``.  The definition is integer arithmetic: every comparison is byte for
byte, images and labels."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest
import torch

from oct_image_segmentation_models_amd.common import augmentation as A

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
# (1,17,65,1): guarded stores, odd rows; (4,64,128,1): packed stores and the shared-shift 4-byte load
SHAPES = [(3, 6, 10, 1), (2, 16, 32, 3), (1, 1, 1, 1), (2, 5, 7, 2), (1, 17, 65, 1), (4, 64, 128, 1)]


@pytest.fixture(scope="module")
def eng():
    from oct_image_segmentation_models_amd.engine import UNetEngine
    return UNetEngine(device="cuda:0", input_channels=1, num_classes=3, image_height=16, image_width=32, start_neurons=8,
                      pool_layers=2, max_batch=1, training=False)


def _batch(shape, seed=0):
    rng = np.random.default_rng(seed)
    B, H, W, _ = shape
    return rng.integers(0, 256, shape, dtype=np.uint8), rng.integers(0, 4, (B, H, W), dtype=np.uint8)


def _rotation(deg, scale=1.0, d=(0.0, 0.0)):
    th = np.radians(deg)
    m = np.array([[np.cos(th), np.sin(th)], [-np.sin(th), np.cos(th)]]) / scale
    t = -m @ (2.0 * np.asarray(d))
    return [int(v) for v in np.rint(65536.0 * np.array([m[0, 0], m[0, 1], m[1, 0], m[1, 1], t[0], t[1]]))]


def _params(H, W):
    """Parameter sets per kind: shifts inside and beyond H in both directions with tilt and sag (a flat one takes the
    shared-shift load), rotations and zooms that put taps outside the image on all four sides, sub-pixel translations."""
    shifts = [[256 * 3, 0, 0], [-256 * (H + 2) - 77, 0, 0], [256 * (2 * H + 1) + 130, 300 * W, -170 * W], [100, -256 * 5, 256 * 4],
              [A.WARP_MAX_SHIFT, -A.WARP_MAX_SHIFT, A.WARP_MAX_SHIFT]]
    affines = [_rotation(30.0, 0.7, (1.3, -0.6)), _rotation(-100.0, 1.3, (-0.4, 2.2)), _rotation(180.0), _rotation(0.0, 0.25),
               _rotation(7.0, 1.0, (W + 3.5, -H - 1.25)), [65536, 0, 0, 65536, 0, 0]]
    return shifts, affines


def _all_ops(B, H, W, which):
    """B descriptors: sample b takes combination ``which + b`` of kind x border x parameter set."""
    shifts, affines = _params(H, W)
    combos = [(0, bd, [0] * 6) for bd in range(3)]
    combos += [(1, bd, p + [0, 0, 0]) for p in shifts for bd in range(3)] + [(2, bd, p) for p in affines for bd in range(3)]
    ops = np.zeros(B, dtype=A.WARP_OP_DTYPE)
    for b in range(B):
        kind, border, p = combos[(which + b) % len(combos)]
        ops[b]["kind"], ops[b]["border"], ops[b]["p"] = kind, border, p
        ops[b]["fill"], ops[b]["fill_label"] = 37 + b, 5 + b
    return ops, len(combos)


def _run(eng, x, lab, ops):
    xo, lo = eng.warp(torch.from_numpy(x).cuda(), None if lab is None else torch.from_numpy(lab).cuda(), ops)
    torch.cuda.synchronize()
    return xo.cpu().numpy(), None if lo is None else lo.cpu().numpy()


@pytest.mark.parametrize("shape", SHAPES)
def test_kernel_equals_the_restatement(eng, shape):
    """Every kind x every border x every parameter set, mixed inside the batches; with labels, and once without."""
    B, H, W, _ = shape
    x, lab = _batch(shape, seed=1)
    n_combos = _all_ops(B, H, W, 0)[1]
    for which in range(0, n_combos, B):
        ops, _ = _all_ops(B, H, W, which)
        ref_x, ref_l = A.warp_reference(x, lab, ops)
        out_x, out_l = _run(eng, x, lab, ops)
        assert out_x.dtype == np.uint8 and np.array_equal(out_x, ref_x), (which, ops)
        assert out_l.dtype == np.uint8 and np.array_equal(out_l, ref_l), (which, ops)
        if which == 0:      # without labels nothing but the images is written
            only_x, none = _run(eng, x, None, ops)
            assert none is None and np.array_equal(only_x, ref_x)


def test_every_kind_and_border_in_one_batch(eng):
    """(9, 12, 20, 1): kinds 0, 1, 2 x borders 0, 1, 2 side by side; each warp moved pixels, and the constant border wrote
    its fill values."""
    shape = (9, 12, 20, 1)
    x, lab = _batch(shape, seed=2)
    ops = np.zeros(9, dtype=A.WARP_OP_DTYPE)
    for b in range(9):
        ops[b]["kind"], ops[b]["border"] = b // 3, b % 3
        ops[b]["p"] = [0] * 6 if b < 3 else ([256 * 4 + 9, 700, -500, 0, 0, 0] if b < 6 else _rotation(40.0, 0.8, (2.5, 1.5)))
        ops[b]["fill"], ops[b]["fill_label"] = 255, 7
    ref_x, ref_l = A.warp_reference(x, lab, ops)
    out_x, out_l = _run(eng, x, lab, ops)
    assert np.array_equal(out_x, ref_x) and np.array_equal(out_l, ref_l)
    for b in range(9):
        assert np.array_equal(out_x[b], x[b]) == (b < 3) and np.array_equal(out_l[b], lab[b]) == (b < 3)
    assert (out_l[5] == 7).any() and (out_l[8] == 7).any() and not (out_l[:5] == 7).any() and not (out_l[6:8] == 7).any()


def test_unaligned_views_take_the_guarded_path(eng):
    """The same bytes from views offset by one byte (inputs, outputs, each alone and all together)."""
    shape = (2, 16, 32, 1)
    B, H, W, Cn = shape
    n = B * H * W
    x, lab = _batch(shape, seed=3)
    ops, _ = _all_ops(B, H, W, 4)
    ref_x, ref_l = A.warp_reference(x, lab, ops)
    for off in [(0, 0, 0, 0), (1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1), (1, 1, 1, 1)]:
        bufs = [torch.zeros(n + 4, dtype=torch.uint8, device="cuda") for _ in range(4)]
        xv, lv, xo, lo = (b[o:o + n] for b, o in zip(bufs, off))
        xv.copy_(torch.from_numpy(x.reshape(-1))); lv.copy_(torch.from_numpy(lab.reshape(-1)))
        eng.warp(xv.view(shape), lv.view(B, H, W), ops, out=(xo.view(shape), lo.view(B, H, W)))
        torch.cuda.synchronize()
        assert np.array_equal(xo.cpu().numpy().reshape(shape), ref_x), off
        assert np.array_equal(lo.cpu().numpy().reshape(B, H, W), ref_l), off
        for b, o in zip(bufs[2:], off[2:]):     # nothing written outside the views
            assert not b[:o].any() and not b[o + n:].any()


def test_determinism_and_batch_position(eng):
    shape = (8, 24, 40, 1)
    x, lab = _batch(shape, seed=4)
    ops, _ = _all_ops(8, 24, 40, 5)
    a = _run(eng, x, lab, ops)
    b = _run(eng, x, lab, ops)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    one = _run(eng, x[6:7], lab[6:7], ops[6:7])
    assert np.array_equal(one[0][0], a[0][6]) and np.array_equal(one[1][0], a[1][6])
    moved = _run(eng, x[[6, 0, 3]], lab[[6, 0, 3]], ops[[6, 0, 3]].copy())
    for k, src in enumerate([6, 0, 3]):
        assert np.array_equal(moved[0][k], a[0][src]) and np.array_equal(moved[1][k], a[1][src])


def test_argument_errors_launch_nothing(eng):
    from oct_image_segmentation_models_amd import _hip
    from oct_image_segmentation_models_amd._hip import OctError
    lib = _hip.lib()
    B, H, W, Cn = 2, 8, 16, 1
    n = B * H * W * Cn
    x = torch.zeros(n, dtype=torch.uint8, device="cuda")
    lab = torch.zeros(B * H * W, dtype=torch.uint8, device="cuda")
    good = np.zeros(B, dtype=A.WARP_OP_DTYPE)
    good["kind"], good["border"] = [1, 2], [2, 2]
    good["p"][0, :3], good["p"][1] = [256 * 3, 0, 0], _rotation(20.0)
    good["fill"], good["fill_label"] = 9, 1
    ops = torch.from_numpy(good.view(np.uint8).copy()).cuda()
    arena = torch.full((4 * n,), 0x5A, dtype=torch.uint8, device="cuda")       # outputs with a sentinel
    out, lab_out = arena[:n], arena[n:2 * n]
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: None if t is None else t.data_ptr()

    def call(x_=x, lab_=lab, ops_=ops, dims=(B, H, W, Cn), out_=out, lab_out_=lab_out):
        return lib.oct_warp_batch(p(x_), p(lab_), p(ops_), *dims, p(out_), p(lab_out_), stream)

    bad = [dict(x_=None), dict(ops_=None), dict(out_=None), dict(dims=(0, H, W, Cn)), dict(dims=(B, -1, W, Cn)),
           dict(dims=(B, H, 0, Cn)), dict(dims=(B, H, W, 0)), dict(dims=(65536, H, W, Cn)), dict(dims=(1, 16385, 1, 1)),
           dict(dims=(1, 1, 16385, 1)), dict(dims=(1, 16384, 16384, 8)),
           dict(lab_=None),                                                                    # labels_out without labels
           dict(out_=arena[n - 4:2 * n - 4]),                                                   # out overlaps labels_out
           dict(x_=arena[:n]), dict(x_=arena[4:n + 4]), dict(lab_=arena[16:16 + n]), dict(x_=arena[n:2 * n]),
           dict(ops_=arena[2 * n - 8:])]
    for kw in bad:
        rc = call(**kw)
        assert rc < 0 and b"warp_batch" in lib.oct_last_error(), kw
    torch.cuda.synchronize()
    assert bool((arena == 0x5A).all())
    assert call() == 0
    torch.cuda.synchronize()
    assert not bool((arena[:n] == 0x5A).any()) and not bool((arena[n:2 * n] == 0x5A).any()) and bool((arena[2 * n:] == 0x5A).all())
    # the Python binding validates descriptors and sizes before upload, and its output tensors
    xv, lv = x.view(B, H, W, Cn), lab.view(B, H, W)
    for field, value, match in [("kind", 3, "kind"), ("border", 3, "border"), ("fill", 256, "fill"), ("fill_label", -1, "fill_label")]:
        wrong = good.copy()
        wrong[field][1] = value
        with pytest.raises(OctError, match=match):
            eng.warp(xv, lv, wrong)
    wrong = good.copy()
    wrong["p"][0, 1] = A.WARP_MAX_SHIFT + 1
    with pytest.raises(OctError, match="column shift"):
        eng.warp(xv, lv, wrong)
    wrong = good.copy()
    wrong["p"][1, 2] = -A.WARP_MAX_M - 1
    with pytest.raises(OctError, match="affine"):
        eng.warp(xv, lv, wrong)
    with pytest.raises(OctError, match="one WARP_OP_DTYPE"):
        eng.warp(xv, lv, good[:1])
    with pytest.raises(OctError, match="overlaps"):
        eng.warp(xv, lv, good, out=(xv, torch.empty_like(lv)))          # the stage cannot run in place
    with pytest.raises(OctError, match=r"out\[0\]"):
        eng.warp(xv, lv, good, out=(torch.empty(xv.shape, dtype=torch.float32, device="cuda"), torch.empty_like(lv)))


def _compiled_model(cfg, seed):
    from oct_image_segmentation_models_amd import optimizers
    from oct_image_segmentation_models_amd.common import custom_losses, custom_metrics
    from oct_image_segmentation_models_amd.models import get_model_class
    model = get_model_class("unet")(**cfg).build_model()
    model.config["seed"] = seed
    nc = cfg["num_classes"]
    loss = custom_losses.custom_loss_objects["dice_loss_macro"]["function"](num_classes=nc, is_y_true_sparse=True)
    metric = custom_metrics.training_monitor_metric_objects["dice_coef_macro"](True, nc)
    model.compile(optimizer=optimizers.Adam(learning_rate=2e-3), loss=loss, metrics=[metric])
    return model


FIT_CFG = dict(input_channels=1, num_classes=3, image_height=32, image_width=64, start_neurons=8, pool_layers=2)
WARPS = [(A.column_shift_aug, {"max_shift": 6, "max_tilt": 4, "max_curvature": 3}),
         (A.affine_aug, {"max_rotation": 15, "scale_range": (0.85, 1.2), "max_translate": (4, 2), "border": "constant", "fill": 0,
                         "fill_label": 0}),
         (A.flip_aug, {"flip_type": "left-right"}), (A.no_aug, {})]


@pytest.mark.parametrize("mode, probs, batch", [("all", (), 4), ("one", (0.4, 0.4, 0.1, 0.1), 3)])
def test_fit_with_warps_equals_the_host_path(mode, probs, batch):
    """2 epochs over 3 images (mode "all": x 4 augmentations, 3 steps of batch 4; mode "one": 1 step of batch 3): the device
    path feeds the network the bits the host path feeds it, so the parameters end bit-identical."""
    from oracle import unet_numpy as on
    from oct_image_segmentation_models_amd.common.data_generator import DataGenerator
    images, labels = on.synth_scans(3, 32, 64, 3, seed=5)
    got = []
    for device_aug in (False, True):
        model = _compiled_model(FIT_CFG, seed=3)
        gen = DataGenerator(images, labels, batch, WARPS, mode, probs, True, None, seed=8, device_aug=device_aug)
        assert gen.oct_device_aug == device_aug and len(gen) == (3 if mode == "all" else 1)
        hist = model.fit(x=gen, epochs=2, verbose=0)
        torch.cuda.synchronize()
        got.append((model.engine.params.cpu().numpy(), model.engine.state.cpu().numpy(), hist.history["loss"]))
        if device_aug:
            assert model.feed.warp_out is not None       # the warp stage ran
    assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1]) and got[0][2] == got[1][2]
    assert np.isfinite(got[0][0]).all() and len(got[0][2]) == 2


def test_train_model_end_to_end_with_affine_and_noise(tmp_path):
    from oct_image_segmentation_models_amd import optimizers
    from oct_image_segmentation_models_amd.common import h5io
    from oct_image_segmentation_models_amd.training.training import train_model
    from oct_image_segmentation_models_amd.training.training_parameters import TrainingParams
    tp = TrainingParams(model_architecture="unet", training_dataset_path=ROOT / "tests" / "golden" / "dataset_small.hdf5",
                        initial_model=None, results_location=tmp_path / "results", opt_con=optimizers.Adam,
                        opt_params={"learning_rate": 4e-3}, loss="dice_loss_macro", metric="dice_coef_macro", epochs=2,
                        batch_size=2, model_hyperparameters={"pool_layers": 2}, seed=3,
                        augmentations=[{"name": "affine", "arguments": {"max_rotation": 10, "scale_range": (0.9, 1.1),
                                                                         "max_translate": (3, 3)}},
                                       {"name": "add_noise", "arguments": {"mode": "gaussian", "variance": 0.01}}],
                        aug_mode="one", aug_probs=(0.5, 0.5), aug_fly=True, aug_val=True, aug_device=True)
    res = train_model(tp, None)
    h = res.history
    assert set(h) == {"loss", "dice_coef_macro", "val_loss", "val_dice_coef_macro"}
    assert all(len(v) == 2 and np.isfinite(v).all() for v in h.values())
    attrs = h5io.load(Path(res.save_foldername) / "training_params.hdf5")
    text = lambda k: bytes(attrs[k]).rstrip(b"\x00").decode()
    assert bool(attrs["attr:aug_device"]) is True and text("attr:aug_mode") == "one"
    assert text("attr:aug_1") == "affine_aug" and float(attrs["attr:aug_1_param: max_rotation"]) == 10.0
    assert np.asarray(attrs["attr:aug_1_param: scale_range"]).tolist() == [0.9, 1.1]
