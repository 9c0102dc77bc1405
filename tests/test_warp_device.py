"""CPU tests of the geometric augmentations' host side: the numpy restatement ``warp_reference`` of ``oct_warp_batch``
(include/oct_unet.h) against independent statements of the same definition (numpy's own flip and roll, a per-pixel Python
loop, exact rationals), the refusals, and the plumbing -- registry, descriptor templates, and the parameter stream that the
host path and the descriptor path of ``DataGenerator`` share.  No GPU, no library call.  Everything is integer arithmetic,
so every comparison is for equality."""
import itertools
from fractions import Fraction
from math import floor

import numpy as np
import pytest

from oct_image_segmentation_models_amd.common import augmentation as A
from oct_image_segmentation_models_amd.common.data_generator import DataGenerator


def _data(n=7, h=6, w=10, c=1, seed=0):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (n, h, w, c), dtype=np.uint8), rng.integers(0, 3, (n, h, w, 1), dtype=np.uint8)


def _op(kind=0, border=0, p=(0,) * 6, fill=0, fill_label=0):
    op = np.zeros(1, dtype=A.WARP_OP_DTYPE)
    op["kind"], op["border"], op["fill"], op["fill_label"] = kind, border, fill, fill_label
    op["p"][0, :len(p)] = p
    return op


def _ops(*ops):
    return np.concatenate(ops)


IDENTITY = (65536, 0, 0, 65536, 0, 0)


def test_descriptor_layout():
    assert A.WARP_OP_DTYPE.itemsize == 40
    offsets = {k: A.WARP_OP_DTYPE.fields[k][1] for k in A.WARP_OP_DTYPE.names}
    assert offsets == {"kind": 0, "border": 4, "p": 8, "fill": 32, "fill_label": 36}
    assert (A.WARP_NONE, A.WARP_COLUMN_SHIFT, A.WARP_AFFINE) == (0, 1, 2)
    assert A.WARP_BORDERS == {"replicate": 0, "wrap": 1, "constant": 2}


@pytest.mark.parametrize("border", [0, 1, 2])
def test_identity_and_flip_of_both_axes(border):
    x, lab = _data(n=2, h=6, w=10, c=3, seed=1)
    ops = _ops(_op(2, border, IDENTITY, fill=7, fill_label=2), _op(2, border, (-65536, 0, 0, -65536, 0, 0), fill=7, fill_label=2))
    out, lo = A.warp_reference(x, lab, ops)
    assert out.dtype == np.uint8 and lo.dtype == np.uint8 and lo.shape == lab.shape
    assert np.array_equal(out[0], x[0]) and np.array_equal(lo[0], lab[0])
    assert np.array_equal(out[1], np.flip(x[1], axis=(0, 1))) and np.array_equal(lo[1], np.flip(lab[1], axis=(0, 1)))
    # kind 0 copies; without labels none come back
    none, no_labels = A.warp_reference(x, None, _ops(_op(0, border), _op(0, border)))
    assert np.array_equal(none, x) and no_labels is None


@pytest.mark.parametrize("k", [0, 1, 3, -2, 6, 13, -17])
def test_column_shift_with_wrap_is_np_roll(k):
    x, lab = _data(n=1, h=6, w=10, c=2, seed=2)
    out, lo = A.warp_reference(x, lab[..., 0], _op(1, 1, (256 * k, 0, 0)))
    assert np.array_equal(out[0], np.roll(x[0], k, axis=0)) and np.array_equal(lo[0], np.roll(lab[0, ..., 0], k, axis=0))


def _src(i, n, border):
    """The border rule for one index, written out: the source index or None for a tap that reads the fill value."""
    if border == 0:
        return min(max(i, 0), n - 1)
    if border == 1:
        return i % n
    return i if 0 <= i < n else None


def _loop_reference(img, lab, op):
    """The definition of include/oct_unet.h pixel by pixel in Python integers (arbitrary precision, floor division)."""
    H, W, C = img.shape
    kind, border, fill, fill_label = (int(op[k]) for k in ("kind", "border", "fill", "fill_label"))
    p = [int(v) for v in op["p"]]
    out, lo = np.zeros_like(img), np.zeros_like(lab)
    D = max(W - 1, 1)
    for y, x in itertools.product(range(H), range(W)):
        if kind == 1:
            t = 2 * x - (W - 1)
            s = (p[0] * D * D + p[1] * t * D + p[2] * t * t + 128 * D * D) // (256 * D * D)
            sy = _src(y - s, H, border)
            out[y, x] = fill if sy is None else img[sy, x]
            lo[y, x] = fill_label if sy is None else lab[sy, x]
            continue
        X, Y = 2 * x - (W - 1), 2 * y - (H - 1)
        sx = (p[0] * X + p[1] * Y + p[4] + (W - 1) * 65536) >> 1
        sy = (p[2] * X + p[3] * Y + p[5] + (H - 1) * 65536) >> 1
        ix, fx, iy, fy = sx >> 16, (sx >> 8) & 255, sy >> 16, (sy >> 8) & 255
        for c in range(C):
            acc = 0
            for dy, wy in ((0, 256 - fy), (1, fy)):
                for dx, wx in ((0, 256 - fx), (1, fx)):
                    yy, xx = _src(iy + dy, H, border), _src(ix + dx, W, border)
                    acc += wx * wy * (fill if yy is None or xx is None else int(img[yy, xx, c]))
            out[y, x, c] = (acc + 32768) >> 16
        yy, xx = _src((sy + 32768) >> 16, H, border), _src((sx + 32768) >> 16, W, border)
        lo[y, x] = fill_label if yy is None or xx is None else lab[yy, xx]
    return out, lo


def _rotation(deg, scale=1.0, d=(0.0, 0.0)):
    th = np.radians(deg)
    m = np.array([[np.cos(th), np.sin(th)], [-np.sin(th), np.cos(th)]]) / scale
    t = -m @ (2.0 * np.asarray(d))
    return tuple(int(v) for v in np.rint(65536.0 * np.array([m[0, 0], m[0, 1], m[1, 0], m[1, 1], t[0], t[1]])))


@pytest.mark.parametrize("border", [0, 1, 2])
def test_borders_against_a_per_pixel_loop(border):
    """5x7x2: shifts beyond H, a tilt and a sag, a rotation with taps outside on all four sides, a zoom-out."""
    x, lab = _data(n=1, h=5, w=7, c=2, seed=3)
    cases = [(1, (256 * 9 + 77, 700, -900)), (1, (-256 * 11, -1300, 500)), (2, _rotation(33.0, 0.8, (1.3, -0.7))),
             (2, _rotation(-75.0, 1.4, (-2.6, 1.1))), (2, _rotation(0.0, 0.3))]
    for kind, p in cases:
        op = _op(kind, border, p, fill=201, fill_label=9)
        want = _loop_reference(x[0], lab[0, ..., 0], op[0])
        got = A.warp_reference(x, lab, op)
        assert np.array_equal(got[0][0], want[0]) and np.array_equal(got[1][0, ..., 0], want[1]), (kind, p)
        if border == 2 and kind == 2:       # taps did fall outside
            assert (got[1] == 9).any()


@pytest.mark.parametrize("W", [1, 2, 7, 64, A.WARP_MAX_DIM])
def test_column_shifts_against_exact_rationals(W):
    M = A.WARP_MAX_SHIFT
    xs = range(W) if W <= 64 else [0, 1, W // 2 - 1, W // 2, W - 2, W - 1]
    for a, b, c in [(M, M, M), (-M, -M, -M), (M, -M, M), (-M, M, -M), (0, 0, 0), (127, 0, 0), (128, 0, 0), (-129, 0, 0),
                    (-128, 0, 0), (5, -1234567, 7654321)]:
        s = A.column_shifts(W, a, b, c)
        assert s.dtype == np.int64 and s.shape == (W,)
        D = max(W - 1, 1)
        for x in xs:
            t = Fraction(2 * x - (W - 1), D)        # -1..1 across the scan
            assert int(s[x]) == floor((a + b * t + c * t * t) / 256 + Fraction(1, 2)), (W, a, b, c, x)


def test_degenerate_sizes():
    for shape in [(2, 1, 9, 1), (2, 8, 1, 2), (1, 1, 1, 3)]:
        B, H, W, C = shape
        rng = np.random.default_rng(4)
        x, lab = rng.integers(0, 256, shape, dtype=np.uint8), rng.integers(0, 3, (B, H, W), dtype=np.uint8)
        for border in (0, 1, 2):
            ops = _ops(*[_op(1 + (b % 2), border, (300, 200, -100) if b % 2 == 0 else _rotation(20.0, 0.9, (0.4, 0.2)), 5, 1)
                         for b in range(B)])
            out, lo = A.warp_reference(x, lab, ops)
            for b in range(B):
                want = _loop_reference(x[b], lab[b], ops[b])
                assert np.array_equal(out[b], want[0]) and np.array_equal(lo[b], want[1])
        out, lo = A.warp_reference(x, lab, _ops(*[_op(2, 0, IDENTITY)] * B))
        assert np.array_equal(out, x) and np.array_equal(lo, lab)


def test_refusals():
    x, lab = _data(n=1)
    M, S = A.WARP_MAX_M, A.WARP_MAX_SHIFT
    bad = [_op(3), _op(-1), _op(1, 3), _op(1, -1), _op(1, 0, (S + 1, 0, 0)), _op(1, 0, (0, -S - 1, 0)), _op(1, 0, (0, 0, S + 1)),
           _op(2, 0, (M + 1, 0, 0, 65536, 0, 0)), _op(2, 0, (65536, 0, -M - 1, 65536, 0, 0)), _op(2, 2, IDENTITY, fill=256),
           _op(2, 2, IDENTITY, fill=-1), _op(2, 2, IDENTITY, fill_label=256)]
    for op in bad:
        with pytest.raises(ValueError):
            A.warp_reference(x, lab, op)
    # the extremes themselves are inside; the translation is any int32
    A.warp_reference(x, lab, _op(1, 1, (S, -S, S)))
    A.warp_reference(x, lab, _op(2, 2, (M, -M, M, -M, 2 ** 31 - 1, -2 ** 31), fill=255, fill_label=255))
    with pytest.raises(ValueError):
        A.check_warp_ops(_op(), A.WARP_MAX_DIM + 1, 8)
    with pytest.raises(ValueError):
        A.check_warp_ops(_op(), 8, 0)
    with pytest.raises(TypeError):
        A.check_warp_ops(np.zeros(1, dtype=A.AUG_OP_DTYPE), 8, 8)
    with pytest.raises(TypeError):
        A.warp_reference(x.astype(np.float32), None, _op())
    with pytest.raises(ValueError):
        A.warp_reference(x, None, _ops(_op(), _op()))          # one descriptor per sample
    bad_args = [(A.column_shift_aug, {"max_shift": -1}), (A.column_shift_aug, {"max_tilt": 1e6}),
                (A.column_shift_aug, {"border": "mirror"}), (A.column_shift_aug, {"max_rotation": 3}),
                (A.affine_aug, {"scale_range": (0.01, 1.0)}), (A.affine_aug, {"scale_range": (1.2, 0.8)}),
                (A.affine_aug, {"scale_range": 1.0}), (A.affine_aug, {"max_translate": (-1, 0)}),
                (A.affine_aug, {"max_translate": (40000, 0)}), (A.affine_aug, {"fill": 300}), (A.affine_aug, {"fill_label": 0.5}),
                (A.affine_aug, {"max_rotation": -5})]
    for entry in bad_args:
        with pytest.raises(ValueError):
            A.warp_ops_from([entry])
        assert A.aug_ops_from([entry]) is None
        with pytest.raises(ValueError):
            DataGenerator(x, lab, 1, [entry], "all", (), True, None, seed=1)


SHIFT = (A.column_shift_aug, {"max_shift": 3, "max_tilt": 2, "max_curvature": 1.5})
AFFINE = (A.affine_aug, {"max_rotation": 25, "scale_range": (0.8, 1.25), "max_translate": (2, 1), "border": "constant",
                         "fill": 9, "fill_label": 2})


def test_registry_and_descriptions():
    assert A.augmentation_map["column_shift"] is A.column_shift_aug and A.augmentation_map["affine"] is A.affine_aug
    assert A.column_shift_aug(None, None, SHIFT[1], True) == "column shift: " + str(SHIFT[1])
    assert A.affine_aug(None, None, AFFINE[1], True) == "affine: " + str(AFFINE[1])
    assert set(A.augmentation_map) == {"add_noise", "flip", "no_augmentation", "column_shift", "affine"}


def test_training_params_accept_the_new_names(tmp_path):
    from oct_image_segmentation_models_amd import optimizers
    from oct_image_segmentation_models_amd.training.training_parameters import TrainingParams
    kw = dict(model_architecture="unet", training_dataset_path=tmp_path / "d.hdf5", initial_model=None,
              results_location=tmp_path, opt_con=optimizers.Adam, loss="dice_loss_macro", metric="dice_coef_macro",
              epochs=1, batch_size=2, aug_mode="one", aug_probs=(0.5, 0.5))
    tp = TrainingParams(augmentations=[{"name": "column_shift", "arguments": SHIFT[1]}, {"name": "affine", "arguments": AFFINE[1]}],
                        **kw)
    assert tp.aug_fn_args == [SHIFT, AFFINE]
    with pytest.raises(SystemExit):
        TrainingParams(augmentations=[{"name": "column_shift"}, {"name": "shear"}], **kw)


def test_templates_of_mixed_lists():
    flips = [(A.flip_aug, {"flip_type": "up-down"}), (A.no_aug, {}), (A.flip_aug, {"flip_type": "left-right"})]
    noise = [(A.add_noise_aug, {"mode": "gaussian", "mean": 0.1, "variance": 0.04}), (A.add_noise_aug, {"mode": "speckle"}),
             (A.add_noise_aug, {"mode": "s&p", "amount": 0.1}), (A.add_noise_aug, {"mode": "salt"}), (A.add_noise_aug, {"mode": "pepper"})]
    # today's lists: no warp templates, and the descriptor templates tests/test_augment_device.py pins
    assert A.warp_ops_from(flips + noise) is None and A.warp_ops_from([]) is None
    ops = A.aug_ops_from(flips + noise)
    assert ops["kind"].tolist() == [1, 0, 2, 3, 4, 5, 5, 5]
    assert ops["p0"][3] == np.float32(0.1) and ops["p1"][3] == np.float32(0.2) and ops["p1"][4] == np.float32(0.1)
    assert ops["p0"][5:].tolist() == [np.float32(0.1), np.float32(0.05), np.float32(0.05)] and ops["p1"][5:].tolist() == [0.5, 1.0, 0.0]
    mixed = [flips[0], SHIFT, noise[0], AFFINE, (A.affine_aug, {})]
    w, a = A.warp_ops_from(mixed), A.aug_ops_from(mixed)
    assert w.dtype == A.WARP_OP_DTYPE and w["kind"].tolist() == [0, 1, 0, 2, 2] and a["kind"].tolist() == [1, 0, 3, 0, 0]
    assert w["border"].tolist() == [0, 1, 0, 2, 0] and w["fill"].tolist() == [0, 0, 0, 9, 0] and w["fill_label"].tolist() == [0, 0, 0, 2, 0]
    assert not w["p"].any()
    assert A.aug_ops_from([SHIFT, (lambda i, m, a: (i, m), {})]) is None


def test_parameter_draws():
    """Uniform within the ranges, rounded to the integer descriptor with rint in float64."""
    u = np.array([[0.0, 0.0, 0.0, 0.0], [0.5, 0.5, 0.5, 0.5], [0.999999, 0.25, 0.75, 0.125]])
    ops = A.draw_warp_ops([SHIFT, AFFINE], [0, 0, 0], u)
    assert ops["kind"].tolist() == [1, 1, 1] and ops["border"].tolist() == [1, 1, 1]
    assert ops["p"][0].tolist() == [-768, -512, -384, 0, 0, 0] and ops["p"][1].tolist() == [0] * 6
    assert ops["p"][2].tolist() == [int(np.rint(256 * 3 * (2 * 0.999999 - 1))), -256, 192, 0, 0, 0]
    ops = A.draw_warp_ops([SHIFT, AFFINE], [1, 1, 0], u)
    assert ops["kind"].tolist() == [2, 2, 1] and ops["fill"].tolist() == [9, 9, 0] and ops["fill_label"].tolist() == [2, 2, 0]
    assert ops["p"][1].tolist() == list(_rotation(0.0, 0.8 + 0.45 * 0.5))       # the middle of every range
    assert ops["p"][0].tolist() == list(_rotation(-25.0, 0.8, (-2.0, -1.0)))
    # a pure translation by d moves the content by +d: out[y, x] = in[y - dy, x - dx]
    x, lab = _data(n=1, h=6, w=10)
    shift = A.draw_warp_ops([(A.affine_aug, {"max_translate": (3, 2), "border": "wrap"})], [0], [[0.5, 0.5, 1.0, 1.0]])
    out, lo = A.warp_reference(x, lab, shift)
    assert np.array_equal(out[0], np.roll(x[0], (2, 3), axis=(0, 1))) and np.array_equal(lo[0], np.roll(lab[0], (2, 3), axis=(0, 1)))
    # a sample whose augmentation is no warp gets kind 0
    assert A.draw_warp_ops([SHIFT, (A.no_aug, {})], [1, 0], u[:2])["kind"].tolist() == [0, 1]


def test_host_functions_are_warp_reference():
    x, lab = _data(n=1, h=8, w=12, c=2, seed=6)
    onehot = np.eye(3, dtype=np.float64)[lab[0, ..., 0]]
    for fn, args in (SHIFT, AFFINE):
        op = A.draw_warp_ops([(fn, args)], [0], [[0.9, 0.2, 0.7, 0.4]])
        want_x, want_l = A.warp_reference(x, lab, op)
        got_x, got_l = fn(x[0], lab[0], dict(args, op=op))
        assert got_x.dtype == np.uint8 and np.array_equal(got_x, want_x[0]) and np.array_equal(got_l, want_l[0])
        assert not np.array_equal(got_x, x[0])
        # the generator's host path: float32(u8 / 255) in and out, one-hot masks moved with the fill class's row outside
        xf = x[0].astype(np.float32) / np.float32(255.0)
        got_f, got_h = fn(xf, onehot, dict(args, op=op))
        assert got_f.dtype == np.float32 and np.array_equal(got_f, want_x[0].astype(np.float32) / np.float32(255.0))
        assert got_h.dtype == np.float64 and np.array_equal(np.argmax(got_h, axis=-1), want_l[0, ..., 0])
        assert np.array_equal(got_h.sum(axis=-1), np.ones((8, 12)))
        # without a descriptor the parameters come from the module's seeded stream
        A.seed(5); a = fn(x[0], None, args)
        A.seed(5); b = fn(x[0], None, args)
        assert a[1] is None and np.array_equal(a[0], b[0])


WARPS = [SHIFT, (A.flip_aug, {"flip_type": "left-right"}), AFFINE, (A.no_aug, {})]
MODES = [("one", (0.3, 0.2, 0.3, 0.2)), ("all", ())]


@pytest.mark.parametrize("mode, probs", MODES)
@pytest.mark.parametrize("fly", [True, False])
def test_host_path_and_descriptor_path_draw_the_same(mode, probs, fly):
    """Same seed: the descriptor walk (warp_reference, then device_aug_reference, what the device stages compute) hands out
    the batches of ``__getitem__`` over 2 epochs, N not a multiple of the batch."""
    im, lb = _data(n=7, h=8, w=12)
    dev = DataGenerator(im, lb, 4, WARPS, mode, probs, fly, None, seed=3, device_aug=True)
    host = DataGenerator(im, lb, 4, WARPS, mode, probs, fly, None, seed=3)
    assert dev.oct_device_aug and not host.oct_device_aug and len(dev) == len(host) > 0
    assert dev.batch_gen.images is None
    warped = 0
    for _ in range(2):
        for i in range(len(dev)):
            x8, lab8, ops, wops = dev.next_batch_aug()
            assert wops.dtype == A.WARP_OP_DTYPE and wops.shape == (4,)
            x, lab = A.device_aug_reference(*A.warp_reference(x8, lab8, wops), ops, seed=1)
            X, y = host[i]
            assert x.dtype == np.float32 and np.array_equal(x, X) and np.array_equal(lab, y[..., 0])
            warped += int((wops["kind"] != 0).sum())
        dev.on_epoch_end(); host.on_epoch_end()
    assert warped > 0


@pytest.mark.parametrize("mode, probs", MODES)
@pytest.mark.parametrize("fly", [True, False])
def test_two_shards_equal_the_whole_batch(mode, probs, fly):
    im, lb = _data(n=9, h=8, w=12)
    whole, r0, r1 = (DataGenerator(im, lb, 6, WARPS, mode, probs, fly, None, seed=5, device_aug=True) for _ in range(3))
    for _ in range(2):
        for _ in range(len(whole)):
            full = whole.next_batch_aug()
            parts = [r0.next_batch_aug(shard=(0, 2)), r1.next_batch_aug(shard=(2, 6))]
            assert len(full) == 4
            for k in range(2):
                assert np.array_equal(np.concatenate([p[k] for p in parts]), full[k])
            for k in range(2, 4):
                assert np.concatenate([p[k] for p in parts]).tobytes() == full[k].tobytes()
        for g in (whole, r0, r1):
            g.on_epoch_end()


def test_lists_without_a_warp_keep_three_arrays():
    im, lb = _data()
    g = DataGenerator(im, lb, 4, [WARPS[1], WARPS[3]], "all", (), True, None, seed=3, device_aug=True)
    assert len(g.next_batch_aug()) == 3 and g.batch_gen.warp_ops is None


def test_training_params_file_names_the_augmentations(tmp_path):
    from oct_image_segmentation_models_amd import optimizers
    from oct_image_segmentation_models_amd.common import h5io
    from oct_image_segmentation_models_amd.training.training import save_training_params_file
    from oct_image_segmentation_models_amd.training.training_parameters import TrainingParams
    tp = TrainingParams(model_architecture="unet", training_dataset_path=tmp_path / "d.hdf5", initial_model=None,
                        results_location=tmp_path, opt_con=optimizers.Adam, loss="dice_loss_macro", metric="dice_coef_macro",
                        epochs=1, batch_size=2, aug_mode="one", aug_probs=(0.25, 0.25, 0.5),
                        augmentations=[{"name": "flip", "arguments": {"flip_type": "up-down"}},
                                       {"name": "column_shift", "arguments": SHIFT[1]}, {"name": "affine", "arguments": AFFINE[1]}])
    save_training_params_file(tmp_path, "summary", {}, "md5", None, "now", tp, optimizers.Adam())
    attrs = h5io.load(tmp_path / "training_params.hdf5")
    text = lambda k: bytes(attrs[k]).rstrip(b"\x00").decode()
    assert text("attr:aug_2") == "column_shift_aug" and text("attr:aug_3") == "affine_aug" and "attr:aug_1" not in attrs
    assert float(attrs["attr:aug_2_param: max_tilt"]) == 2.0 and text("attr:aug_3_param: border") == "constant"
    assert np.asarray(attrs["attr:aug_3_param: scale_range"]).tolist() == [0.8, 1.25]
    assert int(attrs["attr:aug_3_param: fill_label"]) == 2
