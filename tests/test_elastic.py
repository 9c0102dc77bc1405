"""CPU tests of the elastic deformation's host side: the numpy restatement ``elastic_reference`` of ``oct_elastic_batch``
(include/oct_unet.h) against independent statements of the same definition (Python's unbounded integers, a float64
B-spline), the refusals, and the plumbing -- the keyword, the parameter stream that the host path and the descriptor path of
``DataGenerator`` share, ``TrainingParams``.  No GPU, no library call.  The definition is integer arithmetic, so every
comparison but the float64 one is for equality."""
import numpy as np
import pytest

from oct_image_segmentation_models_amd.common import augmentation as A
from oct_image_segmentation_models_amd.common.data_generator import DataGenerator


def _data(n=7, h=8, w=12, c=1, seed=0):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (n, h, w, c), dtype=np.uint8), rng.integers(0, 3, (n, h, w, 1), dtype=np.uint8)


def _op(kind=1, border=0, spacing=4, amp=(300, 500), key=(1, 2), fill=0, fill_label=0):
    op = np.zeros(1, dtype=A.ELASTIC_OP_DTYPE)
    op["kind"], op["border"], op["spacing"], op["fill"], op["fill_label"] = kind, border, spacing, fill, fill_label
    (op["amp_x"], op["amp_y"]), (op["seed_lo"], op["seed_hi"]) = amp, key
    return op


def test_descriptor_layout():
    assert A.ELASTIC_OP_DTYPE.itemsize == 40
    offsets = {k: A.ELASTIC_OP_DTYPE.fields[k][1] for k in A.ELASTIC_OP_DTYPE.names}
    assert offsets == {"kind": 0, "border": 4, "spacing": 8, "amp_x": 12, "amp_y": 16, "seed_lo": 20, "seed_hi": 24, "fill": 28,
                       "fill_label": 32, "reserved": 36}
    assert (A.ELASTIC_MAX_DIM, A.ELASTIC_MIN_SPACING, A.ELASTIC_MAX_SPACING, A.ELASTIC_MAX_AMP) == (16384, 2, 128, 8192)
    assert A.ELASTIC_DRAWS == 3 and A.ELASTIC_TAG == int.from_bytes(b"ELAS", "big")
    assert "elastic" not in A.augmentation_map          # a stage of its own, not a list entry


def test_weights_are_non_negative_and_sum_to_6s3():
    for S in range(2, 129):
        cell, b = A.elastic_weights(3 * S, S)           # every offset k, three cells
        assert b.shape == (3 * S, 4) and (b >= 0).all() and (b.sum(axis=1) == 6 * S ** 3).all()
        assert np.array_equal(cell, np.arange(3 * S) // S) and np.array_equal(b[:S], b[S:2 * S])
        k = np.arange(S)
        assert np.array_equal(b[:S, 0], (S - k) ** 3) and np.array_equal(b[:S, 3], k ** 3)
        assert np.array_equal(b[:S, 1], 3 * k ** 3 - 6 * S * k ** 2 + 4 * S ** 3)
        assert np.array_equal(b[1:S, 2], b[S - 1:0:-1, 1])          # the spline is symmetric: b2(k) = b1(S - k)


@pytest.mark.parametrize("S", [2, 3, 7, 128])
def test_a_constant_control_grid_gives_that_displacement(S):
    H, W = 19, 23
    shape = ((H - 1) // S + 4, (W - 1) // S + 4)
    for cx, cy in [(0, 0), (1, -1), (777, -8192), (8192, 5)]:
        dx, dy = A.elastic_displacement(H, W, _op(spacing=S)[0], control=(np.full(shape, cx), np.full(shape, cy)))
        assert dx.shape == dy.shape == (H, W) and dx.dtype == np.int64
        assert (dx == cx).all() and (dy == cy).all()


def test_control_draws_are_the_documented_philox_blocks():
    H, W, S = 40, 70, 3
    op = _op(spacing=S, amp=(785, 8192), key=(0xDEADBEEF, 0x01234567))[0]
    dx, dy = A.elastic_control(H, W, op)
    assert dx.shape == dy.shape == ((H - 1) // S + 4, (W - 1) // S + 4)
    for i, j in [(0, 0), (3, 5), (dx.shape[0] - 1, dx.shape[1] - 1), (7, 0)]:
        r = A.philox4x32_10(np.array([j, i, 0, 0x454C4153]), np.array([0xDEADBEEF, 0x01234567]))
        assert int(dx[i, j]) == ((int(r[0]) * (2 * 785 + 1)) >> 32) - 785
        assert int(dy[i, j]) == ((int(r[1]) * (2 * 8192 + 1)) >> 32) - 8192
    assert abs(dx).max() <= 785 and abs(dy).max() <= 8192
    # both ends are reached: a small amplitude over a few hundred points
    lo = A.elastic_control(H, W, _op(spacing=S, amp=(1, 2), key=(5, 6))[0])
    assert set(np.unique(lo[0])) == {-1, 0, 1} and set(np.unique(lo[1])) == {-2, -1, 0, 1, 2}


@pytest.mark.parametrize("S, amp", [(2, (8192, 8192)), (5, (1, 785)), (16, (785, 8192)), (128, (8192, 1))])
def test_the_displacement_stays_inside_the_amplitude(S, amp):
    dx, dy = A.elastic_displacement(37, 53, _op(spacing=S, amp=amp, key=(S, 9))[0])
    assert abs(dx).max() <= amp[0] and abs(dy).max() <= amp[1]
    # (a field of amplitude 1 may round to zero everywhere: the spline averages 16 control points)
    assert (dx.any() or amp[0] < 256) and (dy.any() or amp[1] < 256)


def test_amplitude_zero_is_the_identity_and_amp_x_zero_keeps_columns():
    x, lab = _data(n=3, h=13, w=18, c=2, seed=1)
    for border in range(3):
        ops = np.concatenate([_op(border=border, amp=(0, 0), key=(b, 7), fill=9, fill_label=2) for b in range(3)])
        out, lo = A.elastic_reference(x, lab, ops)
        assert np.array_equal(out, x) and np.array_equal(lo, lab)
    op = _op(spacing=5, amp=(0, 2000), key=(3, 4))
    dx, dy = A.elastic_displacement(13, 18, op[0])
    assert not dx.any() and dy.any()
    rows, cols, outside = A.elastic_label_index(13, 18, op[0])
    assert outside is None and np.array_equal(cols, np.broadcast_to(np.arange(18), (13, 18))) and (rows != np.arange(13)[:, None]).any()
    # the image too: every output column is a function of its own input column alone
    y = x[:1].copy()
    y[0, :, 7] ^= 0xFF
    a, b = A.elastic_reference(x[:1], None, op)[0], A.elastic_reference(y, None, op)[0]
    assert not np.array_equal(a[0, :, 7], b[0, :, 7]) and np.array_equal(np.delete(a, 7, axis=2), np.delete(b, 7, axis=2))


def _scalar_displacement(H, W, op):
    """The header's definition, pixel by pixel, in Python's unbounded integers."""
    S = int(op["spacing"])
    ctrl = [[[int(v) for v in row] for row in c] for c in A.elastic_control(H, W, op)]

    def weights(p):
        k = p % S
        return p // S, [(S - k) ** 3, 3 * k ** 3 - 6 * S * k ** 2 + 4 * S ** 3, -3 * k ** 3 + 3 * S * k ** 2 + 3 * S * S * k + S ** 3,
                        k ** 3]
    wx, wy = [weights(x) for x in range(W)], [weights(y) for y in range(H)]
    out = np.empty((2, H, W), dtype=np.int64)
    peak = 0
    for y in range(H):
        cy, by = wy[y]
        for x in range(W):
            cx, bx = wx[x]
            for axis in range(2):
                N = sum(by[a] * bx[b] * ctrl[axis][cy + a][cx + b] for a in range(4) for b in range(4))
                peak = max(peak, abs(N) + 18 * S ** 6)
                out[axis, y, x] = (N + 18 * S ** 6) // (36 * S ** 6)
    return out[0], out[1], peak


def test_no_overflow_at_the_largest_spacing_and_amplitude():
    H, W = 260, 300
    op = _op(spacing=128, amp=(8192, 8192), key=(11, 12))[0]
    sx, sy, peak = _scalar_displacement(H, W, op)
    dx, dy = A.elastic_displacement(H, W, op)
    assert np.array_equal(dx, sx) and np.array_equal(dy, sy)
    assert 2 ** 55 < peak < 2 ** 61         # the sums are that large, and inside int64


@pytest.mark.parametrize("S, amp", [(2, 8192), (7, 785), (32, 2048)])
def test_an_independent_float64_bspline_agrees_within_one_unit(S, amp):
    H, W = 41, 67
    op = _op(spacing=S, amp=(amp, amp), key=(S, amp))[0]
    got = A.elastic_displacement(H, W, op)

    def basis(t):       # the uniform cubic B-spline's four blending functions at t in [0, 1)
        return np.stack([(1 - t) ** 3, 3 * t ** 3 - 6 * t ** 2 + 4, -3 * t ** 3 + 3 * t ** 2 + 3 * t + 1, t ** 3]) / 6.0
    ys, xs = np.arange(H) / S, np.arange(W) / S
    cy, cx = np.floor(ys).astype(int), np.floor(xs).astype(int)
    by, bx = basis(ys - cy), basis(xs - cx)
    for d, g in zip(A.elastic_control(H, W, op), got):
        want = sum(by[a][:, None] * bx[b][None, :] * d[cy[:, None] + a, cx[None, :] + b] for a in range(4) for b in range(4))
        assert np.abs(g - want).max() <= 1.0        # rounding to the nearest unit: half a unit, and float64's own error


def test_labels_are_the_images_nearest_pixel_gather():
    x, _ = _data(n=2, h=21, w=30, seed=2)
    for border in range(3):
        ops = np.concatenate([_op(border=border, spacing=4, amp=(2500, 1800), key=(b, border), fill=3, fill_label=3) for b in range(2)])
        _, lab = A.elastic_reference(x, x[..., 0], ops)
        for b in range(2):
            rows, cols, outside = A.elastic_label_index(21, 30, ops[b])
            want = x[b, rows, cols, 0]
            if border == 2:
                assert outside.any()
                want[outside] = 3
            else:
                assert outside is None
            assert np.array_equal(lab[b], want) and not np.array_equal(lab[b], x[b, ..., 0])


def test_reference_mixes_kinds_and_leaves_its_inputs():
    x, lab = _data(n=3, h=10, w=14, c=3, seed=3)
    keep = x.copy(), lab.copy()
    ops = np.concatenate([_op(kind=0), _op(border=2, amp=(900, 900), fill=200, fill_label=2), _op(kind=0, spacing=0)])
    out, lo = A.elastic_reference(x, lab, ops)
    assert np.array_equal(x, keep[0]) and np.array_equal(lab, keep[1]) and lo.shape == lab.shape
    assert np.array_equal(out[[0, 2]], x[[0, 2]]) and np.array_equal(lo[[0, 2]], lab[[0, 2]])
    assert not np.array_equal(out[1], x[1]) and not np.array_equal(lo[1], lab[1])
    assert A.elastic_reference(x, None, ops)[1] is None
    one = A.elastic_reference(x[1:2], lab[1:2], ops[1:2])       # nothing depends on the batch position
    assert np.array_equal(one[0][0], out[1]) and np.array_equal(one[1][0], lo[1])


def test_check_refuses_each_field_out_of_range():
    good = _op()
    A.check_elastic_ops(good, 16384, 1)
    for field, value in [("kind", 2), ("kind", -1), ("border", 3), ("border", -1), ("spacing", 1), ("spacing", 129), ("amp_x", -1),
                         ("amp_x", 8193), ("amp_y", -1), ("amp_y", 8193), ("fill", 256), ("fill", -1), ("fill_label", 256),
                         ("fill_label", -1), ("reserved", 1)]:
        bad = good.copy()
        bad[field] = value
        with pytest.raises(ValueError, match=field):
            A.check_elastic_ops(bad)
        with pytest.raises(ValueError, match=field):
            A.elastic_reference(np.zeros((1, 4, 4, 1), np.uint8), None, bad)
    for hw in [(0, 4), (4, 16385)]:
        with pytest.raises(ValueError, match="outside 1..16384"):
            A.check_elastic_ops(good, *hw)
    with pytest.raises(TypeError):
        A.check_elastic_ops(np.zeros(1, dtype=A.WARP_OP_DTYPE))
    A.check_elastic_ops(np.zeros(2, dtype=A.ELASTIC_OP_DTYPE))          # kind 0: spacing and amplitudes are not looked at


def test_spec_accepts_and_refuses():
    s = A.elastic_spec({"p": 0.5, "spacing": 32, "max_displacement": 8})
    assert s == {"p": 0.5, "spacing": 32, "amp_x": 2048, "amp_y": 2048, "border": 0, "fill": 0, "fill_label": 0}
    s = A.elastic_spec({"p": 1, "spacing": 2, "max_displacement": (0, 32), "border": "constant", "fill": 7, "fill_label": 2})
    assert (s["amp_x"], s["amp_y"], s["border"], s["fill"], s["fill_label"]) == (0, 8192, 2, 7, 2)
    assert A.elastic_spec({"p": 0, "spacing": 128, "max_displacement": 0.3})["amp_x"] == 77       # rint(76.8)
    base = {"p": 0.5, "spacing": 8, "max_displacement": 4}
    for change in [{"p": -0.1}, {"p": 1.5}, {"spacing": 1}, {"spacing": 129}, {"spacing": 8.5}, {"max_displacement": 32.1},
                   {"max_displacement": -1}, {"max_displacement": (1, 2, 3)}, {"max_displacement": (1, 40)}, {"border": "mirror"},
                   {"fill": 256}, {"fill_label": 1.5}, {"sigma": 3}]:
        with pytest.raises(ValueError):
            A.elastic_spec(dict(base, **change))
    for key in base:
        with pytest.raises(ValueError, match=key):
            A.elastic_spec({k: v for k, v in base.items() if k != key})
    with pytest.raises(ValueError):
        A.elastic_spec([0.5, 8, 4])


def test_draws_for_hand_picked_numbers():
    spec = A.elastic_spec({"p": 0.25, "spacing": 16, "max_displacement": (2, 3), "border": "wrap", "fill": 4, "fill_label": 1})
    u = [[0.0, 0.0, 0.5], [0.2499, 1 - 2.0 ** -33, 2.0 ** -32], [0.25, 0.7, 0.7], [0.9, 0.1, 0.1]]
    ops = A.draw_elastic_ops(spec, u)
    assert ops.dtype == A.ELASTIC_OP_DTYPE and ops["kind"].tolist() == [1, 1, 0, 0]         # u0 < p, strictly
    assert ops["seed_lo"].tolist() == [0, 0xFFFFFFFF, 0, 0] and ops["seed_hi"].tolist() == [0x80000000, 1, 0, 0]
    for name, v in (("border", 1), ("spacing", 16), ("amp_x", 512), ("amp_y", 768), ("fill", 4), ("fill_label", 1)):
        assert ops[name].tolist() == [v, v, 0, 0]
    assert ops[2:].tobytes() == bytes(80) and not ops["reserved"].any()
    rng = np.random.default_rng(0).random((50, 3))
    assert not A.draw_elastic_ops(dict(spec, p=0.0), rng)["kind"].any() and A.draw_elastic_ops(dict(spec, p=1.0), rng)["kind"].all()


def test_host_sample_moves_one_hot_masks():
    x, lab = _data(n=1, h=9, w=11, c=2, seed=4)
    op = _op(border=2, spacing=3, amp=(1500, 1500), fill=40, fill_label=2)
    want_x, want_l = A.elastic_reference(x, lab, op)
    got_x, got_l = A.elastic_sample(x[0], lab[0], op)
    assert got_x.dtype == np.uint8 and np.array_equal(got_x, want_x[0]) and np.array_equal(got_l, want_l[0])
    onehot = np.eye(3, dtype=np.float64)[lab[0, ..., 0]]
    got_h = A.elastic_sample(x[0], onehot, op)[1]
    assert got_h.dtype == np.float64 and np.array_equal(np.argmax(got_h, -1), want_l[0, ..., 0]) and (got_h.sum(-1) == 1).all()
    mask = lab[0]
    assert A.elastic_sample(x[0], None, op)[1] is None and A.elastic_sample(x[0], mask, _op(kind=0))[1] is mask


SHIFT = (A.column_shift_aug, {"max_shift": 3, "max_tilt": 2, "max_curvature": 1})
LIST = [SHIFT, (A.flip_aug, {"flip_type": "left-right"}), (A.flip_aug, {"flip_type": "up-down"}), (A.no_aug, {})]
MODES = [("one", (0.3, 0.2, 0.3, 0.2)), ("all", ())]
ELASTIC = {"p": 0.6, "spacing": 3, "max_displacement": (1.5, 2.5), "border": "constant", "fill": 0, "fill_label": 2}


@pytest.mark.parametrize("mode, probs", MODES)
@pytest.mark.parametrize("fly", [True, False])
def test_host_path_and_descriptor_path_give_the_same_bytes(mode, probs, fly):
    """Same seed: the descriptor walk (elastic_reference, warp_reference, device_aug_reference: what the device stages
    compute) hands out the batches of ``__getitem__`` over 2 epochs, N not a multiple of the batch."""
    im, lb = _data(n=7)
    dev = DataGenerator(im, lb, 4, LIST, mode, probs, fly, None, seed=3, device_aug=True, elastic=ELASTIC)
    host = DataGenerator(im, lb, 4, LIST, mode, probs, fly, None, seed=3, elastic=ELASTIC)
    assert dev.oct_device_aug and not host.oct_device_aug and len(dev) == len(host) > 0 and dev.batch_gen.images is None
    deformed = plain = 0
    for _ in range(2):
        for i in range(len(dev)):
            x8, lab8, ops, wops, eops = dev.next_batch_aug()
            assert eops.dtype == A.ELASTIC_OP_DTYPE and eops.shape == (4,) and wops.dtype == A.WARP_OP_DTYPE
            x, lab = A.device_aug_reference(*A.warp_reference(*A.elastic_reference(x8, lab8, eops), wops), ops, seed=1)
            X, y = host[i]
            assert x.dtype == np.float32 and np.array_equal(x, X) and np.array_equal(lab, y[..., 0])
            deformed += int(eops["kind"].sum()); plain += int((eops["kind"] == 0).sum())
        dev.on_epoch_end(); host.on_epoch_end()
    assert deformed > 0 and plain > 0


@pytest.mark.parametrize("mode, probs", MODES)
@pytest.mark.parametrize("fly", [True, False])
def test_without_the_keyword_nothing_changes_and_the_warp_stream_is_untouched(mode, probs, fly):
    im, lb = _data(n=7)
    for device_aug in (True, False):
        old, none, on = (DataGenerator(im, lb, 4, LIST, mode, probs, fly, None, seed=3, device_aug=device_aug, **kw)
                         for kw in ({}, {"elastic": None}, {"elastic": ELASTIC}))
        for _ in range(2):
            for i in range(len(old)):
                if device_aug:
                    a, b, c = old.next_batch_aug(), none.next_batch_aug(), on.next_batch_aug()
                    assert len(a) == len(b) == 4 and len(c) == 5
                    assert all(p.dtype == q.dtype and p.tobytes() == q.tobytes() for p, q in zip(a, b))
                    assert all(p.tobytes() == q.tobytes() for p, q in zip(a, c[:4]))        # images, labels, ops, WARP descriptors
                else:
                    (ax, ay), (bx, by) = old[i], none[i]
                    assert ax.tobytes() == bx.tobytes() and ay.tobytes() == by.tobytes() and ay.dtype == by.dtype
            for g in (old, none, on):
                g.on_epoch_end()


def test_a_list_without_a_warp_holds_none_in_the_warp_position():
    im, lb = _data()
    g = DataGenerator(im, lb, 4, LIST[1:], "all", (), True, None, seed=3, device_aug=True, elastic=ELASTIC)
    out = g.next_batch_aug()
    assert len(out) == 5 and out[3] is None and out[4].dtype == A.ELASTIC_OP_DTYPE and g.batch_gen.warp_ops is None


@pytest.mark.parametrize("mode, probs", MODES)
@pytest.mark.parametrize("fly", [True, False])
def test_two_shards_equal_the_whole_batch(mode, probs, fly):
    im, lb = _data(n=9)
    whole, r0, r1 = (DataGenerator(im, lb, 6, LIST, mode, probs, fly, None, seed=5, device_aug=True, elastic=ELASTIC) for _ in range(3))
    for _ in range(2):
        for _ in range(len(whole)):
            full = whole.next_batch_aug()
            parts = [r0.next_batch_aug(shard=(0, 2)), r1.next_batch_aug(shard=(2, 6))]
            assert len(full) == 5
            for k in range(5):
                assert np.concatenate([p[k] for p in parts]).tobytes() == full[k].tobytes()
        for g in (whole, r0, r1):
            g.on_epoch_end()


def test_generator_refusals():
    im, lb = _data()
    with pytest.raises(ValueError, match='"one" with a single "no_augmentation" entry'):
        DataGenerator(im, lb, 4, [], "none", (), False, None, seed=3, elastic=ELASTIC)
    with pytest.raises(ValueError, match="spacing"):
        DataGenerator(im, lb, 4, LIST, "all", (), True, None, seed=3, elastic=dict(ELASTIC, spacing=1))
    with pytest.raises(ValueError, match="uint8"):
        DataGenerator(im.astype(np.float32), lb, 4, LIST, "all", (), True, None, seed=3, elastic=ELASTIC)


def test_the_feed_carries_the_descriptors_only_where_a_sample_is_deformed():
    from oct_image_segmentation_models_amd.models.batch_feed import Batch, BatchFeed, ElasticBatch
    im, lb = _data(n=8)
    feed = BatchFeed("cpu")
    seen = set()
    for p in (0.0, 1.0):
        gen, twin = (DataGenerator(im, lb, 4, LIST[1:], "all", (), True, None, seed=3, device_aug=True, elastic=dict(ELASTIC, p=p))
                     for _ in range(2))
        hb = feed.host_batch(gen, 0, 0, 1)
        b = feed.upload(hb, 0)
        eops = twin.next_batch_aug()[4]
        if p == 0.0:        # the stage is skipped: the five-field record of a generator without the keyword
            assert type(hb) is Batch and type(b) is Batch and not eops["kind"].any()
        else:
            assert type(hb) is ElasticBatch and type(b) is ElasticBatch and hb.wops is None and b.wops is None
            assert hb._fields == Batch._fields + ("eops",) and hb.eops.tobytes() == eops.tobytes()
            assert b.eops.dtype.is_floating_point is False and b.eops.numpy().tobytes() == eops.tobytes()
        seen.add(type(b))
    assert seen == {Batch, ElasticBatch}


def _training_params(tmp_path, **kw):
    from oct_image_segmentation_models_amd import optimizers
    from oct_image_segmentation_models_amd.training.training_parameters import TrainingParams
    args = dict(model_architecture="unet", training_dataset_path=tmp_path / "d.hdf5", initial_model=None, results_location=tmp_path,
                opt_con=optimizers.Adam, loss="dice_loss_macro", metric="dice_coef_macro", epochs=1, batch_size=2, aug_mode="one",
                aug_probs=(1.0,), augmentations=[{"name": "no_augmentation"}])
    return TrainingParams(**dict(args, **kw))


def test_training_params_accepts_refuses_and_records(tmp_path):
    from oct_image_segmentation_models_amd import optimizers
    from oct_image_segmentation_models_amd.common import h5io
    from oct_image_segmentation_models_amd.training.training import save_training_params_file
    assert _training_params(tmp_path).elastic is None
    given = {"p": 0.5, "spacing": 32, "max_displacement": (0, 8), "border": "constant", "fill_label": 2}
    tp = _training_params(tmp_path, elastic=given, aug_device=True)
    assert tp.elastic == given and tp.elastic is not given
    for bad in [{"p": 2, "spacing": 32, "max_displacement": 8}, {"p": 0.5, "spacing": 200, "max_displacement": 8},
                {"p": 0.5, "spacing": 32, "max_displacement": 33}, {"p": 0.5, "spacing": 32}, "yes"]:
        with pytest.raises(ValueError):
            _training_params(tmp_path, elastic=bad)
    with pytest.raises(ValueError, match="no_augmentation"):
        _training_params(tmp_path, elastic=given, aug_mode="none", augmentations=[], aug_probs=())
    for params, present in ((tp, True), (_training_params(tmp_path), False)):
        save_training_params_file(tmp_path, "summary", {}, "md5", None, "now", params, optimizers.Adam())
        attrs = h5io.load(tmp_path / "training_params.hdf5")
        keys = {k for k in attrs if "elastic" in k}
        assert keys == ({f"attr:elastic_param: {k}" for k in given} if present else set())
        if present:
            assert float(attrs["attr:elastic_param: p"]) == 0.5 and int(attrs["attr:elastic_param: spacing"]) == 32
            assert np.asarray(attrs["attr:elastic_param: max_displacement"]).tolist() == [0.0, 8.0]
            assert bytes(attrs["attr:elastic_param: border"]).rstrip(b"\x00").decode() == "constant"
