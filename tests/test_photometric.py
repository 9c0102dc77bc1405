"""CPU tests of the photometric augmentation's host side: the numpy restatement ``photometric_reference`` of
``oct_photo_batch`` (include/oct_unet.h) against an independent brute-force statement of the same definition and against
known answers, the helpers and refusals, and the plumbing -- the keyword, the parameter stream that the host path and the
descriptor path of ``DataGenerator`` share, ``BatchFeed``, ``TrainingParams``.  No GPU, no library call.  The definition is
integer arithmetic: every comparison is for equality."""
import numpy as np
import pytest

import photo_cases as pc
from oct_image_segmentation_models_amd.common import augmentation as A
from oct_image_segmentation_models_amd.common.data_generator import DataGenerator


def _images(shape, seed=0):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


def _data(n=7, h=8, w=12, c=1, seed=0):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (n, h, w, c), dtype=np.uint8), rng.integers(0, 3, (n, h, w, 1), dtype=np.uint8)


def test_descriptor_layout():
    assert A.PHOTO_OP_DTYPE.itemsize == 320
    offsets = {k: A.PHOTO_OP_DTYPE.fields[k][1] for k in A.PHOTO_OP_DTYPE.names}
    assert offsets == {"kind": 0, "radius": 4, "w": 8, "n_shadows": 26, "cx": 28, "hw": 36, "y0": 44, "strength": 52,
                       "reserved": 60, "lut": 64}
    assert (A.PHOTO_BLUR, A.PHOTO_SHADOW, A.PHOTO_LUT, A.PHOTO_DRAWS) == (1, 2, 4, 24)
    assert "photometric" not in A.augmentation_map and len(A.augmentation_map) == 5      # a stage of its own, not a list entry


@pytest.mark.parametrize("shape", [(2, 5, 7, 1), (1, 11, 9, 3), (2, 19, 23, 1)])
def test_reference_equals_the_brute_force_statement(shape):
    """Random images; every flag combination, every radius 0..8 and the extreme weights (all in the centre, none in the
    centre and all at +-8), 0..4 shadows, identity and permutation tables."""
    B, H, W, _ = shape
    x = _images(shape, seed=1)
    ops = pc.combos(H, W)
    assert {int(r) for r in ops["radius"]} == set(range(9)) and {int(k) for k in ops["kind"]} == set(range(8))
    assert any(o["w"][0] == 0 and o["w"][8] == 128 for o in ops) and any(o["w"][0] == 256 and o["radius"] == 8 for o in ops)
    for which in range(0, len(ops), B):
        sel = pc.batch_ops(ops, B, which)
        assert np.array_equal(A.photometric_reference(x, sel), pc.brute_force(x, sel)), which


def test_a_constant_image_stays_constant_under_any_blur():
    for v in (0, 1, 127, 254, 255):
        x = np.full((1, 9, 13, 2), v, dtype=np.uint8)
        for wk in pc.WEIGHTS:
            assert (A.photometric_reference(x, np.array([pc.make_op(1, wk)])) == v).all(), (v, wk)
    x = _images((1, 6, 10, 1), seed=2)         # all the weight in the centre: the identity whatever the radius
    assert np.array_equal(A.photometric_reference(x, np.array([pc.make_op(1, "centre")])), x)
    # none in the centre, all at +-8: on a 6 x 10 image rows clamp to the first and last row, columns likewise
    far = A.photometric_reference(x, np.array([pc.make_op(1, "far")]))[0, ..., 0].astype(np.int64)
    r, c = np.arange(6), np.arange(10)
    X = x[0, ..., 0].astype(np.int64)
    h = 128 * (X[:, np.clip(c - 8, 0, 9)] + X[:, np.clip(c + 8, 0, 9)])
    assert np.array_equal(far, (128 * (h[np.clip(r - 8, 0, 5)] + h[np.clip(r + 8, 0, 5)]) + 32768) >> 16)


def test_shadow_known_answers():
    H, W = 6, 9
    x = np.full((1, H, W, 1), 200, dtype=np.uint8)
    run = lambda *sh: A.photometric_reference(x, np.array([pc.make_op(2, 0, list(sh))]))[0, ..., 0]      # noqa: E731
    # hw = 1, strength 256, y0 = 0: exactly column cx goes to 0, every other column is untouched
    out = run((4, 1, 0, 256))
    assert (out[:, 4] == 0).all() and (np.delete(out, 4, axis=1) == 200).all()
    # y0 inside: rows above it untouched; y0 >= H: nothing
    out = run((4, 1, 3, 256))
    assert (out[:3] == 200).all() and (out[3:, 4] == 0).all()
    assert (run((4, 1, H, 256)) == 200).all() and (run((4, 1, 16384, 256)) == 200).all()
    # a centre outside the image: only its flank reaches in.  cx = -2, hw = 4: g(x) = 256 - (256 (2 - x)) // 4 for x < 2
    out = run((-2, 4, 0, 256))
    assert out[0].tolist() == [(200 * g + 128) >> 8 for g in (128, 192)] + [200] * 7
    assert (run((W + 5, 5, 0, 256)) == 200).all() and (run((-32768, 4096, 0, 256)) == 200).all()
    # strength 0 is the identity; two shadows: the minimum of the gains, not their product
    assert (run((4, 3, 0, 0)) == 200).all()
    both = run((4, 2, 0, 128), (5, 2, 0, 128))
    assert both[0].tolist() == [200, 200, 200, 150, 100, 100, 150, 200, 200]
    assert np.array_equal(A.shadow_gain(H, W, pc.make_op(2, 0, [(4, 2, 2, 128)]))[:, 3:6],
                          np.array([[256] * 3] * 2 + [[192, 128, 192]] * 4))


def test_stage_order_is_blur_shadow_table():
    """A random permutation as the table: any other order of the three stages gives other bytes."""
    x = _images((1, 12, 16, 1), seed=3)
    perm = pc.tables()[1]
    sh = [(7, 5, 2, 230)]
    op = np.array([pc.make_op(7, 3, sh, perm)])
    blur, shade, table = (lambda im, o=np.array([pc.make_op(k, 3, sh, perm)]): A.photometric_reference(im, o) for k in (1, 2, 4))
    out = A.photometric_reference(x, op)
    assert np.array_equal(out, table(shade(blur(x))))
    for other in (table(blur(shade(x))), shade(table(blur(x))), blur(table(shade(x))), table(shade(x)), shade(blur(x))):
        assert not np.array_equal(out, other)
    assert np.array_equal(A.photometric_reference(x, np.array([pc.make_op(0, 3, sh, perm)])), x)      # kind 0: a copy
    assert np.array_equal(A.photometric_sample(x[0], op[0]), out[0])


def test_blur_weights_properties():
    for sigma in np.concatenate([np.linspace(0.01, 8.0 / 3.0, 400), [1e-6, 1.0 / 3.0, 8.0 / 3.0]]):
        R, w = A.blur_weights(sigma)
        w = w.astype(np.int64)
        assert R == min(8, int(np.ceil(3 * sigma))) and w.dtype == np.int64 and w.shape == (9,)
        assert w[0] + 2 * w[1:].sum() == 256 and not w[R + 1:].any() and w[0] > 0 and w[0] >= w[1]
        assert (np.diff(w[:R + 1]) <= 0).all()
    assert A.blur_weights(8.0 / 3.0)[1].tolist() == [40, 36, 29, 20, 12, 7, 3, 1, 0] and A.blur_weights(8.0 / 3.0)[0] == 8
    assert A.blur_weights(8.0 / 3.0)[1].dtype == np.uint16 and A.blur_weights(0.05)[1].tolist() == [256] + [0] * 8
    for bad in (0.0, -1.0, 2.67, float("nan")):
        with pytest.raises(ValueError):
            A.blur_weights(bad)


def test_photo_lut_properties():
    ident = np.arange(256)
    assert A.photo_lut().dtype == np.uint8 and np.array_equal(A.photo_lut(), ident) and np.array_equal(A.photo_lut(1.0, 0.0, 1.0), ident)
    for gamma, beta, c in [(0.25, 0, 1), (4, 0, 1), (1, 0.3, 1), (1, -0.3, 1), (1, 0, 0.25), (1, 0, 4), (2.2, -0.1, 1.7)]:
        lut = A.photo_lut(gamma, beta, c).astype(np.int64)
        assert (np.diff(lut) >= 0).all() and not np.array_equal(lut, ident)
        i = np.arange(256) / 255.0
        assert np.array_equal(lut, np.rint(255.0 * np.clip((i - 0.5) * c + 0.5 + beta, 0.0, 1.0) ** gamma).astype(np.int64))
    assert A.photo_lut(4.0)[[0, 255]].tolist() == [0, 255] and (A.photo_lut(2.0)[1:255] < ident[1:255]).all()
    assert (A.photo_lut(1, 1.0, 1) == 255).all() and (A.photo_lut(1, -1.0, 1) == 0).all()
    assert A.photo_lut(1, 0, 3)[[85, 86, 127, 128, 169, 170]].tolist() == [0, 3, 126, 129, 252, 255]        # 3 i - 255: about mid-grey


def test_check_photo_ops_refuses_field_by_field():
    good = np.array([pc.make_op(7, 5, pc.shadow_sets(20, 30)[4], pc.tables()[1]), pc.make_op(0)])
    A.check_photo_ops(good, 20, 30)
    A.check_photo_ops(np.zeros(3, dtype=A.PHOTO_OP_DTYPE), 1, 1)       # the all-zero descriptor: a copy
    A.check_photo_ops(good[:0])

    def bad(field, value, index=None, match=None):
        ops = good.copy()
        if index is None:
            ops[field][0] = value
        else:
            ops[field][0][index] = value
        with pytest.raises(ValueError, match=match or field):
            A.check_photo_ops(ops, 20, 30)
    bad("kind", 8); bad("kind", -1); bad("radius", 9); bad("radius", -1); bad("n_shadows", 5); bad("reserved", 1)
    bad("w", 39, 1, match="256"); bad("w", 1, 8, match="256"); bad("radius", 4, match="k > radius")
    bad("hw", 0, 0); bad("hw", 4097, 3); bad("hw", -5, 1); bad("y0", -1, 2); bad("y0", 16385, 0); bad("strength", 257, 3)
    # a field of a part whose flag is off, or of a shadow beyond n_shadows, is not looked at; cx is any int16
    ops = good.copy()
    ops["kind"][0], ops["w"][0] = 6, 9
    A.check_photo_ops(ops, 20, 30)
    ops = good.copy()
    ops["n_shadows"][0], ops["hw"][0][3], ops["cx"][0][0] = 3, 0, -32768
    A.check_photo_ops(ops, 20, 30)
    for H, W in [(0, 5), (5, 0), (16385, 5), (5, 16385)]:
        with pytest.raises(ValueError):
            A.check_photo_ops(good, H, W)
    with pytest.raises(TypeError):
        A.check_photo_ops(np.zeros(2, dtype=A.ELASTIC_OP_DTYPE))
    with pytest.raises(ValueError, match="one descriptor"):
        A.photometric_reference(_images((3, 4, 4, 1)), good)
    with pytest.raises(TypeError):
        A.photometric_reference(_images((2, 4, 4, 1)).astype(np.float32), good)


FULL = {"p": 0.8, "gamma": (0.5, 2.0), "brightness": 0.2, "contrast": (0.7, 1.5), "blur": {"p": 0.6, "sigma": (0.4, 2.6)},
        "shadows": {"p": 0.7, "max_count": 4, "width": (2, 9), "strength": (0.2, 1.0), "top": (0.1, 0.6)}}


def test_photometric_spec_accepts_and_refuses():
    off = A.photometric_spec({})
    assert off == {"p": 1.0, "gamma": None, "brightness": None, "contrast": None, "blur": None, "shadows": None}
    s = A.photometric_spec(FULL)
    assert s["p"] == 0.8 and s["gamma"] == (0.5, 2.0) and s["brightness"] == 0.2 and s["blur"] == {"p": 0.6, "sigma": (0.4, 2.6)}
    assert s["shadows"] == {"p": 0.7, "max_count": 4, "width": (2.0, 9.0), "strength": (0.2, 1.0), "top": (0.1, 0.6)}
    d = A.photometric_spec({"shadows": {"width": (1, 4096), "strength": (0, 1)}, "blur": {"sigma": (8 / 3, 8 / 3)}})
    assert d["shadows"]["p"] == 1.0 and d["shadows"]["max_count"] == 1 and d["shadows"]["top"] == (0.0, 0.0) and d["blur"]["p"] == 1.0
    for change in [{"p": -0.1}, {"p": 1.5}, {"gamma": (0.2, 1)}, {"gamma": (1, 4.1)}, {"gamma": (2, 1)}, {"gamma": 2}, {"brightness": -0.1},
                   {"brightness": 1.1}, {"contrast": (0.1, 1)}, {"contrast": (1, 5)}, {"contrast": (1, 2, 3)}, {"sharpen": 1},
                   {"blur": {"sigma": (0, 1)}}, {"blur": {"sigma": (1, 2.7)}}, {"blur": {"sigma": (2, 1)}}, {"blur": {"p": 2, "sigma": (1, 2)}},
                   {"blur": {}}, {"blur": {"sigma": (1, 2), "radius": 3}}, {"blur": 1.5},
                   {"shadows": {"width": (2, 9)}}, {"shadows": {"strength": (0, 1)}}, {"shadows": {"width": (0.5, 9), "strength": (0, 1)}},
                   {"shadows": {"width": (2, 5000), "strength": (0, 1)}}, {"shadows": {"width": (2, 9), "strength": (0, 1.1)}},
                   {"shadows": {"width": (2, 9), "strength": (0, 1), "top": (0, 1.5)}},
                   {"shadows": {"width": (2, 9), "strength": (0, 1), "max_count": 5}},
                   {"shadows": {"width": (2, 9), "strength": (0, 1), "max_count": 0}},
                   {"shadows": {"width": (2, 9), "strength": (0, 1), "max_count": 1.5}},
                   {"shadows": {"width": (2, 9), "strength": (0, 1), "depth": 3}}]:
        with pytest.raises(ValueError):
            A.photometric_spec(dict(FULL, **change))
    with pytest.raises(ValueError, match="sharpen"):
        A.photometric_spec({"sharpen": 1})
    with pytest.raises(ValueError):
        A.photometric_spec([1.0])


def test_draws_for_hand_picked_numbers():
    H, W = 40, 100
    spec = A.photometric_spec(FULL)
    u = np.full((5, A.PHOTO_DRAWS), 0.5)
    u[0, 0] = 0.8                                           # u0 < p, strictly: not this one
    u[1, [4, 6]] = 0.6, 0.7                                 # neither blur nor shadows; gamma 1, beta 0, contrast 1.1
    u[2, [1, 2, 3]] = 0.5, 0.5, 0.375                       # ... contrast exactly 1: the identity table, so no flag
    u[2, [4, 6]] = 0.9, 0.9
    u[3, 7] = 0.999
    u[3, 8:24] = [0.0, 0.0, 0.0, 0.0, 0.999, 1 - 1e-12, 1 - 1e-12, 1 - 1e-12, 0.5, 0.5, 0.5, 0.5, 0.25, 0.75, 0.25, 0.75]
    ops = A.draw_photo_ops(spec, u, H, W)
    assert ops.dtype == A.PHOTO_OP_DTYPE and ops.shape == (5,) and ops["kind"].tolist() == [0, 4, 0, 7, 7]
    assert ops[0].tobytes() == bytes(320) and not ops["reserved"].any()
    assert np.array_equal(ops[1]["lut"], A.photo_lut(1.0, 0.0, 1.1)) and ops[1]["n_shadows"] == 0 and not ops[1]["w"].any()
    assert np.array_equal(ops[2]["lut"], np.arange(256))
    R, w = A.blur_weights(1.5)
    assert ops[3]["radius"] == R == 5 and np.array_equal(ops[3]["w"], w)
    assert ops[3]["n_shadows"] == 4 and ops[4]["n_shadows"] == 3 and not ops[4]["hw"][3]
    assert ops[3]["cx"].tolist() == [0, 99, 50, 25] and ops[3]["hw"].tolist() == [2, 9, 6, 7]       # rint(5.5) = 6 (to even)
    assert ops[3]["y0"].tolist() == [4, 23, 14, 9] and ops[3]["strength"].tolist() == [51, 256, 154, 205]
    # gamma is drawn log-uniformly: u = 0.5 of (0.5, 2) is 1, u = 0 is 0.5
    one = A.photometric_spec({"gamma": (0.5, 2.0)})
    g = A.draw_photo_ops(one, np.array([[0.0] * 24, [0.5] * 24, [0.75] * 24]), H, W)
    assert g["kind"].tolist() == [4, 0, 4] and np.array_equal(g[0]["lut"], A.photo_lut(0.5)) and np.array_equal(g[2]["lut"], A.photo_lut(2 ** 0.5))
    # deterministic; nothing given draws nothing; p = 0 and p = 1
    rng = np.random.default_rng(0).random((50, A.PHOTO_DRAWS))
    a, b = A.draw_photo_ops(spec, rng, H, W), A.draw_photo_ops(spec, rng.copy(), H, W)
    assert a.tobytes() == b.tobytes() and len(set(a["kind"].tolist())) > 4
    assert not A.draw_photo_ops(A.photometric_spec({}), rng, H, W)["kind"].any()
    assert not A.draw_photo_ops(dict(spec, p=0.0), rng, H, W)["kind"].any()
    assert (A.draw_photo_ops(A.photometric_spec(dict(FULL, p=1, blur={"sigma": (1, 2)})), rng, H, W)["kind"] & 1).all()


SHIFT = (A.column_shift_aug, {"max_shift": 3, "max_tilt": 2, "max_curvature": 1})
LIST = [SHIFT, (A.flip_aug, {"flip_type": "left-right"}), (A.flip_aug, {"flip_type": "up-down"}), (A.no_aug, {})]
MODES = [("one", (0.3, 0.2, 0.3, 0.2)), ("all", ())]
ELASTIC = {"p": 0.6, "spacing": 3, "max_displacement": (1.5, 2.5), "border": "constant", "fill": 0, "fill_label": 2}
PHOTO = {"p": 0.8, "gamma": (0.5, 2.0), "brightness": 0.2, "contrast": (0.7, 1.5), "blur": {"p": 0.6, "sigma": (0.3, 1.2)},
         "shadows": {"p": 0.7, "max_count": 3, "width": (1, 4), "strength": (0.2, 1.0), "top": (0.0, 0.7)}}


@pytest.mark.parametrize("mode, probs", MODES)
@pytest.mark.parametrize("fly", [True, False])
@pytest.mark.parametrize("elastic", [None, ELASTIC])
def test_host_path_and_descriptor_path_give_the_same_bytes(mode, probs, fly, elastic):
    """Same seed: the descriptor walk (elastic_reference, photometric_reference, warp_reference, device_aug_reference: what
    the device stages compute, in their order) hands out the batches of ``__getitem__`` over 2 epochs."""
    im, lb = _data(n=7)
    dev = DataGenerator(im, lb, 4, LIST, mode, probs, fly, None, seed=3, device_aug=True, elastic=elastic, photometric=PHOTO)
    host = DataGenerator(im, lb, 4, LIST, mode, probs, fly, None, seed=3, elastic=elastic, photometric=PHOTO)
    assert dev.oct_device_aug and not host.oct_device_aug and len(dev) == len(host) > 0 and dev.batch_gen.images is None
    kinds = set()
    for _ in range(2):
        for i in range(len(dev)):
            x8, lab8, ops, wops, eops, pops = dev.next_batch_aug()
            assert pops.dtype == A.PHOTO_OP_DTYPE and pops.shape == (4,) and (eops is None) == (elastic is None)
            if eops is not None:
                x8, lab8 = A.elastic_reference(x8, lab8, eops)
            x, lab = A.device_aug_reference(*A.warp_reference(A.photometric_reference(x8, pops), lab8, wops), ops, seed=1)
            X, y = host[i]
            assert x.dtype == np.float32 and np.array_equal(x, X) and np.array_equal(lab, y[..., 0])
            kinds.update(pops["kind"].tolist())
        dev.on_epoch_end(); host.on_epoch_end()
    assert 0 in kinds and len(kinds) > 3


@pytest.mark.parametrize("mode, probs", MODES)
@pytest.mark.parametrize("fly", [True, False])
def test_without_the_keyword_nothing_changes_and_the_other_streams_are_untouched(mode, probs, fly):
    """One seed: shuffle, augmentation choices, warp descriptors and elastic descriptors are the same with and without the
    keyword; without it (absent or None) the return tuples are exactly as before."""
    im, lb = _data(n=7)
    for device_aug in (True, False):
        old, none, on = (DataGenerator(im, lb, 4, LIST, mode, probs, fly, None, seed=3, device_aug=device_aug, elastic=ELASTIC, **kw)
                         for kw in ({}, {"photometric": None}, {"photometric": PHOTO}))
        bare, bare_on = (DataGenerator(im, lb, 4, LIST, mode, probs, fly, None, seed=3, device_aug=device_aug, **kw)
                         for kw in ({}, {"photometric": PHOTO}))
        for _ in range(2):
            for i in range(len(old)):
                if device_aug:
                    a, b, c = old.next_batch_aug(), none.next_batch_aug(), on.next_batch_aug()
                    assert len(a) == len(b) == 5 and len(c) == 6
                    assert all(p.dtype == q.dtype and p.tobytes() == q.tobytes() for p, q in zip(a, b))
                    assert all(p.tobytes() == q.tobytes() for p, q in zip(a, c[:5]))    # images, labels, ops, warp, ELASTIC descriptors
                    d, e = bare.next_batch_aug(), bare_on.next_batch_aug()
                    assert len(d) == 4 and len(e) == 6 and e[4] is None and e[5].tobytes() == c[5].tobytes()
                    assert all(p.tobytes() == q.tobytes() for p, q in zip(d, e[:4]))
                else:
                    (ax, ay), (bx, by), (cx, cy) = old[i], none[i], on[i]
                    assert ax.tobytes() == bx.tobytes() and ay.tobytes() == by.tobytes() and ay.dtype == by.dtype
                    assert ay.tobytes() == cy.tobytes()             # the labels never notice the stage
            for g in (old, none, on, bare, bare_on):
                g.on_epoch_end()


def test_a_list_without_a_warp_holds_none_in_the_unused_positions():
    im, lb = _data()
    g = DataGenerator(im, lb, 4, LIST[1:], "all", (), True, None, seed=3, device_aug=True, photometric=PHOTO)
    out = g.next_batch_aug()
    assert len(out) == 6 and out[3] is None and out[4] is None and out[5].dtype == A.PHOTO_OP_DTYPE


def test_two_shards_equal_the_whole_batch():
    im, lb = _data(n=9)
    whole, r0, r1 = (DataGenerator(im, lb, 6, LIST, "one", MODES[0][1], True, None, seed=5, device_aug=True, elastic=ELASTIC,
                                   photometric=PHOTO) for _ in range(3))
    for _ in range(2):
        for _ in range(len(whole)):
            full = whole.next_batch_aug()
            parts = [r0.next_batch_aug(shard=(0, 2)), r1.next_batch_aug(shard=(2, 6))]
            for k in range(6):
                assert np.concatenate([p[k] for p in parts]).tobytes() == full[k].tobytes()
        for g in (whole, r0, r1):
            g.on_epoch_end()


def test_generator_refusals():
    im, lb = _data()
    with pytest.raises(ValueError, match='"one" with a single "no_augmentation" entry'):
        DataGenerator(im, lb, 4, [], "none", (), False, None, seed=3, photometric=PHOTO)
    with pytest.raises(ValueError, match="sharpen"):
        DataGenerator(im, lb, 4, LIST, "all", (), True, None, seed=3, photometric={"sharpen": 2})
    with pytest.raises(ValueError, match="uint8"):
        DataGenerator(im.astype(np.float32), lb, 4, LIST, "all", (), True, None, seed=3, photometric=PHOTO)


def test_the_feed_carries_the_descriptors_only_where_a_sample_has_a_kind():
    from oct_image_segmentation_models_amd.models.batch_feed import Batch, BatchFeed, ElasticBatch, PhotoBatch
    im, lb = _data(n=8)
    feed = BatchFeed("cpu")
    seen = []
    for p, elastic in ((0.0, None), (0.0, dict(ELASTIC, p=1.0)), (1.0, None), (1.0, dict(ELASTIC, p=1.0))):
        gen, twin = (DataGenerator(im, lb, 4, LIST[1:], "all", (), True, None, seed=3, device_aug=True, elastic=elastic,
                                   photometric=dict(PHOTO, p=p, blur={"sigma": (1, 1)})) for _ in range(2))
        hb = feed.host_batch(gen, 0, 0, 1)
        b = feed.upload(hb, 0)
        pops = twin.next_batch_aug()[5]
        if p == 0.0:        # the stage is skipped: the record of a generator without the keyword
            want = Batch if elastic is None else ElasticBatch
            assert type(hb) is want and type(b) is want and not pops["kind"].any()
        else:
            assert type(hb) is PhotoBatch and type(b) is PhotoBatch and hb.wops is None and (hb.eops is None) == (elastic is None)
            assert hb._fields == ElasticBatch._fields + ("pops",) and hb.pops.tobytes() == pops.tobytes()
            assert b.pops.dtype.is_floating_point is False and b.pops.numpy().tobytes() == pops.tobytes() and b.pops.numel() == 4 * 320
        seen.append(type(b))
    assert seen == [Batch, ElasticBatch, PhotoBatch, PhotoBatch] and feed.photo_out is None


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
    assert _training_params(tmp_path).photometric is None
    given = {"p": 0.5, "gamma": (0.5, 2.0), "brightness": 0.1, "blur": {"sigma": (0.5, 1.5)}}
    tp = _training_params(tmp_path, photometric=given, aug_device=True)
    assert tp.photometric == given and tp.photometric is not given
    for bad in [{"p": 2}, {"gamma": (0.1, 1)}, {"blur": {"sigma": (1, 3)}}, {"shadows": {"width": (1, 2)}}, {"hue": 1}, "yes"]:
        with pytest.raises(ValueError):
            _training_params(tmp_path, photometric=bad)
    with pytest.raises(ValueError, match="no_augmentation"):
        _training_params(tmp_path, photometric=given, aug_mode="none", augmentations=[], aug_probs=())
    for params, present in ((tp, True), (_training_params(tmp_path), False)):
        save_training_params_file(tmp_path, "summary", {}, "md5", None, "now", params, optimizers.Adam())
        attrs = h5io.load(tmp_path / "training_params.hdf5")
        keys = {k for k in attrs if "photometric" in k}
        assert keys == ({f"attr:photometric_param: {k}" for k in given} if present else set())
        if present:
            assert float(attrs["attr:photometric_param: p"]) == 0.5 and float(attrs["attr:photometric_param: brightness"]) == 0.1
            assert np.asarray(attrs["attr:photometric_param: gamma"]).tolist() == [0.5, 2.0]
            assert bytes(attrs["attr:photometric_param: blur"]).rstrip(b"\x00").decode() == str(given["blur"])
