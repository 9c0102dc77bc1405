"""GPU tests of ``oct_elastic_batch`` (include/oct_unet.h) and of the training path that uses it, against the numpy
restatement ``common.augmentation.elastic_reference``.  The definition is integer arithmetic: every comparison is byte for
byte, images and labels."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

from oct_image_segmentation_models_amd.common import augmentation as A
from oct_image_segmentation_models_amd.common.synthetic import make_scans

pytestmark = pytest.mark.gpu

# (1,5,7,1): smaller than a cell, guarded byte stores; (2,36,68,3): channels, byte stores; (2,64,128,1): whole tiles;
# (1,130,70,1): tiles cut by both image edges, byte stores (70 % 4 != 0); (3,20,34,1) likewise, three samples
SHAPES = [(1, 5, 7, 1), (3, 20, 34, 1), (2, 36, 68, 3), (2, 64, 128, 1), (1, 130, 70, 1)]
SPACINGS = [2, 3, 7, 16, 64, 128]
AMPS = [(0, 0), (1, 1), (785, 785), (8192, 8192), (0, 3000)]
# every spacing x amplitude pair x border, and samples that are copied (kind 0; kind 1 with a spacing outside its range is
# refused on the host, so it cannot be asked of the binding), in a fixed shuffled order: neighbours differ in everything
COMBOS = [(1, S, amp, border) for S, amp, border in itertools.product(SPACINGS, AMPS, range(3))]
COMBOS += [(0, 0, (0, 0), 0), (0, 16, (785, 785), 1), (0, 128, (8192, 8192), 2)] * 4
COMBOS = [COMBOS[k] for k in np.random.default_rng(0).permutation(len(COMBOS))]


@pytest.fixture(scope="module")
def eng():
    from oct_image_segmentation_models_amd.engine import UNetEngine
    return UNetEngine(device="cuda:0", input_channels=1, num_classes=3, image_height=16, image_width=32, start_neurons=8,
                      pool_layers=2, max_batch=1, training=False)


def _batch(shape, seed=0):
    rng = np.random.default_rng(seed)
    B, H, W, _ = shape
    return rng.integers(0, 256, shape, dtype=np.uint8), rng.integers(0, 4, (B, H, W), dtype=np.uint8)


def _ops(B, which):
    """B descriptors: sample b takes combination ``which + b`` of ``COMBOS``."""
    ops = np.zeros(B, dtype=A.ELASTIC_OP_DTYPE)
    for b in range(B):
        k = (which + b) % len(COMBOS)
        kind, S, amp, border = COMBOS[k]
        ops[b]["kind"], ops[b]["spacing"], ops[b]["border"] = kind, S, border
        ops[b]["amp_x"], ops[b]["amp_y"] = amp
        ops[b]["seed_lo"], ops[b]["seed_hi"] = 0x9E3779B9 * (k + 1) & 0xFFFFFFFF, 77 + k
        ops[b]["fill"], ops[b]["fill_label"] = 37 + b, 5 + b
    return ops


def _run(eng, x, lab, ops):
    xo, lo = eng.elastic(torch.from_numpy(x).cuda(), None if lab is None else torch.from_numpy(lab).cuda(), ops)
    torch.cuda.synchronize()
    return xo.cpu().numpy(), None if lo is None else lo.cpu().numpy()


@pytest.mark.parametrize("shape", SHAPES)
def test_kernel_equals_the_restatement(eng, shape):
    """Every spacing x amplitude pair x border, and copied samples, mixed inside the batches; with labels, and once
    without."""
    B, H, W, _ = shape
    x, lab = _batch(shape, seed=1)
    for which in range(0, len(COMBOS), B):
        ops = _ops(B, which)
        ref_x, ref_l = A.elastic_reference(x, lab, ops)
        out_x, out_l = _run(eng, x, lab, ops)
        assert out_x.dtype == np.uint8 and np.array_equal(out_x, ref_x), (which, ops)
        assert out_l.dtype == np.uint8 and np.array_equal(out_l, ref_l), (which, ops)
        if which == 0:      # without labels nothing but the images is written
            only_x, none = _run(eng, x, None, ops)
            assert none is None and np.array_equal(only_x, ref_x)


def test_kinds_borders_and_axes_side_by_side(eng):
    """(8, 40, 132, 1): kind 0 beside kind 1 under the three borders, both axes and axial-only; noise moved where the
    amplitude is a pixel or more, identity where it is 0, columns kept where amp_x is 0, the fill values where the border
    is constant."""
    shape = (8, 40, 132, 1)
    x, lab = _batch(shape, seed=2)
    ops = np.zeros(8, dtype=A.ELASTIC_OP_DTYPE)
    ops["kind"] = [0, 1, 1, 1, 1, 1, 0, 1]
    ops["border"] = [0, 0, 1, 2, 2, 0, 2, 1]
    ops["spacing"] = [0, 7, 16, 5, 32, 9, 64, 3]
    ops["amp_x"] = [0, 2000, 8192, 8192, 0, 0, 8192, 256]
    ops["amp_y"] = [0, 2000, 8192, 8192, 6000, 0, 8192, 256]
    ops["seed_lo"], ops["seed_hi"] = np.arange(8) + 100, 5
    ops["fill"], ops["fill_label"] = 255, 7
    ref_x, ref_l = A.elastic_reference(x, lab, ops)
    out_x, out_l = _run(eng, x, lab, ops)
    assert np.array_equal(out_x, ref_x) and np.array_equal(out_l, ref_l)
    for b in range(8):
        assert np.array_equal(out_x[b], x[b]) == (b in (0, 5, 6))
    assert all(np.array_equal(out_l[b], lab[b]) for b in (0, 5, 6)) and not any(np.array_equal(out_l[b], lab[b]) for b in (1, 2, 3, 4))
    assert (out_l[3] == 7).any() and not (out_l[[0, 1, 2, 5, 6, 7]] == 7).any()      # labels are 0..3: a 7 is the fill
    # axial only: flipping one input column changes that output column and no other
    y = x.copy(); y[4, :, 50] ^= 0xFF
    other = _run(eng, y, lab, ops)[0]
    assert not np.array_equal(other[4, :, 50], out_x[4, :, 50])
    assert np.array_equal(np.delete(other[4], 50, axis=1), np.delete(out_x[4], 50, axis=1))


def test_unaligned_views_take_the_guarded_path(eng):
    """The same bytes from views offset by one byte (inputs, outputs, each alone and all together)."""
    shape = (2, 24, 132, 1)
    B, H, W, Cn = shape
    n = B * H * W
    x, lab = _batch(shape, seed=3)
    ops = _ops(B, 40)
    ref_x, ref_l = A.elastic_reference(x, lab, ops)
    for off in [(0, 0, 0, 0), (1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1), (1, 1, 1, 1)]:
        bufs = [torch.zeros(n + 4, dtype=torch.uint8, device="cuda") for _ in range(4)]
        xv, lv, xo, lo = (b[o:o + n] for b, o in zip(bufs, off))
        xv.copy_(torch.from_numpy(x.reshape(-1))); lv.copy_(torch.from_numpy(lab.reshape(-1)))
        eng.elastic(xv.view(shape), lv.view(B, H, W), ops, out=(xo.view(shape), lo.view(B, H, W)))
        torch.cuda.synchronize()
        assert np.array_equal(xo.cpu().numpy().reshape(shape), ref_x), off
        assert np.array_equal(lo.cpu().numpy().reshape(B, H, W), ref_l), off
        for b, o in zip(bufs[2:], off[2:]):     # nothing written outside the views
            assert not b[:o].any() and not b[o + n:].any()


def test_determinism_and_batch_position(eng):
    shape = (6, 24, 40, 1)
    x, lab = _batch(shape, seed=4)
    ops = _ops(6, 7)
    a = _run(eng, x, lab, ops)
    b = _run(eng, x, lab, ops)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    moved = _run(eng, x[[4, 0, 3]], lab[[4, 0, 3]], ops[[4, 0, 3]].copy())
    for k, src in enumerate([4, 0, 3]):
        assert np.array_equal(moved[0][k], a[0][src]) and np.array_equal(moved[1][k], a[1][src])


def test_argument_errors_launch_nothing(eng):
    from oct_image_segmentation_models_amd import _hip
    from oct_image_segmentation_models_amd._hip import OctError
    lib = _hip.lib()
    B, H, W, Cn = 2, 8, 16, 1
    n = B * H * W * Cn
    x = torch.zeros(n, dtype=torch.uint8, device="cuda")
    lab = torch.zeros(B * H * W, dtype=torch.uint8, device="cuda")
    good = np.zeros(B, dtype=A.ELASTIC_OP_DTYPE)
    good["kind"], good["border"], good["spacing"], good["amp_x"], good["amp_y"] = 1, [2, 0], [4, 128], 700, [900, 0]
    good["fill"], good["fill_label"] = 9, 1
    ops = torch.from_numpy(good.view(np.uint8).copy()).cuda()
    arena = torch.full((4 * n,), 0x5A, dtype=torch.uint8, device="cuda")       # outputs with a sentinel
    out, lab_out = arena[:n], arena[n:2 * n]
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: None if t is None else t.data_ptr()

    def call(x_=x, lab_=lab, ops_=ops, dims=(B, H, W, Cn), out_=out, lab_out_=lab_out):
        return lib.oct_elastic_batch(p(x_), p(lab_), p(ops_), *dims, p(out_), p(lab_out_), stream)

    bad = [dict(x_=None), dict(ops_=None), dict(out_=None), dict(dims=(0, H, W, Cn)), dict(dims=(B, -1, W, Cn)),
           dict(dims=(B, H, 0, Cn)), dict(dims=(B, H, W, 0)), dict(dims=(65536, H, W, Cn)), dict(dims=(1, 16385, 1, 1)),
           dict(dims=(1, 1, 16385, 1)), dict(dims=(1, 16384, 16384, 8)),
           dict(lab_=None),                                                                    # labels_out without labels
           dict(out_=arena[n - 4:2 * n - 4]),                                                   # out overlaps labels_out
           dict(x_=arena[:n]), dict(x_=arena[4:n + 4]), dict(lab_=arena[16:16 + n]), dict(x_=arena[n:2 * n]),
           dict(ops_=arena[2 * n - 8:])]
    for kw in bad:
        rc = call(**kw)
        assert rc < 0 and b"elastic_batch" in lib.oct_last_error(), kw
    torch.cuda.synchronize()
    assert bool((arena == 0x5A).all())
    assert call() == 0
    torch.cuda.synchronize()
    assert not bool((arena[:n] == 0x5A).any()) and not bool((arena[n:2 * n] == 0x5A).any()) and bool((arena[2 * n:] == 0x5A).all())
    # the Python binding validates descriptors and sizes before upload, and its output tensors
    xv, lv = x.view(B, H, W, Cn), lab.view(B, H, W)
    for field, value in [("kind", 2), ("border", 3), ("spacing", 1), ("spacing", 129), ("amp_x", 8193), ("amp_y", -1), ("fill", 256),
                         ("fill_label", -1), ("reserved", 1)]:
        wrong = good.copy()
        wrong[field][1] = value
        with pytest.raises(OctError, match=field):
            eng.elastic(xv, lv, wrong)
    with pytest.raises(OctError, match="one ELASTIC_OP_DTYPE"):
        eng.elastic(xv, lv, good[:1])
    with pytest.raises(OctError, match="overlaps"):
        eng.elastic(xv, lv, good, out=(xv, torch.empty_like(lv)))          # the stage cannot run in place
    with pytest.raises(OctError, match=r"out\[0\]"):
        eng.elastic(xv, lv, good, out=(torch.empty(xv.shape, dtype=torch.float32, device="cuda"), torch.empty_like(lv)))
    torch.cuda.synchronize()
    assert bool((arena[2 * n:] == 0x5A).all())


# ---- the training path ----------------------------------------------------------------------------------------------------------
CFG = dict(input_channels=1, num_classes=3, image_height=32, image_width=64, start_neurons=8, pool_layers=2)
LIST = [(A.flip_aug, {"flip_type": "left-right"}), (A.column_shift_aug, {"max_shift": 6, "max_tilt": 4, "max_curvature": 3}),
        (A.no_aug, {})]
PROBS = (0.4, 0.4, 0.2)
ELASTIC = {"p": 0.7, "spacing": 8, "max_displacement": (3, 5), "border": "constant", "fill": 0, "fill_label": 0}


def _generator(images, labels, batch, **kw):
    from oct_image_segmentation_models_amd.common.data_generator import DataGenerator
    return DataGenerator(images, labels, batch, LIST, "one", PROBS, True, None, seed=8, **kw)


def _compiled_model(seed=3):
    from oct_image_segmentation_models_amd import optimizers
    from oct_image_segmentation_models_amd.common import custom_losses, custom_metrics
    from oct_image_segmentation_models_amd.models import get_model_class
    model = get_model_class("unet")(**CFG).build_model()
    model.config["seed"] = seed
    loss = custom_losses.custom_loss_objects["dice_loss_macro"]["function"](num_classes=3, is_y_true_sparse=True)
    metric = custom_metrics.training_monitor_metric_objects["dice_coef_macro"](True, 3)
    model.compile(optimizer=optimizers.Adam(learning_rate=2e-3), loss=loss, metrics=[metric])
    return model


def test_the_feed_equals_the_host_generator(eng):
    """``BatchFeed``: upload -> elastic -> warp -> augment on an elastic + flip + column_shift configuration hands the
    network the bytes of the host generator's batches, images and labels, over 2 epochs of 3 batches of 4."""
    from oct_image_segmentation_models_amd.models.batch_feed import BatchFeed
    images, labels = make_scans(12, 32, 64, 3, seed=5)
    dev, host = _generator(images, labels, 4, device_aug=True, elastic=ELASTIC), _generator(images, labels, 4, elastic=ELASTIC)
    feed = BatchFeed("cuda:0")
    stages = set()
    for _ in range(2):
        for i in range(len(dev)):
            b = feed.upload(feed.host_batch(dev, i, 0, 1), i % 3)
            torch.cuda.current_stream().wait_event(b.ready)
            x, lab = feed.augment(eng, dev.oct_aug_seed, b)
            torch.cuda.synchronize()
            feed.release(i % 3)
            X, y = host[i]
            assert x.dtype == torch.float32 and np.array_equal(x.cpu().numpy(), X) and np.array_equal(lab.cpu().numpy(), y[..., 0])
            stages.add((getattr(b, "eops", None) is not None, b.wops is not None))
        dev.on_epoch_end(); host.on_epoch_end()
    assert feed.elastic_out is not None and feed.warp_out is not None and (True, True) in stages


def test_fit_with_elastic_equals_the_engine_stepped_by_hand():
    """``Model.fit`` for two steps of batch 4 against a second model of the same seed whose engine is stepped by hand on the
    batches deformed by ``elastic_reference`` on the host: parameters and state end bit-identical."""
    from oct_image_segmentation_models_amd import optimizers
    images, labels = make_scans(8, 32, 64, 3, seed=5)
    gens = [_generator(images, labels, 4, device_aug=True, elastic=ELASTIC) for _ in range(2)]
    assert all(g.oct_device_aug and len(g) == 2 for g in gens)
    model = _compiled_model()
    hist = model.fit(x=gens[0], epochs=1, verbose=0)
    torch.cuda.synchronize()
    fitted = model._engines["train"]
    assert model.feed.elastic_out is not None and fitted.opt_step == 2

    hand = _compiled_model()
    native = hand._ensure_engine(4, True, hw=(32, 64))
    opt = optimizers.Adam(learning_rate=2e-3)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()     # noqa: E731
    acc, deformed = None, 0
    for _ in range(2):
        x8, lab8, ops, wops, eops = gens[1].next_batch_aug()
        deformed += int(eops["kind"].sum())
        x8, lab8 = A.elastic_reference(x8, lab8, eops)
        x, lab = native.warp(up(x8), up(lab8), wops)
        x, lab = native.augment(x, lab, ops, gens[1].oct_aug_seed)
        native.select_loss("dice")
        native.forward(x, training=True, labels=lab, want_probs=False)
        v = native.loss_selected()
        native.backward(lab, macro=True, loss_scale=1.0)
        opt.apply(native)
        acc = v.clone() if acc is None else acc + v
    torch.cuda.synchronize()
    assert deformed > 0
    assert torch.equal(fitted.params, native.params) and torch.equal(fitted.state, native.state)
    assert bool(torch.isfinite(fitted.params).all()) and hist.history["loss"][0] == float((acc / 2).cpu().numpy()[0])


def test_without_the_keyword_the_launches_are_the_same():
    """``elastic=None`` and a generator built without the keyword: one epoch of ``fit`` lists the same launches, and ends on
    the same bits; with the keyword the list has the elastic kernel and is otherwise the same."""
    images, labels = make_scans(8, 32, 64, 3, seed=5)
    runs = []
    for kw in ({}, {"elastic": None}, {"elastic": dict(ELASTIC, p=1.0)}):
        model = _compiled_model()
        e = model._ensure_engine(4, True, hw=(32, 64))
        # the handle-less stages record into the profiler of the engine that last ran on this thread: an inference forward
        # (it changes no weight and no statistic) makes that this engine before the first batch's stages are queued
        e.forward(torch.zeros((4, 32, 64, 1), dtype=torch.uint8, device="cuda"), training=False)
        e.profile_begin()
        model.fit(x=_generator(images, labels, 4, device_aug=True, **kw), epochs=1, verbose=0)
        torch.cuda.synchronize()
        assert model._engines["train"] is e
        runs.append(([(r["kernel"], r["layer"], r["launches"]) for r in e.profile_end()], e.params.clone()))
    assert runs[0][0] == runs[1][0] and torch.equal(runs[0][1], runs[1][1])
    assert not any("elastic" in k for k, _, _ in runs[0][0])
    extra = [r for r in runs[2][0] if r not in runs[0][0]]
    assert extra == [("elastic_k<true>", "elastic", 2)] and len(runs[2][0]) == len(runs[0][0]) + 1
