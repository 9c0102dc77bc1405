"""GPU tests of ``oct_photo_batch`` (include/oct_unet.h) and of the training path that uses it, against the numpy
restatement ``common.augmentation.photometric_reference``.  The definition is integer arithmetic: every comparison is byte
for byte."""
import ctypes as C

import numpy as np
import pytest
import torch

import photo_cases as pc
from oct_image_segmentation_models_amd.common import augmentation as A
from oct_image_segmentation_models_amd.common.synthetic import make_scans

pytestmark = pytest.mark.gpu

# The kernel's tile is 32 x 128 pixels.  (1,5,7,1): smaller than the halo, guarded byte stores; (3,20,34,1) likewise, three
# samples; (2,36,68,3): channels, two tiles down; (2,64,128,1): whole tiles, word stores; (1,130,134,1): five tiles down and
# two across, the second 6 columns wide (narrower than the halo), byte stores (134 % 4 != 0); (1,40,300,1): two tiles down,
# three across with a cut last one, word stores
SHAPES = [(1, 5, 7, 1), (3, 20, 34, 1), (2, 36, 68, 3), (2, 64, 128, 1), (1, 130, 134, 1), (1, 40, 300, 1)]


@pytest.fixture(scope="module")
def eng():
    from oct_image_segmentation_models_amd.engine import UNetEngine
    return UNetEngine(device="cuda:0", input_channels=1, num_classes=3, image_height=16, image_width=32, start_neurons=8,
                      pool_layers=2, max_batch=1, training=False)


def _images(shape, seed=0):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


def _run(eng, x, ops):
    out = eng.photometric(torch.from_numpy(x).cuda(), ops)
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("shape", SHAPES)
def test_kernel_equals_the_restatement(eng, shape):
    """Every flag combination x every radius 0..8 and the extreme weights, 0..4 shadows with their edge cases, identity and
    permutation tables (tests/photo_cases.py), mixed inside the batches in a fixed shuffled order.  The descriptors of one
    shape run as ONE batch over repeated images, so a shape is one launch and one restatement."""
    B, H, W, _ = shape
    ops = pc.combos(H, W)
    x = _images(shape, seed=1)[np.arange(len(ops)) % B]
    out = _run(eng, x, ops)
    ref = A.photometric_reference(x, ops)
    assert out.dtype == np.uint8 and out.shape == x.shape
    wrong = [(i, int(ops[i]["kind"]), int(ops[i]["radius"])) for i in range(len(ops)) if not np.array_equal(out[i], ref[i])]
    assert not wrong, wrong


def test_flags_side_by_side(eng):
    """(8, 40, 132, 1): each flag alone beside kind 0: a copy where the kind is 0 or the part is an identity, other bytes
    elsewhere; a shadow changes its columns below y0 and nothing else."""
    shape = (8, 40, 132, 1)
    x = _images(shape, seed=2)
    sh = [(60, 4, 10, 256)]
    perm = pc.tables()[1]
    ops = np.array([pc.make_op(0, 8, sh, perm), pc.make_op(1, 2), pc.make_op(2, 0, sh), pc.make_op(4, 0, [], perm), pc.make_op(1, "centre"),
                    pc.make_op(4), pc.make_op(2, 0, [(60, 4, 40, 256)]), pc.make_op(7, "far", sh, perm)])
    out = _run(eng, x, ops)
    assert np.array_equal(out, A.photometric_reference(x, ops))
    for b in range(8):
        assert np.array_equal(out[b], x[b]) == (b in (0, 4, 5, 6)), b
    same = out[2] == x[2]
    assert same[:10].all() and same[:, :57].all() and same[:, 64:].all() and (out[2, 10:, 60] == 0).all()
    assert np.array_equal(out[3], perm[x[3]])


def test_unaligned_views_take_the_guarded_path(eng):
    """The same bytes from views offset by one byte (input, output, both), and nothing written outside the view."""
    shape = (2, 40, 132, 1)
    n = int(np.prod(shape))
    x = _images(shape, seed=3)
    ops = np.array([pc.make_op(7, 8, pc.shadow_sets(40, 132)[3], pc.tables()[1]), pc.make_op(3, 3, pc.shadow_sets(40, 132)[2])])
    ref = A.photometric_reference(x, ops)
    for off in [(0, 0), (1, 0), (0, 1), (1, 1), (3, 2)]:
        bufs = [torch.zeros(n + 8, dtype=torch.uint8, device="cuda") for _ in range(2)]
        xv, xo = (b[o:o + n] for b, o in zip(bufs, off))
        xv.copy_(torch.from_numpy(x.reshape(-1)))
        got = eng.photometric(xv.view(shape), ops, out=xo.view(shape))
        torch.cuda.synchronize()
        assert got.data_ptr() == xo.data_ptr() and np.array_equal(xo.cpu().numpy().reshape(shape), ref), off
        assert not bufs[1][:off[1]].any() and not bufs[1][off[1] + n:].any()        # nothing written outside the view


def test_determinism_and_batch_position(eng):
    shape = (6, 40, 140, 1)
    x = _images(shape, seed=4)
    ops = pc.batch_ops(pc.combos(40, 140), 6, 11)
    a, b = _run(eng, x, ops), _run(eng, x, ops)
    assert np.array_equal(a, b)
    moved = _run(eng, x[[4, 0, 3]], ops[[4, 0, 3]].copy())
    for k, src in enumerate([4, 0, 3]):
        assert np.array_equal(moved[k], a[src])


def test_argument_errors_launch_nothing(eng):
    from oct_image_segmentation_models_amd import _hip
    from oct_image_segmentation_models_amd._hip import OctError
    lib = _hip.lib()
    B, H, W, Cn = 2, 8, 16, 1
    n = B * H * W * Cn
    x = torch.zeros(n, dtype=torch.uint8, device="cuda")
    good = np.array([pc.make_op(7, 5, pc.shadow_sets(H, W)[4], pc.tables()[1]), pc.make_op(1, 2)])
    ops = torch.from_numpy(good.view(np.uint8).copy()).cuda()
    arena = torch.full((4 * n + 1024,), 0x5A, dtype=torch.uint8, device="cuda")       # the output, with a sentinel
    out = arena[:n]
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: None if t is None else t.data_ptr()      # noqa: E731

    def call(x_=x, ops_=ops, dims=(B, H, W, Cn), out_=out):
        return lib.oct_photo_batch(p(x_), p(ops_), *dims, p(out_), stream)

    bad = [dict(x_=None), dict(ops_=None), dict(out_=None), dict(dims=(0, H, W, Cn)), dict(dims=(B, -1, W, Cn)),
           dict(dims=(B, H, 0, Cn)), dict(dims=(B, H, W, 0)), dict(dims=(65536, H, W, Cn)), dict(dims=(1, 16385, 1, 1)),
           dict(dims=(1, 1, 16385, 1)), dict(dims=(1, 1, 1, 16385)), dict(dims=(1, 16384, 16384, 8)),
           dict(x_=arena[:n]), dict(x_=arena[4:n + 4]), dict(x_=arena[n - 1:2 * n - 1]),          # out overlaps x
           dict(ops_=arena[n - 4:n - 4 + 640]), dict(ops_=arena[0:640]),                           # out overlaps ops
           dict(ops_=ops[1:])]                                                                 # descriptors off a word boundary
    for kw in bad:
        rc = call(**kw)
        assert rc < 0 and b"photo_batch" in lib.oct_last_error(), kw
    torch.cuda.synchronize()
    assert bool((arena == 0x5A).all())
    assert call() == 0
    torch.cuda.synchronize()
    assert not bool((arena[:n] == 0x5A).any()) and bool((arena[n:] == 0x5A).all())
    # the Python binding validates descriptors and sizes before upload, and its output tensor
    xv = x.view(B, H, W, Cn)
    for field, index, value in [("kind", None, 8), ("radius", None, 9), ("n_shadows", None, 5), ("reserved", None, 1), ("hw", 1, 0),
                                ("y0", 0, -1), ("strength", 2, 257)]:
        wrong = good.copy()
        if index is None:
            wrong[field][0] = value
        else:
            wrong[field][0][index] = value
        with pytest.raises(OctError, match=field):
            eng.photometric(xv, wrong)
    wrong = good.copy()
    wrong["w"][0][0] = 39
    with pytest.raises(OctError, match="256"):
        eng.photometric(xv, wrong)
    with pytest.raises(OctError, match="one PHOTO_OP_DTYPE"):
        eng.photometric(xv, good[:1])
    with pytest.raises(OctError, match="overlaps"):
        eng.photometric(xv, good, out=xv)                              # the stage cannot run in place
    with pytest.raises(OctError, match=r"out\[0\]"):
        eng.photometric(xv, good, out=torch.empty(xv.shape, dtype=torch.float32, device="cuda"))
    torch.cuda.synchronize()
    assert bool((arena[n:] == 0x5A).all())


def test_the_stage_records_into_a_graph(eng):
    """Captured once and replayed twice on new input: no allocation, no host synchronisation inside the call."""
    shape = (3, 40, 132, 1)
    ops_np = pc.batch_ops(pc.combos(40, 132), 3, 5)
    ops = torch.from_numpy(ops_np.view(np.uint8).copy()).cuda()
    xin, out = torch.zeros(shape, dtype=torch.uint8, device="cuda"), torch.zeros(shape, dtype=torch.uint8, device="cuda")
    eng.photometric(xin, ops, out=out)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        eng.photometric(xin, ops, out=out)
    for seed in (5, 6):
        x = _images(shape, seed=seed)
        xin.copy_(torch.from_numpy(x))
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), A.photometric_reference(x, ops_np))


# ---- the training path ----------------------------------------------------------------------------------------------------------
CFG = dict(input_channels=1, num_classes=3, image_height=32, image_width=64, start_neurons=8, pool_layers=2)
LIST = [(A.flip_aug, {"flip_type": "left-right"}), (A.column_shift_aug, {"max_shift": 6, "max_tilt": 4, "max_curvature": 3}),
        (A.no_aug, {})]
PROBS = (0.4, 0.4, 0.2)
ELASTIC = {"p": 0.7, "spacing": 8, "max_displacement": (3, 5), "border": "constant", "fill": 0, "fill_label": 0}
PHOTO = {"p": 0.8, "gamma": (0.5, 2.0), "brightness": 0.2, "contrast": (0.7, 1.5), "blur": {"p": 0.6, "sigma": (0.4, 2.6)},
         "shadows": {"p": 0.7, "max_count": 4, "width": (2, 9), "strength": (0.2, 1.0), "top": (0.1, 0.6)}}


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
    """``BatchFeed``: upload -> elastic -> photometric -> warp -> augment hands the network the bytes of the host
    generator's batches, images and labels, over 2 epochs of 3 batches of 4 at 32 x 64."""
    from oct_image_segmentation_models_amd.models.batch_feed import BatchFeed
    images, labels = make_scans(12, 32, 64, 3, seed=5)
    dev = _generator(images, labels, 4, device_aug=True, elastic=ELASTIC, photometric=PHOTO)
    host = _generator(images, labels, 4, elastic=ELASTIC, photometric=PHOTO)
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
            stages.add((getattr(b, "eops", None) is not None, getattr(b, "pops", None) is not None, b.wops is not None))
        dev.on_epoch_end(); host.on_epoch_end()
    assert feed.elastic_out is not None and feed.photo_out is not None and feed.warp_out is not None and (True, True, True) in stages


def test_fit_with_photometric_equals_the_engine_stepped_by_hand():
    """``Model.fit`` for two steps of batch 4 against a second model of the same seed whose engine is stepped by hand on the
    batches that ``photometric_reference`` changed on the host: parameters, state and loss end bit-identical."""
    from oct_image_segmentation_models_amd import optimizers
    images, labels = make_scans(8, 32, 64, 3, seed=5)
    gens = [_generator(images, labels, 4, device_aug=True, photometric=PHOTO) for _ in range(2)]
    assert all(g.oct_device_aug and len(g) == 2 for g in gens)
    model = _compiled_model()
    hist = model.fit(x=gens[0], epochs=1, verbose=0)
    torch.cuda.synchronize()
    fitted = model._engines["train"]
    assert model.feed.photo_out is not None and model.feed.elastic_out is None and fitted.opt_step == 2

    hand = _compiled_model()
    native = hand._ensure_engine(4, True, hw=(32, 64))
    opt = optimizers.Adam(learning_rate=2e-3)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()     # noqa: E731
    acc, changed = None, 0
    for _ in range(2):
        x8, lab8, ops, wops, eops, pops = gens[1].next_batch_aug()
        assert eops is None
        changed += int((pops["kind"] != 0).sum())
        x8 = A.photometric_reference(x8, pops)
        x, lab = native.warp(up(x8), up(lab8), wops)
        x, lab = native.augment(x, lab, ops, gens[1].oct_aug_seed)
        native.select_loss("dice")
        native.forward(x, training=True, labels=lab, want_probs=False)
        v = native.loss_selected()
        native.backward(lab, macro=True, loss_scale=1.0)
        opt.apply(native)
        acc = v.clone() if acc is None else acc + v
    torch.cuda.synchronize()
    assert changed > 0
    assert torch.equal(fitted.params, native.params) and torch.equal(fitted.state, native.state)
    assert bool(torch.isfinite(fitted.params).all()) and hist.history["loss"][0] == float((acc / 2).cpu().numpy()[0])


def test_without_the_keyword_the_launches_are_the_same():
    """``photometric=None`` and a generator built without the keyword: one epoch of ``fit`` lists the same launches, and
    ends on the same bits; with the keyword the list gains exactly the photometric kernel."""
    images, labels = make_scans(8, 32, 64, 3, seed=5)
    on = {"p": 1.0, "gamma": (1.5, 2.0), "blur": {"sigma": (1.0, 2.0)}}        # every sample has a kind
    runs = []
    for kw in ({}, {"photometric": None}, {"photometric": on}):
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
    assert not any("photo" in k for k, _, _ in runs[0][0])
    extra = [r for r in runs[2][0] if r not in runs[0][0]]
    assert extra == [("photo_k<true>", "photometric", 2)] and len(runs[2][0]) == len(runs[0][0]) + 1
