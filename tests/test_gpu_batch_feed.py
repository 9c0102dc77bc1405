"""GPU tests of the model's input path and loss selection: ``BatchFeed``'s three upload slots driven directly (copies only),
``UNetEngine.select_loss`` bringing a shared engine back to plain Dice, and ``Model.fit`` with every stage at once -- warp,
augment, pad, ignore label -- against the same engine calls made by hand.  Every comparison is bit for bit: bytes that were
copied, or the same kernels on the same geometry with the same weights (``tests/test_gpu_any_size.py``, section 0)."""
import numpy as np
import pytest
import torch

from oct_image_segmentation_models_amd.common import augmentation as A
from tests.test_gpu_any_size import DEV, _cfg, _engine, _scans, _up, _weights
from tests.test_gpu_masked_loss import _compiled

pytestmark = pytest.mark.gpu


# ---- 1. slot reuse -------------------------------------------------------------------------------------------------------------
def _random_records(rng, n, dtype):
    return np.frombuffer(rng.integers(0, 256, n * dtype.itemsize, dtype=np.uint8).tobytes(), dtype=dtype).copy()


def test_three_slots_deliver_what_was_queued():
    """7 batches through the 3 slots in the order of ``Model._run_epoch`` -- batch i+1 is queued before "step" i, which here
    only copies the slot's tensors on the compute stream behind the ready event and records the slot's done event.  The host
    arrays are overwritten directly after each queue call: the pinned copy is taken at queue time."""
    from oct_image_segmentation_models_amd.models.batch_feed import Batch, BatchFeed
    sizes = [4, 4, 4, 4, 2, 4, 4]              # every slot is refilled; slot 1 is remade smaller (batch 4)
    rng = np.random.default_rng(7)
    feed = BatchFeed(DEV)
    queued, got, seen = [], [], []

    def queue(i):
        n = sizes[i]
        hb = Batch(rng.integers(0, 256, (n, 32, 64, 1), dtype=np.uint8), rng.integers(0, 3, (n, 32, 64), dtype=np.uint8), None,
                   _random_records(rng, n, A.AUG_OP_DTYPE), _random_records(rng, n, A.WARP_OP_DTYPE))
        queued.append([a.tobytes() for a in (hb.x, hb.labels, hb.ops, hb.wops)])
        b = feed.upload(hb, i % 3)
        hb.x[...] = 0xEE; hb.labels[...] = 0xEE; hb.ops.view(np.uint8)[...] = 0xEE; hb.wops.view(np.uint8)[...] = 0xEE
        return b

    compute = torch.cuda.current_stream(DEV)
    nxt = queue(0)
    for i in range(len(sizes)):
        b = nxt
        assert b._fields == ("x", "labels", "ready", "ops", "wops") and isinstance(b.ready, torch.cuda.Event)
        compute.wait_event(b.ready)
        if i + 1 < len(sizes):
            nxt = queue(i + 1)
        got.append([t.clone() for t in (b.x, b.labels, b.ops, b.wops)])            # on the compute stream, behind ready
        seen.append(b)
        feed.release(i % 3)
    torch.cuda.synchronize()
    assert feed.copy is not None and feed.copy != compute and set(feed.done) == set(feed.ready) == {0, 1, 2}
    for i, (want, have) in enumerate(zip(queued, got)):
        assert [t.cpu().numpy().tobytes() for t in have] == want, i
        x, lab, ops, wops = have
        assert x.shape == (sizes[i], 32, 64, 1) and lab.shape == (sizes[i], 32, 64) and x.dtype == lab.dtype == torch.uint8
        assert ops.dtype == wops.dtype == torch.uint8 and (ops.numel(), wops.numel()) == (32 * sizes[i], 40 * sizes[i])
    # buffers are reused while shape and dtype match, and remade when they do not
    for f in ("x", "labels", "ops", "wops"):
        assert getattr(seen[3], f) is getattr(seen[0], f) and getattr(seen[6], f) is getattr(seen[0], f)
        assert getattr(seen[5], f) is getattr(seen[2], f)
        assert getattr(seen[4], f) is not getattr(seen[1], f) and getattr(seen[4], f).shape[0] == getattr(seen[1], f).shape[0] // 2
    assert all(feed.pinned[(k, s)].is_pinned() for k in "xlow" for s in range(3))


# ---- 2. the loss state of a shared engine ---------------------------------------------------------------------------------------
CW = (0.5, 1.25, 2.0)


@pytest.mark.parametrize("kind", ["focal", "bce"])
def test_a_shared_engine_comes_back_to_plain_dice(kind):
    """An engine used under focal (class weights) or BCE with ignore label 200, then selected for plain Dice without one: a
    training forward, loss and backward equal those of a fresh engine with the same weights that never left plain Dice
    (its ``loss_selected`` is ``loss_dice``: the kind of an engine that nothing was selected on)."""
    cfg = _cfg(32, 64, pool_layers=3)
    w = _weights(cfg, 5)
    images, labels = _scans(2, 32, 64, 41)
    x, lab = _up(images), _up(labels[..., 0])
    masked = labels[..., 0].copy(); masked[0, 4:20, 8:40] = 200
    shared, fresh = _engine(cfg, w, 2, training=True), _engine(cfg, w, 2, training=True)
    focal = dict(focal_loss_weight=0.35, gamma=2.0, class_weight=CW) if kind == "focal" else {}
    shared.select_loss(kind, ignore_label=200, **focal)
    assert shared.ignore_label == 200 and (shared._focal_active, shared._bce_active) == (kind == "focal", kind == "bce")
    shared.forward(x, training=False, labels=_up(masked), want_probs=False)      # (inference: the moving statistics stay)
    other = shared.loss_selected()
    assert other.numel() == 8 and bool(torch.isfinite(other).all())
    if kind == "focal":          # the same parameters by value select nothing anew; other ones do
        buf = shared._focal_cw
        shared.select_loss(kind, ignore_label=200, **dict(focal, class_weight=list(CW)))
        assert shared._focal_cw is buf
        shared.select_loss(kind, ignore_label=200, **dict(focal, class_weight=(0.5, 1.25, 2.5)))
        assert shared._focal_cw is not buf and shared._focal_cw.cpu().tolist() == [0.5, 1.25, 2.5]
    shared.select_loss("dice")
    assert shared.ignore_label is None and not shared._focal_active and not shared._bce_active
    out = []
    for eng in (shared, fresh):
        eng.set_dropout_step(1)
        eng.forward(x, training=True, labels=lab, want_probs=False)
        v = eng.loss_selected()
        eng.backward(lab, macro=True, loss_scale=1.0)
        out.append((v.cpu().numpy(), eng.grads.cpu().numpy(), eng.state.cpu().numpy()))
    assert out[0][0].shape == (4,) and np.isfinite(out[1][1]).all() and np.abs(out[1][1]).max() > 0
    assert all(np.array_equal(a, b) for a, b in zip(*out))


# ---- 3. all stages at once ------------------------------------------------------------------------------------------------------
AUGS = [(A.flip_aug, {"flip_type": "left-right"}), (A.add_noise_aug, {"mode": "gaussian"}),
        (A.column_shift_aug, {"max_shift": 6, "max_tilt": 4, "max_curvature": 3})]


def test_fit_with_every_stage_equals_the_engine_driven_by_hand():
    """``fit`` over 5 batches of 4 at 36 x 68 with three pool levels (engine: 40 x 72, placement (2, 2)), compiled with
    ``pad_mode="edge"`` and ``ignore_label=200``, over a device-augmenting generator with a flip, a noise and a column shift,
    against a second model of the same seed whose engine is driven by hand: the weights end bit-identical (the criterion of
    the fit-against-engine comparisons of test_gpu_masked_loss.py and test_gpu_warp.py)."""
    from oct_image_segmentation_models_amd import optimizers
    from oct_image_segmentation_models_amd.common.data_generator import DataGenerator
    from oct_image_segmentation_models_amd.common.utils import padded_geometry
    assert padded_geometry(36, 68, 3) == (40, 72, 2, 2)
    cfg = _cfg(32, 64, pool_layers=3)
    w0 = _weights(cfg, 5)
    images, labels = _scans(20, 36, 68, 51)
    labels = labels.copy(); labels[::3, 5:15, 20:50] = 200
    gens = [DataGenerator(images, labels, 4, AUGS, "one", (0.3, 0.3, 0.4), True, None, seed=9, device_aug=True) for _ in range(2)]
    assert all(g.oct_device_aug and len(g) == 5 for g in gens)

    model = _compiled(cfg, w0, ignore_label=200, pad_mode="edge")
    hist = model.fit(x=gens[0], epochs=1, verbose=0)
    torch.cuda.synchronize()
    eng = model._engines["train"]
    assert (eng.cfg.H, eng.cfg.W) == (40, 72) and eng.opt_step == 5 and eng.ignore_label == 200 and len(eng._pad_bufs) == 1
    assert model.feed.warp_out is not None and model.feed.aug_out is not None       # both stages ran

    hand = _compiled(cfg, w0, ignore_label=200, pad_mode="edge")
    native = hand._ensure_engine(4, True, hw=(40, 72))
    opt = optimizers.Adam(learning_rate=2e-3)
    acc, warped = None, 0
    for _ in range(5):
        x8, lab8, ops, wops = gens[1].next_batch_aug()
        warped += int(wops["kind"].any())
        x, lab = native.warp(_up(x8), _up(lab8), wops)
        x, lab = native.augment(x, lab, ops, gens[1].oct_aug_seed)
        xp = native.pad(x, 40, 72, 2, 2, "edge", 0.0)
        lp = native.pad(lab.view(4, 36, 68, 1), 40, 72, 2, 2, "constant", 200)
        native.select_loss("dice", ignore_label=200)
        native.forward(xp, training=True, labels=lp, want_probs=False)
        v = native.loss_selected()
        native.backward(lp, macro=True, loss_scale=1.0)
        opt.apply(native)
        acc = v.clone() if acc is None else acc + v
    torch.cuda.synchronize()
    assert warped > 0
    assert torch.equal(eng.params, native.params) and torch.equal(eng.state, native.state)
    got, want = model.get_weights(), hand.get_weights()
    assert len(got) == len(want) == len(w0) and all(np.array_equal(a, b) for a, b in zip(got, want))
    assert not all(np.array_equal(a, b) for a, b in zip(got, w0)) and all(np.isfinite(a).all() for a in got)
    acc = (acc / 5).cpu().numpy()
    assert hist.history["loss"][0] == float(acc[0]) and hist.history["dice_coef_macro"][0] == float(acc[2])
