"""CPU tests of ``models.batch_feed.BatchFeed``, the input path of ``Model.fit`` / ``evaluate``, on ``Model(..., device="cpu")``
without an engine: the three routes of ``host_batch`` (device augmentation, the uint8 fast path, a Keras ``Sequence``), the
five-field record every stage hands on, the upload without a GPU (host tensors, no event), the per-rank slices and the staging
buffers behind ``Model._staged``.  No GPU, no library call; every comparison is for equality."""
import numpy as np
import pytest
import torch

from oct_image_segmentation_models_amd import parallel
from oct_image_segmentation_models_amd.common import augmentation as A
from oct_image_segmentation_models_amd.common.data_generator import DataGenerator
from oct_image_segmentation_models_amd.models.batch_feed import Batch, BatchFeed
from oct_image_segmentation_models_amd.models.engine_model import Model

H, W, C = 8, 12, 3
SHIFT = (A.column_shift_aug, {"max_shift": 3, "max_tilt": 2, "max_curvature": 1.5})
FLIP = (A.flip_aug, {"flip_type": "left-right"})
NONE = (A.no_aug, {})


def _data(n=12, seed=0):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (n, H, W, 1), dtype=np.uint8), rng.integers(0, C, (n, H, W, 1), dtype=np.uint8)


def _feed():
    m = Model("unet", dict(input_channels=1, num_classes=C, image_height=H, image_width=W, pool_layers=2), device="cpu")
    assert m._feed is None                                     # made at first use, on the device the model has by then
    feed = m.feed
    assert isinstance(feed, BatchFeed) and m.feed is feed and feed.device == torch.device("cpu") and m._engine is None
    return m, feed


class _Sequence:
    """``keras.utils.Sequence`` duck type: float64 images in a non-contiguous layout, one-hot or (B,H,W,1) sparse labels."""

    def __init__(self, batch, one_hot, n=12):
        self.images, self.labels = _data(n, seed=batch)
        self.batch, self.one_hot = batch, one_hot

    def __len__(self):
        return len(self.images) // self.batch

    def __getitem__(self, i):
        x = np.asfortranarray(self.images[i * self.batch:(i + 1) * self.batch].astype(np.float64) / 255.0)
        lab = self.labels[i * self.batch:(i + 1) * self.batch]
        return x, (np.eye(C, dtype=np.float64)[lab[..., 0]] if self.one_hot else lab.astype(np.float64))


def _fields(b):
    assert isinstance(b, Batch) and b._fields == ("x", "labels", "ready", "ops", "wops") and len(b) == 5
    return b


@pytest.mark.parametrize("one_hot", [True, False])
def test_keras_route(one_hot):
    _, feed = _feed()
    seq = _Sequence(4, one_hot)
    hb = _fields(feed.host_batch(seq, 1, 0, 1))
    assert hb.ready is None and hb.ops is None and hb.wops is None
    assert hb.x.dtype == np.float32 and hb.x.flags["C_CONTIGUOUS"] and hb.x.shape == (4, H, W, 1)
    assert np.array_equal(hb.x, (seq.images[4:8].astype(np.float64) / 255.0).astype(np.float32))
    assert hb.labels.dtype == np.uint8 and hb.labels.shape == (4, H, W)         # arg-max of one-hot / sparse reshaped
    assert np.array_equal(hb.labels, seq.labels[4:8, ..., 0])
    b = _fields(feed.upload(hb, 1))
    assert b.ready is None and b.ops is None and b.wops is None                  # no GPU: host tensors and no event
    assert isinstance(b.x, torch.Tensor) and b.x.device.type == "cpu" and b.x.dtype == torch.float32
    assert np.array_equal(b.x.numpy(), hb.x) and b.labels.dtype == torch.uint8 and np.array_equal(b.labels.numpy(), hb.labels)
    feed.release(1)                                                              # nothing to record without a copy stream
    assert feed.copy is None and feed.done == {} and feed.ready == {} and feed.dev == {}


def test_fast_path_route():
    _, feed = _feed()
    im, lb = _data()
    gen, twin = (DataGenerator(im, lb, 4, [], "none", (), False, None, seed=5) for _ in range(2))
    assert gen.oct_fast_path and not gen.oct_device_aug
    for i in range(len(gen)):
        hb = _fields(feed.host_batch(gen, i, 0, 1))
        X, lab = twin.next_batch_u8()
        assert hb.ready is None and hb.ops is None and hb.wops is None
        assert hb.x.dtype == np.uint8 and np.array_equal(hb.x, X) and hb.labels.dtype == np.uint8 and np.array_equal(hb.labels, lab)
        b = _fields(feed.upload(hb, i % 3))
        assert b.ready is None and b.ops is None and b.wops is None and b.x.dtype == torch.uint8
        assert np.array_equal(b.x.numpy(), X) and np.array_equal(b.labels.numpy(), lab)


def test_device_aug_route_without_a_warp_in_the_list():
    _, feed = _feed()
    im, lb = _data()
    gen, twin = (DataGenerator(im, lb, 4, [FLIP, NONE], "all", (), True, None, seed=3, device_aug=True) for _ in range(2))
    assert gen.oct_device_aug
    hb = _fields(feed.host_batch(gen, 0, 0, 1))
    x, lab, ops = twin.next_batch_aug()
    assert hb.ready is None and hb.wops is None and hb.ops.dtype == A.AUG_OP_DTYPE and hb.ops.tobytes() == ops.tobytes()
    assert hb.x.dtype == np.uint8 and np.array_equal(hb.x, x) and np.array_equal(hb.labels, lab)
    b = _fields(feed.upload(hb, 0))
    assert b.ready is None and b.wops is None and b.ops.dtype == torch.uint8 and b.ops.numpy().tobytes() == ops.tobytes()


def test_device_aug_route_drops_the_warp_descriptors_of_a_slice_without_a_warped_sample():
    """Mode "all" over [no_aug, column_shift], global batch 2: sample 0 of every batch is not warped, sample 1 is.  Rank 0 of 2
    holds no warped sample -- ``wops`` is None, the stage is skipped --, rank 1 and the one-rank run hold one."""
    _, feed = _feed()
    im, lb = _data()
    make = lambda: DataGenerator(im, lb, 2, [NONE, SHIFT], "all", (), True, None, seed=3, device_aug=True)      # noqa: E731
    for rank, world, shard in ((0, 2, (0, 1)), (1, 2, (1, 2)), (0, 1, None)):
        gen, twin = make(), make()
        for i in range(3):
            hb = _fields(feed.host_batch(gen, i, rank, world))
            x, lab, ops, wops = twin.next_batch_aug(shard)
            assert np.array_equal(hb.x, x) and np.array_equal(hb.labels, lab) and hb.ops.tobytes() == ops.tobytes()
            b = _fields(feed.upload(hb, i % 3))
            assert b.ready is None and b.ops.numpy().tobytes() == ops.tobytes()
            if (rank, world) == (0, 2):
                assert not wops["kind"].any() and hb.wops is None and b.wops is None
            else:
                assert wops["kind"].any() and hb.wops.dtype == A.WARP_OP_DTYPE and hb.wops.tobytes() == wops.tobytes()
                assert b.wops.dtype == torch.uint8 and b.wops.numpy().tobytes() == wops.tobytes()


def _routes(batch):
    """One Sequence per route and call (the generators are stateful), all of global batch ``batch``."""
    im, lb = _data()
    return {"keras": lambda: _Sequence(batch, True),
            "fast": lambda: DataGenerator(im, lb, batch, [], "none", (), False, None, seed=5),
            "device_aug": lambda: DataGenerator(im, lb, batch, [FLIP, SHIFT], "one", (0.5, 0.5), True, None, seed=5, device_aug=True)}


@pytest.mark.parametrize("route", ["keras", "fast", "device_aug"])
def test_two_ranks_take_the_slices_of_shard_batch(route):
    """Global batch 6: the slices of ranks 0 and 1 of 2 are ``parallel.shard_batch``'s and concatenate to the one-rank batch.
    Global batch 5 does not split evenly: ``shard_batch`` refuses it (equal shards are what makes the mean of the replicas'
    macro Dice the global one), and so does every route, on every rank."""
    _, feed = _feed()
    make = _routes(6)[route]
    whole = feed.host_batch(make(), 0, 0, 1)
    parts = [feed.host_batch(make(), 0, rank, 2) for rank in (0, 1)]
    assert whole.x.shape[0] == 6
    for rank, part in enumerate(parts):
        lo, hi = parallel.shard_batch(6, rank, 2)
        assert (lo, hi) == (3 * rank, 3 * rank + 3)
        for got, full in zip(_fields(part), whole):
            if full is not None and got is not None:        # (wops: a slice without a warped sample drops them)
                assert got.dtype == full.dtype and got.tobytes() == full[lo:hi].tobytes()
        assert (part.ops is None) == (whole.ops is None) and part.ready is None
    for k in (0, 1):
        assert np.array_equal(np.concatenate([p[k] for p in parts]), whole[k])
    for rank in (0, 1):
        with pytest.raises(ValueError, match="not divisible"):
            feed.host_batch(_routes(5)[route](), 0, rank, 2)
    assert feed.host_batch(_routes(5)[route](), 0, 0, 1).x.shape[0] == 5


def test_staged_buffers():
    m, feed = _feed()
    a = np.arange(24, dtype=np.uint8).reshape(2, 3, 4)
    src = a.copy()
    buf = m._staged(("x", 0), src)
    assert isinstance(buf, torch.Tensor) and buf.dtype == torch.uint8 and buf.is_pinned() == torch.cuda.is_available()
    src[...] = 0                                                       # the buffer holds a copy
    assert np.array_equal(buf.numpy(), a)
    again = m._staged(("x", 0), a + 1)                                 # same key, shape and dtype: the same buffer, refilled
    assert again is buf and np.array_equal(buf.numpy(), a + 1) and feed.pinned[("x", 0)] is buf
    assert feed.staged(("x", 0), a) is buf
    other_key = m._staged(("l", 0), a)
    assert other_key is not buf and np.array_equal(other_key.numpy(), a)
    smaller = m._staged(("x", 0), a[:1])                               # another shape: a new buffer
    assert smaller is not buf and smaller.shape == (1, 3, 4) and np.array_equal(smaller.numpy(), a[:1])
    as_f32 = m._staged(("x", 0), a[:1].astype(np.float32))             # another dtype: a new buffer
    assert as_f32 is not smaller and as_f32.dtype == torch.float32 and np.array_equal(as_f32.numpy(), a[:1])
    strided = m._staged(("s", 0), a[:, ::2])                           # a non-contiguous source is packed
    assert strided.is_contiguous() and np.array_equal(strided.numpy(), a[:, ::2])
