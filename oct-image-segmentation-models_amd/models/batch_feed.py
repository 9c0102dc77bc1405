"""``BatchFeed``: the host-to-device input path of ``Model.fit`` / ``evaluate`` -- one GLOBAL batch of the Sequence -> this
rank's host arrays -> pinned staging -> device slot on the copy stream -> the elastic, photometric, warp and augment stages on
the compute stream.  One feed per ``Model``; every stage hands on the same five-field ``Batch`` record (``ElasticBatch``, one
field more, for a batch with an elastically deformed sample; ``PhotoBatch``, two more, for one with a sample that goes
through the photometric stage)."""
from __future__ import annotations

from typing import NamedTuple, Optional

import numpy as np
import torch

from .. import parallel


class Batch(NamedTuple):
    """One batch on its way into a step.  A field that does not apply is None."""
    x: object                       # images: host array, or (uploaded) tensor
    labels: object                  # sparse uint8 labels, likewise
    ready: Optional[torch.cuda.Event] = None    # the H2D copies of this batch have executed; None: host tensors
    ops: object = None              # device augmentation: one AUG_OP_DTYPE descriptor per sample (uploaded: their bytes)
    wops: object = None             # one WARP_OP_DTYPE descriptor per sample, where the slice holds a warped sample


class ElasticBatch(NamedTuple):
    """A ``Batch`` whose slice holds an elastically deformed sample: the same fields, and the stage's descriptors."""
    x: object
    labels: object
    ready: Optional[torch.cuda.Event] = None
    ops: object = None
    wops: object = None
    eops: object = None             # one ELASTIC_OP_DTYPE descriptor per sample (uploaded: their bytes)


class PhotoBatch(NamedTuple):
    """A ``Batch`` whose slice holds a sample that goes through the photometric stage: ``ElasticBatch``'s fields (``eops``
    is None where no sample is deformed), and the stage's descriptors."""
    x: object
    labels: object
    ready: Optional[torch.cuda.Event] = None
    ops: object = None
    wops: object = None
    eops: object = None
    pops: object = None             # one PHOTO_OP_DTYPE descriptor per sample (uploaded: their bytes)


def _record(x, labels, ready, ops, wops, eops, pops=None):
    if pops is not None:
        return PhotoBatch(x, labels, ready, ops, wops, eops, pops)
    return Batch(x, labels, ready, ops, wops) if eops is None else ElasticBatch(x, labels, ready, ops, wops, eops)


def _pair(pair, x, lab, dtype):
    """``pair`` while it still fits (x, lab), else a new (images of ``dtype``, labels) pair beside them."""
    if pair is None or pair[0].shape != x.shape or pair[1].shape != lab.shape or pair[0].device != x.device:
        pair = (torch.empty(x.shape, dtype=dtype, device=x.device), torch.empty_like(lab))
    return pair


class BatchFeed:
    def __init__(self, device):
        self.device = torch.device(device)
        self.copy = None        # the copy stream, made at the first upload to a GPU
        self.pinned = {}        # key, e.g. ("x", slot) -> staging buffer (pinned where there is a GPU), holding a copy of the array
        self.dev = {}           # (kind, slot) -> device buffer
        self.ready = {}         # slot -> event: the H2D copies that last read the slot's pinned buffers
        self.done = {}          # slot -> event: the step that last read the slot's device buffers
        self.elastic_out = None # the elastic stage's (images uint8, labels) pair
        self.photo_out = None   # the photometric stage's uint8 images (it leaves the labels alone)
        self.warp_out = None    # the warp stage's (images uint8, labels) pair
        self.aug_out = None     # the augment stage's (images float32, labels) pair

    def host_batch(self, seq, index, rank, world) -> Batch:
        """One GLOBAL batch from the Sequence -> this rank's (x, sparse uint8 labels) host arrays; for a Sequence that
        augments on the device (``oct_device_aug``) the raw uint8 images and ``ops``, the per-sample descriptors --
        and ``wops``, the warp descriptors, where this rank's slice holds a sample that is warped; likewise ``eops``, the
        elastic descriptors (an ``ElasticBatch``), where it holds a sample that is deformed, and ``pops``, the photometric
        descriptors (a ``PhotoBatch``), where it holds a sample with a non-zero ``kind``."""
        if getattr(seq, "oct_device_aug", False):
            hb = seq.next_batch_aug(parallel.shard_batch(seq.batch_size, rank, world) if world > 1 else None)
            # no sample of a stage's kind in the slice: the stage is skipped
            wops, eops, pops = (hb[k] if len(hb) > k and hb[k] is not None and hb[k]["kind"].any() else None for k in (3, 4, 5))
            return _record(hb[0], hb[1], None, hb[2], wops, eops, pops)
        if getattr(seq, "oct_fast_path", False):
            if world > 1:      # gather this rank's slice only (8 ranks: 1/8 of the host work per step and rank)
                return Batch(*seq.next_batch_u8(parallel.shard_batch(seq.batch_size, rank, world)))
            X, lab = seq.next_batch_u8()
        else:
            X, y = seq[index]
            X = np.ascontiguousarray(X, dtype=np.float32)
            y = np.asarray(y)
            lab = (np.argmax(y, axis=-1) if (y.ndim == 4 and y.shape[-1] > 1) else y.reshape(y.shape[:3])).astype(np.uint8)
        lo, hi = parallel.shard_batch(X.shape[0], rank, world)
        return Batch(X[lo:hi], lab[lo:hi])

    def upload(self, hb: Batch, slot: int) -> Batch:
        """Queue the upload of one batch into device slot ``slot`` on the COPY stream (never on the compute stream: 8 MB of
        uint8 per 32-scan batch would otherwise sit in front of every step).  Pinned staging buffers and device buffers come
        in THREE slots: slot s is refilled only after the step that last read its device tensors has finished -- a HOST
        wait on that step's event, two steps back, which also keeps this thread at most two steps ahead of the GPU.  (With two
        slots the copy had to wait for the previous step on the copy stream; the H2D call then held the host until that
        step was over and every step started with the launch latency exposed: 0.91 of the resident-input rate.)
        ``ops`` (device augmentation: one 32-byte descriptor per sample) travels through the same slot as raw bytes, and so
        does ``wops`` (one 40-byte warp descriptor per sample) and ``eops`` (one 40-byte elastic descriptor per sample)
        and ``pops`` (one 320-byte photometric descriptor per sample).
        Returns the batch on the device with its ready event; without a GPU, host tensors and no event."""
        raw = lambda a: None if a is None else np.ascontiguousarray(a).view(np.uint8)       # noqa: E731
        host = {"x": np.ascontiguousarray(hb.x), "l": np.ascontiguousarray(hb.labels), "o": raw(hb.ops), "w": raw(hb.wops),
                "e": raw(getattr(hb, "eops", None)), "p": raw(getattr(hb, "pops", None))}
        if self.device.type != "cuda":
            return _record(torch.from_numpy(host["x"]), torch.from_numpy(host["l"]), None,
                           *(None if host[k] is None else torch.from_numpy(host[k].copy()) for k in "owep"))
        if self.copy is None:
            self.copy = torch.cuda.Stream(device=self.device)
        if slot in self.done:
            self.done[slot].synchronize()         # host: the step that read this slot three batches ago is over
        if slot in self.ready:
            self.ready[slot].synchronize()        # host: the H2D copies that last read this slot's pinned buffers have executed
        pairs = []          # (device buffer, pinned source) per array; both are reused while shape and dtype match
        for k, a in host.items():
            p = d = None
            if a is not None:
                p, d = self.staged((k, slot), a), self.dev.get((k, slot))
                if d is None or d.shape != p.shape or d.dtype != p.dtype:
                    d = self.dev[(k, slot)] = torch.empty(p.shape, dtype=p.dtype, device=self.device)
            pairs.append((d, p))
        with torch.cuda.stream(self.copy):
            for d, p in pairs:
                if d is not None:
                    d.copy_(p, non_blocking=True)
            ev = self.ready[slot] = torch.cuda.Event(); ev.record(self.copy)
        x, lab, ops, wops, eops, pops = (d for d, _ in pairs)
        return _record(x, lab, ev, ops, wops, eops, pops)

    def augment(self, eng, seed: int, b: Batch):
        """Device augmentation of one uploaded batch on the compute stream (behind the slot's ready event) into ONE
        feed-owned pair of buffers: the next step's augment is queued on the same stream behind this step's backward, the
        last reader of the pair, so one pair is enough.  With warp descriptors the batch first goes through ``warp`` into
        a second, uint8 pair under the same rule: its only reader is the ``augment`` queued right behind it.  With elastic
        descriptors ``elastic`` runs in front of both, into a third pair: its only reader is the stage queued right behind.
        With photometric descriptors ``photometric`` runs directly behind ``elastic``, into an image buffer of its own under
        the same one-reader rule; the labels pass it by."""
        x, lab = b.x, b.labels
        if getattr(b, "eops", None) is not None:
            self.elastic_out = _pair(self.elastic_out, x, lab, x.dtype)
            x, lab = eng.elastic(x, lab, b.eops, out=self.elastic_out)
        if getattr(b, "pops", None) is not None:
            if self.photo_out is None or self.photo_out.shape != x.shape or self.photo_out.device != x.device:
                self.photo_out = torch.empty_like(x)
            x = eng.photometric(x, b.pops, out=self.photo_out)
        if b.wops is not None:
            self.warp_out = _pair(self.warp_out, x, lab, x.dtype)
            x, lab = eng.warp(x, lab, b.wops, out=self.warp_out)
        self.aug_out = _pair(self.aug_out, x, lab, torch.float32)
        return eng.augment(x, lab, b.ops, seed, out=self.aug_out)

    def release(self, slot: int) -> None:
        """The compute stream is done reading device slot ``slot`` (recorded behind the step that used it)."""
        if self.copy is not None:
            e = torch.cuda.Event(); e.record(torch.cuda.current_stream(self.device)); self.done[slot] = e

    def staged(self, key, arr: np.ndarray) -> torch.Tensor:
        arr = np.ascontiguousarray(arr)
        buf = self.pinned.get(key)
        if buf is None or buf.shape != arr.shape or buf.numpy().dtype != arr.dtype:
            buf = torch.from_numpy(np.empty_like(arr))
            if torch.cuda.is_available():
                buf = buf.pin_memory()
            self.pinned[key] = buf
        buf.numpy()[...] = arr
        return buf
