"""The inference-only path of BASELINE configs[4]: ``evaluate_model`` / ``predict`` at device batch 128 --
a hipGraph-captured forward over fixed buffers, raw uint8 images uploaded from pinned double buffers on a copy
stream, uint8 arg-max class maps and uint8 boundary maps (not fp32 probabilities) downloaded into pinned double
buffers, the host min-path post-process fanned out to a process pool; under ``torchrun`` the test set is sharded by
``parallel.shard_range`` (no collective).  Reference: evaluation/evaluation.py:108-135,289-315 and
prediction/prediction.py:70-81,134-143 (one ``predict`` call and one graph build per image there).

Results are bit-identical to the per-image path (``Model.predict_labels``): inference is independent of batch
composition (tests/test_gpu_workflow.py::test_batched_pipeline_equals_per_image_path)."""
from __future__ import annotations

import time
from typing import Iterable, Iterator, NamedTuple, Optional, Tuple

import numpy as np
import torch

from ..common.utils import check_contrast, check_pad_mode, check_tta, padded_geometry
from ..min_path_processing.device_search import DeviceMinPath, LazyPool, merge_ties
from ..min_path_processing.pool import SegmentPool, default_workers
from .calibration import CalibrationCounts, check_bins, check_temperature
from .components import ComponentRule, Components, check_components
from .dice_device import ConfusionCounts, DelineationLabels, check_ignore_label
from .ordered import OrderedDecode, check_ordered
from .render import PngRenderer, batch_pictures
from .surface import SurfaceDistances


class Batch(NamedTuple):
    """What the device yields for images ``lo:hi`` of a run.  A new device-side post-process is one more field here and
    one more entry of ``_stages``, and nothing else: ``BatchedPredictor`` and ``host_batches`` walk that list."""
    lo: int
    hi: int
    labels: np.ndarray                             # (n, H, W) uint8 arg-max class maps
    maps: Optional[np.ndarray] = None              # (n, C-1, H, W) uint8 boundary maps
    surface: Optional[np.ndarray] = None           # (n, C-1, 6) float64 surface-distance rows
    minpath: Optional[Tuple[np.ndarray, ...]] = None   # rows (n, C-1, W) uint16, cost (n, C-1) float64, tied (n, C-1) bool
    confusion: Optional[np.ndarray] = None         # (n, C, C) uint32 confusion counts [gt][pred] of labels against the ground truth

    # Monte-Carlo dropout runs (mc_samples > 0) and test-time-augmentation runs (tta) also carry two (n, H, W) float32 maps:
    # the predictive entropy (nats) and the mutual information (BALD) of the samples / views.  They are ATTRIBUTES, not tuple
    # fields -- the seven fields above are what every positional construction and unpacking of a record relies on -- and
    # None on every other record.
    entropy = None
    mutual_info = None
    # Runs with calibration_bins > 0 carry the reliability counts of the class probabilities against the ground truth:
    # (counts (n, M, 3) uint64 = [pixels, correct, sum of floor(conf 2^28)], sums (n, 4) float64 = [sum nll, sum brier, counted,
    # 0]) -- evaluation/calibration.py.  An ATTRIBUTE for the same reason, None on every other record.
    calibration = None
    # Runs with the ordered decode carry its result for the batch's (mean, tempered, cropped) class probabilities: (labels
    # (n, H, W) uint8, rows (n, C-1, W) uint16, score (n, W) uint32) -- evaluation/ordered.py.  An ATTRIBUTE likewise.
    ordered = None
    # Runs with a component rule carry the cleaned arg-max maps and the component statistics: (clean_labels (n, H, W) uint8,
    # stats (n, C, 2) uint32 = [components, pixels of the largest] of the ARG-MAX map, removed (n, C) uint32) --
    # evaluation/components.py.  An ATTRIBUTE likewise.
    components = None

    def _with(self, **attrs) -> "Batch":
        b = _UncertainBatch(*self)
        for k in ("entropy", "mutual_info", "calibration", "ordered", "components"):
            setattr(b, k, attrs.get(k, getattr(self, k)))
        return b

    def with_uncertainty(self, entropy: np.ndarray, mutual_info: np.ndarray) -> "Batch":
        """This record with ``entropy`` / ``mutual_info`` set."""
        return self._with(entropy=entropy, mutual_info=mutual_info)

    def with_calibration(self, calibration) -> "Batch":
        """This record with ``calibration`` set."""
        return self._with(calibration=calibration)

    def with_ordered(self, ordered) -> "Batch":
        """This record with ``ordered`` set."""
        return self._with(ordered=ordered)

    def with_components(self, components) -> "Batch":
        """This record with ``components`` set."""
        return self._with(components=components)


class _UncertainBatch(Batch):
    """A ``Batch`` that can hold the attributes (a NamedTuple instance has no dictionary; an instance of this has)."""


class _Stage(NamedTuple):
    """One per-batch device post-process: the ``Batch`` field it fills, the wrapper that runs it -- ``run(*inputs, *outs)``
    queues it on the current stream, ``run.outs`` are its own output buffers for a full batch, ``run.to_host`` turns
    output rows into the field's value -- and what it reads: the boundary maps, or else the ground truth with the arg-max
    maps or (``on_probs``) with the class probabilities, or (without ``needs_gt``) the class probabilities (``on_probs``) or the arg-max maps alone."""
    field: str
    run: object
    on_maps: bool
    on_probs: bool = False
    needs_gt: bool = True             # (a stage on the boundary maps never reads the ground truth, whatever this says)

    @property
    def reads_gt(self) -> bool:
        return self.needs_gt and not self.on_maps

    def launch(self, n: int, outs, labels, gt, maps, probs=None) -> None:
        inputs = (maps[:n],) if self.on_maps else (probs[:n] if self.on_probs else labels[:n],) + ((gt[:n],) if self.needs_gt else ())
        self.run(*inputs, *(t[:n] for t in outs))

    def to_host(self, n: int, outs, first_image: int):
        return self.run.to_host(*(t[:n] for t in outs), first_image=first_image)


def _stages(surface, confusion, minpath, have_gt: bool = True, calibration=None, ordered=None, components=None) -> list:
    """The stages to run, in their order on the stream; those that read the ground truth only when there is one."""
    every = (_Stage("surface", surface, False), _Stage("confusion", confusion, False),
             _Stage("calibration", calibration, False, True), _Stage("ordered", ordered, False, True, False),
             _Stage("components", components, False, False, False), _Stage("minpath", minpath, True))
    return [st for st in every if st.run is not None and (have_gt or not st.reads_gt)]


class BatchedPredictor:
    """Fixed-batch graph replay with overlapped transfers.  ``run(images_u8)`` yields one ``Batch`` per device batch, in
    order; ``maps`` is None without ``want_maps``.

    With ``surface`` (an ``evaluation.surface.SurfaceDistances`` for this batch and shape), ``run(images_u8, gt_u8)``
    also uploads the ground-truth class maps (n,H,W) double-buffered like the images, runs the surface-distance kernels on
    the arg-max maps behind their copy, and fills ``Batch.surface``.

    With ``minpath`` (a ``min_path_processing.device_search.DeviceMinPath`` for this batch, C-1 maps and shape) the min-path
    search runs on the boundary maps behind ``boundary_maps`` on the main stream and fills ``Batch.minpath``, downloaded
    through pinned double buffers next to the labels and maps.

    With ``confusion`` (an ``evaluation.dice_device.ConfusionCounts`` for this batch and shape) the ground truth is
    uploaded in the same way and ``oct_confusion_counts`` runs on the arg-max maps next to the surface distances;
    ``Batch.confusion`` holds the matrices, and a label outside 0..C-1 raises when the batch is collected.

    With ``soft_maps`` the graph also writes the class probabilities, into a buffer that never leaves the device, and
    ``maps`` are the soft boundary maps of those (``oct_boundary_maps_soft``) instead of the binary maps of the arg-max.
    Labels, surface distances, confusion counts, the min-path stage behind the maps and every transfer are the same.

    With ``mc_samples`` > 0 every batch is a Monte-Carlo dropout prediction: no graph is captured, and the per-batch graph
    launch is the eager ``engine.infer(mc=...)`` on the same fixed input buffer -- ``mc_samples`` forwards with the bottleneck dropout on,
    dropout steps ``mc_step0 .. mc_step0+mc_samples-1`` for EVERY batch.  The arg-max maps and (with ``soft_maps``) the
    probabilities are then those of the MEAN prediction, everything behind them is unchanged, and ``Batch.entropy`` /
    ``Batch.mutual_info`` carry the two uncertainty maps, downloaded through pinned double buffers like the labels.  The
    dropout stream is indexed by the position in the batch's bottleneck tensor and seeded per rank: an image's result
    depends on its position in its batch and on the rank that predicts it.

    With ``hw`` -- the images' true size (H, W), no multiple of 2^pool_layers -- and a ``pad_mode`` ("edge", "reflect" or
    "constant" with ``pad_value``) the engine is one built at the padded size (``common.utils.padded_geometry``): the
    captured graph is then ``oct_pad_batch`` of the true-size input, the forward and ``oct_crop_batch`` of the arg-max maps
    (and of the probabilities with ``soft_maps``), the pinned upload buffers and everything behind the graph are true-size,
    and every stage runs on the cropped tensors.  A Monte-Carlo batch is the same chain run eagerly: the pad in front, the crops
    of its arg-max, entropy, mutual information and mean probabilities behind.  Without ``hw`` nothing is launched that was not before.

    With ``tta`` -- 1..4 distinct view names of ``common.utils.TTA_VIEWS`` -- every batch is a test-time-augmented
    prediction, and unlike the Monte-Carlo one it IS a graph: the graph captured here is ``engine.infer(tta=..., capture=True)`` (per
    view the flip of the input, the forward and the mirrored fold; with ``hw`` the pad in front, the views taken of the
    padded batch, and the crops behind).  As for ``mc_samples`` the arg-max maps and (with ``soft_maps``) the probabilities
    are those of the MEAN prediction and ``Batch.entropy`` / ``Batch.mutual_info`` carry the two maps over the views;
    the result does not depend on the batch an image sits in.  ``tta`` with ``mc_samples`` > 0 is refused.

    With ``calibration`` (an ``evaluation.calibration.CalibrationCounts`` for this batch and shape) the chain is asked for the
    class probabilities, which stay on the device; the ground truth is uploaded as for ``confusion``, ``oct_calibration_counts``
    runs on the (cropped; with ``mc_samples`` / ``tta`` the MEAN) probabilities, and ``Batch.calibration`` holds ``(counts,
    sums)``.  With ``temperature`` != 1 ``oct_temperature_apply`` tempers the probabilities in place behind the chain, in
    front of the soft maps and the counts; the arg-max maps do not depend on it.  It is refused together with ``mc_samples`` or
    ``tta``: the samples would have to be tempered before the fold.  With ``temperature`` == 1.0 nothing is launched.

    With ``ordered`` (an ``evaluation.ordered.OrderedDecode`` for this batch and shape) the chain is asked for the class
    probabilities in the same way and ``oct_ordered_decode`` runs on them -- cropped; with ``mc_samples`` / ``tta`` the MEAN;
    with a ``temperature`` the TEMPERED ones, behind ``oct_temperature_apply``: the decode weighs rows against each other and is
    not invariant to the temperature as the arg-max is.  It reads no ground truth, and ``Batch.ordered`` holds ``(labels,
    rows, score)``.  It depends on none of ``soft_maps``, ``minpath``, ``confusion``; without it nothing is launched.

    With ``components`` (an ``evaluation.components.Components`` for this batch and shape) ``oct_components`` and
    ``oct_component_filter`` run on the batch's copy of the arg-max maps -- the MEAN prediction's under ``mc_samples`` / ``tta``,
    the cropped ones under ``hw``; a ``temperature`` does not move the arg-max -- and ``Batch.components`` holds ``(clean_labels,
    stats, removed)``.  It reads neither the ground truth nor the probabilities and writes only buffers of its own: labels,
    maps, the search and every other stage see the arg-max maps as before.  Without it nothing is launched.

    With ``contrast`` (a spec of ``common.utils.check_contrast``: CLAHE or a percentile stretch) the per-batch device copy of
    the landing buffer into the chain's fixed input becomes ``engine.contrast(landing buffer, spec, out=fixed input)``
    (``oct_contrast_batch``): the graph, the pad in front of the forward, the TTA views and the Monte-Carlo chain see the
    normalised batch, normalised at the true size.  Labels and maps equal those of a run on ``contrast_reference(images)``.
    Without it the copy stays and nothing is launched."""

    def __init__(self, engine, batch: int, want_maps: bool = True, bg_ilm: bool = True, bg_csi: bool = False,
                 surface=None, minpath=None, confusion=None, soft_maps: bool = False, mc_samples: int = 0, mc_step0: int = 0,
                 hw=None, pad_mode: Optional[str] = None, pad_value=0, tta=None, calibration=None, temperature: float = 1.0,
                 ordered=None, components=None, contrast=None):
        self.temperature = check_temperature(temperature)
        if self.temperature != 1.0 and (mc_samples or tta):
            raise ValueError("temperature != 1 with mc_samples or tta: the samples would have to be tempered before they are "
                             "folded, which is not implemented")
        if soft_maps and not want_maps:
            raise ValueError("soft_maps: needs want_maps=True")
        if not 0 <= int(mc_samples) <= 64:
            raise ValueError(f"mc_samples must be in 0..64, not {mc_samples}")
        self.tta = check_tta(tta, mc_samples)
        self.pad_mode, self.pad_value = check_pad_mode(pad_mode, pad_value)
        self.soft_maps, self.mc_samples, self.mc_step0 = bool(soft_maps), int(mc_samples), int(mc_step0)
        if not 1 <= batch <= engine.cfg.max_batch:
            raise ValueError(f"batch {batch} outside 1..max_batch={engine.cfg.max_batch}")
        self.eng, self.B, self.want_maps, self.bg = engine, int(batch), want_maps, (bg_ilm, bg_csi)
        dev, H, W, C = engine.device, engine.cfg.H, engine.cfg.W, engine.cfg.n_cls
        ic = engine.cfg.in_ch
        self.at = None                                      # (top, left) of the images inside the engine's geometry, if padded
        if hw is not None and (int(hw[0]), int(hw[1])) != (H, W):
            Hp, Wp, top, left = padded_geometry(int(hw[0]), int(hw[1]), engine.cfg.pool_layers)
            if self.pad_mode is None or (Hp, Wp) != (H, W):
                raise ValueError(f"images of {hw[0]}x{hw[1]} on an engine built for {H}x{W}: needs a pad_mode and the engine of "
                                 f"the padded size {Hp}x{Wp}")
            (H, W), self.at = (int(hw[0]), int(hw[1])), (top, left)
        self.hw = (H, W)
        self.contrast = check_contrast(contrast, hw=self.hw)      # at the true size: normalise first, pad afterwards
        self.x_dev = torch.zeros((self.B, H, W, ic), dtype=torch.uint8, device=dev)       # the graph's fixed input (true size)
        self.x_stage = [torch.empty_like(self.x_dev) for _ in range(2)]                    # H2D landing buffers
        self.x_pin = [torch.empty((self.B, H, W, ic), dtype=torch.uint8).pin_memory() for _ in range(2)]
        self.lab_pin = [torch.empty((self.B, H, W), dtype=torch.uint8).pin_memory() for _ in range(2)]
        self.map_pin = [torch.empty((self.B, C - 1, H, W), dtype=torch.uint8).pin_memory() for _ in range(2)] if want_maps else None
        self.lab_dev = [torch.empty((self.B, H, W), dtype=torch.uint8, device=dev) for _ in range(2)]
        self.map_dev = [torch.empty((self.B, C - 1, H, W), dtype=torch.uint8, device=dev) for _ in range(2)] if want_maps else None
        self.wrappers, self.calibration, self.ordered = (surface, confusion, minpath), calibration, ordered
        self.more = {"components": components} if components is not None else {}      # (the keyword is only passed when set)
        self.out_dev, self.out_pin = {}, {}                 # per stage field: device and pinned double buffers
        every = _stages(*self.wrappers, calibration=calibration, ordered=ordered, **self.more)
        for st in every:
            if st.on_maps and not want_maps:
                raise ValueError(f"{st.field}: needs want_maps=True")
            if st.run.geometry != ((self.B, C - 1, H, W) if st.on_maps else (self.B, H, W, C)):
                raise ValueError(f"{st.field}: {type(st.run).__name__} built for another batch / shape")
            self.out_dev[st.field] = [tuple(torch.empty_like(t) for t in st.run.outs) for _ in range(2)]
            self.out_pin[st.field] = [tuple(torch.empty(t.shape, dtype=t.dtype).pin_memory() for t in st.run.outs) for _ in range(2)]
        self.gt_pin = self.gt_dev = (None, None)
        if any(st.reads_gt for st in every):
            self.gt_pin =[torch.empty((self.B, H, W), dtype=torch.uint8).pin_memory() for _ in range(2)]
            self.gt_dev = [torch.empty((self.B, H, W), dtype=torch.uint8, device=dev) for _ in range(2)]
        self.copy_in = torch.cuda.Stream(device=dev)
        self.copy_out = torch.cuda.Stream(device=dev)
        self.unc_dev = self.unc_pin = None                  # (entropy, mutual_info) double buffers
        if self.mc_samples or self.tta:
            self.unc_dev = [tuple(torch.empty((self.B, H, W), dtype=torch.float32, device=dev) for _ in range(2)) for _ in range(2)]
            self.unc_pin = [tuple(torch.empty((self.B, H, W), dtype=torch.float32).pin_memory() for _ in range(2)) for _ in range(2)]
        # THE chain over the fixed input: captured once and replayed per batch, or -- Monte-Carlo -- repeated eagerly per batch
        pad = None if self.at is None else (*self.at, self.pad_mode, self.pad_value)
        self._infer = lambda capture: engine.infer(self.x_dev, mc=(self.mc_samples, self.mc_step0) if self.mc_samples else None,
                                                   tta=self.tta or None, pad=pad, want_argmax=True,
                                                   want_probs=(self.soft_maps or calibration is not None or ordered is not None
                                                               or self.temperature != 1.0),
                                                   capture=capture)
        self.out = self._infer(not self.mc_samples)         # the maps every batch refills (engine-owned buffers)
        self.am, self.probs = self.out["argmax"], self.out.get("mean_probs", self.out.get("probs"))

    def run(self, images_u8: np.ndarray, gt_u8: Optional[np.ndarray] = None) -> Iterator[Batch]:
        images_u8 = np.ascontiguousarray(images_u8)
        if images_u8.dtype != np.uint8:
            raise TypeError("the batched pipeline takes raw uint8 images (the /255 happens on the device)")
        have_gt = gt_u8 is not None
        stages = _stages(*self.wrappers, have_gt=have_gt, calibration=self.calibration, ordered=self.ordered, **self.more)
        if have_gt:
            if not any(st.reads_gt for st in stages):
                raise ValueError("ground-truth maps given to a BatchedPredictor built without surface=, confusion= or calibration=")
            gt_u8 = np.ascontiguousarray(gt_u8)
            if gt_u8.dtype != np.uint8 or gt_u8.shape != images_u8.shape[:3]:
                raise TypeError(f"gt_u8 must be uint8 class maps of shape {images_u8.shape[:3]}")
        n, B, eng = images_u8.shape[0], self.B, self.eng
        main = torch.cuda.current_stream(eng.device)
        nb = (n + B - 1) // B
        up_done = [torch.cuda.Event() for _ in range(2)]
        x_free = [torch.cuda.Event() for _ in range(2)]
        out_done = [torch.cuda.Event() for _ in range(2)]
        out_ready = [torch.cuda.Event() for _ in range(2)]
        gt_free = [torch.cuda.Event() for _ in range(2)]

        def upload(i):
            lo, hi, s = i * B, min(n, (i + 1) * B), i & 1
            if i >= 2:
                # the async H2D of batch i-2 READS this pinned buffer: the host must not overwrite it before that copy has
                # run (the device-side wait below only protects the staging buffer; no other host sync orders copy_in)
                up_done[s].synchronize()
            self.x_pin[s][:hi - lo].copy_(torch.from_numpy(images_u8[lo:hi]))       # host gather into pinned memory
            if have_gt:
                self.gt_pin[s][:hi - lo].copy_(torch.from_numpy(gt_u8[lo:hi]))
            with torch.cuda.stream(self.copy_in):
                if i >= 2:
                    self.copy_in.wait_event(x_free[s])                                  # staging buffer consumed by batch i-2
                    if have_gt:
                        self.copy_in.wait_event(gt_free[s])                             # gt maps of batch i-2 consumed
                self.x_stage[s][:hi - lo].copy_(self.x_pin[s][:hi - lo], non_blocking=True)
                if have_gt:
                    self.gt_dev[s][:hi - lo].copy_(self.gt_pin[s][:hi - lo], non_blocking=True)
                up_done[s].record(self.copy_in)

        pending = None
        if nb:
            upload(0)
        for i in range(nb):
            lo, hi, s = i * B, min(n, (i + 1) * B), i & 1
            if i + 1 < nb:
                upload(i + 1)                                                           # overlaps the forward of batch i
            main.wait_event(up_done[s])
            if self.contrast is None:
                self.x_dev.copy_(self.x_stage[s])                                       # D2D, then the staging buffer is free
            else:                                                                       # the same move through the contrast stage
                eng.contrast(self.x_stage[s], self.contrast, out=self.x_dev)
            x_free[s].record(main)
            if self.mc_samples:
                self._infer(False)
            else:
                eng.graph_launch()
            mc = self.out if self.unc_dev is not None else None
            if i >= 2:
                main.wait_event(out_done[s])                                            # device out buffers of batch i-2 downloaded
            self.lab_dev[s].copy_(self.am)
            if self.temperature != 1.0:                                                 # in place, in front of the soft maps and the counts
                eng.temperature_apply(self.probs, 1.0 / self.temperature, out=self.probs)
            if mc is not None:
                self.unc_dev[s][0].copy_(mc["entropy"]); self.unc_dev[s][1].copy_(mc["mutual_info"])
            outs = [self.out_dev[st.field][s] for st in stages]
            # (the probabilities are the chain's own buffer: the stage that reads them is queued in front of the next batch's launch)
            srcs = (self.lab_dev[s], self.gt_dev[s], self.map_dev[s] if self.want_maps else None, self.probs)
            for st, o in zip(stages, outs):
                if not st.on_maps:
                    st.launch(hi - lo, o, *srcs)
            if have_gt:
                gt_free[s].record(main)
            if self.want_maps:
                if self.soft_maps:
                    self.map_dev[s].copy_(eng.boundary_maps_soft(self.probs, bg_ilm=self.bg[0], bg_csi=self.bg[1]))
                else:
                    self.map_dev[s].copy_(eng.boundary_maps(self.am, bg_ilm=self.bg[0], bg_csi=self.bg[1]))
            for st, o in zip(stages, outs):
                if st.on_maps:
                    st.launch(hi - lo, o, *srcs)
            out_ready[s].record(main)
            with torch.cuda.stream(self.copy_out):
                self.copy_out.wait_event(out_ready[s])
                self.lab_pin[s].copy_(self.lab_dev[s], non_blocking=True)
                if self.want_maps:
                    self.map_pin[s].copy_(self.map_dev[s], non_blocking=True)
                if mc is not None:
                    for t_pin, t_dev in zip(self.unc_pin[s], self.unc_dev[s]):
                        t_pin.copy_(t_dev, non_blocking=True)
                for st, o in zip(stages, outs):
                    for t_pin, t_dev in zip(self.out_pin[st.field][s], o):
                        t_pin.copy_(t_dev, non_blocking=True)
                out_done[s].record(self.copy_out)
            if pending is not None:
                yield self._collect(*pending, stages)
            pending = (lo, hi, s, out_done[s])
        if pending is not None:
            yield self._collect(*pending, stages)

    def _collect(self, lo, hi, s, ev, stages=()):
        ev.synchronize()
        labels = self.lab_pin[s][:hi - lo].numpy().copy()
        maps = self.map_pin[s][:hi - lo].numpy().copy() if self.want_maps else None
        fields = {st.field: st.to_host(hi - lo, self.out_pin[st.field][s], lo) for st in stages}
        calibration, ordered = fields.pop("calibration", None), fields.pop("ordered", None)
        components = fields.pop("components", None)
        batch = Batch(lo, hi, labels, maps, **fields)
        if components is not None:
            batch = batch.with_components(components)
        if calibration is not None:
            batch = batch.with_calibration(calibration)
        if ordered is not None:
            batch = batch.with_ordered(ordered)
        if self.unc_pin is not None:
            batch = batch.with_uncertainty(*(t[:hi - lo].numpy().copy() for t in self.unc_pin[s]))
        return batch


def host_batches(model, images: np.ndarray, batch: int, *, gt_u8: Optional[np.ndarray] = None, surface=None,
                 minpath=None, confusion=None, soft_maps: bool = False, mc_samples: int = 0, mc_step0: int = 0,
                 pad_mode: Optional[str] = None, pad_value=0, tta=None, calibration_bins: int = 0,
                 temperature: float = 1.0, ordered=None, components=None, contrast=None) -> Iterator[Batch]:
    """The same records for images that are not uint8: x / 255 on the host (``Model.predict_labels``), one synchronous
    forward per batch, no overlap.  ``surface`` / ``minpath`` / ``confusion`` / ``soft_maps`` / ``mc_samples`` /
    ``mc_step0`` / ``tta`` as in ``BatchedPredictor``; each stage writes its own output buffers.  ``pad_mode`` / ``pad_value`` (in raw
    counts) go to ``Model.predict_labels``, which pads and crops on the device.  ``calibration_bins`` / ``temperature``: refused
    here -- calibration exists for raw uint8 images only.  ``ordered`` (anything true, an ``OrderedDecode`` included):
    ``Model.predict_labels`` runs the ordered decode on the batch's probabilities while they are on the device, and
    ``Batch.ordered`` is filled as by ``BatchedPredictor``.  ``components`` (a ``Components``): a stage like the others, on the
    uploaded class maps; ``Batch.components`` likewise.  ``contrast``: refused here -- the contrast stage is defined on bytes."""
    if check_bins(calibration_bins) or check_temperature(temperature) != 1.0:
        raise ValueError("calibration_bins / temperature need raw uint8 images: the path for other dtypes (host_batches) has no "
                         "calibration stage")
    if contrast is not None:
        raise ValueError("contrast needs raw uint8 images: the path for other dtypes (host_batches) has no contrast stage")
    pad_mode, pad_value = check_pad_mode(pad_mode, pad_value)
    tta = check_tta(tta, mc_samples)
    stages = _stages(surface, confusion, minpath, have_gt=gt_u8 is not None, **({"components": components} if components is not None else {}))
    on_labels, on_maps = any(not st.on_maps for st in stages), any(st.on_maps for st in stages)

    def upload(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(stages[0].run.device)

    more = {"ordered": True} if ordered else {}             # (the keyword is only passed when set)
    for lo in range(0, images.shape[0], batch):
        hi = min(lo + batch, images.shape[0])
        labels, maps, *unc = model.predict_labels(images[lo:hi], batch_size=batch, want_maps=True, bg_ilm=True, bg_csi=False,
                                                  soft_maps=soft_maps, mc_samples=mc_samples, mc_step0=mc_step0,
                                                  pad_mode=pad_mode, pad_value=pad_value, tta=tta, **more)
        decoded = unc.pop() if ordered else None
        lab_dev = upload(labels.astype(np.uint8)) if on_labels else None
        gt_dev = upload(gt_u8[lo:hi]) if on_labels and gt_u8 is not None else None
        maps_dev = upload(maps) if on_maps else None
        fields = {}
        for st in stages:
            st.launch(hi - lo, st.run.outs, lab_dev, gt_dev, maps_dev)
            fields[st.field] = st.to_host(hi - lo, st.run.outs, lo)
        cleaned = fields.pop("components", None)
        record = Batch(lo, hi, labels, maps, **fields)
        if cleaned is not None:
            record = record.with_components(cleaned)
        if decoded is not None:
            record = record.with_ordered(decoded)
        yield record.with_uncertainty(*unc) if unc else record


class InferenceRun:
    """One pass of a loaded model over ``images`` (a rank's slice) for ``evaluate_model`` / ``predict``: iterating it
    yields the ``Batch`` records, ``graph_search(batch, truths)`` gives a batch's delineations, and leaving the ``with``
    block closes the worker pools on every path.  It picks

    * the search: none, the host ``SegmentPool`` (started here, BEFORE the first GPU call of the run), or with
      ``gs_device`` a ``DeviceMinPath`` behind the boundary maps plus a ``LazyPool`` that only starts when a tied map
      arrives and ``gs_device_ties == "host"``;
    * ``SurfaceDistances`` when ground-truth class maps ``gt`` (n,H,W) are given and ``surface`` is left on, and
      ``ConfusionCounts`` when they are given and ``confusion`` is set: arg-max maps against them on the device;
    * the source: ``BatchedPredictor`` (hipGraph replay, pinned double-buffered transfers) for uint8 images,
      ``host_batches`` for every other dtype.

    ``soft_maps`` is passed to whichever source is built: ``Batch.maps`` are then the soft boundary maps of the class
    probabilities, and everything behind them (either search, ``gs_labels``) works on those.

    ``mc_samples`` > 0 (with ``mc_step0``) is passed on likewise: every batch is then a Monte-Carlo dropout prediction,
    ``Batch.labels`` / ``Batch.maps`` are those of the mean prediction, and ``Batch.entropy`` / ``Batch.mutual_info`` are
    filled (see ``BatchedPredictor`` for what the result depends on).

    ``tta`` (1..4 distinct view names of ``common.utils.TTA_VIEWS``; None or () : off) is passed on likewise: every batch is
    then the mean prediction over the flipped views, with the same two maps filled.  With ``mc_samples`` > 0 it is refused.

    The engine follows the images: the model is asked for the engine of ``images.shape[1:3]``, whatever its config
    records.  ``pad_mode`` ("edge", "reflect", "constant" with ``pad_value`` in raw counts; None: off) admits sizes that are
    no multiple of 2^pool_layers: the engine is then the one of the padded size, the source pads in front of the forward and
    crops directly behind the head, and every stage, search and picture works at the true size.  For sizes that are
    multiples nothing changes and nothing more is launched.

    ``ignore_label`` (None, or an int in num_classes..255) marks ground-truth pixels whose class is unknown: ``gt`` may then
    hold that value, and it is handed to the ``surface`` and ``confusion`` stages and to ``gs_labels``, which run their
    masked kernels.  Labels, maps, searches and pictures do not depend on it.

    ``calibration_bins`` > 0 with ``gt``: a ``CalibrationCounts`` stage with that many confidence bins fills
    ``Batch.calibration``.  ``temperature`` != 1 tempers the probabilities on the device in front of the
    soft maps and the counts; with ``mc_samples`` or ``tta`` it is refused.  Both need raw uint8 images: for another dtype
    either keyword is a ``ValueError``.

    ``ordered_decode``: an ``OrderedDecode`` stage fills ``Batch.ordered`` from the class probabilities -- the mean ones under
    ``mc_samples`` / ``tta``, the tempered ones under ``temperature``, the cropped ones under ``pad_mode``.
    It needs 2..16 classes and a height of at most 4096, works for every image dtype and without ``gt``, and does not depend on
    ``soft_maps``, ``gs_device`` or ``confusion``.

    ``components`` (a ``ComponentRule`` or a dict of its keywords; None: off): a ``Components`` stage fills ``Batch.components``
    from the arg-max maps the chain yields -- the mean prediction's under ``mc_samples`` / ``tta``, the cropped ones under
    ``pad_mode``, the same under any ``temperature``.  It works for every image dtype and without ``gt``
    and changes no output of ``ordered_decode``, ``gs_device``, ``confusion`` or ``calibration_bins``; the searches keep reading
    the arg-max maps.  A rule that does not fit ``num_classes`` is a ``ValueError``.

    ``contrast`` (a spec of ``common.utils.check_contrast``; None: off) is passed to ``BatchedPredictor``: every batch is
    normalised on the device, at the true size and in front of the pad, before the chain sees it.  It
    needs raw uint8 images: for another dtype it is a ``ValueError``.  Pictures keep showing the scans as given.

    ``batches`` replaces the model by a ready source of records (tests of the host side: no device is touched)."""

    def __init__(self, model, images: np.ndarray, batch: int, num_classes: int, *, gt: Optional[np.ndarray] = None,
                 graph_search: bool = False, gsgrad: int = 1, gs_device: bool = False, gs_device_ties: str = "host",
                 gs_workers: Optional[int] = None, batches: Optional[Iterable[Batch]] = None, surface: bool = True,
                 confusion: bool = False, soft_maps: bool = False, mc_samples: int = 0, mc_step0: int = 0,
                 pad_mode: Optional[str] = None, pad_value=0, ignore_label: Optional[int] = None, tta=None,
                 calibration_bins: int = 0, temperature: float = 1.0, ordered_decode: bool = False, components=None,
                 contrast=None):
        pad_mode, pad_value = check_pad_mode(pad_mode, pad_value)
        contrast = check_contrast(contrast, hw=images.shape[1:3])
        if images.dtype != np.uint8 and contrast is not None:
            raise ValueError("contrast needs raw uint8 images: the path for other dtypes (host_batches) has no contrast stage")
        rule = ComponentRule.coerce(components)
        if rule is not None:
            rule.check(num_classes)
            check_components(num_classes, images.shape[1], images.shape[2])
        self.tta = tta = check_tta(tta, mc_samples)
        if ordered_decode:
            check_ordered(num_classes, images.shape[1])
        calibration_bins, temperature = check_bins(calibration_bins), check_temperature(temperature)
        if temperature != 1.0 and (mc_samples or tta):
            raise ValueError("temperature != 1 with mc_samples or tta: the samples would have to be tempered before they are "
                             "folded, which is not implemented")
        if images.dtype != np.uint8 and (calibration_bins or temperature != 1.0):
            raise ValueError("calibration_bins / temperature need raw uint8 images: the path for other dtypes (host_batches) has "
                             "no calibration stage")
        n, (H, W), C = images.shape[0], images.shape[1:3], int(num_classes)
        self.ignore_label = ignore_label = check_ignore_label(ignore_label, C)
        self.pool = self.host_ties = None
        self._gs = self._gs_geom = None                   # gs_labels' own device buffers: made by its first call
        self._png = None                                  # render_pngs' own device and pinned buffers, likewise
        self._cc_surface = None                           # label_surface's own wrapper, likewise
        self.ties, self._batches = gs_device_ties, (() if batches is None else batches)
        if n == 0:
            return
        gt_u8 = None
        if gt is not None:
            if ignore_label is not None:
                bad = np.nonzero(((gt < 0) | (gt >= C)) & (gt != ignore_label))[0]
                if bad.size:
                    raise ValueError(f"image {int(bad[0])}: ground-truth labels outside 0..{C - 1} that are not the ignore "
                                     f"label {ignore_label}")
            elif gt.min() < 0 or gt.max() >= C:
                raise ValueError(f"ground-truth labels outside 0..{C - 1}")
            gt_u8 = np.ascontiguousarray(gt.astype(np.uint8))
        if graph_search and gs_device:
            self.host_ties = LazyPool((H, W), gsgrad, gs_workers)
        elif graph_search:
            self.pool = SegmentPool((H, W), gsgrad, gs_workers)
        if batches is not None:
            return
        try:
            bs, dev = max(1, min(int(batch), n)), model._dev()
            geom, _ = model._geometry((H, W), pad_mode)      # refuses a size that is no multiple, before anything is built
            self._gs_geom = (bs, H, W, C, dev)
            minpath = DeviceMinPath(bs, C - 1, H, W, gsgrad, dev) if self.host_ties is not None else None
            surface = SurfaceDistances(bs, H, W, C, dev, ignore_label=ignore_label) if gt_u8 is not None and surface else None
            confusion = ConfusionCounts(bs, H, W, C, dev, ignore_label=ignore_label) if gt_u8 is not None and confusion else None
            more = {"components": Components(bs, H, W, C, rule, dev)} if rule is not None else {}      # (only passed when set)
            if contrast is not None:
                more["contrast"] = contrast
            if images.dtype != np.uint8:
                if surface is None and confusion is None:
                    gt_u8 = None
                self._batches = host_batches(model, images, bs, gt_u8=gt_u8, surface=surface, minpath=minpath,
                                             confusion=confusion, soft_maps=soft_maps, mc_samples=mc_samples,
                                             mc_step0=mc_step0, pad_mode=pad_mode, pad_value=pad_value, tta=tta,
                                             calibration_bins=calibration_bins, temperature=temperature,
                                             **({"ordered": True} if ordered_decode else {}), **more)
            else:
                ordered = OrderedDecode(bs, H, W, C, dev) if ordered_decode else None
                calibration = (CalibrationCounts(bs, H, W, C, dev, calibration_bins, ignore_label=ignore_label)
                               if gt_u8 is not None and calibration_bins else None)
                if surface is None and confusion is None and calibration is None:
                    gt_u8 = None
                predictor = BatchedPredictor(model._ensure_engine(bs, False, hw=geom), bs, want_maps=True, bg_ilm=True,
                                             bg_csi=False, surface=surface, minpath=minpath, confusion=confusion,
                                             soft_maps=soft_maps, mc_samples=mc_samples, mc_step0=mc_step0,
                                             hw=(H, W), pad_mode=pad_mode, pad_value=pad_value, tta=tta,
                                             calibration=calibration, temperature=temperature,
                                             **({"ordered": ordered} if ordered is not None else {}), **more)
                self._batches = predictor.run(images, gt_u8)
        except BaseException:
            self.close()
            raise

    def __iter__(self) -> Iterator[Batch]:
        return iter(self._batches)

    def graph_search(self, batch: Batch, truths: Optional[np.ndarray] = None) -> Optional[list]:
        """[(gs_pred_segs uint16 (C-1, W), errors float64 (C-1, W)), ...] per image of the batch -- every entry equals
        ``graph_search.segment_maps`` of the image's maps, but for the tied maps under ``gs_device_ties == "device"`` --
        or None without graph search.  The host part of the search runs in this call, not while the batch is fetched."""
        if self.pool is not None:
            return self.pool.segment(batch.maps, truths)
        if self.host_ties is not None:
            rows, _, tied = batch.minpath
            return merge_ties(batch.maps, rows, tied, truths, self.host_ties, self.ties)
        return None

    def _delineation_labels(self) -> DelineationLabels:
        if self._gs is None:
            self._gs = DelineationLabels(*self._gs_geom, ignore_label=self.ignore_label)
        return self._gs

    def gs_labels(self, batch: Batch, found: list, gt: Optional[np.ndarray] = None) -> Tuple[np.ndarray, Optional[np.ndarray]]:
        """The class maps the batch's final delineations enclose -- ``found`` is what ``graph_search`` returned for the
        batch, so every search mode feeds it -- as (n,H,W) uint8, each equal to ``labels_from_delineations`` of the image;
        with the batch's ground-truth class maps ``gt`` (n,H,W) also their (n, C, C) uint32 confusion counts against it
        (else None).  The delineations and the ground truth are uploaded here, into buffers of this method: the
        predictor's own ground-truth buffers are recycled by the upload two batches ahead, while the host may still be
        searching this batch.  Waits for the device."""
        if self._gs_geom is None:
            raise RuntimeError("gs_labels needs the device: this run was built over injected batches")
        if len(found) != batch.hi - batch.lo:
            raise ValueError(f"gs_labels: {len(found)} delineations for a batch of {batch.hi - batch.lo} images")
        return self._delineation_labels()(np.stack([f[0] for f in found]), gt, first_image=batch.lo)

    def render_pngs(self, batch: Batch, images: np.ndarray, found: Optional[list] = None, *,
                    gt: Optional[np.ndarray] = None, truths: Optional[np.ndarray] = None, gs_labels: Optional[np.ndarray] = None,
                    pred_map: bool = True, col_range=None, ignore_label: Optional[int] = None) -> dict:
        """The PNG pictures of a batch as host RGBA arrays (n,H,W,4) uint8, rasterised on the device by
        ``oct_render_rgba`` (``evaluation.render.batch_pictures`` names the keys): ``raw`` of the batch's ``images``
        (n,H,W,ic), ``pred`` of the arg-max maps (unless ``pred_map`` is off), with the ground-truth class maps ``gt``
        (n,H,W) ``gt``, with the ground-truth boundaries ``truths`` (n,M,W) ``truth``, and with ``found`` -- what
        ``graph_search`` returned for the batch -- ``gs_map``, ``gs_bounds`` (columns ``col_range``) and, where ``truths``
        are given, ``gs_both``.  ``gs_labels`` are the class maps of the delineations where the caller has them
        (``gs_labels()``); otherwise ``oct_area_labels`` makes them here, on the device.  Everything is uploaded here,
        into buffers of this method -- the predictor's double buffers are recycled two batches ahead -- and nothing of
        the batch is referenced once the call returns.  With ``ignore_label`` the pixels of ``gt`` that carry it are
        mid-grey in ``gt`` and under the truth overlays (``batch_pictures``).  Waits for the device."""
        if self._gs_geom is None:
            raise RuntimeError("render_pngs needs the device: this run was built over injected batches")
        bs, H, W, C, dev = self._gs_geom
        n = batch.hi - batch.lo
        if images.shape[0] != n or (found is not None and len(found) != n):
            raise ValueError(f"render_pngs: a batch of {n} images needs {n} scans and delineations")
        if self._png is None:
            self._png = PngRenderer(bs, H, W, dev)
        gs_segs = None
        if found is not None:
            gs_segs = np.stack([f[0] for f in found]).astype(np.uint16)
            if gs_labels is None:
                gs_labels = self._delineation_labels().area(torch.from_numpy(np.ascontiguousarray(gs_segs).view(np.int16)).to(dev))
        return batch_pictures(self._png, C, images, pred_labels=batch.labels if pred_map else None, gt_labels=gt,
                              truths=truths, gs_segs=gs_segs, gs_labels=gs_labels,
                              both_overlay=truths is not None and gs_segs is not None, col_range=col_range,
                              ignore_label=ignore_label)

    def ordered_counts(self, batch: Batch, gt: np.ndarray) -> np.ndarray:
        """The (n, C, C) uint32 confusion counts of the batch's ordered class maps (``Batch.ordered``) against its ground-truth
        class maps ``gt`` (n,H,W), by the kernel of ``gs_labels`` and with the run's ``ignore_label``.  Both are uploaded here,
        into buffers of this method.  Waits for the device."""
        if self._gs_geom is None:
            raise RuntimeError("ordered_counts needs the device: this run was built over injected batches")
        counts, dev = self._delineation_labels().counts, self._gs_geom[4]
        pred = torch.from_numpy(np.ascontiguousarray(batch.ordered[0])).to(dev)
        gt_dev = torch.from_numpy(np.ascontiguousarray(gt, dtype=np.uint8)).to(dev)
        return counts.to_host(counts(pred, gt_dev), batch.lo)

    def label_counts(self, labels: np.ndarray, gt: np.ndarray, first_image: int = 0) -> np.ndarray:
        """The (n, C, C) uint32 confusion counts of class maps ``labels`` (n,H,W) uint8 -- the cleaned maps of
        ``Batch.components`` -- against the ground-truth class maps ``gt`` (n,H,W), as ``ordered_counts`` forms them.  Waits for
        the device."""
        if self._gs_geom is None:
            raise RuntimeError("label_counts needs the device: this run was built over injected batches")
        counts, dev = self._delineation_labels().counts, self._gs_geom[4]
        pred = torch.from_numpy(np.ascontiguousarray(labels, dtype=np.uint8)).to(dev)
        gt_dev = torch.from_numpy(np.ascontiguousarray(gt, dtype=np.uint8)).to(dev)
        return counts.to_host(counts(pred, gt_dev), first_image)

    def label_surface(self, labels: np.ndarray, gt: np.ndarray) -> np.ndarray:
        """The (n, C-1, 6) float64 surface-distance rows of class maps ``labels`` (n,H,W) uint8 -- the cleaned maps of
        ``Batch.components`` -- against ``gt`` (n,H,W), by the kernels and with the ``ignore_label`` of the run's ``surface``
        stage.  Waits for the device."""
        if self._gs_geom is None:
            raise RuntimeError("label_surface needs the device: this run was built over injected batches")
        bs, H, W, C, dev = self._gs_geom
        if self._cc_surface is None:
            self._cc_surface = SurfaceDistances(bs, H, W, C, dev, ignore_label=self.ignore_label)
        pred = torch.from_numpy(np.ascontiguousarray(labels, dtype=np.uint8)).to(dev)
        gt_dev = torch.from_numpy(np.ascontiguousarray(gt, dtype=np.uint8)).to(dev)
        return self._cc_surface.to_host(self._cc_surface(pred, gt_dev))

    def render_labels(self, labels: np.ndarray) -> np.ndarray:
        """Class maps (n,H,W) uint8 -> (n,H,W,4) RGBA on the host through the region colours, as the ``pred`` picture of
        ``render_pngs`` (the cleaned maps of ``Batch.components``).  Waits for the device."""
        if self._gs_geom is None:
            raise RuntimeError("render_labels needs the device: this run was built over injected batches")
        from ..common import plotting
        bs, H, W, C, dev = self._gs_geom
        if self._png is None:
            self._png = PngRenderer(bs, H, W, dev)
        return self._png.render(np.ascontiguousarray(labels, dtype=np.uint8), palette=plotting.region_palette(C))

    def render_ordered(self, batch: Batch, images: np.ndarray, col_range=None) -> dict:
        """The two pictures of a batch's ordered decode as host RGBA arrays (n,H,W,4) uint8 (``evaluation.render.OD_PNG_NAMES``
        names the keys): ``od_map``, the ordered class maps through the region colours, and ``od_bounds``, the scans with the
        ordered rows solid in the truth colours, as ``gs_bounds`` draws the delineations (a row of 0 is not drawn).  Waits
        for the device."""
        if self._gs_geom is None:
            raise RuntimeError("render_ordered needs the device: this run was built over injected batches")
        bs, H, W, C, dev = self._gs_geom
        if self._png is None:
            self._png = PngRenderer(bs, H, W, dev)
        labels, rows, _ = batch.ordered
        pics = batch_pictures(self._png, C, images, gs_segs=rows, gs_labels=labels, col_range=col_range)
        return {"od_map": pics["gs_map"], "od_bounds": pics["gs_bounds"]}

    def render_gray(self, gray_u8: np.ndarray) -> np.ndarray:
        """(n,H,W) uint8 -> (n,H,W,4) RGBA on the host: the values as a gray scan with no lines, through the renderer of
        ``render_pngs`` (``predict`` draws the quantised predictive entropy with it).  Waits for the device."""
        if self._gs_geom is None:
            raise RuntimeError("render_gray needs the device: this run was built over injected batches")
        bs, H, W, _, dev = self._gs_geom
        if self._png is None:
            self._png = PngRenderer(bs, H, W, dev)
        return self._png.render(np.ascontiguousarray(gray_u8, dtype=np.uint8)[..., None])

    def close(self) -> None:
        for p in (self.pool, self.host_ties):
            if p is not None:
                p.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


def bench_fields(engine, images_u8: np.ndarray, num_classes: int, batch: Optional[int] = None, n_batches: int = 6,
                 labels_u8: Optional[np.ndarray] = None) -> dict:
    """``bench.py`` fields for BASELINE configs[4] / BASELINE.md 5.4: host post-process cost (1 thread and the pool) and
    end-to-end inference ms per B-scan (upload + graph forward + boundary maps + download + pooled min-path), beside the
    GPU-only figure the bench already reports.

    What the graph search costs depends on its input: the bench's network is randomly initialised and a few steps old, its
    boundary maps are noise, and Dijkstra over noise is 5-20x slower than over the single clean ridge a trained model
    emits (and varies from run to run with the weights).  With ``labels_u8`` (the synthetic ground-truth class maps of
    the same scans) the headline figures use the boundary maps OF THOSE LABELS -- computed on the device by the same
    ``oct_boundary_maps`` kernel -- as the post-process input, while the GPU side still runs the full pipeline on the
    images; the figures for the network's own (noise) maps are reported beside them as ``*_untrained_maps``."""
    B = int(batch or engine.cfg.max_batch)
    H, W = engine.cfg.H, engine.cfg.W
    reps = (B * n_batches + images_u8.shape[0] - 1) // images_u8.shape[0]
    imgs = np.tile(images_u8, (reps, 1, 1, 1))[:B * n_batches]
    workers = default_workers()
    pred = BatchedPredictor(engine, B, want_maps=True)
    clean = None
    if labels_u8 is not None:
        lab = np.ascontiguousarray(np.tile(labels_u8.reshape((-1, H, W)), (reps, 1, 1))[:B])
        clean = engine.boundary_maps(torch.from_numpy(lab).to(engine.device)).cpu().numpy()
    out = {}
    with SegmentPool((H, W), gsgrad=1, workers=workers) as pool, SegmentPool((H, W), gsgrad=1, workers=1) as solo:
        first = next(iter(pred.run(imgs[:B])))                      # warm-up: graph, pinned buffers, worker start-up
        maps0 = first.maps
        pool.segment(maps0[:min(B, 2 * workers)])
        ns = min(B, 8)

        def host_cost(maps):
            t0 = time.perf_counter(); solo.segment(maps[:ns]); t1 = time.perf_counter()
            pool.segment(maps); t2 = time.perf_counter()
            return round((t1 - t0) / ns * 1e3, 3), round((t2 - t1) / B * 1e3, 4)

        def e2e(maps_for_pool):
            # GPU batches pipelined against the pool (post-process of batch i runs while batch i+1 is on the GPU)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            jobs = []
            for b in pred.run(imgs):
                jobs.append(pool.segment_async(b.maps if maps_for_pool is None else maps_for_pool[:b.hi - b.lo]))
            for j in jobs:
                j.get()
            return round((time.perf_counter() - t0) / imgs.shape[0] * 1e3, 4)

        one, pooled = host_cost(maps0 if clean is None else clean)
        out["host_postprocess"] = {"what": f"segment_maps over the {num_classes - 1} boundary maps of one {H}x{W} B-scan "
                                           "(native liboct_minpath.so Dijkstra, identical results to the reference)",
                                   "maps": "the network's own" if clean is None else "boundary maps of the synthetic ground-truth class maps (what a trained model emits)",
                                   "ms_per_scan_1_thread": one, "pool_workers": workers, "ms_per_scan_pool": pooled}
        out["inference_e2e_ms_per_scan"] = e2e(clean)
        if clean is not None:
            one_u, pooled_u = host_cost(maps0)
            out["host_postprocess"]["untrained_maps"] = {"ms_per_scan_1_thread": one_u, "ms_per_scan_pool": pooled_u}
            out["inference_e2e_ms_per_scan_untrained_maps"] = e2e(None)
        t0 = time.perf_counter()
        for _ in pred.run(imgs):
            pass
        dt = time.perf_counter() - t0
        out["inference_gpu_pipeline_ms_per_scan"] = round(dt / imgs.shape[0] * 1e3, 4)
        out["inference_e2e"] = {"batch": B, "scans": int(imgs.shape[0]), "stages": "pinned u8 upload -> hipGraph forward + "
                                "arg-max -> boundary maps -> u8 download -> pooled segment_maps (BASELINE configs[4])"}
    return out
