"""``Model``: the duck-typed subset of ``tf.keras.Model`` that the reference's callers use
(``compile/fit/predict/summary/save/get_weights/set_weights/stop_training``, ``.name``,
``.output.shape[-1]``), backed by the HIP engine instead of TensorFlow.

Reference call sites this object serves: training/training.py:262-266 (compile), :345,:400 (summary),
:401-407 (fit with Sequence generators + callbacks), evaluation/evaluation.py:129-135 and
prediction/prediction.py:75-81 (predict), evaluation_parameters.py:85 (``output.shape[-1]``).

Data parallelism: when ``torch.distributed`` is initialised (one process per GPU), ``fit`` takes this rank's
contiguous slice of every GLOBAL batch the generator yields, scales the loss by 1/world and sum-all-reduces
the flat gradient buffer -- the semantics of ``MirroredStrategy`` (training.py:185-188,243).
"""
from __future__ import annotations

import json
import time
from pathlib import Path
from types import SimpleNamespace
from typing import List, Optional

import numpy as np
import torch

from .. import parallel
from .._hip import OctError
from .batch_feed import BatchFeed

WEIGHTS_FORMAT = "oct_unet_weights_v1"


class Callback:
    """Minimal ``keras.callbacks.Callback`` protocol."""
    model = None

    def set_model(self, model): self.model = model
    def on_train_begin(self, logs=None): pass
    def on_train_end(self, logs=None): pass
    def on_epoch_begin(self, epoch, logs=None): pass
    def on_epoch_end(self, epoch, logs=None): pass


class ModelCheckpoint(Callback):
    """``ModelCheckpoint(filepath, save_best_only, monitor, mode)`` as used at training.py:319-326;
    ``filepath`` may contain ``{epoch:02d}`` (1-based)."""

    def __init__(self, filepath, save_best_only=False, monitor="val_loss", mode="auto", verbose=0):
        self.filepath, self.save_best_only, self.monitor = str(filepath), save_best_only, monitor
        if mode == "auto":
            mode = "max" if ("acc" in monitor or "dice" in monitor) else "min"
        self.sign = 1.0 if mode == "max" else -1.0
        self.best = -np.inf
        self.saved: List[str] = []

    def on_epoch_end(self, epoch, logs=None):
        logs = logs or {}
        path = self.filepath.format(epoch=epoch + 1, **logs)
        if self.save_best_only:
            cur = logs.get(self.monitor)
            if cur is None or not np.isfinite(cur) or self.sign * cur <= self.best:
                return
            self.best = self.sign * cur
        self.saved.append(str(self.model.save(path)))


class EarlyStopping(Callback):
    """``EarlyStopping(monitor, mode, patience, restore_best_weights)`` as used at training.py:335-342."""

    def __init__(self, monitor="val_loss", mode="auto", patience=0, restore_best_weights=False, min_delta=0.0):
        if mode == "auto":
            mode = "max" if ("acc" in monitor or "dice" in monitor) else "min"
        self.monitor, self.patience, self.restore_best_weights, self.min_delta = monitor, patience, restore_best_weights, min_delta
        self.sign = 1.0 if mode == "max" else -1.0
        self.best, self.wait, self.best_weights, self.stopped_epoch = -np.inf, 0, None, 0

    def on_train_begin(self, logs=None):
        self.best, self.wait, self.best_weights, self.stopped_epoch = -np.inf, 0, None, 0

    def on_epoch_end(self, epoch, logs=None):
        cur = (logs or {}).get(self.monitor)
        if cur is None:
            return
        if self.restore_best_weights and self.best_weights is None:
            self.best_weights = self.model.get_weights()
        if np.isfinite(cur) and self.sign * cur - self.min_delta > self.best:
            self.best, self.wait = self.sign * cur, 0
            if self.restore_best_weights:
                self.best_weights = self.model.get_weights()
            return
        self.wait += 1
        if self.wait >= self.patience and epoch > 0:
            self.stopped_epoch = epoch
            self.model.stop_training = True
            if self.restore_best_weights and self.best_weights is not None:
                self.model.set_weights(self.best_weights)


class History(Callback):
    def on_train_begin(self, logs=None):
        self.history, self.epoch = {}, []

    def on_epoch_end(self, epoch, logs=None):
        self.epoch.append(epoch)
        for k, v in (logs or {}).items():
            self.history.setdefault(k, []).append(v)


class Model:
    def __init__(self, name: str, config: dict, device: Optional[str] = None):
        self.name = name
        self.config = dict(config)
        self.output = SimpleNamespace(shape=(None, None, None, int(config["num_classes"])))
        self.stop_training = False
        self.optimizer = None
        self._loss_name = self._metric_name = self._focal = None      # _focal: focal_dice_loss's parameters
        self._feed = self._reducer = None     # the input path of fit / evaluate (``feed``); the training engine's GradReducer
        self._engine = None             # the ACTIVE engine: the one that holds the model's current weights
        self._engines = {}              # the geometry cache: {"train": engine, "other": engine}, at most these two
        self._wver = 0                  # version of the model's weights; an engine's _wver says which version it holds
        self._pending_weights = None
        # the model's default for predict / predict_mc / predict_labels on sizes that are no multiple of 2^pool_layers:
        # None (refuse them), "edge", "reflect" or "constant" with pad_value; a call's own pad_mode goes first
        # fit / evaluate consult the same pair, but only in a model compiled for it (compile(pad_mode=...), which also sets
        # the pair): a batch of such a size is then padded on the device behind the augmentations and its label frame
        # filled with the ignore label, so that the loss sees the window only.  Setting the
        # attributes alone keeps padding to inference and fit refuses such sizes, as before
        self.pad_mode, self.pad_value = None, 0
        self._pad_fit = False
        # label value whose pixels do not count in the loss, the Dice metrics or the gradient (compile(ignore_label=...));
        # None: every pixel counts
        self.ignore_label = None
        self._dice_shape, self._edge_weight = None, None
        self._device = device
        self.history = None

    # ---- engine lifetime ----------------------------------------------------------------------------
    def _dev(self):
        if self._device is not None:
            return torch.device(self._device)
        _, local_rank, _ = parallel.env_rank()
        return torch.device("cuda", local_rank if torch.cuda.is_available() and local_rank < max(torch.cuda.device_count(), 1) else 0)

    def _geometry(self, hw=None, pad_mode=None):
        """The engine geometry for images of size ``hw`` (None: the config's) and where they sit in it:
        ``((He, We), None)`` for a size that is a multiple of 2^pool_layers, ``((Hp, Wp), (top, left))`` for another one
        under a ``pad_mode``, and an ``OctError`` for another one without."""
        from ..common.utils import padded_geometry
        c = self.config
        H, W = (int(c["image_height"]), int(c["image_width"])) if hw is None else (int(hw[0]), int(hw[1]))
        m = 1 << int(c.get("pool_layers", 4))
        if H < 1 or W < 1:
            raise OctError(f"image size {H}x{W}: both dimensions must be positive")
        if H % m == 0 and W % m == 0:
            return (H, W), None
        if pad_mode is None:
            raise OctError(f"image size {H}x{W} is not a multiple of {m} (2^pool_layers) in both dimensions: crop or pad the "
                           f"images, or predict with pad_mode='edge' | 'reflect' | 'constant' to pad them on the device "
                           f"(pad_mode is None)")
        Hp, Wp, top, left = padded_geometry(H, W, c.get("pool_layers", 4))
        return (Hp, Wp), (top, left)

    def _cfg_kwargs(self, hw=None) -> dict:
        """The architecture keywords of ``make_cfg`` / ``UNetEngine`` from the config, at geometry ``hw`` -- None: the config's
        size, padded where it is no multiple of 2^pool_layers."""
        c = self.config
        H, W = hw or self._geometry(None, "edge")[0]
        return dict(input_channels=c["input_channels"], num_classes=c["num_classes"], image_height=H, image_width=W,
                    start_neurons=c.get("start_neurons", 8), pool_layers=c.get("pool_layers", 4),
                    conv_layers=c.get("conv_layers", 2), enc_kernel=tuple(c.get("enc_kernel", (3, 3))),
                    dec_kernel=tuple(c.get("dec_kernel", (2, 2))),
                    dtype=c.get("dtype", "float32"),   # extension key: 'bfloat16' = bf16 activation storage (BASELINE configs[2])
                    max_classes=16)                    # the model follows the data: every class count the library takes

    def _mark_changed(self, eng) -> None:
        """``eng`` -- the active engine -- has changed the model's weights (an optimizer step, ``set_weights``, the moving
        statistics of a training forward): every other cached engine is stale from here on."""
        self._wver += 1
        eng._wver = self._wver

    def _activate(self, eng):
        """Make ``eng`` the active engine; if another engine changed the weights since ``eng`` last held them, they move
        first: a device-to-device copy of the two flat tensors, whose layout does not depend on H, W."""
        cur = self._engine
        if cur is not None and cur is not eng and eng._wver != self._wver:
            eng.params.copy_(cur.params); eng.state.copy_(cur.state)
        eng._wver = self._wver
        self._engine = eng
        return eng

    def _ensure_engine(self, batch: int, training: bool, hw=None):
        """The engine for ``batch`` images of size ``hw`` -- (H, W), a multiple of 2^pool_layers; None: the config's
        geometry -- holding the model's current weights.  Engines are cached by geometry, at most two: the most recent
        training engine and the most recent other one (a training engine also serves inference at its geometry)."""
        from ..engine import UNetEngine
        (H, W), _ = self._geometry(hw)
        fits = lambda e: (e.cfg.H, e.cfg.W) == (H, W)       # noqa: E731
        serves = lambda e: fits(e) and e.cfg.max_batch >= batch and (e.cfg.training or not training)      # noqa: E731
        cache = self._engines
        for e in (self._engine, cache.get("train"), cache.get("other")):
            if e is not None and serves(e):
                return self._activate(e)
        # build: a cached engine of this geometry is replaced (its batch and its training flag are kept)
        old = [e for e in cache.values() if fits(e)]
        max_batch = max([batch] + [e.cfg.max_batch for e in old])
        training = training or any(bool(e.cfg.training) for e in old)
        seed, rank = int(self.config.get("seed", 0)), parallel.env_rank()[0]
        new = UNetEngine(device=self._dev(), max_batch=max_batch, training=training, seed=seed * 1000003 + rank, init_seed=seed,
                         **self._cfg_kwargs((H, W)))
        if self._engine is None and self._pending_weights is not None:
            new.set_weights(self._pending_weights)
        self._pending_weights = None
        if training:
            # the optimizer slots follow the training engine; failing one, the engine of this geometry that is replaced
            donor = cache.get("train") or next(iter(old), None)
            if donor is not None:
                new._opt, new.opt_step = donor._opt, donor.opt_step
        for k in [k for k, e in cache.items() if fits(e)]:
            del cache[k]
        cache["train" if training else "other"] = new
        return self._activate(new)

    def release_engines(self) -> None:
        """Drop every cached engine (their device memory goes back once nothing else refers to them).  The model keeps its
        weights -- the next use builds an engine and loads them -- but not the optimizer slots."""
        if self._engine is not None:
            self._pending_weights = self._engine.get_weights()
        self._engine = None
        self._engines = {}
        self._reducer = None

    @property
    def engine(self):
        return self._engine if self._engine is not None else self._ensure_engine(1, False)

    # ---- keras.Model surface -------------------------------------------------------------------------
    def compile(self, optimizer=None, loss=None, metrics=None, ignore_label=None, pad_mode=None, pad_value=0, **kwargs):
        """``ignore_label``: a label value in ``num_classes..255`` whose pixels ``fit`` / ``evaluate`` leave out of the loss,
        the Dice metrics and the gradient (``UNetEngine.set_ignore_label``); ``None``: every pixel counts.
        ``pad_mode`` ("edge", "reflect" or "constant" with ``pad_value``): sets the model's ``pad_mode`` / ``pad_value``
        attributes and lets ``fit`` / ``evaluate`` consult them, i.e. pad batches whose size is no multiple of 2^pool_layers
        and keep the frame out of the loss.  ``None`` leaves the attributes alone and ``fit`` / ``evaluate`` refusing such
        sizes whatever the attributes say (they then serve inference only)."""
        from ..common.utils import check_pad_mode
        if pad_mode is not None:
            try:
                self.pad_mode, self.pad_value = check_pad_mode(pad_mode, pad_value)
            except ValueError as e:
                raise OctError(f"compile(pad_mode=...): {e}") from None
        self._pad_fit = pad_mode is not None
        if ignore_label is not None:
            if int(ignore_label) != ignore_label or not int(self.config["num_classes"]) <= int(ignore_label) <= 255:
                raise OctError(f"compile(ignore_label=...): must be None or an integer in num_classes..255, not {ignore_label!r}")
            ignore_label = int(ignore_label)
        self.ignore_label = ignore_label
        loss_name = getattr(loss, "oct_loss", None) if loss is not None else None
        if loss is not None and loss_name not in ("dice_loss_macro", "dice_loss_micro", "focal_dice_loss", "bce_dice_loss"):
            raise OctError("compile(loss=...): only the Dice losses, focal_dice_loss and bce_dice_loss from common.custom_losses are "
                           "implemented by the HIP engine (the loss arithmetic is fused into the head kernels)")
        self._focal = dict(getattr(loss, "oct_focal", None) or {}) if loss_name == "focal_dice_loss" else None
        # the shape of the Dice term (the factories' alpha / beta / tversky_gamma / dice_class_weight; None: plain Dice): every
        # engine this model steps gets it with the loss kind, per batch (select_loss), the padded-size training engine included
        self._dice_shape = getattr(loss, "oct_dice_shape", None) if loss is not None else None
        # border weights of the pixel term (the factories' edge_weight; None: none): the map is built per batch on the device,
        # behind the augmentations and the pad (_run_epoch)
        self._edge_weight = getattr(loss, "oct_edge_weight", None) if loss is not None else None
        metric_name = None
        for m in metrics or []:
            metric_name = getattr(m, "oct_metric", None)
            if metric_name not in ("dice_coef_macro", "dice_coef_micro"):
                raise OctError("compile(metrics=...): only dice_coef_macro / dice_coef_micro are implemented")
        if optimizer is not None and not hasattr(optimizer, "apply"):
            raise OctError("compile(optimizer=...): pass an instance of one of the optimizers.Optimizer classes "
                           "(SGD, Adam, Adamax, RMSprop, Adagrad, Adadelta)")
        self.optimizer, self._loss_name, self._metric_name = optimizer, loss_name, metric_name

    def count_params(self) -> int:
        from ..engine import make_cfg
        from .. import _hip
        import ctypes as C
        cfg = make_cfg(**self._cfg_kwargs())    # (the padded geometry's table where the config's size is no multiple of 2^pool_layers)
        l = _hip.lib()
        return int(l.oct_unet_param_count(C.byref(cfg)) + l.oct_unet_state_count(C.byref(cfg)))

    def summary(self, print_fn=print):
        from ..engine import make_cfg, layer_table
        cfg = make_cfg(**self._cfg_kwargs())    # (the padded geometry's table where the config's size is no multiple of 2^pool_layers)
        print_fn(f'Model: "{self.name}"  (MI355X HIP engine)')
        print_fn(f"{'layer':14s}{'kernel':>8s}{'in':>6s}{'out':>6s}{'HxW':>12s}{'params':>10s}")
        tot = 0
        for L in layer_table(cfg):
            n = L["kh"] * L["kw"] * L["cin"] * L["cout"] + L["cout"] + (4 * L["cout"] if L["has_bn"] else 0)
            tot += n
            print_fn(f"{L['name']:14s}{str(L['kh']) + 'x' + str(L['kw']):>8s}{L['cin']:>6d}{L['cout']:>6d}"
                     f"{str(L['out_h']) + 'x' + str(L['out_w']):>12s}{n:>10d}")
        print_fn(f"Total params: {tot}")

    def get_weights(self):
        if self._engine is None:
            if self._pending_weights is not None:
                return [np.array(w) for w in self._pending_weights]
            return self.engine.get_weights()
        return self._engine.get_weights()

    def set_weights(self, weights):
        if self._engine is None:
            self._pending_weights = [np.asarray(w, np.float32) for w in weights]
        else:
            self._engine.set_weights(weights)
            self._mark_changed(self._engine)

    def save(self, filepath, **kwargs) -> Path:
        """Write architecture config + weights (Keras ``get_weights()`` order).  A ``.h5`` / ``.hdf5`` path is
        written in the Keras HDF5 weight layout when ``h5py`` is importable (``common/keras_h5.py``: loadable by the
        reference's ``UNet(**cfg).build_model().load_weights``); otherwise -- and for any other suffix -- an ``.npz``
        container is written (``foo.hdf5`` becomes ``foo.hdf5.npz``)."""
        from ..common import keras_h5
        path = Path(filepath)
        as_h5 = path.suffix in (".h5", ".hdf5") and keras_h5.have_h5py()
        if not as_h5 and path.suffix != ".npz":
            path = Path(str(path) + ".npz")
        w = self.get_weights()
        if parallel.world_size() > 1 and self._engine is not None:
            # BN moving statistics are per replica; they are mean-reduced when read
            avg = parallel.average_moving_stats(self._engine.state)
            keep = self._engine.state.clone(); self._engine.state.copy_(avg)
            w = self._engine.get_weights(); self._engine.state.copy_(keep)
        payload = {f"w{i:03d}": a for i, a in enumerate(w)}
        payload["format"] = np.array(WEIGHTS_FORMAT)
        payload["name"] = np.array(self.name)
        payload["config_json"] = np.array(json.dumps(self.config))
        if parallel.env_rank()[0] == 0:
            path.parent.mkdir(parents=True, exist_ok=True)
            if as_h5:
                keras_h5.export_keras_h5(path, w, self.config)
            else:
                np.savez(path, **payload)
        return path

    # ---- training -------------------------------------------------------------------------------------
    @property
    def feed(self) -> BatchFeed:
        """The model's input path, made at first use (the device may be set after construction)."""
        self._feed = self._feed or BatchFeed(self._dev())
        return self._feed

    def _staged(self, key, arr: np.ndarray) -> torch.Tensor: return self.feed.staged(key, arr)

    def _pad_batch(self, eng, x, lab, at, pad_mode, pad_value, ignore):
        """One batch of a size that is no multiple of 2^pool_layers -> the engine's geometry, on the compute stream: the images
        by ``pad_mode``, the labels -- same kernel, it moves bytes -- in ``constant`` mode with the ignore label.  The padded
        pair belongs to ``eng`` and is made once per batch size (and image type): its last reader, this step's backward,
        is queued on the same stream in front of the next step's pad, so one pair is enough."""
        B, (Hp, Wp) = x.shape[0], (eng.cfg.H, eng.cfg.W)
        pair = eng._pad_bufs.get((B, x.dtype))
        if pair is None:
            pair = eng._pad_bufs[(B, x.dtype)] = (torch.empty((B, Hp, Wp, x.shape[3]), dtype=x.dtype, device=x.device),
                                                  torch.empty((B, Hp, Wp, 1), dtype=torch.uint8, device=x.device))
        xp = eng.pad(x, Hp, Wp, *at, pad_mode, pad_value, out=pair[0])
        lp = eng.pad(lab.view(B, x.shape[1], x.shape[2], 1), Hp, Wp, *at, "constant", ignore, out=pair[1])
        return xp, lp

    def _loss_plan(self):
        """``(kind, focal parameters)`` for ``UNetEngine.select_loss``, ``macro`` for the backward, and the index of the logged
        loss in the loss vector of that kind (bce_dice_loss is bce + dice_loss_micro: the micro combination only)."""
        f = self._focal
        kind = "focal" if f else "bce" if self._loss_name == "bce_dice_loss" else "dice"
        macro = f["dice_macro"] if f else self._loss_name not in ("dice_loss_micro", "bce_dice_loss")
        params = (f["focal_loss_weight"], f["gamma"], f["class_weight"]) if f else ()
        return kind, params, macro, (0 if kind == "dice" else 5) + (0 if macro else 1)

    def _run_epoch(self, seq, training: bool, rank: int, world: int):
        kind, focal, macro, loss_at = self._loss_plan()
        pad_mode, pad_value = self._pad_options(None, 0) if self._pad_fit else (None, 0.0)
        feed, acc, n = self.feed, None, len(seq)
        # the upload of batch i+1 (host gather -> pinned buffers -> H2D on the copy stream) is queued before step i is
        # launched, so it runs under that step
        queue = lambda i: feed.upload(feed.host_batch(seq, i, rank, world), i % 3)      # noqa: E731
        nxt = queue(0) if n else None
        for i in range(n):
            b = nxt
            if b.ready is not None:
                torch.cuda.current_stream(b.x.device).wait_event(b.ready)
            if i + 1 < n:
                nxt = queue(i + 1)
            # validation data may have another size; one that is no multiple of 2^pool_layers runs on the engine of the padded
            # geometry under the model's pad_mode (None, or a model not compiled with one: the OctError of _geometry)
            x, lab = b.x, b.labels
            hw, raw_u8 = tuple(x.shape[1:3]), x.dtype == torch.uint8
            try:
                geom, at = self._geometry(hw, pad_mode)
            except OctError as e:
                raise OctError(f"{e}; fit / evaluate pad such batches in a model compiled with compile(pad_mode=...)") from None
            eng = self._ensure_engine(x.shape[0], training, hw=geom)
            if b.ops is not None:
                x, lab = feed.augment(eng, seq.oct_aug_seed, b)    # at the true size: the frame is not warped or flipped
            ignore = self.ignore_label
            if at is not None:
                ignore = 255 if ignore is None else ignore
                # pad_value is in the units of the Sequence's batches: raw counts where the augment stage has turned them to [0, 1]
                x, lab = self._pad_batch(eng, x, lab, at, pad_mode, pad_value / 255.0 if raw_u8 and x.dtype != torch.uint8 else pad_value,
                                         ignore)
            eng.select_loss(kind, *focal, ignore_label=ignore, dice_shape=self._dice_shape,      # per batch: the engine may be new, or another model's last
                            edge_weight=self._edge_weight)
            if self._edge_weight:
                # the border weight map of the labels as the loss sees them: deformed, flipped, padded (the frame is unknown
                # and makes no edge), in training and validation alike; into the engine's buffer, set before the forward
                eng.edge_weight_step(lab, self._edge_weight)
            eng.forward(x, training=training, labels=lab, want_probs=False)
            loss = eng.loss_selected()
            if training:
                if self._reducer is None or self._reducer.engine is not eng:       # _ensure_engine may have built a new engine
                    self._reducer = parallel.GradReducer(eng, overlap=True)
                # backward + all-reduce (the decoder half on a side stream under the encoder backward)
                self._reducer.backward_and_reduce(lab, macro=macro, loss_scale=1.0 / world)
                self.optimizer.apply(eng)
                self._mark_changed(eng)      # (the training forward's moving statistics included)
            acc = loss.clone() if acc is None else acc + loss
            feed.release(i % 3)
        if acc is None:
            return {}
        acc = acc / n
        if world > 1:
            torch.distributed.all_reduce(acc); acc /= world
        v = acc.cpu().numpy()
        out = {"loss": float(v[loss_at])}
        if self._metric_name:
            out[self._metric_name] = float(v[2] if self._metric_name == "dice_coef_macro" else v[3])
        return out

    def fit(self, x=None, validation_data=None, epochs: int = 1, callbacks=None, verbose: int = 1,
            initial_epoch: int = 0, **kwargs):
        if self.optimizer is None or self._loss_name is None:
            raise OctError("fit() before compile(optimizer=..., loss=...)")
        rank, _, world = parallel.env_rank()
        world = parallel.world_size() if world > 1 else 1
        hist = History()
        cbs = list(callbacks or []) + [hist]
        for cb in cbs:
            cb.set_model(self)
        self.stop_training = False
        for cb in cbs:
            cb.on_train_begin({})
        for epoch in range(initial_epoch, epochs):
            for cb in cbs:
                cb.on_epoch_begin(epoch, {})
            t0 = time.time()
            logs = self._run_epoch(x, True, rank, world)
            if hasattr(x, "on_epoch_end"):
                x.on_epoch_end()
            if validation_data is not None:
                vlogs = self._run_epoch(validation_data, False, rank, world)
                logs.update({"val_" + k: v for k, v in vlogs.items()})
                if hasattr(validation_data, "on_epoch_end"):
                    validation_data.on_epoch_end()
            if verbose and rank == 0:
                msg = " - ".join(f"{k}: {v:.4f}" for k, v in logs.items())
                print(f"Epoch {epoch + 1}/{epochs} - {time.time() - t0:.1f}s - {msg}")
            for cb in cbs:
                cb.on_epoch_end(epoch, logs)
            if self.stop_training:
                break
        for cb in cbs:
            cb.on_train_end({})
        self.history = hist
        return hist

    def evaluate(self, x, verbose: int = 0, **kwargs):
        rank, _, world = parallel.env_rank()
        world = parallel.world_size() if world > 1 else 1
        logs = self._run_epoch(x, False, rank, world)
        return [logs.get("loss")] + ([logs[self._metric_name]] if self._metric_name else [])

    # ---- inference --------------------------------------------------------------------------------------
    def _pad_options(self, pad_mode, pad_value):
        """The validated (pad_mode, pad_value) of a call: its own, or with ``pad_mode=None`` the model's attributes."""
        from ..common.utils import check_pad_mode
        if pad_mode is None:
            pad_mode, pad_value = self.pad_mode, self.pad_value
        return check_pad_mode(pad_mode, pad_value)

    @staticmethod
    def _contrast_option(contrast, x: np.ndarray):
        """The validated ``contrast=`` spec of a predict call on host array ``x``: None (off), or a spec that fits the images'
        size; only raw uint8 images have a contrast stage."""
        from ..common.utils import check_contrast
        if contrast is not None and x.dtype != np.uint8:
            raise ValueError(f"contrast needs raw uint8 images, not {x.dtype}")
        return check_contrast(contrast, hw=x.shape[1:3])

    def _inference_batches(self, x: np.ndarray, bs: int, pad, contrast=None, **kind):
        """The loop of the predict methods over host array ``x`` in batches of ``bs`` under the validated ``pad`` = (pad_mode,
        pad_value): yields per batch the host slice bounds ``lo, hi``, the engine of the images' geometry and the maps of
        ``UNetEngine.infer(batch, **kind)``, of the images' size.  For a size that is no multiple of 2^pool_layers the engine is
        that of the padded geometry and ``infer`` pads in front and crops behind.  ``contrast`` (a validated spec): the uploaded
        batch goes through ``UNetEngine.contrast`` in place first, at its true size."""
        n, (H, W) = x.shape[0], x.shape[1:3]
        geom, at = self._geometry((H, W), pad[0])
        eng = self._ensure_engine(min(bs, n), False, hw=geom)
        for lo in range(0, n, bs):
            xb = torch.from_numpy(np.ascontiguousarray(x[lo:lo + bs])).to(eng.device)
            if contrast is not None:
                eng.contrast(xb, contrast, out=xb)
            yield lo, min(lo + bs, n), eng, eng.infer(xb, pad=None if at is None else (*at, *pad), **kind)

    def predict(self, x, verbose=0, batch_size: Optional[int] = None, pad_mode: Optional[str] = None, pad_value=0,
                temperature: Optional[float] = None, contrast=None, **kwargs) -> np.ndarray:
        """(n,H,W,C) float input ALREADY preprocessed to [0,1] (or raw uint8) -> (n,H,W,num_classes) float32.  The engine
        follows the images' size, whatever the config records.  A size that is no multiple of 2^pool_layers needs
        ``pad_mode`` ("edge", "reflect" or "constant" with ``pad_value``, in the units of ``x``): the batch is padded on
        the device in front of the forward and the output cropped behind it (placement: ``common.utils.padded_geometry``).
        ``pad_mode=None`` takes the model's ``pad_mode`` / ``pad_value`` attributes, which are None / 0 unless set.
        ``temperature`` (a number in [1/16, 16]; None or 1.0: off): the probabilities are tempered on the device --
        softmax(logits / temperature), formed from the probabilities themselves (``UNetEngine.temperature_apply``).
        ``contrast`` (a spec of ``common.utils.check_contrast``; None: off; raw uint8 ``x`` only): every batch is normalised on
        the device in front of the pad and the forward -- the output is that of ``predict(contrast_reference(x, contrast))``.
        It is a keyword of the call and not an attribute of the model: ``train_model(contrast=)`` hands ``fit`` arrays that
        are already normalised."""
        from ..evaluation.calibration import check_temperature
        temperature = 1.0 if temperature is None else check_temperature(temperature)
        pad = self._pad_options(pad_mode, pad_value)
        x = np.asarray(x)
        if x.dtype != np.uint8:
            x = np.ascontiguousarray(x, dtype=np.float32)   # Keras casts the float64 the reference passes to float32
        contrast = self._contrast_option(contrast, x)
        out = np.empty(x.shape[:3] + (self.config["num_classes"],), np.float32)
        for lo, hi, eng, maps in self._inference_batches(x, int(batch_size or min(x.shape[0], 32)), pad, contrast=contrast,
                                                         want_probs=True, want_argmax=False):
            probs = maps["probs"]
            if temperature != 1.0:
                eng.temperature_apply(probs, 1.0 / temperature, out=probs)
            out[lo:hi] = probs.cpu().numpy()
        return out

    def fit_temperature(self, x_u8, labels, batch_size: Optional[int] = None, ignore_label: Optional[int] = None,
                        pad_mode: Optional[str] = None):
        """The temperature that minimises the NLL of this model's probabilities on ``x_u8`` (input as for ``predict``) against
        ``labels`` (n,H,W[,1]), class maps in which ``ignore_label`` (None, or an int in num_classes..255) marks pixels that do
        not count (temperature scaling, Guo et al. 2017).  ``evaluation.calibration.fit_beta`` drives it;
        each of its steps is one pass over the data -- per batch the forward, then ``UNetEngine.temperature_nll`` on the
        probabilities, which never leave the device -- and the per-image sums are added on the host in image order.  Returns a
        record with ``temperature``, ``beta`` = 1 / temperature, ``nll_before`` / ``nll_after`` (mean NLL per counted pixel at
        temperature 1 and at the result), ``steps``, ``counted`` and ``at_bound`` (the optimum lies outside [1/16, 16]).
        ``pad_mode`` as for ``predict`` (None: the model's attributes)."""
        from ..evaluation.calibration import fit_with
        from ..evaluation.dice_device import check_ignore_label
        ignore_label = check_ignore_label(ignore_label, self.config["num_classes"])
        pad = self._pad_options(pad_mode, 0)
        x = np.asarray(x_u8)
        if x.dtype != np.uint8:
            x = np.ascontiguousarray(x, dtype=np.float32)
        lab = np.asarray(labels)
        lab = lab[..., 0] if lab.ndim == 4 else lab
        if lab.shape != x.shape[:3]:
            raise ValueError(f"labels of shape {np.asarray(labels).shape} for images of shape {x.shape}")
        C = int(self.config["num_classes"])
        if ((lab < 0) | ((lab >= C) & (lab != (-1 if ignore_label is None else ignore_label)))).any():
            raise ValueError(f"labels outside 0..{C - 1}" + ("" if ignore_label is None else f" that are not the ignore label {ignore_label}"))
        lab = np.ascontiguousarray(lab.astype(np.uint8))
        bs = int(batch_size or min(x.shape[0], 32))

        def sums_at(beta):
            tot, n = np.zeros(3), 0.0
            for lo, hi, eng, maps in self._inference_batches(x, bs, pad, want_probs=True, want_argmax=False):
                y = torch.from_numpy(lab[lo:hi]).to(eng.device)
                s, cnt = eng.temperature_nll(maps["probs"], y, [beta], ignore_label)
                s, cnt = s.cpu().numpy(), cnt.cpu().numpy()
                for i in range(hi - lo):
                    tot, n = tot + s[i, 0], n + cnt[i]
            return tot, n

        return fit_with(sums_at)

    def predict_mc(self, x, samples: int, batch_size: Optional[int] = None, step0: int = 0):
        """Monte-Carlo dropout prediction: ``samples`` stochastic forwards per batch with the bottleneck dropout on (dropout
        steps ``step0 .. step0+samples-1``, the same for every batch; ``UNetEngine.infer(mc=...)``), reduced on the device.
        Input as for ``predict``; returns ``(mean_probs (n,H,W,num_classes), entropy (n,H,W), mutual_info (n,H,W))``
        float32.  The dropout stream is indexed by the element's position in the bottleneck tensor of its BATCH and seeded
        per rank, so an image's result depends on its position in its batch (hence on ``batch_size``) and on the rank.
        Padding as for ``predict``, from the model's ``pad_mode`` / ``pad_value`` attributes (this method's parameter list
        is fixed): the three maps are cropped on the device."""
        x = np.asarray(x)
        if x.dtype != np.uint8:
            x = np.ascontiguousarray(x, dtype=np.float32)
        keys = ("mean_probs", "entropy", "mutual_info")
        mean = np.empty(x.shape[:3] + (self.config["num_classes"],), np.float32)
        ent, mi = np.empty(x.shape[:3], np.float32), np.empty(x.shape[:3], np.float32)
        for lo, hi, _, out in self._inference_batches(x, int(batch_size or min(x.shape[0], 32)), self._pad_options(None, 0),
                                                      mc=(samples, step0), want_probs=True, want_argmax=True):
            mean[lo:hi], ent[lo:hi], mi[lo:hi] = (out[k].cpu().numpy() for k in keys)
        return mean, ent, mi

    def predict_tta(self, x, views, batch_size: Optional[int] = None):
        """Test-time-augmented prediction: one forward per view of ``views`` -- 1..4 distinct names of
        ``common.utils.TTA_VIEWS``, e.g. ``("identity", "flip_lr")`` -- on the batch mirrored by it, mirrored back and
        averaged on the device (``UNetEngine.infer(tta=...)``).  Input as for ``predict``; returns ``(mean_probs
        (n,H,W,num_classes) float32, argmax (n,H,W) uint8 of the mean, entropy (n,H,W), mutual_info (n,H,W))``, the last two
        float32: the predictive entropy of the mean and the mutual information over the views.  Deterministic, and
        independent of the batch an image sits in.  Padding as for ``predict_mc``, from the model's ``pad_mode`` /
        ``pad_value`` attributes: the views are flips of the PADDED batch and the four maps are cropped on the device."""
        x = np.asarray(x)
        if x.dtype != np.uint8:
            x = np.ascontiguousarray(x, dtype=np.float32)
        keys = ("mean_probs", "argmax", "entropy", "mutual_info")
        mean = np.empty(x.shape[:3] + (self.config["num_classes"],), np.float32)
        am, ent, mi = np.empty(x.shape[:3], np.uint8), np.empty(x.shape[:3], np.float32), np.empty(x.shape[:3], np.float32)
        for lo, hi, _, out in self._inference_batches(x, int(batch_size or min(x.shape[0], 32)), self._pad_options(None, 0),
                                                      tta=views, want_probs=True, want_argmax=True):
            mean[lo:hi], am[lo:hi], ent[lo:hi], mi[lo:hi] = (out[k].cpu().numpy() for k in keys)
        return mean, am, ent, mi

    def predict_ordered(self, x, batch_size: Optional[int] = None):
        """Topology-correct class maps: per column the best labelling whose class index never decreases with depth, decoded on
        the device from the class probabilities (``UNetEngine.ordered_decode``).  Input as for
        ``predict``; returns ``(labels (n,H,W) uint8, rows (n,C-1,W) uint16)`` -- ``rows[i]`` is the first row of a class above
        i in the column (0: the column starts below boundary i; H: no such class), so the rows never cross.  The label map is
        the authoritative one.  Needs 2..16 classes and H <= 4096.  Padding as for ``predict_mc``, from the model's ``pad_mode``
        / ``pad_value`` attributes: the probabilities are cropped in front of the decode."""
        from ..evaluation.ordered import check_ordered
        x = np.asarray(x)
        if x.dtype != np.uint8:
            x = np.ascontiguousarray(x, dtype=np.float32)
        C = int(self.config["num_classes"])
        check_ordered(C, x.shape[1], "predict_ordered")
        labels, rows = np.empty(x.shape[:3], np.uint8), np.empty((x.shape[0], C - 1, x.shape[2]), np.uint16)
        for lo, hi, eng, maps in self._inference_batches(x, int(batch_size or min(x.shape[0], 32)), self._pad_options(None, 0),
                                                         want_probs=True, want_argmax=False):
            lab, r, _ = eng.ordered_decode(maps["probs"])
            labels[lo:hi], rows[lo:hi] = lab.cpu().numpy(), r.cpu().numpy().view(np.uint16)
        return labels, rows

    def predict_components(self, x, rule, batch_size: Optional[int] = None):
        """Island removal and component counts of the arg-max class maps, on the device (``oct_components`` /
        ``oct_component_filter``).  Input as for ``predict``; ``rule`` is an
        ``evaluation.components.ComponentRule`` or a dict of its keywords.  Returns ``(labels (n,H,W) uint8, stats (n,C,2) uint32,
        removed (n,C) uint32)``: the cleaned maps, per class (components, pixels of the largest one) of the ARG-MAX maps, and the
        removed pixels per class.  Padding as for ``predict_mc``, from the model's ``pad_mode`` / ``pad_value`` attributes: the
        arg-max maps are cropped in front of the labelling."""
        from ..evaluation.components import ComponentRule, Components, check_components
        x = np.asarray(x)
        if x.dtype != np.uint8:
            x = np.ascontiguousarray(x, dtype=np.float32)
        C = int(self.config["num_classes"])
        rule = ComponentRule.coerce(rule, "predict_components")
        if rule is None:
            raise ValueError("predict_components: needs a rule")
        rule.check(C, "predict_components")
        check_components(C, x.shape[1], x.shape[2], "predict_components")
        n, bs = x.shape[0], int(batch_size or min(x.shape[0], 32))
        labels, stats, removed = np.empty(x.shape[:3], np.uint8), np.empty((n, C, 2), np.uint32), np.empty((n, C), np.uint32)
        stage = None
        for lo, hi, eng, maps in self._inference_batches(x, bs, self._pad_options(None, 0), want_probs=False, want_argmax=True):
            if stage is None:
                stage = Components(bs, x.shape[1], x.shape[2], C, rule, eng.device)
            labels[lo:hi], stats[lo:hi], removed[lo:hi] = stage.to_host(*stage(maps["argmax"].reshape(hi - lo, *x.shape[1:3])))
        return labels, stats, removed

    def predict_labels(self, x_u8: np.ndarray, batch_size: int = 32, want_maps: bool = False, bg_ilm: bool = True,
                       bg_csi: bool = False, soft_maps: bool = False, mc_samples: int = 0, mc_step0: int = 0,
                       pad_mode: Optional[str] = None, pad_value=0, tta=None, ordered: bool = False, contrast=None):
        """Raw uint8 images -> uint8 arg-max class maps (n,H,W), computed on the device (1 B/px back instead of
        4*C B/px).  With ``want_maps`` also the (n, C-1, H, W) uint8 boundary maps of
        ``convert_predictions_to_maps_semantic``, computed on the device from the class maps -- or, with ``soft_maps``,
        from the class probabilities, which stay on the device (``UNetEngine.boundary_maps_soft``).
        With ``mc_samples`` > 0 every batch is a Monte-Carlo dropout prediction (``predict_mc``): the class maps and
        boundary maps are those of the mean prediction, and the (n,H,W) float32 predictive entropy and mutual information
        are returned behind them -- ``(labels, entropy, mutual_info)`` or ``(labels, maps, entropy, mutual_info)``.
        With ``tta`` (view names as for ``predict_tta``; not together with ``mc_samples``) every batch is the mean prediction
        over the flipped views instead, returned in the same form.
        ``pad_mode`` / ``pad_value`` (in raw counts, like ``x_u8``) as for ``predict``: the arg-max maps -- and the
        probabilities and uncertainty maps where they are made -- are cropped on the device directly behind the head, and
        the boundary maps are those of the cropped tensors.
        With ``ordered`` the ordered decode (``predict_ordered``) of the same probabilities -- the mean ones under
        ``mc_samples`` / ``tta`` -- is appended as the LAST element: ``(labels (n,H,W) uint8, rows (n,C-1,W) uint16, score (n,W)
        uint32)``.
        ``contrast`` as for ``predict`` (uint8 images only): the result is that of ``predict_labels(contrast_reference(x_u8,
        contrast))``."""
        if soft_maps and not want_maps:
            raise ValueError("soft_maps: needs want_maps=True")
        from ..common.utils import check_tta
        tta = check_tta(tta, mc_samples)
        pad_mode, pad_value = self._pad_options(pad_mode, pad_value)
        x_u8 = np.ascontiguousarray(x_u8)
        contrast = self._contrast_option(contrast, x_u8)
        if x_u8.dtype != np.uint8:
            # the reference normalises x / 255 whatever the dtype (models/unet.py:87-91); the engine's float32 input
            # path means "already normalised", so do the division here rather than silently skipping it
            x_u8 = np.ascontiguousarray(x_u8.astype(np.float32) / np.float32(255.0))
            pad_value = float(np.float32(pad_value) / np.float32(255.0))
        out = np.empty(x_u8.shape[:3], np.uint8)
        maps = np.empty((x_u8.shape[0], self.config["num_classes"] - 1) + tuple(x_u8.shape[1:3]), np.uint8) if want_maps else None
        unc = (np.empty(x_u8.shape[:3], np.float32), np.empty(x_u8.shape[:3], np.float32)) if mc_samples or tta else ()
        C = int(self.config["num_classes"])
        dec = ((np.empty(x_u8.shape[:3], np.uint8), np.empty((x_u8.shape[0], C - 1, x_u8.shape[2]), np.uint16),
                np.empty((x_u8.shape[0], x_u8.shape[2]), np.uint32)),) if ordered else ()
        kind = dict(mc=(mc_samples, mc_step0) if mc_samples else None, tta=tta or None, want_probs=soft_maps or bool(ordered),
                    want_argmax=True)
        for lo, hi, eng, mc in self._inference_batches(x_u8, batch_size, (pad_mode, pad_value), contrast=contrast, **kind):
            probs, am = mc.get("mean_probs", mc.get("probs")), mc["argmax"]
            if dec:
                for o, t, dt in zip(dec[0], eng.ordered_decode(probs), (np.uint8, np.uint16, np.uint32)):
                    o[lo:hi] = t.cpu().numpy().view(dt)
            if unc:
                unc[0][lo:hi], unc[1][lo:hi] = mc["entropy"].cpu().numpy(), mc["mutual_info"].cpu().numpy()
            out[lo:hi] = am.cpu().numpy()
            if want_maps:
                dev_maps = (eng.boundary_maps_soft(probs, bg_ilm=bg_ilm, bg_csi=bg_csi) if soft_maps
                            else eng.boundary_maps(am, bg_ilm=bg_ilm, bg_csi=bg_csi))
                maps[lo:hi] = dev_maps.cpu().numpy()
        if dec:
            return ((out, maps) if want_maps else (out,)) + unc + dec
        return ((out, maps) if want_maps else out) if not unc else ((out, maps) + unc if want_maps else (out,) + unc)


def load_model(path) -> Model:
    """Counterpart of ``tf.keras.models.load_model(compile=False)`` for files written by ``Model.save``.
    Only arrays and JSON are read (``allow_pickle=False``)."""
    from ..common import keras_h5
    path = Path(path)
    if keras_h5.is_keras_h5_path(path):
        # a Keras HDF5 checkpoint (written by the reference's ModelCheckpoint, or by Model.save with h5py present)
        config = keras_h5.read_embedded_config(path)
        if config is None:
            with open(path.parent / "model_config.json", "r") as fh:     # reference: common/utils.py:68-69
                config = json.load(fh)
        m = Model(name=config.get("name", "unet") if isinstance(config.get("name"), str) else "unet", config=config)
        m.set_weights(keras_h5.import_keras_h5(path, config))
        return m
    if not path.exists() and Path(str(path) + ".npz").exists():
        path = Path(str(path) + ".npz")
    with np.load(path, allow_pickle=False) as z:
        if str(z["format"]) != WEIGHTS_FORMAT:
            raise OctError(f"{path}: unknown weights format {z['format']}")
        config = json.loads(str(z["config_json"]))
        name = str(z["name"])
        weights = [z[k] for k in sorted(k for k in z.files if k.startswith("w") and k[1:].isdigit())]
    m = Model(name=name, config=config)
    m.set_weights(weights)
    return m
