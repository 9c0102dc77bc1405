"""Batch generator with the reference's input contract
(oct_image_segmentation_models/common/data_generator.py:10-416), re-stated with all three augmentation modes:

* ``X = float32(images / 255)`` of shape (B,H,W,C) -- the reference computes ``u8/255*255/255``
  (data_generator.py:76,239 + models/unet.py:89), within one ulp of this;
* labels are passed through unchanged (one-hot for dense losses, (B,H,W,1) for sparse ones);
* ``len() = floor(total_samples / batch_size)`` (tail dropped); the generator is stateful, ignores the
  ``index`` argument and must be consumed sequentially; ``on_epoch_end`` composes a fresh permutation onto
  the previous one (``sample_shuffle = sample_shuffle[s]``), seeded from the OS unless a seed is given.

Augmentation (reference :140-283): ``aug_fn_args`` is a list of ``(function, arguments)`` pairs
from ``common.augmentation``; mode "all" repeats every image once per augmentation (``total_samples = N * n_augs``),
mode "one" draws one augmentation per sample with ``aug_probs``; ``aug_fly=False`` pre-computes the augmented set.
The pre-computed set is kept in float32 (the reference stores the [0,1] floats into a uint8 array, which zeroes
every image -- a defect not reproduced here).  Augmented batches take the float32 input path of the engine.

Without augmentation, batches are assembled with one fancy-indexing gather instead of the reference's per-sample Python loop
(SURVEY 3.1 hot loop ii).  ``next_batch_u8`` is the engine's fast path: uint8 images + uint8 sparse labels,
so the /255 happens on the GPU while the first conv loads the image.

``device_aug=True`` (off by default) moves the augmentations of ``common.augmentation.augmentation_map`` to the device:
``next_batch_aug`` walks the generator's state exactly as ``get_batch_list`` does but returns the raw uint8 samples and one
``oct_aug_op`` descriptor per sample; the engine's ``oct_augment_batch`` applies them (flips exactly; noise from its own
documented Philox stream, not from numpy's).  Nothing is pre-computed or kept in float on the host in that mode.

The geometric augmentations (``column_shift``, ``affine``) draw their per-sample parameters from a SECOND stream of the
generator, spawned from its seed: ``WARP_DRAWS`` uniform numbers per sample handed out, whatever augmentation the sample gets,
in the order of the global sample walk (``aug_fly``), or one table entry per (image, augmentation) pair (pre-computed set).
``augmentation.draw_warp_ops`` turns them into integer descriptors for the host path (one sample at a time) and the device
path (``next_batch_aug`` then returns a fourth array, one ``oct_warp_op`` per sample) alike, so both apply the same warp.

``elastic`` (a dict, ``augmentation.elastic_spec``) puts the elastic deformation in FRONT of whatever the list gives a sample:
every sample of an augmenting generator is deformed with probability ``p``.  Its ``ELASTIC_DRAWS`` numbers per sample come from
a THIRD stream, ``SeedSequence(seed).spawn(2)[1]``, handed out like the warps' (global sample walk, or one table entry per
pair); the other two streams do not notice.  The host path deforms the uint8 sample (``augmentation.elastic_sample``) before the
list's function sees ``float32(u8) / 255``; ``next_batch_aug`` returns the descriptors as a fifth array (the fourth is then
``None`` for a list without a warp).

``photometric`` (a dict, ``augmentation.photometric_spec``) puts blur, column shadows and a gamma / brightness / contrast
table directly BEHIND the elastic stage and in front of the list's own augmentation, on the uint8 sample; labels never
change.  Its ``PHOTO_DRAWS`` numbers per sample come from a FOURTH stream, ``SeedSequence(seed).spawn(3)[2]``, handed out
like the elastic stream's; the other three do not notice.  ``next_batch_aug`` returns the descriptors as a sixth array, with
``None`` in the unused earlier positions."""
from __future__ import annotations

import logging as log
import os
from math import floor
from typing import Callable, List, Optional, Tuple

import numpy as np

from . import augmentation


class BatchGenerator:
    def __init__(self, images: np.ndarray, labels: np.ndarray, batch_size: int, aug_fn_args: List[Tuple],
                 aug_mode: str, aug_probs: Tuple, aug_fly: bool, preprocess_input_fn: Callable,
                 seed: Optional[int] = None, device_aug: bool = False, elastic: Optional[dict] = None,
                 photometric: Optional[dict] = None):
        if aug_mode not in ("none", "one", "all"):
            log.error(f"Unrecognized augmentation mode: {aug_mode}. Allowed values: 'none', 'one', 'all'. Exiting...")
            exit(1)
        self.images_u8 = np.ascontiguousarray(images)
        self.labels = labels
        self.batch_size = int(batch_size)
        self.aug_fn_args, self.aug_mode, self.aug_probs, self.aug_fly = aug_fn_args, aug_mode, aug_probs, aug_fly
        self.preprocess_input_fn = preprocess_input_fn
        self.total_full_images = self.images_u8.shape[0]
        self.total_raw_samples = self.total_full_images
        self.total_augs = 0 if aug_mode == "none" else len(aug_fn_args)
        self.total_samples = self.total_raw_samples * self.total_augs if aug_mode == "all" else self.total_raw_samples
        if aug_mode != "none" and self.total_augs == 0:
            raise ValueError("aug_mode '%s' needs at least one augmentation function" % aug_mode)
        if aug_mode == "one" and (len(aug_probs) != self.total_augs or abs(sum(aug_probs) - 1.0) > 1e-6):
            raise ValueError("aug_probs must hold one probability per augmentation and sum to 1")
        self.image_height, self.image_width, self.num_channels = self.images_u8.shape[1:4]
        self.labels_shape = self.labels.shape
        self.batch_labels_shape = (self.batch_size,) + tuple(self.labels_shape[1:])
        self.sample_shuffle = np.arange(self.total_full_images)
        self.num_batches = int(floor(1.0 * self.total_samples / self.batch_size))
        self._rng = np.random.default_rng(seed)  # seed=None: OS entropy, as the reference's np.random.seed()
        self._sparse_cache = None
        self.batch_counter = self.full_counter = self.aug_counter = 0
        self.images = None
        self.aug_ops = None         # descriptor templates of aug_fn_args (device path)
        self.samples_drawn = 0      # GLOBAL-batch samples handed out by next_batch_aug since construction
        self.warp_ops = None        # warp descriptor templates: aug_fn_args holds a column_shift / affine
        if aug_mode != "none":
            self.warp_ops = augmentation.warp_ops_from(aug_fn_args)      # (refuses arguments outside the definition)
            if device_aug:
                self.aug_ops = augmentation.aug_ops_from(aug_fn_args)
        if self.warp_ops is not None:
            # the parameter stream of the warps: a child of the seed, beside the stream of the shuffle and the choices
            self._warp_rng = np.random.default_rng(np.random.SeedSequence(seed).spawn(1)[0])
            if aug_fly is False:    # pre-computed set: one parameter draw per (image, augmentation) pair, for good
                self._warp_table = self._warp_rng.random((self.total_full_images, self.total_augs, augmentation.WARP_DRAWS))
        self.elastic = None         # the validated ``elastic`` keyword: the stage in front of the list's augmentations
        if elastic is not None:
            if aug_mode == "none":
                raise ValueError('elastic needs an augmentation mode: to deform otherwise un-augmented samples use aug_mode '
                                 '"one" with a single "no_augmentation" entry')
            if self.images_u8.dtype != np.uint8:
                raise ValueError(f"elastic needs a uint8 image array, the dataset holds {self.images_u8.dtype}")
            self.elastic = augmentation.elastic_spec(elastic)
            # its parameter stream: a further child of the seed (the warps' is spawn(1)[0], the first child of the same parent)
            self._elastic_rng = np.random.default_rng(np.random.SeedSequence(seed).spawn(2)[1])
            if aug_fly is False:
                self._elastic_table = self._elastic_rng.random((self.total_full_images, self.total_augs, augmentation.ELASTIC_DRAWS))
        self.photometric = None     # the validated ``photometric`` keyword: the stage behind the elastic one
        if photometric is not None:
            if aug_mode == "none":
                raise ValueError('photometric needs an augmentation mode: for otherwise un-augmented samples use aug_mode '
                                 '"one" with a single "no_augmentation" entry')
            if self.images_u8.dtype != np.uint8:
                raise ValueError(f"photometric needs a uint8 image array, the dataset holds {self.images_u8.dtype}")
            self.photometric = augmentation.photometric_spec(photometric)
            # its parameter stream: the third child of the seed (the warps' is the first, the elastic stage's the second)
            self._photo_rng = np.random.default_rng(np.random.SeedSequence(seed).spawn(3)[2])
            if aug_fly is False:
                self._photo_table = self._photo_rng.random((self.total_full_images, self.total_augs, augmentation.PHOTO_DRAWS))
        if aug_mode != "none" and self.aug_ops is None:
            self._setup_host_aug()
        self.handle_epoch_end()

    def _setup_host_aug(self):
        """Host path: the float32 copy of the dataset and, with ``aug_fly=False``, the pre-computed augmented set."""
        self.images = self.images_u8.astype(np.float32) / np.float32(255.0)
        if self.aug_fly is False:
            self.aug_images, self.aug_labels = self.setup_augnofly_data()

    def setup_augnofly_data(self):
        """Pre-computed augmentations: (N, n_augs, H, W, C) float32 images and (N, n_augs, ...) labels."""
        aug_images = np.zeros((self.total_full_images, self.total_augs) + self.images.shape[1:], dtype=np.float32)
        aug_labels = np.zeros((self.total_full_images, self.total_augs) + tuple(self.labels_shape[1:]), dtype=self.labels.dtype)
        for i in range(self.total_full_images):
            for j, (aug_fn, aug_arg) in enumerate(self.aug_fn_args):
                aug_arg = self._with_warp_op(j, aug_arg, None if self.warp_ops is None else self._warp_table[i, j])
                img, lab = self._deformed(i, None if self.elastic is None else self._elastic_table[i, j],
                                          None if self.photometric is None else self._photo_table[i, j])
                aug_images[i, j], aug_labels[i, j] = aug_fn(img, lab, aug_arg)
        return aug_images, aug_labels

    def _deformed(self, ind, u, pu=None):
        """Image ``ind`` in [0, 1] and its labels as the list's function gets them: through the elastic stage where it is
        configured and the sample's uniform numbers ``u`` say so, then through the photometric stage likewise (``pu``)."""
        img8, lab = None, self.labels[ind]
        if self.elastic is not None:
            op = augmentation.draw_elastic_ops(self.elastic, u)
            if op["kind"][0]:
                img8, lab = augmentation.elastic_sample(self.images_u8[ind], lab, op)
        if self.photometric is not None:
            op = augmentation.draw_photo_ops(self.photometric, pu, self.image_height, self.image_width)
            if op["kind"][0]:
                img8 = augmentation.photometric_sample(self.images_u8[ind] if img8 is None else img8, op)
        if img8 is None:
            return self.images[ind], lab
        return img8.astype(np.float32) / np.float32(255.0), lab

    def _with_warp_op(self, j, aug_arg, u):
        """``aug_arg`` of augmentation ``j`` with the sample's warp descriptor, drawn from its uniform numbers ``u``, under
        "op" -- where that augmentation is a warp."""
        if self.warp_ops is None or self.warp_ops[j]["kind"] == 0:
            return aug_arg
        return dict(aug_arg or {}, op=augmentation.draw_warp_ops(self.aug_fn_args, [j], u))

    def _next_augmented(self):
        """One (image in [0,1], label) sample with the reference's counter semantics (get_aug_fly / get_aug_nofly)."""
        ind = self.sample_shuffle[self.full_counter]
        if self.aug_mode == "all":
            j = self.aug_counter
            self.aug_counter += 1
            if self.aug_counter == self.total_augs:
                self.aug_counter = 0
                self.full_counter += 1
        else:  # "one"
            j = int(self._rng.choice(np.arange(self.total_augs), p=self.aug_probs))
            self.full_counter += 1
        if self.aug_fly:
            aug_fn, aug_arg = self.aug_fn_args[j]
            if self.warp_ops is not None:       # every sample takes its numbers, whatever its augmentation
                aug_arg = self._with_warp_op(j, aug_arg, self._warp_rng.random(augmentation.WARP_DRAWS))
            # (likewise: deformed or not, a sample takes its numbers from the elastic stream)
            img, lab = self._deformed(ind, None if self.elastic is None else self._elastic_rng.random(augmentation.ELASTIC_DRAWS),
                                      None if self.photometric is None else self._photo_rng.random(augmentation.PHOTO_DRAWS))
            img, lab = aug_fn(img, lab, aug_arg)
        else:
            img, lab = self.aug_images[ind, j], self.aug_labels[ind, j]
        if self.full_counter == self.total_full_images:
            self.full_counter = 0
        return img, lab

    def _next_indices(self) -> np.ndarray:
        idx = np.empty(self.batch_size, dtype=np.int64)
        for k in range(self.batch_size):
            idx[k] = self.sample_shuffle[self.full_counter]
            self.full_counter += 1
            if self.full_counter == self.total_full_images:
                self.full_counter = 0
        self.batch_counter += 1
        if self.batch_counter == self.num_batches:
            self.batch_counter = 0
        return idx

    def get_batch_list(self):
        if self.aug_mode != "none":
            if self.images is None:     # a device-augmentation generator asked for host batches after all
                self._setup_host_aug()
            batch_images = np.zeros((self.batch_size,) + self.images.shape[1:], dtype="float32")
            batch_labels = np.zeros(self.batch_labels_shape)
            for k in range(self.batch_size):
                batch_images[k], batch_labels[k] = self._next_augmented()
            self.batch_counter += 1
            if self.batch_counter == self.num_batches:
                self.batch_counter = 0
            return [batch_images, batch_labels]
        idx = self._next_indices()
        batch_images = (self.images_u8[idx].astype(np.float32)) / np.float32(255.0)
        batch_labels = np.asarray(self.labels[idx], dtype=np.float64)  # the reference's label buffer is float64
        return [batch_images, batch_labels]

    def sparse_labels(self) -> np.ndarray:
        """uint8 (N,H,W) class map of the label array (argmax of a one-hot array, or the squeezed sparse map)."""
        if self._sparse_cache is None:
            lab = self.labels
            if lab.ndim == 4 and lab.shape[-1] > 1:
                lab = np.argmax(lab, axis=-1)
            elif lab.ndim == 4:
                lab = lab[..., 0]
            # (no copy for the usual (N,H,W,1) uint8 array: a view -- the copy was 1 GB per 8192 scans, inside the first epoch)
            self._sparse_cache = np.ascontiguousarray(lab, dtype=np.uint8)
        return self._sparse_cache

    def next_batch_u8(self, shard: Optional[Tuple[int, int]] = None):
        """The next GLOBAL batch; with ``shard = (lo, hi)`` only samples lo..hi-1 of it are gathered (a DP rank's slice:
        every rank advances the same shuffled order, none of them assembles the other ranks' scans)."""
        if self.images_u8.dtype != np.uint8:
            raise TypeError(f"next_batch_u8 needs a uint8 image array, the dataset holds {self.images_u8.dtype}; "
                            "use get_batch_list() (float32(images) / 255)")
        idx = self._next_indices()
        if shard is not None:
            idx = idx[shard[0]:shard[1]]
        return self.images_u8[idx], self.sparse_labels()[idx]

    def next_batch_aug(self, shard: Optional[Tuple[int, int]] = None):
        """The next GLOBAL batch for the device augmentation: ``(images uint8, labels uint8 (B,H,W), ops)`` with one
        ``augmentation.AUG_OP_DTYPE`` descriptor per sample.  The generator's state (shuffle walk, ``aug_counter`` /
        ``full_counter`` wraps, one draw of ``self._rng`` per sample in mode "one") advances exactly as in
        ``get_batch_list``, so one seed gives one sequence of (image, augmentation) pairs through either path.
        ``noise_id``: with ``aug_fly`` a running count of the samples drawn since construction (fresh noise every epoch); without,
        ``image_index * n_augs + j`` (the same noise for a pair in every epoch: what the pre-computed set means).  With
        ``shard = (lo, hi)`` only samples lo..hi-1 are gathered; their descriptors are those of the one-rank run.
        A list with a ``column_shift`` / ``affine`` returns a fourth array, one ``augmentation.WARP_OP_DTYPE`` descriptor per
        sample (kind 0 for a sample that is not warped), drawn for the GLOBAL batch and sliced like the others.  With
        ``elastic`` a fifth, one ``augmentation.ELASTIC_OP_DTYPE`` descriptor per sample drawn and sliced the same way; the
        fourth position then holds ``None`` for a list without a warp.  With ``photometric`` a sixth, one
        ``augmentation.PHOTO_OP_DTYPE`` descriptor per sample, likewise; unused earlier positions hold ``None``."""
        if self.aug_ops is None:
            raise TypeError("next_batch_aug needs device_aug=True, an augmentation mode and augmentations the device "
                            "implements (augmentation.aug_ops_from)")
        if self.images_u8.dtype != np.uint8:
            raise TypeError(f"next_batch_aug needs a uint8 image array, the dataset holds {self.images_u8.dtype}")
        B, N, A = self.batch_size, self.total_full_images, self.total_augs
        if self.aug_mode == "all":
            t = self.full_counter * A + self.aug_counter + np.arange(B)
            idx, j = self.sample_shuffle[(t // A) % N], t % A
            self.full_counter, self.aug_counter = int((t[-1] + 1) // A % N), int((t[-1] + 1) % A)
        else:  # "one": Generator.choice(size=B) consumes the stream like B single draws
            idx = self.sample_shuffle[(self.full_counter + np.arange(B)) % N]
            j = self._rng.choice(A, size=B, p=self.aug_probs)
            self.full_counter = (self.full_counter + B) % N
        self.batch_counter += 1
        if self.batch_counter == self.num_batches:
            self.batch_counter = 0
        ops = self.aug_ops[j]
        if self.aug_fly:
            ops["noise_id"] = self.samples_drawn + np.arange(B, dtype=np.uint64)
        else:
            ops["noise_id"] = idx.astype(np.uint64) * np.uint64(A) + j.astype(np.uint64)
        self.samples_drawn += B
        wops = None
        if self.warp_ops is not None:
            u = self._warp_rng.random((B, augmentation.WARP_DRAWS)) if self.aug_fly else self._warp_table[idx, j]
            wops = augmentation.draw_warp_ops(self.aug_fn_args, j, u)
        eops = None
        if self.elastic is not None:
            u = self._elastic_rng.random((B, augmentation.ELASTIC_DRAWS)) if self.aug_fly else self._elastic_table[idx, j]
            eops = augmentation.draw_elastic_ops(self.elastic, u)
        pops = None
        if self.photometric is not None:
            u = self._photo_rng.random((B, augmentation.PHOTO_DRAWS)) if self.aug_fly else self._photo_table[idx, j]
            pops = augmentation.draw_photo_ops(self.photometric, u, self.image_height, self.image_width)
        if shard is not None:
            idx, ops = idx[shard[0]:shard[1]], ops[shard[0]:shard[1]]
            wops = None if wops is None else wops[shard[0]:shard[1]]
            eops = None if eops is None else eops[shard[0]:shard[1]]
            pops = None if pops is None else pops[shard[0]:shard[1]]
        if pops is not None:
            return self.images_u8[idx], self.sparse_labels()[idx], ops, wops, eops, pops
        if eops is not None:
            return self.images_u8[idx], self.sparse_labels()[idx], ops, wops, eops
        if wops is not None:
            return self.images_u8[idx], self.sparse_labels()[idx], ops, wops
        return self.images_u8[idx], self.sparse_labels()[idx], ops

    def handle_epoch_end(self):
        self.batch_counter = 0
        self.full_counter = 0
        self.aug_counter = 0
        s = self._rng.permutation(self.total_raw_samples)
        self.sample_shuffle = self.sample_shuffle[s]


class DataGenerator:
    """``keras.utils.Sequence`` duck type: ``__len__``, ``__getitem__``, ``on_epoch_end``."""

    def __init__(self, images: np.ndarray, labels: np.ndarray, batch_size: int, aug_fn_args: List[Tuple],
                 aug_mode: str, aug_probs: Tuple, aug_fly: bool, preprocess_input_fn: Callable,
                 seed: Optional[int] = None, device_aug: bool = False, elastic: Optional[dict] = None,
                 photometric: Optional[dict] = None):
        # uint8 fast path (the /255 happens on the GPU) only without augmentation AND only for uint8 storage: the
        # reference divides by 255 whatever the dataset's dtype (data_generator.py:76), so any other dtype goes through
        # get_batch_list(), which computes float32(images) / 255 on the host
        self.oct_fast_path = aug_mode == "none" and np.asarray(images).dtype == np.uint8
        is_u8 = np.asarray(images).dtype == np.uint8
        self.batch_gen = BatchGenerator(images=images, labels=labels, batch_size=batch_size, aug_fn_args=aug_fn_args,
                                        aug_mode=aug_mode, aug_probs=aug_probs, aug_fly=aug_fly,
                                        preprocess_input_fn=preprocess_input_fn, seed=seed, device_aug=device_aug and is_u8,
                                        elastic=elastic, photometric=photometric)
        # augmentation on the device (Model.fit: uint8 upload + oct_augment_batch) where it was asked for and is possible
        self.oct_device_aug = self.batch_gen.aug_ops is not None
        if device_aug and aug_mode != "none" and not self.oct_device_aug:
            why = ("an augmentation is not one of augmentation_map's functions with arguments the device implements" if is_u8
                   else f"the dataset holds {np.asarray(images).dtype}, not uint8")
            log.warning(f"device_aug: augmenting on the host ({why})")
        # Philox key of the device noise: the generator's seed (shared by all DP ranks), or OS entropy drawn once
        self.oct_aug_seed = (int(seed) if seed is not None else int.from_bytes(os.urandom(8), "little")) & 0xFFFFFFFFFFFFFFFF

    def next_batch_aug(self, shard: Optional[Tuple[int, int]] = None):
        return self.batch_gen.next_batch_aug(shard)

    def __len__(self):
        return self.batch_gen.num_batches

    def __getitem__(self, index):
        X, y = self.batch_gen.get_batch_list()
        return X, y

    def next_batch_u8(self, shard: Optional[Tuple[int, int]] = None):
        return self.batch_gen.next_batch_u8(shard)

    @property
    def batch_size(self) -> int:
        return self.batch_gen.batch_size

    def on_epoch_end(self):
        self.batch_gen.handle_epoch_end()

    def get_total_samples(self) -> int:
        return self.batch_gen.total_samples
