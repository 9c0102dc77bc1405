"""``train_model``: the reference's training workflow
(oct_image_segmentation_models/training/training.py:135-408) on the HIP engine.

Same control flow and on-disk contract: read ``train_/val_`` images+labels, ``num_classes =
len(np.unique(train_labels))``, look the loss and metric up by name, build the model through the plugin
registry, checkpoint on the monitored validation metric, rolling ``stats_epochNN`` file, early stopping,
``model_config.json`` + ``training_params`` file.  MLflow calls are dropped (out of scope); ``initial_model``
works here (the reference's branch calls a non-existent ``utils.load_model``).
Under ``torchrun`` every rank runs this function; rank 0 writes the files."""
from __future__ import annotations

import json
import logging as log
import os
from pathlib import Path

import numpy as np

from .. import parallel
from ..common import augmentation, custom_losses, custom_metrics, data_generator as data_gen, dataset_loader, h5io, utils
from ..models import get_model_class
from ..models.engine_model import EarlyStopping, ModelCheckpoint
from . import training_callbacks
from .training_parameters import TrainingParams


SHAPE_KEYS = ("alpha", "beta", "tversky_gamma", "dice_class_weight")     # the loss factories' keywords that shape the Dice term


def save_training_params_file(save_foldername: Path, model_summary: str, model_config: dict,
                              training_dataset_md5: str, class_weight, timestamp, train_params: TrainingParams, opt):
    """``model_config.json`` + ``training_params.hdf5`` attributes (training.py:39-132)."""
    with open(save_foldername / Path("model_config.json"), "w") as config_file:
        json.dump(model_config, config_file)
    attrs = {
        "timestamp": np.array(timestamp, dtype="S100"),
        "model_summary": np.array(model_summary.encode("ascii", "replace")[:4000]),
        "train_dataset_md5": np.array(training_dataset_md5, dtype="S1000"),
        "epochs": train_params.epochs,
        "loss_name": np.array(train_params.loss, dtype="S1000"),
        "metric_name": np.array(train_params.metric, dtype="S1000"),
        "class_weight": np.array("None" if class_weight is None else "array", dtype="S1000"),
        "metric": np.array(train_params.metric, dtype="S100"),
        "loss": np.array(train_params.loss, dtype="S100"),
        "batch_size": train_params.batch_size,
        "shuffle": train_params.shuffle,
        "aug_mode": np.array(train_params.aug_mode, dtype="S100"),
        "aug_device": bool(train_params.aug_device),
        "optimizer": np.array(train_params.opt_con.__name__, dtype="S100"),
    }
    # the geometric augmentations, in the reference file's scheme for an augmentation list (training.py:79-112): "aug_<n>" =
    # the function's name, "aug_<n>_param: <key>" = each argument (n counts the whole list from 1)
    if train_params.aug_mode != "none":
        for n, (aug_fn, aug_arg) in enumerate(train_params.aug_fn_args, start=1):
            if aug_fn not in (augmentation.column_shift_aug, augmentation.affine_aug):
                continue
            attrs[f"aug_{n}"] = np.array(aug_fn.__name__, dtype="S100")
            for key, val in (aug_arg or {}).items():
                attrs[f"aug_{n}_param: {key}"] = (np.array(val, dtype="S100") if isinstance(val, str) else
                                                  val if np.isscalar(val) else np.asarray(val, dtype=np.float64))
    # the elastic stage: "elastic_param: <key>" = each key of the keyword, only when it was given
    for key, val in (getattr(train_params, "elastic", None) or {}).items():
        attrs[f"elastic_param: {key}"] = (np.array(val, dtype="S100") if isinstance(val, str) else
                                          val if np.isscalar(val) else np.asarray(val, dtype=np.float64))
    # the photometric stage likewise: "photometric_param: <key>"; a part that is itself a dict as its repr
    for key, val in (getattr(train_params, "photometric", None) or {}).items():
        attrs[f"photometric_param: {key}"] = (np.array(str(val), dtype="S200") if isinstance(val, (str, dict)) else
                                              val if np.isscalar(val) else np.asarray(val, dtype=np.float64))
    for key, val in opt.get_config().items():
        attrs["opt_param: " + key] = np.bytes_(str(val)) if isinstance(val, (dict, str)) else val
    # the shape of the Dice term: only the keys that were given (loss_fn_kwargs, or apply_class_weight's), so that a run
    # without them writes the file it always wrote
    for key, val in (getattr(train_params, "loss_shape_kwargs", None) or {}).items():
        attrs["loss_param: " + key] = np.array(val, dtype="S100") if isinstance(val, str) else \
            val if np.isscalar(val) else np.asarray(val, dtype=np.float64)
    # the border weights of the pixel term: "edge_weight_param: <key>" = each key of the validated spec, only when the
    # keyword was given
    for key, val in (getattr(train_params, "edge_weight_kwargs", None) or {}).items():
        if val is not None:
            attrs[f"edge_weight_param: {key}"] = np.array(val, dtype="S100") if isinstance(val, str) else val
    datasets = {} if class_weight is None else {"class_weight": np.asarray(class_weight)}
    h5io.save(save_foldername / Path("training_params.hdf5"), datasets, attrs)


def _balanced_class_weight(labels: np.ndarray, ignore_label=None) -> np.ndarray:
    """sklearn ``compute_class_weight("balanced")``: n_samples / (n_classes * bincount), over the pixels whose label is not
    ``ignore_label``."""
    if ignore_label is not None:
        labels = labels[labels != ignore_label]
    classes, counts = np.unique(labels, return_counts=True)
    return labels.size / (len(classes) * counts.astype(np.float64))


def loss_factory_kwargs(training_params: TrainingParams, c_weight) -> dict:
    """The keywords ``train_model`` gives the loss factory: ``loss_fn_kwargs``, and with ``apply_class_weight`` the computed
    class weights as ``dice_class_weight`` -- for ``focal_dice_loss`` also as the focal term's ``class_weight`` -- where
    ``loss_fn_kwargs`` does not name them."""
    kw = dict(training_params.loss_fn_kwargs)
    if getattr(training_params, "apply_class_weight", False) and c_weight is not None:
        kw.setdefault("dice_class_weight", [float(w) for w in c_weight])
        if training_params.loss == "focal_dice_loss":
            kw.setdefault("class_weight", [float(w) for w in c_weight])
    return kw


def _count_classes(train_labels: np.ndarray, ignore_label=None) -> int:
    """The reference's ``len(np.unique(train_labels))``, the ignore label not counted."""
    values = np.unique(train_labels)
    return int(len(values) - (ignore_label is not None and ignore_label in values))


def train_model(training_params: TrainingParams, mlflow_params=None):
    if mlflow_params is not None:
        log.warning("MLflow tracking is outside the accelerated path; mlflow_params is ignored")
    rank, _, _ = parallel.init()

    training_dataset_path = training_params.training_dataset_path
    data = dataset_loader.open_dataset(training_dataset_path)
    train_images, train_labels = dataset_loader.load_training_data(data)
    val_images, val_labels = dataset_loader.load_validation_data(data)
    # contrast normalisation: once, here, in front of everything that reads the images (the generators, fit_temperature)
    contrast = getattr(training_params, "contrast", None)
    if contrast is not None:
        for name, arr in (("training", train_images), ("validation", val_images)):
            if np.asarray(arr).dtype != np.uint8:
                raise ValueError(f"contrast needs a uint8 dataset: the {name} images are {np.asarray(arr).dtype}")
        train_images = utils.contrast_images(np.asarray(train_images), contrast)
        val_images = utils.contrast_images(np.asarray(val_images), contrast)

    ignore_label = training_params.ignore_label
    num_classes = _count_classes(train_labels, ignore_label)
    log.info(f"Detected {num_classes} classes")
    _, image_height, image_width, input_channels = train_images.shape
    log.info(f"Detected input image dimensions (h x w): {image_height} x {image_width}.")
    log.info(f"Detected {input_channels} input channels.")
    log.info(f"Number of devices: {parallel.world_size()}")

    optimizer = training_params.opt_con(**training_params.opt_params)

    loss = custom_losses.custom_loss_objects.get(training_params.loss)
    if loss is None:
        log.error(f"Loss '{training_params.loss}' not found. Exiting...")
        exit(1)
    if training_params.class_weight == "balanced":
        c_weight = _balanced_class_weight(np.concatenate((train_labels, val_labels)), ignore_label)
    elif type(training_params.class_weight) == list:
        c_weight = np.array(training_params.class_weight)
    else:
        c_weight = None
    # as in the reference, the weights are recorded but do not reach the loss (Appendix D.2) -- unless apply_class_weight asks
    loss_kwargs = loss_factory_kwargs(training_params, c_weight)
    training_params.loss_shape_kwargs = {k: loss_kwargs[k] for k in SHAPE_KEYS if k in loss_kwargs}
    sparse_labels = loss["takes_sparse"]
    try:
        loss_fn = loss["function"](num_classes=num_classes, is_y_true_sparse=sparse_labels, **loss_kwargs)
    except NotImplementedError as e:
        log.error(e)
        exit(1)

    training_params.edge_weight_kwargs = getattr(loss_fn, "oct_edge_weight", None)

    metric = custom_metrics.training_monitor_metric_objects.get(training_params.metric)
    if metric is None:
        log.error(f"Metric '{training_params.metric}' not found. Exiting...")
        exit(1)
    metric_fn = metric(sparse_labels, num_classes)

    # The reference one-hot encodes the label arrays here for dense losses (training.py:225-227); the engine
    # consumes sparse uint8 labels and one-hot encodes on the fly, so the arrays stay sparse (32x less memory).
    training_dataset_md5 = utils.md5(training_dataset_path) if Path(training_dataset_path).exists() else \
        utils.md5(Path(str(training_dataset_path) + ".npz"))

    model_architecture = training_params.model_architecture
    if training_params.initial_model:
        log.info(f"Starting training from model: {training_params.initial_model}")
        model, model_config = utils.load_model_and_config(Path(training_params.initial_model))
        model_architecture = model.name
        try:
            model_container = get_model_class(model_architecture)(**model_config)
        except ValueError as e:
            log.error(e)
            exit(1)
    else:
        log.info(f"Starting training from scratch {model_architecture} model")
        try:
            model_class = get_model_class(model_architecture)
        except ValueError as e:
            log.error(e)
            exit(1)
        model_container = model_class(input_channels=input_channels, num_classes=num_classes,
                                      image_height=image_height, image_width=image_width,
                                      **training_params.model_hyperparameters)
        model = model_container.build_model()
        if training_params.seed is not None:
            model.config["seed"] = int(training_params.seed)
    # scans whose size is no multiple of 2^pool_layers: with a pad_mode fit and its validation pad each batch on the device
    # and keep the frame out of the loss (pad_mode None: they raise, as ever)
    model.compile(optimizer=optimizer, loss=loss_fn, metrics=[metric_fn], ignore_label=ignore_label,
                  pad_mode=training_params.pad_mode, pad_value=training_params.pad_value)

    batch_size = training_params.batch_size
    aug_val_mode = training_params.aug_mode if training_params.aug_val else "none"

    monitor = training_params.model_save_monitor
    timestamp = parallel.broadcast_object(utils.get_timestamp())   # one results folder for all ranks
    save_foldername = training_params.results_location / Path(timestamp + "_" + model_architecture)
    if rank == 0:
        os.makedirs(save_foldername, exist_ok=True)
        if contrast is not None:      # beside the checkpoints: the model config cannot carry it (it is UNet(**model_config))
            with open(save_foldername / Path(utils.CONTRAST_FILE), "w") as f:
                json.dump(contrast, f, sort_keys=True)
    parallel.barrier()

    savemodel = ModelCheckpoint(filepath=save_foldername / Path("model_epoch{epoch:02d}.hdf5"),
                                save_best_only=training_params.model_save_best, monitor=monitor[0], mode=monitor[1])
    callbacks_list = [savemodel]
    if rank == 0:
        callbacks_list.append(training_callbacks.SaveEpochInfo(save_folder=save_foldername, train_params=training_params))
    if training_params.early_stopping:
        callbacks_list.append(EarlyStopping(monitor=f"val_{training_params.metric}", mode="max",
                                            patience=training_params.patience,
                                            restore_best_weights=training_params.restore_best_weights))

    model_summary = []
    model.summary(print_fn=lambda line: model_summary.append(line))
    if rank == 0:
        save_training_params_file(save_foldername, "\n".join(model_summary), model_container.get_config(),
                                  training_dataset_md5, c_weight, timestamp, training_params, optimizer)

    # every rank draws the SAME global batches (its slice of each is taken in BatchFeed.host_batch): an unseeded
    # run gets one OS-entropy seed from rank 0, not one per rank
    seed = parallel.shared_seed(training_params.seed) if parallel.world_size() > 1 else training_params.seed
    elastic = getattr(training_params, "elastic", None)      # the stage goes wherever the list's augmentations go
    photometric = getattr(training_params, "photometric", None)      # (likewise)
    train_gen = data_gen.DataGenerator(train_images, train_labels, batch_size, training_params.aug_fn_args, training_params.aug_mode,
                                       training_params.aug_probs, training_params.aug_fly,
                                       model_container.get_preprocess_input_fn(), seed=seed,
                                       device_aug=training_params.aug_device, elastic=elastic,
                                       photometric=photometric)
    val_gen = data_gen.DataGenerator(val_images, val_labels, batch_size,
                                     training_params.aug_fn_args if aug_val_mode != "none" else [], aug_val_mode,
                                     training_params.aug_probs if aug_val_mode != "none" else (),
                                     training_params.aug_fly if aug_val_mode != "none" else False,
                                     model_container.get_preprocess_input_fn(),
                                     seed=None if seed is None else seed + 1, device_aug=training_params.aug_device,
                                     elastic=elastic if aug_val_mode != "none" else None,
                                     photometric=photometric if aug_val_mode != "none" else None)

    for name, gen in (("training", train_gen), ("validation", val_gen)):
        if batch_size > gen.get_total_samples():
            log.error(f"The batch size ({batch_size}) cannot be larger than the number of {name} samples "
                      f"({gen.get_total_samples()})")
            exit(1)
    log.info(f"Train generator total number of samples: {train_gen.get_total_samples()}")
    log.info(f"Validation generator total number of samples: {val_gen.get_total_samples()}")

    history = model.fit(x=train_gen, validation_data=val_gen, epochs=training_params.epochs,
                        callbacks=callbacks_list, verbose=1)
    if getattr(training_params, "fit_temperature", False):
        # the temperature of the weights the model now holds, on the validation scans as they are (no augmentation)
        if rank == 0:
            from ..evaluation.calibration import TEMPERATURE_FILENAME, write_temperature
            # (raw uint8 scans go as they are, any other dtype through the model's own preprocessing; compile() above has set
            # the model's pad_mode / pad_value)
            x_val = val_images if val_images.dtype == np.uint8 else model_container.get_preprocess_input_fn()(val_images)
            record = model.fit_temperature(x_val, val_labels, batch_size, ignore_label=ignore_label)
            write_temperature(save_foldername / Path(TEMPERATURE_FILENAME), record)
        parallel.barrier()
    return SimpleTrainingResult(model, save_foldername, history, savemodel.saved)


class SimpleTrainingResult:
    """What the reference leaves on disk, also handed back to the caller (the reference returns None)."""

    def __init__(self, model, save_foldername, history, checkpoints):
        self.model, self.save_foldername, self.history, self.checkpoints = model, save_foldername, history.history, checkpoints


train = train_model  # north_star alias
