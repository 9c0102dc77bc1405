"""``TrainingParams`` with the reference's constructor contract
(oct_image_segmentation_models/training/training_parameters.py:11-135)."""
from __future__ import annotations

import logging as log
from pathlib import Path
from typing import List, Tuple, Union

from ..common import AUG_MODES
from ..common import augmentation as aug


class TrainingParams:
    def __init__(self, model_architecture: Union[str, None], training_dataset_path: Path,
                 initial_model: Union[Path, None], results_location: Path, opt_con, loss: str, metric: str,
                 epochs: int, batch_size: int, model_hyperparameters: dict = {}, opt_params: dict = {},
                 loss_fn_kwargs: dict = {}, augmentations: List[dict] = [], aug_mode: str = "none",
                 aug_probs: Tuple = (), aug_fly: bool = False, aug_val: bool = True, shuffle: bool = True,
                 model_save_best: bool = True, model_save_monitor=("val_acc", "max"),
                 class_weight: Union[list, str, None] = None, channels_last: bool = True,
                 early_stopping: bool = True, restore_best_weights: bool = True, patience: int = 50,
                 seed: Union[int, None] = None, aug_device: bool = False, pad_mode: Union[str, None] = None,
                 pad_value=0, ignore_label: Union[int, None] = None, apply_class_weight: bool = False,
                 fit_temperature: bool = False, elastic: Union[dict, None] = None, contrast: Union[dict, None] = None,
                 photometric: Union[dict, None] = None):
        # extension: photometric augmentation (common.augmentation.photometric_spec: p, gamma, brightness, contrast, blur,
        # shadows) of every sample the augmentation list applies to, directly behind the elastic stage; on the device with
        # aug_device, on the host without.  None: no such stage, nothing changes
        if photometric is not None:
            aug.photometric_spec(photometric)       # (ValueError for anything outside the definition)
            if aug_mode == "none":
                raise ValueError('photometric needs an augmentation mode: for otherwise un-augmented samples use aug_mode '
                                 '"one" with a single "no_augmentation" entry')
        self.photometric = None if photometric is None else dict(photometric)
        # extension: contrast normalisation (common.utils.check_contrast: {"method": "clahe" | "stretch", "tiles", "clip" |
        # "percentiles"}).  train_model normalises the training and validation images once, directly
        # after loading them (uint8 datasets only), so the run equals one on a dataset holding contrast_reference(images); the
        # spec is written as contrast.json into the run folder, where EvaluationParameters / PredictionParams(contrast="model")
        # find it.  None: nothing changes, no such file
        from ..common.utils import check_contrast
        self.contrast = check_contrast(contrast)
        # extension: elastic deformation (common.augmentation.elastic_spec: p, spacing, max_displacement[, border, fill,
        # fill_label]) of every sample the augmentation list applies to, in front of the list's own augmentation; on the device
        # with aug_device, on the host without.  None: no such stage, nothing changes
        if elastic is not None:
            aug.elastic_spec(elastic)       # (ValueError for anything outside the definition)
            if aug_mode == "none":
                raise ValueError('elastic needs an augmentation mode: to deform otherwise un-augmented samples use aug_mode '
                                 '"one" with a single "no_augmentation" entry')
        self.elastic = None if elastic is None else dict(elastic)
        # extension: after fit returns, rank 0 fits the temperature of the trained model on the un-augmented validation arrays
        # (Model.fit_temperature, with the ignore_label / pad_mode above) and writes temperature.json into the run folder
        # (evaluation.calibration.read_temperature reads it).  Off: no such file, nothing launched
        self.fit_temperature = bool(fit_temperature)
        if (model_architecture is None and initial_model is None) or (
                model_architecture is not None and initial_model is not None):
            log.error("Either 'model_architecture' or 'initial_model' need to be provided in the `config.json`.")
            exit(1)
        self.model_architecture = model_architecture
        self.model_hyperparameters = model_hyperparameters
        self.training_dataset_path = Path(training_dataset_path)
        self.initial_model = initial_model
        self.results_location = Path(results_location)
        self.opt_con = opt_con
        self.opt_params = opt_params
        self.loss = loss
        self.loss_fn_kwargs = loss_fn_kwargs
        self.metric = metric
        self.epochs = epochs
        self.batch_size = batch_size
        if aug_mode not in AUG_MODES:
            log.error(f"Augmentation mode: '{aug_mode}' is not supported.")
            exit(1)
        self.aug_mode = aug_mode
        self.aug_fn_args = []
        for augmentation in augmentations:
            aug_fn = aug.augmentation_map.get(augmentation["name"])
            if aug_fn is None:
                log.error(f"Augmentation: '{augmentation['name']}' is not supported.")
                exit(1)
            self.aug_fn_args.append((aug_fn, augmentation.get("arguments", {})))
        self.augmentations = augmentations
        self.aug_probs = aug_probs
        self.aug_fly = aug_fly
        self.aug_val = aug_val
        # extension: apply the augmentations on the GPU (oct_augment_batch; the noise then comes from its Philox stream,
        # not from numpy's).  Off by default.
        self.aug_device = bool(aug_device)
        self.shuffle = shuffle
        self.model_save_best = model_save_best
        self.model_save_monitor = model_save_monitor
        self.class_weight = class_weight
        self.channels_last = channels_last
        self.early_stopping = early_stopping
        self.restore_best_weights = restore_best_weights
        self.patience = patience
        # extensions: scans whose size is no multiple of 2^pool_layers are padded on the device ("edge", "reflect" or "constant"
        # with pad_value, in raw counts; None refuses them), and pixels labelled ignore_label (a value that is no class) stay
        # out of the class count, the balanced class weights, the loss and its gradient
        self.pad_mode = pad_mode
        self.pad_value = pad_value
        self.ignore_label = ignore_label
        # extension: hand the computed class weights ("balanced" or a list) to the loss factory as dice_class_weight -- and, for
        # focal_dice_loss, as the focal term's class_weight -- unless loss_fn_kwargs names them.  Off: they are only recorded
        self.apply_class_weight = bool(apply_class_weight)
        self.seed = seed  # extension: reproducible shuffling / init (the reference is unseeded)
        if self.model_save_monitor[0] == "val_acc":
            self.model_save_monitor = ["val_" + self.metric, model_save_monitor[1]]
