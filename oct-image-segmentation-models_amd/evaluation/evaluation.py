"""``evaluate_model``: the reference's evaluation workflow
(oct_image_segmentation_models/evaluation/evaluation.py:73-448, savers :451-700, aggregation :722-941).

The forward pass is batched on the GPU (device arg-max, 1 B/px back to the host) instead of one
``predict`` call per image; everything after it -- one-hot, boundary maps, Dice
metrics, optional graph search, per-image result files, dataset aggregates -- is the reference's host logic
re-stated.  The surface-distance metrics (average surface distance, Hausdorff-95; :207-262) are computed on the
device from the arg-max maps and the uploaded ground truth (``evaluation/surface.py``).  With
``EvaluationParameters(metrics_device=True)`` the Dice metrics come from confusion counts made on the device and the
graph-search class maps from ``oct_area_labels`` (``evaluation/dice_device.py``): the same files, byte for byte.  Under ``torchrun`` the test
set is sharded by contiguous index range (no collective); rank 0 aggregates.  With ``EvaluationParameters(png_plots=True)``
the reference's PNG pictures of every image are rasterised on the device (``oct_render_rgba``, ``evaluation/render.py``) and
written by ``common/png.py``; each rank writes those of its own shard.  ``performance_plot.png`` and
``categorical_pred_N.png`` are out of scope.  With ``EvaluationParameters(ignore_label=...)`` ground-truth pixels of that value
are unknown: out of every Dice count, no surface element at their rim, no truth boundary under them, mid-grey in the
ground-truth pictures; without it the value is refused and every file is what it was."""
from __future__ import annotations

import json
import logging as log
import os
import time
import warnings
from pathlib import Path
from typing import List

import numpy as np

from .. import parallel
from ..common import (EVALUATION_METRIC_AVERAGE_SURFACE_DISTANCE, EVALUATION_METRIC_DICE_CLASSES,
                      EVALUATION_METRIC_DICE_MACRO, EVALUATION_METRIC_DICE_MICRO,
                      EVALUATION_METRIC_HAUSDORFF_DISTANCE, custom_metrics, dataset_loader as dl, h5io)
from ..common import utils as common_utils
from ..min_path_processing import graph_search, utils
from ..models import get_model_class
from .calibration import CALIBRATION_METRICS, calibration_from_counts, counts_as_float, pooled_calibration
from .dice_device import DICE_METRICS, MAX_EXACT_PIXELS, dice_from_counts
from .evaluation_parameters import EvaluationParameters
from .ordered import layer_thickness
from .pipeline import InferenceRun
from .render import CC_PNG_NAMES, EVALUATION_PNG_NAMES, OD_PNG_NAMES, write_pictures
from .surface import datasets as surface_datasets

EVALUATION_RESULTS_FILENAME = "evaluation_results.hdf5"
GS_EVALUATION_RESULTS_FILENAME = "gs_evaluation_results.hdf5"
OD_EVALUATION_RESULTS_FILENAME = "od_evaluation_results.hdf5"
CC_EVALUATION_RESULTS_FILENAME = "cc_evaluation_results.hdf5"
OVERALL_EVALUATION_RESULTS_FILENAME_HDF5 = "overall_evaluation_results.hdf5"
OVERALL_EVALUATION_RESULTS_FILENAME_CSV = "overall_evaluation_results.csv"


class EvaluationOutput:
    def __init__(self, image, image_name, image_segments, image_output_dir, predicted_labels, categorical_pred,
                 boundary_maps, gs_pred_segs, errors, mean_abs_err, mean_err, abs_err_sd, err_sd,
                 dice_classes=None, dice_macro=None, dice_micro=None, average_surface_distances=None,
                 average_surface_distances_gt_to_pred=None, average_surface_distances_pred_to_gt=None,
                 hausdorff_distances=None) -> None:
        self.image = image
        self.image_name = image_name
        self.image_segments = image_segments
        self.image_output_dir = image_output_dir
        self.predicted_labels = predicted_labels
        self.categorical_pred = categorical_pred
        self.boundary_maps = boundary_maps
        self.gs_pred_segs = gs_pred_segs
        self.errors = errors
        self.mean_abs_err = mean_abs_err
        self.mean_err = mean_err
        self.abs_err_sd = abs_err_sd
        self.err_sd = err_sd
        self.dice_classes, self.dice_macro, self.dice_micro = dice_classes, dice_macro, dice_micro
        self.average_surface_distances = average_surface_distances
        self.average_surface_distances_gt_to_pred = average_surface_distances_gt_to_pred
        self.average_surface_distances_pred_to_gt = average_surface_distances_pred_to_gt
        self.hausdorff_distances = hausdorff_distances


def _dice_metrics(metrics, num_classes, label_onehot_hw, categorical_pred, transposed=False):
    """Dice classes / macro / micro exactly as evaluation.py:175-208 (and :335-375 for the graph-search maps,
    where both operands live in the transposed (W,H) frame)."""
    axes = (2, 1, 0) if transposed else (2, 0, 1)
    label_class_first = np.expand_dims(np.transpose(label_onehot_hw, axes=axes), axis=0)
    dc = dm = dmi = None
    if EVALUATION_METRIC_DICE_CLASSES in metrics:
        dc = custom_metrics.soft_dice_class(label_class_first, categorical_pred)
    if EVALUATION_METRIC_DICE_MACRO in metrics:
        f = custom_metrics.dice_coef_macro(is_y_true_sparse=False, num_classes=num_classes)
        lab = np.expand_dims(np.transpose(label_onehot_hw, axes=[1, 0, 2]) if transposed else label_onehot_hw, axis=0)
        dm = np.array(f(lab, np.transpose(categorical_pred, axes=[0, 2, 3, 1])))
    if EVALUATION_METRIC_DICE_MICRO in metrics:
        f = custom_metrics.dice_coef_micro(is_y_true_sparse=False, num_classes=num_classes)
        dmi = np.array(f(label_class_first, categorical_pred))
    return dc, dm, dmi


def _batch_dice(metrics, num_classes, batch, k, label_onehot_hw, categorical_pred):
    """Dice classes / macro / micro of image ``k`` of a batch: from the device's confusion counts where the batch carries
    them (``Batch.confusion``), else from the one-hot arrays on the host.  The same values, dtypes and shapes either way."""
    if batch.confusion is not None:
        return dice_from_counts(batch.confusion[k], metrics)
    return _dice_metrics(metrics, num_classes, label_onehot_hw, categorical_pred)


def _masked_onehot(labels_hw, num_classes, ignore_label):
    """(H,W) ground-truth labels with ``ignore_label`` -> the one-hot truth (H,W,C) float32 with an all-zero vector at the
    ignored pixels, and ``keep`` (H,W) bool, the counted pixels (``masked_loss_reference`` forms the same pair)."""
    keep = labels_hw != ignore_label
    onehot = common_utils.to_categorical(np.where(keep, labels_hw, 0), num_classes)
    onehot[~keep] = 0.0
    return onehot, keep


def _surface_metrics(metrics, rows):
    """Per-image surface-distance datasets (evaluation.py:207-262) from one (C-1, 6) row block of the device, restricted
    to the metrics asked for."""
    if rows is None:
        return {}
    d = surface_datasets(rows)
    keep = []
    if EVALUATION_METRIC_AVERAGE_SURFACE_DISTANCE in metrics:
        keep += ["average_surface_distances", "average_surface_distances_gt_to_pred", "average_surface_distances_pred_to_gt"]
    if EVALUATION_METRIC_HAUSDORFF_DISTANCE in metrics:
        keep.append("hausdorff_distances")
    return {k: d[k] for k in keep}


def evaluate_model(eval_params: EvaluationParameters) -> List[EvaluationOutput]:
    """With ``eval_params.metrics_device`` the ``graph_time`` attribute of gs_evaluation_results.hdf5 is the time of the
    batch's device stage (class maps of the delineations and their confusion counts) divided by the batch's image count,
    not a per-image host time; it stays an attribute, and every dataset and CSV file equals the host path's."""
    rank, _, _ = parallel.init()
    world = parallel.world_size()

    data = dl.open_dataset(eval_params.test_dataset_path)
    eval_images, eval_labels, eval_image_names = dl.load_testing_data(data)
    n_images = eval_images.shape[0]
    if not eval_image_names:
        eval_image_names = [Path(f"image_{i}") for i in range(n_images)]
    eval_image_output_dirs = [eval_params.save_foldername / Path(f"image_{i}") for i in range(n_images)]

    num_classes = eval_params.num_classes
    # ignore_label: ground-truth pixels of that value are unknown; None is the reference's workflow
    ignore_label = getattr(eval_params, "ignore_label", None)
    if ignore_label is None:
        eval_segments = np.swapaxes(utils.generate_boundary(np.squeeze(eval_labels, axis=3), axis=1), 0, 1)
    else:
        label_maps = np.squeeze(eval_labels, axis=3)
        bad = np.nonzero(((label_maps < 0) | (label_maps >= num_classes)) & (label_maps != ignore_label))[0]
        if bad.size:
            raise ValueError(f"image {int(bad[0])}: ground-truth labels outside 0..{num_classes - 1} that are not the ignore "
                             f"label {ignore_label}")
        eval_segments = np.swapaxes(utils.generate_boundary_masked(label_maps, num_classes, ignore_label, axis=1), 0, 1)
    if rank == 0:
        os.makedirs(eval_params.save_foldername, exist_ok=True)
        save_eval_config_file(eval_params)
    parallel.barrier()

    try:
        model_class = get_model_class(eval_params.loaded_model.name)
    except ValueError as e:
        log.error(e)
        exit(1)
    model_class(**eval_params.model_config)  # validates the stored config exactly as the reference does

    lo, hi = parallel.shard_range(n_images, rank, world)
    eval_outputs: List[EvaluationOutput] = []
    # surface distances (evaluation.py:207-262) run on the device next to the forward: arg-max maps against the uploaded
    # ground-truth class maps, spacing (0.01111111, 0.01111111), percent 95
    want_surface = any(m in eval_params.metrics for m in (EVALUATION_METRIC_AVERAGE_SURFACE_DISTANCE,
                                                           EVALUATION_METRIC_HAUSDORFF_DISTANCE))
    want_dice = any(m in eval_params.metrics for m in DICE_METRICS)
    # metrics_device: Dice from device confusion counts, graph-search class maps from the device.  The host's float32 sums
    # are exact (hence order-free, hence reproduced bit for bit) only up to MAX_EXACT_PIXELS: larger images keep the host path
    metrics_device = bool(getattr(eval_params, "metrics_device", False))
    if metrics_device and eval_images.shape[1] * eval_images.shape[2] > MAX_EXACT_PIXELS:
        log.info(f"metrics_device: images above {MAX_EXACT_PIXELS} pixels keep the host metrics")
        metrics_device = False
    # calibration_bins / temperature: reliability counts of the (tempered) probabilities on the device
    calibration_bins, temperature = getattr(eval_params, "calibration_bins", 0), getattr(eval_params, "temperature", 1.0)
    # ordered_decode: the topology-correct class maps of the probabilities, decoded on the device
    ordered_decode = bool(getattr(eval_params, "ordered_decode", False))
    # components: island removal and component counts of the arg-max maps on the device
    components = getattr(eval_params, "components", None)
    need_gt = want_surface or (metrics_device and want_dice) or calibration_bins > 0
    gt_maps = np.squeeze(eval_labels[lo:hi], axis=3) if need_gt else None
    # BASELINE configs[4] path (evaluation/pipeline.py::InferenceRun): search mode, batch source and worker pools
    # png_plots: the pictures of evaluation.py:488-548 and :673-695 of the reference, under its save_params conditions
    png_plots = bool(getattr(eval_params, "png_plots", False)) and eval_params.save_params.png_images is True
    with InferenceRun(eval_params.loaded_model, eval_images[lo:hi], eval_params.batch_size, num_classes,
                      gt=gt_maps, surface=want_surface, confusion=metrics_device and want_dice,
                      graph_search=eval_params.graph_search, gsgrad=eval_params.gsgrad, gs_device=eval_params.gs_device,
                      gs_device_ties=eval_params.gs_device_ties, gs_workers=eval_params.gs_workers,
                      soft_maps=not getattr(eval_params, "binarize", True),
                      pad_mode=getattr(eval_params, "pad_mode", None), pad_value=getattr(eval_params, "pad_value", 0),
                      ignore_label=ignore_label, tta=getattr(eval_params, "tta", None),
                      calibration_bins=calibration_bins, temperature=temperature,
                      **({"ordered_decode": True} if ordered_decode else {}),
                      **({"components": components} if components is not None else {}),
                      **({"contrast": eval_params.contrast} if getattr(eval_params, "contrast", None) is not None else {})) as run:
        t_prev = time.time()
        for batch in run:
            b0, b1 = lo + batch.lo, lo + batch.hi
            predict_time = (time.time() - t_prev) / (b1 - b0)
            cc_counts = cc_surface = cc_pictures = None
            if components is not None:
                if metrics_device and want_dice:
                    cc_counts = run.label_counts(batch.components[0], gt_maps[batch.lo:batch.hi], batch.lo)
                if want_surface:
                    cc_surface = run.label_surface(batch.components[0], gt_maps[batch.lo:batch.hi])
                if png_plots:
                    cc_pictures = {"cc_map": run.render_labels(batch.components[0])}
            od_counts = od_pictures = None
            if ordered_decode:
                if metrics_device and want_dice:
                    od_counts = run.ordered_counts(batch, gt_maps[batch.lo:batch.hi])
                if png_plots:
                    od_pictures = run.render_ordered(batch, eval_images[b0:b1])
            gs_found = run.graph_search(batch, eval_segments[b0:b1])
            gs_labels = gs_counts = None
            if metrics_device and eval_params.graph_search:
                start_stage_time = time.time()
                gs_labels, gs_counts = run.gs_labels(batch, gs_found, gt_maps[batch.lo:batch.hi] if want_dice else None)
                gs_stage_time = (time.time() - start_stage_time) / (b1 - b0)
            pictures = None
            if png_plots:
                pictures = run.render_pngs(batch, eval_images[b0:b1], gs_found, gt=np.squeeze(eval_labels[b0:b1], axis=3),
                                           truths=eval_segments[b0:b1], gs_labels=gs_labels,
                                           pred_map=eval_params.save_params.predicted_labels is True,
                                           ignore_label=ignore_label)
            for ind in range(b0, b1):
                eval_image, eval_image_name = eval_images[ind], eval_image_names[ind]
                eval_seg, eval_image_output_dir = eval_segments[ind], eval_image_output_dirs[ind]
                keep = raw_label = None
                if ignore_label is None:
                    eval_label = common_utils.to_categorical(eval_labels[ind], num_classes)        # (H,W,C)
                else:                                                     # zero one-hot vectors at the ignored pixels
                    raw_label = np.squeeze(eval_labels[ind], axis=2)
                    eval_label, keep = _masked_onehot(raw_label, num_classes, ignore_label)
                os.makedirs(eval_image_output_dir, exist_ok=True)
                predicted_labels = batch.labels[ind - b0:ind - b0 + 1].astype(np.int64)        # (1,H,W)
                categorical_pred = common_utils.labels_to_categorical(predicted_labels, num_classes)
                # on device: == convert_predictions_to_maps_semantic(categorical_pred); with binarize=False, of the probabilities
                boundary_maps = batch.maps[ind - b0:ind - b0 + 1]
                dice_classes, dice_macro, dice_micro = _batch_dice(eval_params.metrics, num_classes, batch, ind - b0,
                                                                   eval_label, categorical_pred if keep is None
                                                                   else categorical_pred * keep.astype(np.float32))
                surface_ds = _surface_metrics(eval_params.metrics, None if batch.surface is None else batch.surface[ind - b0])

                predicted_labels = np.squeeze(predicted_labels, axis=0)
                categorical_pred = np.squeeze(categorical_pred, axis=0)
                boundary_maps = np.squeeze(boundary_maps, axis=0)
                _save_image_evaluation_results(eval_params, eval_image, eval_image_name, predicted_labels, categorical_pred,
                                               eval_label, eval_seg, dice_classes, dice_macro, dice_micro, predict_time,
                                               eval_image_output_dir, surface_ds, raw_label,
                                               None if batch.calibration is None else tuple(t[ind - b0] for t in batch.calibration))

                gs_pred_segs = errors = mean_abs_err = mean_err = abs_err_sd = err_sd = None
                if eval_params.graph_search:
                    eval_image_t = np.transpose(eval_image, axes=[1, 0, 2])
                    start_graph_time = time.time()
                    gs_pred_segs, errors = gs_found[ind - b0]      # == graph_search.segment_maps(boundary_maps_t, eval_seg, grid)
                    if gs_labels is not None:
                        gs_eval_label = gs_labels[ind - b0]
                        gs_dc, gs_dm, gs_dmi = (dice_from_counts(gs_counts[ind - b0], eval_params.metrics) if want_dice
                                                else (None, None, None))
                        graph_time = gs_stage_time
                    else:
                        gs_eval_label, reconstructed_maps = common_utils.labels_from_delineations(eval_image_t.shape,
                                                                                                 gs_pred_segs, num_classes)
                        if keep is not None:                              # (1, C, W, H): the search's transposed frame
                            reconstructed_maps = reconstructed_maps * np.transpose(keep).astype(np.float32)
                        gs_dc, gs_dm, gs_dmi = _dice_metrics(eval_params.metrics, num_classes, eval_label,
                                                             reconstructed_maps, transposed=True)
                        graph_time = time.time() - start_graph_time
                    mean_abs_err, mean_err, abs_err_sd, err_sd = graph_search.calculate_overall_errors(errors)
                    _save_graph_based_evaluation_results(eval_params, eval_image_name, gs_eval_label, gs_pred_segs, gs_dc,
                                                         gs_dm, gs_dmi, errors, mean_abs_err, mean_err, abs_err_sd, err_sd,
                                                         graph_time, eval_image_output_dir)
                if ordered_decode:
                    od_labels, od_rows = batch.ordered[0][ind - b0], batch.ordered[1][ind - b0]
                    if od_counts is not None:
                        od_dice = dice_from_counts(od_counts[ind - b0], eval_params.metrics)
                    else:
                        od_cat = common_utils.labels_to_categorical(od_labels[None].astype(np.int64), num_classes)
                        od_dice = _dice_metrics(eval_params.metrics, num_classes, eval_label,
                                                od_cat if keep is None else od_cat * keep.astype(np.float32))
                    _save_ordered_evaluation_results(eval_params, eval_image_name, od_labels, od_rows, od_dice,
                                                     graph_search.calc_errors(od_rows, eval_seg),
                                                     int(np.count_nonzero(od_labels != predicted_labels)), eval_image_output_dir)
                    if od_pictures is not None:
                        write_pictures(eval_image_output_dir, od_pictures, ind - b0, OD_PNG_NAMES)
                if components is not None:
                    cc_labels = batch.components[0][ind - b0]
                    if cc_counts is not None:
                        cc_dice = dice_from_counts(cc_counts[ind - b0], eval_params.metrics)
                    else:
                        cc_cat = common_utils.labels_to_categorical(cc_labels[None].astype(np.int64), num_classes)
                        cc_dice = _dice_metrics(eval_params.metrics, num_classes, eval_label,
                                                cc_cat if keep is None else cc_cat * keep.astype(np.float32))
                    _save_components_evaluation_results(
                        eval_params, eval_image_name, cc_labels, batch.components[1][ind - b0], batch.components[2][ind - b0],
                        cc_dice, _surface_metrics(eval_params.metrics, None if cc_surface is None else cc_surface[ind - b0]),
                        int(np.count_nonzero(cc_labels != predicted_labels)), eval_image_output_dir)
                    if cc_pictures is not None:
                        write_pictures(eval_image_output_dir, cc_pictures, ind - b0, CC_PNG_NAMES)
                if pictures is not None:
                    write_pictures(eval_image_output_dir, pictures, ind - b0, EVALUATION_PNG_NAMES)
                eval_outputs.append(EvaluationOutput(
                    image=eval_image, image_name=eval_image_name, image_segments=eval_seg,
                    image_output_dir=eval_image_output_dir, predicted_labels=predicted_labels,
                    categorical_pred=categorical_pred, boundary_maps=boundary_maps, gs_pred_segs=gs_pred_segs, errors=errors,
                    mean_abs_err=mean_abs_err, mean_err=mean_err, abs_err_sd=abs_err_sd, err_sd=err_sd,
                    dice_classes=dice_classes, dice_macro=dice_macro, dice_micro=dice_micro, **surface_ds))
            t_prev = time.time()
    parallel.barrier()
    if rank == 0:
        _calc_overall_dataset_errors(eval_params, eval_image_names)
    return eval_outputs


def _save_image_evaluation_results(eval_params, eval_image, image_name, predicted_labels, categorical_pred, eval_labels,
                                   eval_segs, dice_classes, dice_macro, dice_micro, predict_time, output_dir,
                                   surface_ds=None, raw_labels=None, calibration=None):
    """``raw_labels`` (H,W): the ground truth as given, where ``eval_labels`` is a one-hot array with ignored pixels zeroed
    (``ignore_label``): the files store it, ignore value included.  ``calibration``: the image's ``(counts (M, 3) uint64,
    sums (4,))`` of ``Batch.calibration``; the file gains ``calibration_counts`` and the four metrics made of them."""
    with open(output_dir / "input_image_name.txt", "w") as f:
        f.write(str(image_name))
    np.savetxt(output_dir / Path("predicted_segmentation_map.csv"), predicted_labels, fmt="%d", delimiter=",")
    ds = {}
    if eval_params.save_params.categorical_pred is True:
        ds["categorical_pred"] = categorical_pred.astype("uint8")
    if eval_params.save_params.predicted_labels is True:
        ds["predicted_segmentation_map"] = predicted_labels.astype("uint8")
    ds["raw_image"] = eval_image.astype("uint8")
    eval_labels = np.argmax(eval_labels, axis=2) if raw_labels is None else raw_labels
    ds["eval_labels"] = eval_labels.astype("uint8")
    np.savetxt(output_dir / Path("ground_truth_segmentation_map.csv"), eval_labels, fmt="%d", delimiter=",")
    ds["raw_segs"] = eval_segs.astype("uint16")
    if dice_classes is not None:
        ds[EVALUATION_METRIC_DICE_CLASSES] = np.squeeze(dice_classes).astype("float64")
    if dice_macro is not None:
        ds[EVALUATION_METRIC_DICE_MACRO] = np.expand_dims(dice_macro, axis=0).astype("float64")
    if dice_micro is not None:
        ds[EVALUATION_METRIC_DICE_MICRO] = np.expand_dims(dice_micro, axis=0).astype("float64")
    for k, v in (surface_ds or {}).items():          # evaluation.py:573-597
        ds[k] = np.asarray(v, dtype="float64")
    if calibration is not None:
        ds["calibration_counts"] = counts_as_float(calibration[0])
        for k, v in calibration_from_counts(*calibration).items():
            ds[k] = np.array([v], dtype="float64")
    attrs = common_utils.result_attrs(eval_params.model_path, image_name, predict_time=np.array(predict_time))
    if getattr(eval_params, "tta", None):
        attrs["tta_views"] = np.array(",".join(eval_params.tta), dtype="S1000")      # only when set: other files stay as they were
    if getattr(eval_params, "contrast", None) is not None:
        attrs["contrast"] = np.array(json.dumps(eval_params.contrast, sort_keys=True), dtype="S1000")      # likewise
    h5io.save(output_dir / Path(EVALUATION_RESULTS_FILENAME), ds, attrs)


def _save_graph_based_evaluation_results(eval_params, image_name, gs_eval_label, gs_pred_segs, gs_dice_classes,
                                         gs_dice_macro, gs_dice_micro, errors, mean_abs_err, mean_err, abs_err_sd,
                                         err_sd, graph_time, output_dir):
    np.savetxt(output_dir / Path("gs_boundaries.csv"), gs_pred_segs, delimiter=",", fmt="%d")
    np.savetxt(output_dir / Path("gs_predicted_segmentation_map.csv"), gs_eval_label, fmt="%d", delimiter=",")
    ds = {"gs_pred_segs": gs_pred_segs.astype("uint16"), "errors": errors.astype("float64"),
          "mean_abs_err": mean_abs_err.astype("float64"), "mean_err": mean_err.astype("float64"),
          "abs_err_sd": abs_err_sd.astype("float64"), "err_sd": err_sd.astype("float64"),
          "gs_predicted_labels": gs_eval_label.astype("uint8")}
    if gs_dice_classes is not None:
        ds[EVALUATION_METRIC_DICE_CLASSES] = np.squeeze(gs_dice_classes).astype("float64")
    if gs_dice_macro is not None:
        ds[EVALUATION_METRIC_DICE_MACRO] = np.expand_dims(gs_dice_macro, axis=0).astype("float64")
    if gs_dice_micro is not None:
        ds[EVALUATION_METRIC_DICE_MICRO] = np.expand_dims(gs_dice_micro, axis=0).astype("float64")
    attrs = common_utils.result_attrs(eval_params.model_path, image_name, graph_time=np.array(graph_time))
    h5io.save(output_dir / Path(GS_EVALUATION_RESULTS_FILENAME), ds, attrs)


def _save_ordered_evaluation_results(eval_params, image_name, od_labels, od_rows, dice, errors, changed_pixels, output_dir):
    """The ordered decode's files of one image: ``od_labels`` (H,W) uint8 and ``od_rows`` (C-1,W) uint16 of
    ``Batch.ordered``, ``dice`` = (classes, macro, micro) as for the arg-max map, ``errors`` = ``calc_errors(od_rows, truth)``,
    ``changed_pixels`` the pixels where the ordered map differs from the arg-max."""
    np.savetxt(output_dir / Path("od_boundaries.csv"), od_rows, delimiter=",", fmt="%d")
    np.savetxt(output_dir / Path("od_predicted_segmentation_map.csv"), od_labels, fmt="%d", delimiter=",")
    mean_abs_err, mean_err, abs_err_sd, err_sd = graph_search.calculate_overall_errors(errors)
    ds = {"od_pred_segs": od_rows.astype("uint16"), "od_predicted_labels": od_labels.astype("uint8"),
          "errors": errors.astype("float64"), "mean_abs_err": mean_abs_err.astype("float64"),
          "mean_err": mean_err.astype("float64"), "abs_err_sd": abs_err_sd.astype("float64"), "err_sd": err_sd.astype("float64"),
          "changed_pixels": np.array([changed_pixels], dtype="int64")}
    dice_classes, dice_macro, dice_micro = dice
    if dice_classes is not None:
        ds[EVALUATION_METRIC_DICE_CLASSES] = np.squeeze(dice_classes).astype("float64")
    if dice_macro is not None:
        ds[EVALUATION_METRIC_DICE_MACRO] = np.expand_dims(dice_macro, axis=0).astype("float64")
    if dice_micro is not None:
        ds[EVALUATION_METRIC_DICE_MICRO] = np.expand_dims(dice_micro, axis=0).astype("float64")
    thickness, mean_thickness = layer_thickness(od_rows)
    if thickness is not None:
        ds["layer_thickness"], ds["mean_layer_thickness"] = thickness, mean_thickness
    h5io.save(output_dir / Path(OD_EVALUATION_RESULTS_FILENAME), ds, common_utils.result_attrs(eval_params.model_path, image_name))


def _save_components_evaluation_results(eval_params, image_name, cc_labels, stats, removed, dice, surface_ds, changed_pixels,
                                        output_dir):
    """The component stage's file of one image: ``cc_labels`` (H,W) uint8, ``stats`` (C,2) and ``removed``
    (C,) uint32 of ``Batch.components``, ``dice`` = (classes, macro, micro) and ``surface_ds`` of the cleaned map, formed as for
    the arg-max map, ``changed_pixels`` the pixels where the cleaned map differs from the arg-max."""
    ds = {"cc_predicted_labels": cc_labels.astype("uint8"), "component_count": stats[:, 0].astype("uint32"),
          "largest_component_pixels": stats[:, 1].astype("uint32"), "removed_pixels": removed.astype("uint32"),
          "changed_pixels": np.array([changed_pixels], dtype="int64")}
    dice_classes, dice_macro, dice_micro = dice
    if dice_classes is not None:
        ds[EVALUATION_METRIC_DICE_CLASSES] = np.squeeze(dice_classes).astype("float64")
    if dice_macro is not None:
        ds[EVALUATION_METRIC_DICE_MACRO] = np.expand_dims(dice_macro, axis=0).astype("float64")
    if dice_micro is not None:
        ds[EVALUATION_METRIC_DICE_MICRO] = np.expand_dims(dice_micro, axis=0).astype("float64")
    for k, v in (surface_ds or {}).items():
        ds[k] = np.asarray(v, dtype="float64")
    h5io.save(output_dir / Path(CC_EVALUATION_RESULTS_FILENAME), ds, common_utils.result_attrs(eval_params.model_path, image_name))


def save_eval_config_file(eval_params: EvaluationParameters):
    p = eval_params.test_dataset_path
    md5_path = p if Path(p).exists() else Path(str(p) + ".npz")
    attrs = {"model_filename": np.array(str(eval_params.model_path), dtype="S1000"),
             "mlflow_tracking_uri": np.array(str(eval_params.mlflow_tracking_uri), dtype="S1000"),
             "test_dataset_path": np.array(str(eval_params.test_dataset_path), dtype="S1000"),
             "test_dataset_md5": np.array(common_utils.md5(md5_path), dtype="S1000"),
             "gsgrad": np.array(eval_params.gsgrad)}
    if not getattr(eval_params, "binarize", True):
        attrs["binarize"] = np.array(False)      # recorded only when it departs from the default: binarize=True files stay as they were
    if getattr(eval_params, "png_plots", False):
        attrs["png_plots"] = np.array(True)      # likewise
    if getattr(eval_params, "pad_mode", None) is not None:
        attrs["pad_mode"] = np.array(str(eval_params.pad_mode), dtype="S1000")      # likewise, with the constant
        attrs["pad_value"] = np.array(float(getattr(eval_params, "pad_value", 0)))
    if getattr(eval_params, "ignore_label", None) is not None:
        attrs["ignore_label"] = np.array(int(eval_params.ignore_label))      # likewise
    if getattr(eval_params, "tta", None):
        attrs["tta_views"] = np.array(",".join(eval_params.tta), dtype="S1000")      # likewise
    if getattr(eval_params, "contrast", None) is not None:
        attrs["contrast"] = np.array(json.dumps(eval_params.contrast, sort_keys=True), dtype="S1000")      # likewise
    if getattr(eval_params, "calibration_bins", 0):
        attrs["calibration_bins"] = np.array(int(eval_params.calibration_bins))      # likewise
    if getattr(eval_params, "temperature", 1.0) != 1.0:
        attrs["temperature"] = np.array(float(eval_params.temperature))      # likewise
    if getattr(eval_params, "ordered_decode", False):
        attrs["ordered_decode"] = np.array(True)      # likewise
    if getattr(eval_params, "components", None) is not None:
        attrs["components"] = np.array(repr(eval_params.components), dtype="S1000")      # likewise
    h5io.save(eval_params.save_foldername / Path("eval_params.hdf5"), {}, attrs)


def _calc_overall_dataset_errors(eval_params: EvaluationParameters, eval_image_names: List[Path]):
    """Mean / sd over images of every per-image metric, re-read from the per-image result files
    (evaluation.py:722-941): ``inf -> nan``, ``nanmean`` / ``nanstd`` over axis 0; boundary-error statistics."""
    output_dir, metrics = eval_params.save_foldername, eval_params.metrics
    dir_list = [Path(output_dir) / Path(f"image_{i}") for i in range(len(eval_image_names))]

    def stack(files, name):
        return np.concatenate([np.expand_dims(f[name], axis=0) for f in files], axis=0)

    files = [h5io.load(d / Path(EVALUATION_RESULTS_FILENAME)) for d in dir_list]
    gs_files = [h5io.load(d / Path(GS_EVALUATION_RESULTS_FILENAME)) for d in dir_list] if eval_params.graph_search else []
    out = {"image_names": np.array([str(n) for n in eval_image_names], dtype="S1000")}
    lines = []

    def save_metric(metric_name: str, metric: np.ndarray):
        out[metric_name] = metric.copy()
        metric = metric.astype(np.float64)
        metric[metric == np.inf] = np.nan
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", category=RuntimeWarning)
            mean_metric, sd_metric = np.nanmean(metric, axis=0), np.nanstd(metric, axis=0)
        out[f"mean_{metric_name}"], out[f"sd_{metric_name}"] = mean_metric, sd_metric
        lines.append(f"Mean {metric_name}," + ",".join(f"{e:.7f}" for e in np.atleast_1d(mean_metric)))
        lines.append(f"SD {metric_name}," + ",".join(f"{e:.7f}" for e in np.atleast_1d(sd_metric)))

    for m in (EVALUATION_METRIC_DICE_CLASSES, EVALUATION_METRIC_DICE_MACRO, EVALUATION_METRIC_DICE_MICRO):
        if m in metrics:
            save_metric(m, stack(files, m))
    if EVALUATION_METRIC_AVERAGE_SURFACE_DISTANCE in metrics:          # evaluation.py:870-880
        for name in ("average_surface_distances", "average_surface_distances_gt_to_pred",
                     "average_surface_distances_pred_to_gt"):
            save_metric(name, stack(files, name))
    if EVALUATION_METRIC_HAUSDORFF_DISTANCE in metrics:
        save_metric("hausdorff_distances", stack(files, "hausdorff_distances"))
    if getattr(eval_params, "calibration_bins", 0):
        for m in CALIBRATION_METRICS:
            save_metric(m, stack(files, m))
        # the POOLED values: of the counts summed over the images, re-read from the per-image files (ranks exchange nothing)
        tables = stack(files, "calibration_counts")
        out["calibration_counts"], pooled = pooled_calibration(tables, stack(files, "nll")[:, 0], stack(files, "brier")[:, 0])
        for m in CALIBRATION_METRICS:
            out[f"pooled_{m}"] = np.array([pooled[m]], dtype="float64")
            lines.append(f"Pooled {m},{pooled[m]:.7f}")
    if eval_params.graph_search:
        for m in (EVALUATION_METRIC_DICE_CLASSES, EVALUATION_METRIC_DICE_MACRO, EVALUATION_METRIC_DICE_MICRO):
            if m in metrics:
                save_metric(f"gs_{m}", stack(gs_files, m))
        errors = stack(gs_files, "errors")
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", category=RuntimeWarning)
            mean_abs_errors_samples = np.nanmean(np.abs(errors), axis=2)
            mean_errors_samples = np.nanmean(errors, axis=2)
            out.update({
                "mean_abs_errors_cols": np.nanmean(np.abs(errors), axis=0),
                "mean_abs_errors_samples": mean_abs_errors_samples,
                "mean_abs_errors": np.nanmean(mean_abs_errors_samples, axis=0),
                "sd_abs_errors": np.nanstd(mean_abs_errors_samples, axis=0),
                "median_abs_errors": np.nanmedian(mean_abs_errors_samples, axis=0),
                "sd_abs_errors_samples": np.nanstd(np.abs(errors), axis=2),
                "mean_errors_cols": np.nanmean(errors, axis=0),
                "mean_errors_samples": mean_errors_samples,
                "mean_errors": np.nanmean(mean_errors_samples, axis=0),
                "sd_errors": np.nanstd(mean_errors_samples, axis=0),
                "median_errors": np.nanmedian(mean_errors_samples, axis=0),
                "errors": errors})
        for title, key in (("Mean abs errors", "mean_abs_errors"), ("Mean errors", "mean_errors"),
                           ("Median absolute errors", "median_abs_errors"), ("SD abs errors", "sd_abs_errors"),
                           ("SD errors", "sd_errors")):
            lines.append(f"{title}," + ",".join(f"{e:.7f}" for e in out[key]))
    if getattr(eval_params, "ordered_decode", False):
        # the ordered decode: the aggregates the graph search gets above, under od_ names, behind everything that was there
        od_files = [h5io.load(d / Path(OD_EVALUATION_RESULTS_FILENAME)) for d in dir_list]
        for m in (EVALUATION_METRIC_DICE_CLASSES, EVALUATION_METRIC_DICE_MACRO, EVALUATION_METRIC_DICE_MICRO):
            if m in metrics:
                save_metric(f"od_{m}", stack(od_files, m))
        errors = stack(od_files, "errors")
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", category=RuntimeWarning)
            abs_samples, samples = np.nanmean(np.abs(errors), axis=2), np.nanmean(errors, axis=2)
            out.update({
                "od_mean_abs_errors_cols": np.nanmean(np.abs(errors), axis=0), "od_mean_abs_errors_samples": abs_samples,
                "od_mean_abs_errors": np.nanmean(abs_samples, axis=0), "od_sd_abs_errors": np.nanstd(abs_samples, axis=0),
                "od_median_abs_errors": np.nanmedian(abs_samples, axis=0),
                "od_sd_abs_errors_samples": np.nanstd(np.abs(errors), axis=2),
                "od_mean_errors_cols": np.nanmean(errors, axis=0), "od_mean_errors_samples": samples,
                "od_mean_errors": np.nanmean(samples, axis=0), "od_sd_errors": np.nanstd(samples, axis=0),
                "od_median_errors": np.nanmedian(samples, axis=0), "od_errors": errors})
        for title, key in (("OD mean abs errors", "od_mean_abs_errors"), ("OD mean errors", "od_mean_errors"),
                           ("OD median absolute errors", "od_median_abs_errors"), ("OD SD abs errors", "od_sd_abs_errors"),
                           ("OD SD errors", "od_sd_errors")):
            lines.append(f"{title}," + ",".join(f"{e:.7f}" for e in out[key]))
        save_metric("od_changed_pixels", stack(od_files, "changed_pixels"))
        if od_files and "mean_layer_thickness" in od_files[0]:
            save_metric("od_mean_layer_thickness", stack(od_files, "mean_layer_thickness"))
    if getattr(eval_params, "components", None) is not None:
        # the component stage: means and standard deviations under cc_ names, behind everything that was there
        cc_files = [h5io.load(d / Path(CC_EVALUATION_RESULTS_FILENAME)) for d in dir_list]
        for m in (EVALUATION_METRIC_DICE_CLASSES, EVALUATION_METRIC_DICE_MACRO, EVALUATION_METRIC_DICE_MICRO):
            if m in metrics:
                save_metric(f"cc_{m}", stack(cc_files, m))
        if EVALUATION_METRIC_AVERAGE_SURFACE_DISTANCE in metrics:
            for name in ("average_surface_distances", "average_surface_distances_gt_to_pred",
                         "average_surface_distances_pred_to_gt"):
                save_metric(f"cc_{name}", stack(cc_files, name))
        if EVALUATION_METRIC_HAUSDORFF_DISTANCE in metrics:
            save_metric("cc_hausdorff_distances", stack(cc_files, "hausdorff_distances"))
        for name in ("component_count", "largest_component_pixels", "removed_pixels", "changed_pixels"):
            save_metric(f"cc_{name}", stack(cc_files, name))
    h5io.save(output_dir / Path(OVERALL_EVALUATION_RESULTS_FILENAME_HDF5), out)
    with open(output_dir / Path(OVERALL_EVALUATION_RESULTS_FILENAME_CSV), "w") as f:
        f.write("\n".join(lines) + "\n")
    return out


eval_model = evaluate_model  # README / north_star alias
