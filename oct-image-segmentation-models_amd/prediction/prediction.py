"""``predict``: the reference's prediction workflow
(oct_image_segmentation_models/prediction/prediction.py:48-186, savers :189-329) -- the evaluation stack
without labels/metrics.  Batched device forward with device arg-max; host tail re-stated.  With
``PredictionParams(png_plots=True)`` the reference's PNG pictures (prediction.py:243-263, :307-320) are rasterised on the
device (``oct_render_rgba``, ``evaluation/render.py``); ``categorical_pred_N.png`` is out of scope."""
from __future__ import annotations

import json
import logging as log
import os
import time
from pathlib import Path
from typing import List, Union

import numpy as np

from .. import parallel
from ..common import h5io, utils
from ..evaluation.pipeline import InferenceRun
from ..evaluation.ordered import layer_thickness
from ..evaluation.render import CC_PNG_NAMES, OD_PNG_NAMES, PREDICTION_PNG_NAMES, write_pictures
from ..min_path_processing import graph_search  # noqa: F401  (re-exported: callers build graph structures through it)
from ..models import get_model_class
from .prediction_parameters import PredictionParams


class PredictionOutput:
    def __init__(self, image: np.ndarray, image_name: Path, image_output_dir: Path, predicted_labels: np.ndarray,
                 categorical_pred: np.ndarray, boundary_maps: np.ndarray, gs_pred_segs: Union[np.ndarray, None],
                 predictive_entropy: Union[np.ndarray, None] = None, mutual_information: Union[np.ndarray, None] = None) -> None:
        self.image = image
        self.image_name = image_name
        self.image_output_dir = image_output_dir
        self.predicted_labels = predicted_labels
        self.categorical_pred = categorical_pred
        self.boundary_maps = boundary_maps
        self.gs_pred_segs = gs_pred_segs
        # (H,W) float32 maps of a Monte-Carlo dropout prediction (PredictionParams.mc_samples > 0), else None
        self.predictive_entropy = predictive_entropy
        self.mutual_information = mutual_information


def predict(predict_params: PredictionParams) -> List[PredictionOutput]:
    """With ``predict_params.gs_labels_device`` the graph-search class maps come from the device, a batch at a time, and
    the ``graph_time`` attribute of graph_search_prediction_info.hdf5 is that stage's time divided by the batch's image
    count; every dataset and CSV file equals the host path's.

    With ``predict_params.mc_samples`` > 0 every batch is a Monte-Carlo dropout prediction (``InferenceRun(mc_samples=)``):
    every file describes the MEAN prediction, prediction_info.hdf5 gains the float32 (H,W) datasets ``predictive_entropy``
    and ``mutual_information`` and the attribute ``mc_samples``, and with the PNG pictures on ``uncertainty_map.png`` (the
    entropy over ln C as a gray scan) is written too.  With 0 every file is byte for byte what it was.

    With ``predict_params.tta`` (view names, ``common.utils.TTA_VIEWS``) every batch is the mean prediction over the flipped
    views (``InferenceRun(tta=)``): the same two datasets and picture, and the attribute ``tta_views`` -- the names joined
    by commas -- in place of ``mc_samples``.  Unset, nothing more is launched and every file is byte for byte what it was."""
    rank, _, _ = parallel.init()
    world = parallel.world_size()
    dataset = predict_params.dataset
    images = np.asarray(dataset.images)
    if rank == 0:
        os.makedirs(predict_params.config_output_dir, exist_ok=True)
        save_predict_config_file(predict_params)
    try:
        model_class = get_model_class(predict_params.loaded_model.name)
    except ValueError as e:
        log.error(e)
        exit(1)
    model_class(**predict_params.model_config)
    num_classes = predict_params.num_classes

    outputs: List[PredictionOutput] = []
    lo, hi = parallel.shard_range(len(images), rank, world)
    png_plots = bool(getattr(predict_params, "png_plots", False)) and predict_params.save_params.png_images is True
    mc_samples = int(getattr(predict_params, "mc_samples", 0))
    ordered_decode = bool(getattr(predict_params, "ordered_decode", False))
    components = getattr(predict_params, "components", None)
    # the device pipeline of evaluate_model (evaluation/pipeline.py::InferenceRun), without ground truth
    with InferenceRun(predict_params.loaded_model, images[lo:hi], predict_params.batch_size, num_classes,
                      graph_search=predict_params.graph_search, gs_device=predict_params.gs_device,
                      gs_device_ties=predict_params.gs_device_ties, gs_workers=predict_params.gs_workers,
                      soft_maps=not getattr(predict_params, "binarize", True),
                      mc_samples=mc_samples, mc_step0=getattr(predict_params, "mc_step0", 0),
                      pad_mode=getattr(predict_params, "pad_mode", None),
                      pad_value=getattr(predict_params, "pad_value", 0), tta=getattr(predict_params, "tta", None),
                      temperature=getattr(predict_params, "temperature", 1.0),
                      **({"ordered_decode": True} if ordered_decode else {}),
                      **({"components": components} if components is not None else {}),
                      **({"contrast": predict_params.contrast} if getattr(predict_params, "contrast", None) is not None
                         else {})) as run:
        t0 = time.time()
        for batch in run:
            b0, b1 = lo + batch.lo, lo + batch.hi
            predict_time = (time.time() - t0) / (b1 - b0)
            gs_found = run.graph_search(batch)
            gs_labels = None
            if predict_params.graph_search and getattr(predict_params, "gs_labels_device", False):
                start_stage_time = time.time()
                gs_labels, _ = run.gs_labels(batch, gs_found)
                gs_stage_time = (time.time() - start_stage_time) / (b1 - b0)
            pictures = None
            if png_plots:
                pictures = run.render_pngs(batch, images[b0:b1], gs_found, gs_labels=gs_labels,
                                           pred_map=predict_params.save_params.predicted_labels is True,
                                           col_range=(predict_params.col_error_range[0], predict_params.col_error_range[-1]))
                if batch.entropy is not None:
                    pictures["uncertainty"] = run.render_gray(utils.entropy_to_u8(batch.entropy, num_classes))
            od_pictures = None
            if png_plots and ordered_decode:
                od_pictures = run.render_ordered(batch, images[b0:b1],
                                                 col_range=(predict_params.col_error_range[0], predict_params.col_error_range[-1]))
            cc_pictures = {"cc_map": run.render_labels(batch.components[0])} if png_plots and components is not None else None
            for i in range(b0, b1):
                predict_image, image_name, image_output_dir = images[i], dataset.image_names[i], Path(dataset.image_output_dirs[i])
                os.makedirs(image_output_dir, exist_ok=True)
                log.info(f"Inferring image {i}: {image_name}")
                start_convert_time = time.time()
                predicted_labels = batch.labels[i - b0:i - b0 + 1].astype(np.int64)
                categorical_pred = utils.labels_to_categorical(predicted_labels, num_classes)
                # on device: == convert_predictions_to_maps_semantic(categorical_pred); with binarize=False, of the probabilities
                boundary_maps = batch.maps[i - b0:i - b0 + 1]
                convert_time = time.time() - start_convert_time
                predicted_labels = np.squeeze(predicted_labels, axis=0)
                categorical_pred = np.squeeze(categorical_pred, axis=0)
                boundary_maps = np.squeeze(boundary_maps, axis=0)
                entropy = mutual_info = None
                if batch.entropy is not None:
                    entropy, mutual_info = batch.entropy[i - b0], batch.mutual_info[i - b0]
                save_image_prediction_results(predict_params, predict_image, image_name, predicted_labels, categorical_pred,
                                              boundary_maps, predict_time, convert_time, image_output_dir,
                                              entropy=entropy, mutual_info=mutual_info,
                                              ordered=None if batch.ordered is None else tuple(t[i - b0] for t in batch.ordered),
                                              **({"components": tuple(t[i - b0] for t in batch.components)}
                                                 if batch.components is not None else {}))
                if cc_pictures is not None:
                    write_pictures(image_output_dir, cc_pictures, i - b0, CC_PNG_NAMES)
                if od_pictures is not None:
                    write_pictures(image_output_dir, od_pictures, i - b0, OD_PNG_NAMES)
                gs_pred_segs = None
                if predict_params.graph_search:
                    predict_image_t = np.transpose(predict_image, axes=[1, 0, 2])
                    start_graph_time = time.time()
                    gs_pred_segs = gs_found[i - b0][0]           # == graph_search.segment_maps(boundary_maps_t, None, grid)
                    if gs_labels is not None:
                        gs_prediction_label, graph_time = gs_labels[i - b0], gs_stage_time
                    else:
                        gs_prediction_label, _ = utils.labels_from_delineations(predict_image_t.shape, gs_pred_segs, num_classes)
                        graph_time = time.time() - start_graph_time
                    save_graph_based_prediction_results(predict_params, image_name, gs_prediction_label, gs_pred_segs,
                                                        graph_time, image_output_dir)
                if pictures is not None:
                    write_pictures(image_output_dir, pictures, i - b0, PREDICTION_PNG_NAMES)
                outputs.append(PredictionOutput(image=predict_image, image_name=image_name, image_output_dir=image_output_dir,
                                                predicted_labels=predicted_labels, categorical_pred=categorical_pred,
                                                boundary_maps=boundary_maps, gs_pred_segs=gs_pred_segs,
                                                predictive_entropy=entropy, mutual_information=mutual_info))
            t0 = time.time()
    parallel.barrier()
    return outputs


def save_predict_config_file(predict_params: PredictionParams):
    attrs = {"model_filename": np.array(str(predict_params.model_path), dtype="S1000"),
             "error_col_inc_range": np.array((predict_params.col_error_range[0], predict_params.col_error_range[-1]))}
    if not getattr(predict_params, "binarize", True):
        attrs["binarize"] = np.array(False)      # recorded only when it departs from the default: binarize=True files stay as they were
    if getattr(predict_params, "png_plots", False):
        attrs["png_plots"] = np.array(True)      # likewise
    if getattr(predict_params, "mc_samples", 0):
        attrs["mc_samples"] = np.array(int(predict_params.mc_samples))      # likewise, with the first dropout step
        attrs["mc_step0"] = np.array(int(getattr(predict_params, "mc_step0", 0)))
    if getattr(predict_params, "tta", None):
        attrs["tta_views"] = np.array(",".join(predict_params.tta), dtype="S1000")      # likewise
    if getattr(predict_params, "contrast", None) is not None:
        attrs["contrast"] = np.array(json.dumps(predict_params.contrast, sort_keys=True), dtype="S1000")      # likewise
    if getattr(predict_params, "pad_mode", None) is not None:
        attrs["pad_mode"] = np.array(str(predict_params.pad_mode), dtype="S1000")      # likewise, with the constant
        attrs["pad_value"] = np.array(float(getattr(predict_params, "pad_value", 0)))
    if getattr(predict_params, "temperature", 1.0) != 1.0:
        attrs["temperature"] = np.array(float(predict_params.temperature))      # likewise
    if getattr(predict_params, "ordered_decode", False):
        attrs["ordered_decode"] = np.array(True)      # likewise
    if getattr(predict_params, "components", None) is not None:
        attrs["components"] = np.array(repr(predict_params.components), dtype="S1000")      # likewise
    h5io.save(predict_params.config_output_dir / Path("prediction_params.hdf5"), {}, attrs)


def save_image_prediction_results(pred_params, predict_image, image_name, predicted_labels, categorical_pred,
                                  boundary_maps, predict_time, convert_time, output_dir, entropy=None, mutual_info=None,
                                  ordered=None, components=None):
    """``entropy`` / ``mutual_info``: the (H,W) maps of a Monte-Carlo dropout or test-time-augmented prediction, stored
    (with the sample count, or the views) only when given: without them the file is what it always was.  ``ordered``: the
    image's ``(labels (H,W), rows (C-1,W), score (W))`` of ``Batch.ordered``, likewise: the file gains ``od_predicted_labels``,
    ``od_pred_segs`` and (from 3 classes) ``layer_thickness``, and the two od_ CSV files are written.  ``components``: the image's
    ``(clean_labels (H,W), stats (C,2), removed (C))`` of ``Batch.components``, likewise: the file gains ``cc_predicted_labels``,
    ``component_count``, ``largest_component_pixels`` and ``removed_pixels``."""
    ds = {}
    if pred_params.save_params.categorical_pred is True:
        ds["categorical_pred"] = categorical_pred.astype("uint8")
    np.savetxt(output_dir / Path("segmentation_map.csv"), predicted_labels, fmt="%d", delimiter=",")
    if pred_params.save_params.predicted_labels is True:
        ds["predicted_labels"] = predicted_labels.astype("uint8")
    if pred_params.save_params.boundary_maps is True:
        ds["boundary_maps"] = boundary_maps.astype("uint8")
    ds["raw_image"] = predict_image.astype("uint8")
    attrs = utils.result_attrs(pred_params.model_path, image_name, predict_time=np.array(predict_time), convert_time=convert_time)
    if entropy is not None:
        ds["predictive_entropy"] = np.asarray(entropy, np.float32)
        ds["mutual_information"] = np.asarray(mutual_info, np.float32)
        if getattr(pred_params, "tta", None):
            attrs["tta_views"] = np.array(",".join(pred_params.tta), dtype="S1000")
        else:
            attrs["mc_samples"] = np.array(int(getattr(pred_params, "mc_samples", 0)))
    if getattr(pred_params, "temperature", 1.0) != 1.0:
        attrs["temperature"] = np.array(float(pred_params.temperature))      # only when set
    if getattr(pred_params, "contrast", None) is not None:
        attrs["contrast"] = np.array(json.dumps(pred_params.contrast, sort_keys=True), dtype="S1000")      # only when set
    if ordered is not None:
        od_labels, od_rows = ordered[0], ordered[1]
        np.savetxt(output_dir / Path("od_boundaries.csv"), od_rows, delimiter=",", fmt="%d")
        np.savetxt(output_dir / Path("od_predicted_segmentation_map.csv"), od_labels, fmt="%d", delimiter=",")
        ds["od_predicted_labels"], ds["od_pred_segs"] = od_labels.astype("uint8"), od_rows.astype("uint16")
        thickness, _ = layer_thickness(od_rows)
        if thickness is not None:
            ds["layer_thickness"] = thickness
    if components is not None:
        cc_labels, stats, removed = components
        ds["cc_predicted_labels"] = cc_labels.astype("uint8")
        ds["component_count"], ds["largest_component_pixels"] = stats[:, 0].astype("uint32"), stats[:, 1].astype("uint32")
        ds["removed_pixels"] = removed.astype("uint32")
    h5io.save(output_dir / Path("prediction_info.hdf5"), ds, attrs)


def save_graph_based_prediction_results(predict_params, image_name, gs_prediction_label, gs_pred_segs, graph_time,
                                        output_dir):
    np.savetxt(output_dir / Path("gs_boundaries.csv"), gs_pred_segs, delimiter=",", fmt="%d")
    np.savetxt(output_dir / Path("gs_segmentation_map.csv"), gs_prediction_label, fmt="%d", delimiter=",")
    ds = {"gs_pred_segs": gs_pred_segs.astype("uint16"), "gs_predicted_labels": gs_prediction_label.astype("uint8")}
    attrs = utils.result_attrs(predict_params.model_path, image_name, graph_time=np.array(graph_time))
    h5io.save(output_dir / Path("graph_search_prediction_info.hdf5"), ds, attrs)
