"""``EvaluationParameters`` / ``EvaluationSaveParams`` with the reference's constructor contract
(oct_image_segmentation_models/evaluation/evaluation_parameters.py:12-85); the model is loaded in the
constructor, as there."""
from __future__ import annotations

import logging as log
from pathlib import Path
from typing import List, Optional

from ..common import EVALUATION_METRICS, plotting, utils
from .dice_device import check_ignore_label


class EvaluationSaveParams:
    def __init__(self, predicted_labels: bool = True, categorical_pred: bool = False, png_images: bool = True,
                 boundary_maps: bool = True) -> None:
        self.predicted_labels = predicted_labels
        self.categorical_pred = categorical_pred
        # takes effect with EvaluationParameters(png_plots=True): False keeps every PNG picture from being written
        self.png_images = png_images
        self.boundary_maps = boundary_maps


class EvaluationParameters:
    def __init__(self, model_path: Path, mlflow_tracking_uri: Optional[str], mlflow_run_uuid: Optional[str],
                 test_dataset_path: Path, save_foldername: Path, save_params: EvaluationSaveParams,
                 graph_search: bool, metrics: List[str], gsgrad=1, dice_errors: bool = True, binarize: bool = True,
                 bg_ilm: bool = True, bg_csi: bool = False, batch_size: int = 32, gs_device: bool = False,
                 gs_device_ties: str = "host", gs_workers: Optional[int] = None, metrics_device: bool = False,
                 png_plots: bool = False, pad_mode: Optional[str] = None, pad_value=0, ignore_label: Optional[int] = None,
                 tta=None, calibration_bins: int = 0, temperature: float = 1.0, ordered_decode: bool = False,
                 components=None, contrast=None):
        # extension: contrast normalisation of the uint8 scans in front of the prediction.  None: off; a
        # spec of common.utils.check_contrast ({"method": "clahe" | "stretch", "tiles", "clip" | "percentiles"}); or "model": the
        # contrast.json that train_model(contrast=) wrote beside the checkpoint -- an error if that file is absent.  Every batch
        # is normalised on the device, at the scans' own size and in front of the pad; the result files record the spec's JSON
        # as the attribute contrast; the pictures keep showing the scans as given.  With None and a contrast.json present: one
        # warning, nothing changes, nothing is launched
        self.contrast = utils.resolve_contrast(contrast, model_path)
        # extension: connected components of the arg-max class map.  A ComponentRule, or a dict of its
        # keywords (connectivity, min_pixels, keep_largest, fill): components that the rule removes -- islands below min_pixels,
        # all but the largest of a class -- are refilled on the device.  Every image gains cc_evaluation_results.hdf5
        # (cc_predicted_labels, component_count / largest_component_pixels of the arg-max map and removed_pixels per class,
        # changed_pixels, the Dice metrics and surface distances asked for, of the cleaned map), the overall results the cc_
        # aggregates; with png_plots one picture.  The rule must fit the model's classes (checked once the model is loaded).
        # None: nothing is launched, no file changes
        from .components import ComponentRule
        self.components = ComponentRule.coerce(components, "components")
        # extension: the ordered layer decode.  Per column the best class map whose class index never
        # decreases with depth, decoded on the device from the class probabilities (the mean ones with tta, the tempered ones with
        # temperature).  Every image gains od_evaluation_results.hdf5 (od_pred_segs, od_predicted_labels, errors and their four
        # statistics, the Dice metrics asked for, layer_thickness, mean_layer_thickness, changed_pixels), od_boundaries.csv and
        # od_predicted_segmentation_map.csv, the overall results the od_ aggregates; with png_plots two pictures.  Needs 2..16
        # classes (checked once the model is loaded).  False: nothing is launched, no file changes
        self.ordered_decode = bool(ordered_decode)
        # extension: calibration of the class probabilities.  calibration_bins, an int in 0..64: with
        # M > 0 the reliability counts of the probabilities against the ground truth are made on the device in M confidence
        # bins; each image's results gain calibration_counts (M, 3) = [n, correct, sum of confidences], ece, mce, nll and brier,
        # the overall results their mean / sd and the pooled values.  With tta the counts are those of the mean prediction.
        # temperature, a number in [1/16, 16]: the probabilities are tempered on the device (softmax(logits / temperature)) in
        # front of the binarize=False maps and the counts; not together with tta.  Defaults: nothing is launched, no file changes
        from .calibration import check_bins, check_temperature
        self.calibration_bins, self.temperature = check_bins(calibration_bins), check_temperature(temperature)
        if self.temperature != 1.0 and utils.check_tta(tta):
            raise ValueError("temperature != 1 together with tta: the views would have to be tempered before they are averaged, "
                             "which is not implemented")
        # extension: test-time augmentation.  1..4 distinct view names out of common.utils.TTA_VIEWS ("identity", "flip_lr",
        # "flip_ud", "flip_both"): every batch is predicted once per view on the mirrored scans, the softmax outputs are mirrored
        # back and averaged on the device, and all metrics, boundary maps, graph-search delineations and pictures come from
        # that mean prediction; the result files record tta_views.  Everything behind the prediction is unchanged, so it
        # combines with pad_mode, ignore_label, binarize=False, metrics_device, gs_device and png_plots.  None or (): off
        self.tta = utils.check_tta(tta)
        # extension: scans whose size is no multiple of 2^pool_layers (the reference raises on them) are padded on the
        # device in front of the forward -- "edge", "reflect" or "constant" with pad_value in raw counts -- and the arg-max
        # maps (with binarize=False the probabilities too) are cropped directly behind the head: metrics, searches, files
        # and pictures have the scans' own size.  None: such sizes are refused.  Sizes that are multiples are never padded;
        # the engine follows the dataset's size, whatever model_config.json records
        self.pad_mode, self.pad_value = utils.check_pad_mode(pad_mode, pad_value)
        self.model_path = Path(model_path)
        self.mlflow_tracking_uri = mlflow_tracking_uri
        self.mlflow_run_uuid = mlflow_run_uuid
        self.test_dataset_path = Path(test_dataset_path)
        # binarize=False (the reference's perform_argmax(bin=False)): the boundary maps are
        # convert_predictions_to_maps_semantic of the class PROBABILITIES, built on the device (oct_boundary_maps_soft), and
        # everything behind the graph search follows them: gs_pred_segs, errors, the graph-search class maps, their Dice,
        # the CSV files.  predicted_labels, the arg-max Dice and the surface distances do not change, and categorical_pred
        # stays the one-hot of the arg-max: the files store it as uint8, for which truncated probabilities mean nothing
        self.binarize = bool(binarize)
        self.save_params = save_params
        self.graph_search = graph_search
        if not set(metrics).issubset(EVALUATION_METRICS):
            log.error(f"Some of the provided metrics are invalid. Provided metrics: {metrics}.")
            exit(1)
        self.metrics = metrics
        self.gsgrad = gsgrad
        self.dice_errors = dice_errors
        self.bg_ilm = bg_ilm
        self.bg_csi = bg_csi
        self.save_foldername = Path(save_foldername)
        self.batch_size = batch_size   # extension: device batch (the reference predicts one image per call)
        # extension: the min-path search on the device (min_path_processing/device_search.py).  "host" ties: maps whose
        # minimum-cost path is not unique go back to the host search (outputs identical to gs_device=False); "device"
        # ties: they keep the device's documented rule and no host search runs
        if gs_device_ties not in ("host", "device"):
            raise ValueError('gs_device_ties must be "host" or "device"')
        self.gs_device = bool(gs_device)
        self.gs_device_ties = gs_device_ties
        self.gs_workers = gs_workers   # extension: host-search worker processes (None: the CPU share, 1: inline)
        # extension: the Dice metrics from confusion counts made on the device and the graph-search class maps from
        # oct_area_labels (evaluation/dice_device.py).  Every dataset and CSV file equals the host path's; the graph_time
        # attribute becomes the batch's stage time divided by its image count
        self.metrics_device = bool(metrics_device)
        # extension: write the reference's PNG pictures of every image (raw_image, predicted / ground-truth / graph-search
        # segmentation maps, truth_plot and the two graph-search overlays), rasterised on the device by oct_render_rgba and
        # encoded by common/png.py, under the reference's save_params conditions (png_images; predicted_labels for the
        # prediction map).  Off by default like every device post-process: no other output changes either way
        self.png_plots = bool(png_plots)
        self.loaded_model, self.model_config = utils.load_model_and_config(
            self.model_path, mlflow_tracking_uri=mlflow_tracking_uri, mlflow_run_uuid=mlflow_run_uuid)
        self.num_classes = self.loaded_model.output.shape[-1]
        plotting.check_png_classes(self.png_plots, self.num_classes)     # pictures exist up to 9 classes: refused here, up front
        if self.ordered_decode:
            from .ordered import check_ordered
            check_ordered(self.num_classes, 1)
        if self.components is not None:
            self.components.check(self.num_classes)
        # extension: the test set's labels are known in part only (annotated column ranges, masked optic-nerve heads): ground-truth
        # pixels of this value, an int in num_classes..255, are "unknown" wherever a metric, a truth boundary or a ground-truth
        # picture is formed -- out of the Dice counts, no surface element at their rim, no truth boundary underneath them,
        # mid-grey in the pictures.  The predictions and everything made of them alone do not depend on
        # it.  None: such values are refused, and no file changes
        self.ignore_label = check_ignore_label(ignore_label, self.num_classes)
