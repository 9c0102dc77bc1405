"""``PredictionParams`` / ``PredictionSaveParams`` with the reference's constructor contract
(oct_image_segmentation_models/prediction/prediction_parameters.py:12-63)."""
from __future__ import annotations

from pathlib import Path
from typing import Union

from ..common import plotting, utils
from ..common.dataset import Dataset


class PredictionSaveParams:
    def __init__(self, predicted_labels: bool = True, categorical_pred: bool = False, png_images: bool = True,
                 boundary_maps: bool = True) -> None:
        self.predicted_labels = predicted_labels
        self.categorical_pred = categorical_pred
        # takes effect with PredictionParams(png_plots=True): False keeps every PNG picture from being written
        self.png_images = png_images
        self.boundary_maps = boundary_maps


class PredictionParams:
    def __init__(self, model_path: Path, mlflow_tracking_uri: Union[str, None], mlflow_run_uuid: Union[str, None],
                 dataset: Dataset, config_output_dir: Path, save_params: PredictionSaveParams,
                 graph_search: bool = False, trim_maps: bool = False, trim_ref_ind: int = 0,
                 trim_window: tuple = (0, 0), col_error_range: tuple = None, batch_size: int = 32, gs_device: bool = False,
                 gs_device_ties: str = "host", gs_workers: Union[int, None] = None, gs_labels_device: bool = False,
                 binarize: bool = True, png_plots: bool = False, mc_samples: int = 0, mc_step0: int = 0,
                 pad_mode: Union[str, None] = None, pad_value=0, tta=None, temperature: float = 1.0,
                 ordered_decode: bool = False, components=None, contrast=None) -> None:
        # extension: contrast normalisation of the uint8 scans in front of the prediction.  None: off; a
        # spec of common.utils.check_contrast ({"method": "clahe" | "stretch", "tiles", "clip" | "percentiles"}); or "model": the
        # contrast.json that train_model(contrast=) wrote beside the checkpoint -- an error if that file is absent.  Every batch
        # is normalised on the device, at the scans' own size and in front of the pad; the result files record the spec's JSON
        # as the attribute contrast; the pictures keep showing the scans as given.  With None and a contrast.json present: one
        # warning, nothing changes, nothing is launched
        self.contrast = utils.resolve_contrast(contrast, model_path)
        # extension, as EvaluationParameters.components (a ComponentRule or a dict of its keywords): prediction_info.hdf5 gains
        # cc_predicted_labels, component_count, largest_component_pixels and removed_pixels; with png_plots
        # cc_predicted_segmentation_map.png is written.  None: nothing is launched, every file as it was
        from ..evaluation.components import ComponentRule
        self.components = ComponentRule.coerce(components, "components")
        # extension, as EvaluationParameters.ordered_decode: prediction_info.hdf5 gains od_predicted_labels, od_pred_segs and
        # (from 3 classes) layer_thickness, and od_boundaries.csv / od_predicted_segmentation_map.csv are written.  False: nothing is
        # launched, every file as it was
        self.ordered_decode = bool(ordered_decode)
        if not 0 <= int(mc_samples) <= 64:
            raise ValueError(f"mc_samples must be in 0..64, not {mc_samples}")
        # extension: temperature scaling.  A number in [1/16, 16], e.g. the one train_model(fit_temperature=True)
        # wrote into temperature.json: the class probabilities are tempered on the device, softmax(logits / temperature).  There is
        # no ground truth here, so it changes the binarize=False maps (and what the search makes of them) and nothing else; the
        # result files record it when set.  Not together with mc_samples or tta.  1.0: nothing is launched, every file as it was
        from ..evaluation.calibration import check_temperature
        self.temperature = check_temperature(temperature)
        if self.temperature != 1.0 and (int(mc_samples) or utils.check_tta(tta, mc_samples)):
            raise ValueError("temperature != 1 together with mc_samples or tta: the samples would have to be tempered before they "
                             "are averaged, which is not implemented")
        # extension: test-time augmentation.  1..4 distinct view names out of common.utils.TTA_VIEWS ("identity", "flip_lr",
        # "flip_ud", "flip_both"): every batch is predicted once per view on the mirrored scans and the softmax outputs are
        # mirrored back and averaged on the device; every file describes the mean prediction, and prediction_info.hdf5 gains
        # predictive_entropy / mutual_information and the attribute tta_views.  Deterministic; not combined with mc_samples.
        # None or (): one view per scan, every file as it was
        self.tta = utils.check_tta(tta, mc_samples)
        # extension: scans whose size is no multiple of 2^pool_layers (the reference raises on them) are padded on the
        # device in front of the forward -- "edge", "reflect" or "constant" with pad_value in raw counts -- and every output
        # is cropped directly behind the head, so every file has the scans' own size.  None: such sizes are refused.  Sizes
        # that are multiples are never padded; the engine follows the dataset's size, whatever model_config.json records
        self.pad_mode, self.pad_value = utils.check_pad_mode(pad_mode, pad_value)
        self.model_path = Path(model_path)
        self.mlflow_tracking_uri = mlflow_tracking_uri
        self.mlflow_run_uuid = mlflow_run_uuid
        self.dataset = dataset
        self.loaded_model, self.model_config = utils.load_model_and_config(
            self.model_path, mlflow_tracking_uri=mlflow_tracking_uri, mlflow_run_uuid=mlflow_run_uuid)
        self.num_classes = self.loaded_model.output.shape[-1]
        if self.ordered_decode:
            from ..evaluation.ordered import check_ordered
            check_ordered(self.num_classes, 1)
        if self.components is not None:
            self.components.check(self.num_classes)
        self.config_output_dir = Path(config_output_dir)
        self.save_params = save_params
        self.graph_search = graph_search
        self.trim_maps = trim_maps
        self.trim_ref_ind = trim_ref_ind
        self.trim_window = trim_window
        self.batch_size = batch_size
        # extension: the min-path search on the device (see EvaluationParameters)
        if gs_device_ties not in ("host", "device"):
            raise ValueError('gs_device_ties must be "host" or "device"')
        self.gs_device = bool(gs_device)
        self.gs_device_ties = gs_device_ties
        self.gs_workers = gs_workers   # extension: host-search worker processes (None: the CPU share, 1: inline)
        # extension: gs_prediction_label from oct_area_labels (evaluation/dice_device.py) instead of the host loop; the
        # same files, and the graph_time attribute becomes the batch's stage time divided by its image count
        self.gs_labels_device = bool(gs_labels_device)
        # extension, as EvaluationParameters.binarize: False = soft boundary maps of the class probabilities
        self.binarize = bool(binarize)
        # extension, as EvaluationParameters.png_plots: segmentation_map.png, raw_image.png and, with graph search,
        # gs_predicted_segmentation_map.png and gs_predicted_boundaries_ovelay_plot.png (columns col_error_range)
        self.png_plots = bool(png_plots)
        plotting.check_png_classes(self.png_plots, self.num_classes)     # pictures exist up to 9 classes: refused here, up front
        # extension: Monte-Carlo dropout prediction.  mc_samples > 0: every batch is predicted mc_samples times with the
        # bottleneck dropout on (dropout steps mc_step0 .. mc_step0+mc_samples-1, the same for every batch); the class maps,
        # boundary maps and everything behind them are those of the mean prediction, and prediction_info.hdf5 gains
        # predictive_entropy / mutual_information.  A result depends on the image's position in its batch (batch_size) and
        # on the rank that predicts it (the dropout stream is seeded per rank).  0: the deterministic prediction
        self.mc_samples, self.mc_step0 = int(mc_samples), int(mc_step0)
        self.col_error_range = col_error_range
        if col_error_range is None:
            self.col_error_range = range(dataset.images[0].shape[1])  # image_width
