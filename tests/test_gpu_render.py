"""GPU tests of the PNG pictures: ``oct_render_rgba`` against ``common.plotting.render_reference`` -- byte equality
everywhere -- on the smallest shapes at which the kernel can go wrong (tile edges, halo, steep segments, clipped lines, the
int64 bound), in a stream capture and on bad arguments; ``PngRenderer`` in chunks; ``evaluate_model`` / ``predict`` with
``png_plots=True`` in the three search / metric modes: the files they write, their pixels, and everything else unchanged."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest
import torch

from oracle import unet_numpy as on
from tests import render_cases as rc
from tests.helpers import save_untrained_model

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
FILL = 0xAB


def _hip():
    from oct_image_segmentation_models_amd import _hip
    return _hip


def _pl():
    from oct_image_segmentation_models_amd.common import plotting
    return plotting


def _style(W, palette=None, colours=None, styles=None, col_range=None, half_width=22, n_lines=None):
    st = _hip().RenderStyle()
    pal = np.zeros((1, 3), np.uint8) if palette is None else np.asarray(palette, np.uint8).reshape(-1, 3)
    colours = np.zeros((0, 3), np.int64) if colours is None else np.asarray(colours, np.int64).reshape(-1, 3)
    K = colours.shape[0] if n_lines is None else n_lines
    styles = [0] * K if styles is None else styles
    st.n_cls, st.n_lines, st.half_width = pal.shape[0], K, half_width
    st.col_lo, st.col_hi = (0, W - 1) if col_range is None else (col_range[0], col_range[-1])
    for i, v in enumerate(pal.reshape(-1)[:96]):
        st.palette[i] = int(v)
    for i, v in enumerate(colours.reshape(-1)[:48]):
        st.line_rgb[i] = int(v)
    for i, v in enumerate(styles[:16]):
        st.line_style[i] = int(v)
    return st


def _call(mode, base_dev, ic, rows_dev, st, B, H, W, out_dev):
    return _hip().lib().oct_render_rgba(mode, None if base_dev is None else base_dev.data_ptr(), ic,
                                        None if rows_dev is None else rows_dev.data_ptr(),
                                        None if st is None else C.byref(st), B, H, W,
                                        None if out_dev is None else out_dev.data_ptr(),
                                        torch.cuda.current_stream().cuda_stream)


def _device_inputs(base, palette=None, lines=None, **kw):
    B, H, W = base.shape[:3]
    mode = _hip().RENDER_BASE_LABELS if palette is not None else _hip().RENDER_BASE_IMAGE
    ic = 1 if base.ndim == 3 else base.shape[3]
    base_dev = torch.from_numpy(np.ascontiguousarray(base)).cuda()
    rows_dev = None if lines is None else torch.from_numpy(np.ascontiguousarray(lines).view(np.int16)).cuda()
    st = _style(W, palette=palette, **kw)
    return mode, base_dev, ic, rows_dev, st, B, H, W


def _render(**case):
    """The kernel's picture of a ``render_reference`` keyword set; the bytes behind the output stay untouched."""
    args = _device_inputs(**case)
    B, H, W = args[-3:]
    buf = torch.full((B * H * W * 4 + 64,), FILL, dtype=torch.uint8, device="cuda")
    out = buf[:B * H * W * 4].view(B, H, W, 4)
    assert _call(*args, out) == 0, _hip().lib().oct_last_error()
    assert (buf[B * H * W * 4:] == FILL).all()
    return out.cpu().numpy()


def _same(**case):
    got, want = _render(**case), _pl().render_reference(**case)
    assert got.shape == want.shape and np.array_equal(got, want), np.argwhere(got != want)[:5]
    return got


@pytest.mark.parametrize("B,H,W,ic", [(3, 8, 20, 1), (2, 36, 68, 3), (1, 1, 1, 1), (2, 5, 7, 2), (1, 17, 65, 1)])
def test_base_image(B, H, W, ic):
    got = _same(base=rc.scans(B, H, W, ic, seed=B + W))
    assert (got[..., 3] == 255).all()


@pytest.mark.parametrize("Cc", [3, 8])
def test_base_labels_with_stray_pixels(Cc):
    lab = rc.label_maps(2, 36, 68, Cc, seed=Cc)
    assert (lab >= Cc).sum() == 6
    got = _same(base=lab, palette=rc.palette(Cc))
    assert (got[lab >= Cc][:, :3] == 0).all()


def test_flat_line_known_answer_on_the_device():
    got = _same(**rc.flat_line())[0]
    bg, col = 100, np.array(rc.LINE_RGB[0])
    edge = (4 * col + 12 * bg + 8) >> 4
    for r in range(16):
        want = col if 6 <= r <= 10 else edge if r in (5, 11) else np.array([bg] * 3)
        assert (got[r, :, :3] == want).all(), r


@pytest.mark.parametrize("col_range", [(5, 30), None, (12, 12), (0, 0), (67, 67), (60, 67)], ids=str)
def test_mixed_lines_and_column_ranges(col_range):
    """Solid and dotted lines, a 30-row jump, a run of zeros, rows >= H, lines clipped at the top and bottom edge and two
    lines on one row; a range of one column holds no segment and leaves the base."""
    case = rc.mixed_lines(col_range=col_range)
    got = _same(**case)
    if col_range is not None and col_range[0] == col_range[1]:
        assert np.array_equal(got[..., :3], np.repeat(case["base"], 3, axis=3))
    else:
        assert not np.array_equal(got[..., :3], np.repeat(case["base"], 3, axis=3))


def test_fourteen_crossing_lines():
    _same(**rc.crossing_lines())


@pytest.mark.parametrize("B,H,W,ic", [(5, 12, 130, 1), (5, 9, 67, 3), (2, 33, 64, 1), (3, 16, 129, 1)])
def test_widths_that_divide_no_tile_and_odd_batches(B, H, W, ic):
    _same(**rc.wavy_lines(B, H, W, K=3, seed=W, ic=ic))


def test_one_column():
    _same(base=rc.scans(2, 9, 1, 1), lines=np.full((2, 2, 1), 4, np.uint16), colours=rc.LINE_RGB[:2], styles=[0, 1])


def test_tall_image_with_a_full_height_jump():
    got = _same(**rc.tall_jump())
    assert (got[0, 2048, :, 0] != rc.tall_jump()["base"][0, 2048, :, 0]).any()   # the steep segments pass through the middle


@pytest.mark.parametrize("half_width", [1, 9, 64])
def test_half_widths(half_width):
    _same(**rc.mixed_lines(half_width=half_width))
    _same(**rc.wavy_lines(1, 40, 150, K=2, seed=half_width), half_width=half_width, col_range=(70, 140))


def test_call_records_into_a_graph_and_replays():
    first, second = rc.wavy_lines(3, 20, 70, seed=1), rc.wavy_lines(3, 20, 70, seed=2)
    mode, base_dev, ic, rows_dev, st, B, H, W = _device_inputs(**first)
    out = torch.full((B, H, W, 4), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        assert _call(mode, base_dev, ic, rows_dev, st, B, H, W, out) == 0
    st.half_width = 3                                       # the style went by value: the capture holds its own copy
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), _pl().render_reference(**first))
    base_dev.copy_(torch.from_numpy(second["base"]))
    rows_dev.copy_(torch.from_numpy(second["lines"].view(np.int16)))
    out.fill_(FILL)
    graph.replay()
    torch.cuda.synchronize()
    want = _pl().render_reference(**second)
    assert np.array_equal(out.cpu().numpy(), want)
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), want)


def test_argument_errors_launch_nothing():
    case = rc.mixed_lines()
    mode, base_dev, ic, rows_dev, st, B, H, W = _device_inputs(**case)
    out = torch.full((B, H, W, 4), FILL, dtype=torch.uint8, device="cuda")
    lib = _hip().lib()
    LAB = _hip().RENDER_BASE_LABELS

    def style(**kw):
        s = _style(W, colours=case["colours"], styles=case["styles"])
        for k, v in kw.items():
            setattr(s, k, v)
        return s
    bad = [(mode, None, ic, rows_dev, st, B, H, W, out), (mode, base_dev, ic, None, st, B, H, W, out),
           (mode, base_dev, ic, rows_dev, None, B, H, W, out), (mode, base_dev, ic, rows_dev, st, B, H, W, None),
           (mode, base_dev, ic, rows_dev, st, 0, H, W, out), (mode, base_dev, ic, rows_dev, st, B, 0, W, out),
           (mode, base_dev, ic, rows_dev, st, B, H, -3, out), (mode, base_dev, 0, rows_dev, st, B, H, W, out),
           (2, base_dev, ic, rows_dev, st, B, H, W, out), (mode, base_dev, ic, rows_dev, st, 1, 4097, 2, out),
           (LAB, base_dev, 1, rows_dev, style(n_cls=0), B, H, W, out), (LAB, base_dev, 1, rows_dev, style(n_cls=33), B, H, W, out),
           (mode, base_dev, ic, rows_dev, style(n_lines=17), B, H, W, out), (mode, base_dev, ic, rows_dev, style(n_lines=-1), B, H, W, out),
           (mode, base_dev, ic, rows_dev, style(half_width=0), B, H, W, out), (mode, base_dev, ic, rows_dev, style(half_width=65), B, H, W, out),
           (mode, base_dev, ic, rows_dev, style(col_lo=9, col_hi=8), B, H, W, out), (mode, base_dev, ic, rows_dev, style(col_lo=-1), B, H, W, out),
           (mode, base_dev, ic, rows_dev, style(col_hi=W), B, H, W, out)]
    for i, args in enumerate(bad):
        assert _call(*args) < 0 and b"render_rgba" in lib.oct_last_error(), i
    # an output inside an input, and an input inside the output
    wide = torch.full((B * H * W * 4 + 4096,), FILL, dtype=torch.uint8, device="cuda")
    assert _call(mode, wide[128:], ic, rows_dev, st, B, H, W, wide) < 0 and b"overlap" in lib.oct_last_error()
    assert _call(mode, base_dev, ic, wide[B * H * W * 4 - 2:].view(torch.int16), st, B, H, W, wide) < 0
    assert _call(mode, wide, ic, rows_dev, st, B, H, W, wide[B * H * W - 4:]) < 0
    torch.cuda.synchronize()
    assert (out == FILL).all() and (wide == FILL).all()
    assert np.array_equal(base_dev.cpu().numpy(), case["base"])


def test_renderer_chunks_and_takes_host_and_device_inputs():
    from oct_image_segmentation_models_amd.evaluation.render import PngRenderer
    from oct_image_segmentation_models_amd._hip import OctError
    B, H, W = 7, 20, 34
    case = rc.wavy_lines(B, H, W, K=3, seed=6, ic=3)
    want = _pl().render_reference(**case)
    r = PngRenderer(B, H, W, "cuda:0", staging_bytes=3 * H * W * 4 + 5)        # chunks of 3, 3 and 1
    assert r.chunk == 3 and r.out_pin.numel() <= 3 * H * W * 4 + 5 and r.out_pin.is_pinned()
    assert PngRenderer(128, 256, 512, "cuda:0").out_pin.numel() <= 64 << 20
    lines = {k: case[k] for k in ("lines", "colours", "styles")}
    assert np.array_equal(r.render(case["base"], **lines), want)
    assert np.array_equal(r.render(torch.from_numpy(case["base"]).cuda(), **lines), want)
    dev_lines = dict(lines, lines=torch.from_numpy(case["lines"].view(np.int16)).cuda())
    assert np.array_equal(r.render(torch.from_numpy(case["base"]).cuda(), **dev_lines), want)
    assert np.array_equal(r.render(case["base"][:2, ..., 0], col_range=(3, 9)), _pl().render_reference(case["base"][:2, ..., :1]))
    lab = rc.label_maps(B, H, W, 5)
    assert np.array_equal(r.render(lab, palette=rc.palette(5)), _pl().render_reference(lab, palette=rc.palette(5)))
    for bad in (dict(base=case["base"][:, :-1]), dict(base=case["base"].astype(np.int32)),
                dict(base=np.concatenate([case["base"]] * 2)), dict(base=case["base"], lines=case["lines"][:3]),
                dict(base=case["base"], lines=case["lines"], colours=case["colours"][:1])):
        with pytest.raises(OctError):
            r.render(**bad)


# ---- workflows on tests/golden/dataset_small.hdf5 with an untrained net, 3 classes, batch 2 -------------------------------
CC, BATCH = 3, 2
METRICS = ["dice_coef_classes", "dice_coef_macro", "dice_coef_micro"]
EVAL_PNGS = {"predicted_segmentation_map.png", "raw_image.png", "ground_truth_segmentation_map.png", "truth_plot.png",
             "gs_predicted_segmentation_map.png", "gs_pred_and_truth_overlay_plot.png",
             "gs_predicted_boundaries_ovelay_plot.png"}
PRED_PNGS = {"segmentation_map.png", "raw_image.png", "gs_predicted_segmentation_map.png",
             "gs_predicted_boundaries_ovelay_plot.png"}
TIMES = {"attr:graph_time", "attr:predict_time", "attr:convert_time", "attr:timestamp"}


class _Workflows:
    def __init__(self, tmp_path):
        from oct_image_segmentation_models_amd.common import dataset_loader as dl
        self.root = tmp_path
        self.data = ROOT / "tests" / "golden" / "dataset_small.hdf5"
        self.images, self.labels, _ = dl.load_testing_data(dl.open_dataset(self.data))
        self.n, self.H, self.W = self.images.shape[:3]
        save_untrained_model(tmp_path, self.H, self.W, CC, 8, 2)
        self.cols = range(3, self.W - 5)

    def evaluate(self, name, save=None, graph_search=True, **kw):
        from oct_image_segmentation_models_amd.evaluation import eval_model
        from oct_image_segmentation_models_amd.evaluation.evaluation_parameters import EvaluationParameters, EvaluationSaveParams
        ep = EvaluationParameters(model_path=self.root / "model" / "model.npz", mlflow_tracking_uri=None, mlflow_run_uuid=None,
                                  test_dataset_path=self.data, save_foldername=self.root / name,
                                  save_params=EvaluationSaveParams(**(save or {})), graph_search=graph_search, metrics=METRICS,
                                  batch_size=BATCH, **kw)
        ep.gs_workers = 1
        return eval_model(ep)

    def predict(self, name, save=None, graph_search=True, **kw):
        from oct_image_segmentation_models_amd.common.dataset import Dataset
        from oct_image_segmentation_models_amd.prediction import predict
        from oct_image_segmentation_models_amd.prediction.prediction_parameters import PredictionParams, PredictionSaveParams
        ds = Dataset(self.images, [Path(f"volume_{i}.tiff") for i in range(self.n)],
                     [self.root / name / f"image_{i}" for i in range(self.n)])
        pp = PredictionParams(model_path=self.root / "model" / "model.npz", mlflow_tracking_uri=None, mlflow_run_uuid=None,
                              dataset=ds, config_output_dir=self.root / name, save_params=PredictionSaveParams(**(save or {})),
                              graph_search=graph_search, batch_size=BATCH, col_error_range=self.cols, **kw)
        pp.gs_workers = 1
        return predict(pp)


def _files(root: Path):
    return sorted(p.relative_to(root) for p in root.rglob("*") if p.is_file())


def _pngs_of(root: Path, i: int):
    return {p.name for p in (root / f"image_{i}").iterdir() if p.suffix == ".png"}


def _others_equal(on_dir: Path, off_dir: Path, config: str):
    """Every non-PNG file of the run with the switch on equals its twin of the run with it off (times aside); the
    config file differs by the png_plots attribute alone."""
    from oct_image_segmentation_models_amd.common import h5io
    fa = [f for f in _files(on_dir) if f.suffix != ".png"]
    assert fa == _files(off_dir) and len(fa) > 5
    for rel in fa:
        if ".hdf5" in rel.suffixes:
            x, y = h5io.load(on_dir / rel), h5io.load(off_dir / rel)
            extra = {"attr:png_plots"} if rel.name.startswith(config) else set()
            assert set(x) - extra == set(y), rel
            assert extra <= set(x) and all(bool(x[k]) for k in extra)
            for k in set(y) - TIMES:
                u, v = np.asarray(x[k]), np.asarray(y[k])
                assert u.dtype == v.dtype and u.shape == v.shape, (rel, k)
                assert np.array_equal(u, v, equal_nan=u.dtype.kind == "f"), (rel, k)
        else:
            assert (on_dir / rel).read_bytes() == (off_dir / rel).read_bytes(), rel


@pytest.mark.parametrize("mode", ["host", "gs_device", "metrics_device"])
def test_workflows_write_the_pictures_of_their_result_files(tmp_path, mode):
    from oct_image_segmentation_models_amd.common import h5io, png
    pl = _pl()
    wf = _Workflows(tmp_path)
    e_kw, p_kw = {"host": ({}, {}), "gs_device": (dict(gs_device=True),) * 2,
                  "metrics_device": (dict(metrics_device=True), dict(gs_labels_device=True))}[mode]
    wf.evaluate("eval_off", **e_kw)
    wf.evaluate("eval_on", png_plots=True, **e_kw)
    wf.predict("pred_off", **p_kw)
    wf.predict("pred_on", png_plots=True, **p_kw)
    _others_equal(tmp_path / "eval_on", tmp_path / "eval_off", "eval_params")
    _others_equal(tmp_path / "pred_on", tmp_path / "pred_off", "prediction_params")
    assert not [f for f in _files(tmp_path / "eval_off") + _files(tmp_path / "pred_off") if f.suffix == ".png"]
    palette = pl.region_palette(CC)
    differ = 0
    for i in range(wf.n):
        d = tmp_path / "eval_on" / f"image_{i}"
        assert _pngs_of(tmp_path / "eval_on", i) == EVAL_PNGS
        f, g = h5io.load(d / "evaluation_results.hdf5"), h5io.load(d / "gs_evaluation_results.hdf5")
        raw, truths, segs = f["raw_image"][None], f["raw_segs"][None], g["gs_pred_segs"][None]
        M = truths.shape[1]
        want = {
            "raw_image.png": pl.render_reference(raw),
            "predicted_segmentation_map.png": pl.render_reference(f["predicted_segmentation_map"][None], palette=palette),
            "ground_truth_segmentation_map.png": pl.render_reference(f["eval_labels"][None], palette=palette),
            "truth_plot.png": pl.render_reference(raw, lines=truths, colours=pl.TRUTH_COLOURS[:M]),
            "gs_predicted_segmentation_map.png": pl.render_reference(g["gs_predicted_labels"][None], palette=palette),
            "gs_pred_and_truth_overlay_plot.png": pl.render_reference(
                raw, lines=np.concatenate([truths, segs], axis=1), colours=pl.TRUTH_COLOURS[:M] + pl.PREDICT_COLOURS[:M],
                styles=[0] * M + [1] * M),
            "gs_predicted_boundaries_ovelay_plot.png": pl.render_reference(raw, lines=segs, colours=pl.TRUTH_COLOURS[:M]),
        }
        for name, rgba in want.items():
            got = png.read_rgba(d / name)
            assert got.shape == (wf.H, wf.W, 4) and np.array_equal(got, rgba[0]), (i, name)
        differ += not np.array_equal(want["truth_plot.png"], want["raw_image.png"])
        d = tmp_path / "pred_on" / f"image_{i}"
        assert _pngs_of(tmp_path / "pred_on", i) == PRED_PNGS
        f, g = h5io.load(d / "prediction_info.hdf5"), h5io.load(d / "graph_search_prediction_info.hdf5")
        raw, segs = f["raw_image"][None], g["gs_pred_segs"][None]
        want = {
            "raw_image.png": pl.render_reference(raw),
            "segmentation_map.png": pl.render_reference(f["predicted_labels"][None], palette=palette),
            "gs_predicted_segmentation_map.png": pl.render_reference(g["gs_predicted_labels"][None], palette=palette),
            "gs_predicted_boundaries_ovelay_plot.png": pl.render_reference(
                raw, lines=segs, colours=pl.TRUTH_COLOURS[:segs.shape[1]], col_range=(wf.cols[0], wf.cols[-1])),
        }
        for name, rgba in want.items():
            assert np.array_equal(png.read_rgba(d / name), rgba[0]), (i, name)
    assert differ == wf.n                                                    # the overlays do carry lines
    assert h5io.load(tmp_path / "eval_on" / "eval_params.hdf5")["attr:png_plots"]
    assert "attr:png_plots" not in h5io.load(tmp_path / "eval_off" / "eval_params.hdf5")


def test_save_params_conditions_and_no_graph_search(tmp_path):
    wf = _Workflows(tmp_path)
    wf.evaluate("eval_plain")
    wf.evaluate("eval_nopng", save=dict(png_images=False), png_plots=True)
    wf.predict("pred_nopng", save=dict(png_images=False), png_plots=True)
    wf.predict("pred_plain")
    for a, b in (("eval_nopng", "eval_plain"), ("pred_nopng", "pred_plain")):
        assert [f for f in _files(tmp_path / a) if f.suffix == ".png"] == []
        assert _files(tmp_path / a) == _files(tmp_path / b)
    wf.evaluate("eval_nolab", save=dict(predicted_labels=False), png_plots=True)
    wf.predict("pred_nolab", save=dict(predicted_labels=False), png_plots=True)
    wf.evaluate("eval_nogs", graph_search=False, png_plots=True)
    wf.predict("pred_nogs", graph_search=False, png_plots=True)
    for i in range(wf.n):
        assert _pngs_of(tmp_path / "eval_nolab", i) == EVAL_PNGS - {"predicted_segmentation_map.png"}
        assert _pngs_of(tmp_path / "pred_nolab", i) == PRED_PNGS - {"segmentation_map.png"}
        assert _pngs_of(tmp_path / "eval_nogs", i) == {n for n in EVAL_PNGS if not n.startswith("gs_")}
        assert _pngs_of(tmp_path / "pred_nogs", i) == {n for n in PRED_PNGS if not n.startswith("gs_")}
