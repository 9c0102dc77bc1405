"""CPU tests of the PNG pictures: ``common.plotting.render_reference`` (the numpy statement of ``oct_render_rgba``) against
pixels recorded from the reference under matplotlib and against known answers of the rule, its refusals, the PNG codec of
``common/png.py``, the two ``save_*_plot`` functions and the ``png_plots`` switch of the parameter classes."""
import inspect
import os

import numpy as np
import pytest

from tests import render_cases as rc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "png_reference_golden.npz")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def _pl():
    from oct_image_segmentation_models_amd.common import plotting
    return plotting


def _png():
    from oct_image_segmentation_models_amd.common import png
    return png


def test_label_maps_and_rgb_scan_equal_the_reference(golden):
    pl = _pl()
    for C in (3, 8):
        lab = golden[f"labels{C}_in"]
        assert lab.min() == 0 and lab.max() == C - 1
        assert np.array_equal(pl.render_reference(lab[None], palette=pl.region_palette(C))[0], golden[f"labels{C}_out"])
    assert np.array_equal(pl.render_reference(golden["scan3_in"][None])[0], golden["scan3_out"])


def test_one_channel_scans_differ_from_the_reference_by_its_gray_rounding_only(golden):
    """matplotlib's gray picture is a function of the level alone that is one lower than the identity at the levels the
    golden's own ramp shows (24 of them); the project renders the identity."""
    pl = _pl()
    ramp = golden["ramp_in"]
    assert set(np.unique(ramp).tolist()) == set(range(256))
    ref = golden["ramp_out"]
    assert (ref[..., 3] == 255).all() and (ref[..., 0] == ref[..., 1]).all() and (ref[..., 0] == ref[..., 2]).all()
    table = np.full(256, -1)
    for lv in range(256):
        vals = np.unique(ref[..., 0][ramp[..., 0] == lv])
        assert vals.size == 1
        table[lv] = vals[0]
    low = set(np.nonzero(table != np.arange(256))[0].tolist())
    assert len(low) == 24 and all(table[lv] == lv - 1 for lv in low)
    for name in ("ramp", "scan1"):
        src, want = golden[f"{name}_in"], golden[f"{name}_out"]
        got = pl.render_reference(src[None])[0]
        diff = got.astype(int) - want.astype(int)
        assert np.abs(diff).max() <= 1 and (got[..., 3] == 255).all()
        differing = set(src[..., 0][diff[..., 0] != 0].tolist())
        assert differing == (low if name == "ramp" else low & set(np.unique(src).tolist()))
        assert np.array_equal(got[..., 0], src[..., 0]) and np.array_equal(want[..., 0], table[src[..., 0]])


def test_flat_solid_line_known_answer():
    pl = _pl()
    bg, col = 100, np.array(rc.LINE_RGB[0])
    out = pl.render_reference(**rc.flat_line())[0]
    edge = (4 * col + 12 * bg + 8) >> 4
    for r in range(16):
        want = col if 6 <= r <= 10 else edge if r in (5, 11) else np.array([bg] * 3)
        assert (out[r, :, :3] == want).all(), r
    assert (out[..., 3] == 255).all()


def test_column_range_bounds_the_line_and_its_caps():
    pl = _pl()
    out = pl.render_reference(**rc.flat_line(col_range=(5, 30)))[0]
    touched = np.nonzero((out[..., :3] != 100).any(axis=(0, 2)))[0]
    assert touched.min() == 2 and touched.max() == 33
    assert (out[8, 5:31, :3] == np.array(rc.LINE_RGB[0])).all()
    # a range of one column has a vertex and no segment: nothing is drawn
    one = pl.render_reference(**rc.flat_line(col_range=(7, 7)))[0]
    assert (one[..., :3] == 100).all()


def test_dotted_line_pattern_by_column():
    pl = _pl()
    cov = pl.line_coverage(np.full(40, 8), 16, 5, 35, 22, True)
    period = [8] + [16] * 5 + [8] + [0] * 8
    assert cov[8, 5:35].tolist() == (period * 2)[:30]
    assert (cov[8, :5] == 0).all()
    out = pl.render_reference(**rc.flat_line(col_range=(5, 35), styles=[1]))[0]
    col = np.array(rc.LINE_RGB[0])
    assert (out[8, 6, :3] == col).all() and (out[8, 5, :3] == ((8 * col + 8 * 100 + 8) >> 4)).all() and (out[8, 13, :3] == 100).all()


def test_isolated_vertices_zero_rows_and_rows_beyond_the_image_draw_nothing():
    pl = _pl()
    rows = np.zeros((1, 1, 40), np.uint16)
    rows[0, 0, ::2] = 8                                      # every vertex isolated
    rows[0, 0, 21] = 16                                      # == H: missing
    kw = rc.flat_line()
    kw["lines"] = rows
    assert (pl.render_reference(**kw)[0][..., :3] == 100).all()
    rows[0, 0, 21] = 15                                      # H - 1 is a vertex: two steep segments appear
    assert (pl.render_reference(**kw)[0][..., :3] != 100).any()


def test_lines_compose_in_index_order():
    pl = _pl()
    kw = rc.mixed_lines(B=1)
    out = pl.render_reference(**kw)[0]
    H = 36
    # row H-1: line 2 (solid) everywhere, line 3 (dotted) over it in its "on" columns
    assert (out[H - 1, 1, :3] == np.array(rc.LINE_RGB[3])).all() and (out[H - 1, 10, :3] == np.array(rc.LINE_RGB[2])).all()
    swapped = dict(kw, lines=kw["lines"][:, [0, 1, 3, 2]], colours=[kw["colours"][i] for i in (0, 1, 3, 2)], styles=[0, 1, 1, 0])
    assert (pl.render_reference(**swapped)[0][H - 1, 1, :3] == np.array(rc.LINE_RGB[2])).all()


def test_tall_image_with_a_full_height_jump_stays_exact_and_quick():
    """4096 x 12 with a 1 -> 4095 jump: |w|^2 den reaches 1.15e18, inside int64.  Python integers give the same answer
    at the pixels next to the steep segment."""
    import time
    pl = _pl()
    kw = rc.tall_jump()
    t0 = time.perf_counter()
    cov = pl.line_coverage(kw["lines"][0, 0], 4096, 0, 11, 22, False)
    assert time.perf_counter() - t0 < 5.0
    v = kw["lines"][0, 0].astype(int)
    for r in (0, 1, 2047, 2048, 4094, 4095):
        for c in (4, 5, 6, 7):
            n = 0
            for oy in (-3, -1, 1, 3):
                for ox in (-3, -1, 1, 3):
                    hit = False
                    for j in range(11):
                        wx, wy, dy = 8 * c + ox - 8 * j, 8 * r + oy - 8 * v[j], 8 * (v[j + 1] - v[j])
                        t, den, ww = 8 * wx + wy * dy, 64 + dy * dy, wx * wx + wy * wy
                        if t <= 0:
                            hit |= ww <= 484
                        elif t >= den:
                            hit |= (wx - 8) ** 2 + (wy - dy) ** 2 <= 484
                        else:
                            hit |= ww * den - t * t <= 484 * den
                    n += hit
            assert cov[r, c] == n, (r, c)
    assert cov[2048, 5] > 0 or cov[2048, 6] > 0


@pytest.mark.parametrize("bad", [
    dict(half_width=0), dict(half_width=65), dict(col_range=(6, 5)), dict(col_range=(-1, 5)), dict(col_range=(0, 40)),
    dict(styles=[2]), dict(colours=[]), dict(base=np.zeros((1, 4097, 2, 1), np.uint8), lines=None, colours=None),
    dict(base=np.zeros((0, 4, 4, 1), np.uint8), lines=None, colours=None),
    dict(base=np.zeros((1, 16, 40, 1), np.int16)),
    dict(lines=np.ones((1, 17, 40), np.uint16), colours=[(1, 2, 3)] * 17),
    dict(lines=np.ones((1, 1, 39), np.uint16)),
])
def test_refusals(bad):
    pl = _pl()
    with pytest.raises(ValueError):
        pl.render_reference(**dict(rc.flat_line(), **bad))


def test_palette_refusals_and_stray_labels():
    pl = _pl()
    lab = rc.label_maps(1, 8, 20, 3)
    out = pl.render_reference(lab, palette=pl.region_palette(3))[0]
    assert (out[lab[0] >= 3][:, :3] == 0).all() and (out[..., 3] == 255).all()
    assert (out[0, 1, :3] == np.array(pl.REGION_COLOURS[1])).all()
    with pytest.raises(ValueError):
        pl.render_reference(lab, palette=np.zeros((33, 3), np.uint8))
    with pytest.raises(ValueError):
        pl.render_reference(lab, palette=np.zeros((0, 3), np.uint8))
    with pytest.raises(ValueError):
        pl.render_reference(lab[..., None], palette=pl.region_palette(3))
    assert len(pl.REGION_COLOURS) == len(pl.TRUTH_COLOURS) == len(pl.PREDICT_COLOURS) == 12


@pytest.mark.parametrize("shape", [(1, 1), (3, 5), (36, 68)], ids=lambda s: "x".join(map(str, s)))
def test_png_round_trip(tmp_path, shape):
    png = _png()
    arr = np.random.default_rng(shape[0]).integers(0, 256, shape + (4,), dtype=np.uint8)
    for arr_ in (arr, np.full(shape + (4,), 37, np.uint8)):
        seen = set()
        for f in (None, png.FILTER_NONE, png.FILTER_SUB, png.FILTER_UP):
            for level in (None, 0, 9):
                path = tmp_path / "x.png"
                png.write_rgba(path, arr_, f, level)
                data = path.read_bytes()
                assert data == png.encode_rgba(arr_, f, level)                     # a pure function of the array
                got = png.read_rgba(path)
                assert got.dtype == np.uint8 and np.array_equal(got, arr_)
                seen.add(data)
                try:
                    from PIL import Image
                except ImportError:
                    continue
                with Image.open(path) as im:
                    assert im.mode == "RGBA" and np.array_equal(np.array(im), arr_)
        assert len(seen) > 1


def test_png_reader_takes_every_filter_type_and_refuses_other_files(tmp_path):
    import struct
    import zlib
    png = _png()
    arr = np.random.default_rng(4).integers(0, 256, (6, 7, 4), dtype=np.uint8)
    # a file whose rows use filter types 0..4 in turn, filtered here by the definitions of the PNG specification
    a = arr.astype(int)
    lines = []
    for r in range(6):
        f = r % 5
        row = bytearray([f])
        for c in range(7):
            for ch in range(4):
                left = a[r, c - 1, ch] if c else 0
                up = a[r - 1, c, ch] if r else 0
                ul = a[r - 1, c - 1, ch] if r and c else 0
                p = left + up - ul
                paeth = left if abs(p - left) <= abs(p - up) and abs(p - left) <= abs(p - ul) else up if abs(p - up) <= abs(p - ul) else ul
                pred = (0, left, up, (left + up) // 2, paeth)[f]
                row.append((a[r, c, ch] - pred) & 255)
        lines.append(bytes(row))

    def chunk(kind, data):
        return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data))
    body = zlib.compress(b"".join(lines))
    data = png.SIGNATURE + chunk(b"IHDR", struct.pack(">IIBBBBB", 7, 6, 8, 6, 0, 0, 0)) + chunk(b"IDAT", body[:9]) + \
        chunk(b"IDAT", body[9:]) + chunk(b"IEND", b"")
    assert np.array_equal(png.decode_rgba(data), arr)
    with pytest.raises(ValueError):
        png.decode_rgba(b"GIF89a" + data)
    with pytest.raises(ValueError):
        png.decode_rgba(data[:40] + bytes([data[40] ^ 1]) + data[41:])          # CRC
    with pytest.raises(ValueError):
        png.decode_rgba(png.SIGNATURE + chunk(b"IHDR", struct.pack(">IIBBBBB", 7, 6, 8, 2, 0, 0, 0)) + chunk(b"IEND", b""))
    for bad in (arr[..., :3], arr.astype(np.int32), arr[0]):
        with pytest.raises(ValueError):
            png.encode_rgba(bad)


def test_save_plots_write_what_render_reference_gives(tmp_path):
    pl, png = _pl(), _png()
    assert [p for p in inspect.signature(pl.save_image_plot).parameters] == ["image", "filename", "cmap", "vmin", "vmax"]
    assert [p for p in inspect.signature(pl.save_segmentation_plot).parameters] == \
        ["image", "image_cmap", "filename", "truths", "predictions", "column_range", "linewidth", "color"]
    kw = rc.wavy_lines(1, 36, 68, K=3, seed=2)
    image, segs = kw["base"][0], kw["lines"][0]
    pl.save_image_plot(image, tmp_path / "raw.png", cmap="gray", vmin=0, vmax=255)
    assert np.array_equal(png.read_rgba(tmp_path / "raw.png"), pl.render_reference(image[None])[0])
    pl.save_image_plot(image[:, :, 0], tmp_path / "raw2.png", cmap=None)
    assert (tmp_path / "raw2.png").read_bytes() == (tmp_path / "raw.png").read_bytes()
    rgb = rc.scans(1, 36, 68, 3, seed=8)[0]
    pl.save_image_plot(rgb, tmp_path / "rgb.png", cmap=None)
    assert np.array_equal(png.read_rgba(tmp_path / "rgb.png")[..., :3], rgb)
    lab = rc.label_maps(1, 36, 68, 4, stray=0)[0]
    pl.save_image_plot(lab, tmp_path / "lab.png", cmap=pl.region_palette(4))
    assert np.array_equal(png.read_rgba(tmp_path / "lab.png"), pl.render_reference(lab[None], palette=pl.region_palette(4))[0])
    other = np.roll(segs, 3, axis=1)
    pl.save_segmentation_plot(image, "gray", tmp_path / "both.png", segs, other, column_range=range(4, 60))
    want = pl.render_reference(image[None], lines=np.concatenate([segs, other])[None],
                               colours=pl.TRUTH_COLOURS[:3] + pl.PREDICT_COLOURS[:3], styles=[0, 0, 0, 1, 1, 1],
                               col_range=(4, 59), half_width=22)[0]
    assert np.array_equal(png.read_rgba(tmp_path / "both.png"), want)
    assert not np.array_equal(want, pl.render_reference(image[None])[0])
    pl.save_segmentation_plot(image, "gray", tmp_path / "pred.png", None, other, color=(1, 2, 3), linewidth=2.0)
    want = pl.render_reference(image[None], lines=other[None], colours=[(1, 2, 3)] * 3, styles=[1, 1, 1], half_width=11)[0]
    assert np.array_equal(png.read_rgba(tmp_path / "pred.png"), want)
    with pytest.raises(ValueError):
        pl.save_segmentation_plot(image, "gray", tmp_path / "none.png", None, None)


def test_parameter_classes_take_png_plots_and_default_to_off():
    from oct_image_segmentation_models_amd.evaluation.evaluation_parameters import EvaluationParameters, EvaluationSaveParams
    from oct_image_segmentation_models_amd.prediction.prediction_parameters import PredictionParams, PredictionSaveParams
    for cls in (EvaluationParameters, PredictionParams):
        p = inspect.signature(cls.__init__).parameters["png_plots"]
        assert p.default is False
        src = inspect.getsource(cls.__init__)
        assert "self.png_plots = bool(png_plots)" in src
    assert EvaluationSaveParams().png_images is True and PredictionSaveParams().png_images is True
    assert EvaluationSaveParams(png_images=False).png_images is False


def test_inference_run_over_injected_batches_refuses_render_pngs():
    from oct_image_segmentation_models_amd.evaluation.pipeline import Batch, InferenceRun
    images = np.zeros((1, 8, 8, 1), np.uint8)
    batch = Batch(0, 1, np.zeros((1, 8, 8), np.uint8))
    with InferenceRun(None, images, 1, 3, batches=[batch]) as run:
        with pytest.raises(RuntimeError, match="render_pngs needs the device"):
            run.render_pngs(batch, images)
