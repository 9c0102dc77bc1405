"""The column-recurrence form of the min-path boundary search (min_path_processing/device_search.py::delineate_dp, the
CPU-testable definition of what oct_minpath_device computes) against vectors captured from the REAL reference's
``segment_maps`` (tests/golden/make_minpath_device_golden.py), and the merge that keeps ``evaluate_model`` / ``predict``
identical to the host search.  Everything is exact: fp64 ``==`` on costs, integer rows."""
import os

import numpy as np
import pytest

import __graft_entry__ as ge

G = np.load(os.path.join(os.path.dirname(__file__), "golden", "minpath_device_golden.npz"))
FAMILIES = [str(f) for f in G["families"]]
SHAPES = [(int(h), int(w)) for h, w in G["shapes"]]


def cases():
    for H, W in SHAPES:
        tag = f"s{H}x{W}"
        for g in G[f"{tag}_max_grads"]:
            yield tag, H, W, int(g)


@pytest.fixture(scope="module")
def dp_results():
    """delineate_dp of every fixture map and max_grad, computed once: {(tag, g): (rows, cost, tied)} with M = 1."""
    from oct_image_segmentation_models_amd.min_path_processing.device_search import delineate_dp
    out = {}
    for tag, H, W, g in cases():
        rows, cost, tied = delineate_dp(G[f"{tag}_maps"][:, None], g)
        assert rows.dtype == np.uint16 and cost.dtype == np.float64 and tied.dtype == bool
        out[tag, g] = rows[:, 0], cost[:, 0], tied[:, 0]
    return out


def test_fixture_covers_the_families_shapes_and_gradients():
    assert FAMILIES == ["noise", "ridge_noise", "ridge_clean", "ridge_jump3", "ridge_salt", "zeros", "full"]
    assert SHAPES == [(16, 24), (12, 40), (70, 33), (3, 9), (2, 9), (1, 5)]
    for H, W in SHAPES:
        tag = f"s{H}x{W}"
        grads = [int(g) for g in G[f"{tag}_max_grads"]]
        assert grads[:3] == [1, 2, 3] and grads[3] == min(16, H + 3)      # larger than H wherever the limit of 16 allows
        assert G[f"{tag}_maps"].dtype == np.uint8 and G[f"{tag}_maps"].shape[1:] == (H, W)
        assert sorted(set(G[f"{tag}_family"].tolist())) == list(range(len(FAMILIES)))
    assert any(g > H for _, H, _, g in cases())


def test_cost_equals_the_reference_distance_exactly(dp_results):
    for tag, H, W, g in cases():
        assert np.array_equal(dp_results[tag, g][1], G[f"{tag}_g{g}_cost"]), (tag, g)


def test_rows_equal_the_reference_on_every_untied_map(dp_results):
    for tag, H, W, g in cases():
        rows, _, tied = dp_results[tag, g]
        same = (rows == G[f"{tag}_g{g}_rows"]).all(axis=1)
        assert same[~tied].all(), (tag, g, np.nonzero(~same & ~tied)[0])


def test_rows_respect_max_grad(dp_results):
    for tag, H, W, g in cases():
        rows = dp_results[tag, g][0].astype(np.int64)
        assert rows.min() >= 0 and rows.max() < H
        assert (np.abs(np.diff(rows, axis=1)) <= g).all(), (tag, g)


def test_tie_flag_is_neither_always_true_nor_blind(dp_results):
    """The fixture's seeds are chosen so that the flag has to discriminate.  At least half of the uniform-noise maps are
    untied; a 255 ridge over noise below 200 or over zeros with steps <= 1 is the ONLY zero-cost path for any
    max_grad >= 1, so every such map is untied; a ridge with a step of exactly 3 over zeros cannot be followed with
    max_grad 1 or 2, the detour's cost is a small integer that many detours share, and every such map is tied (the three
    shapes with H >= 12 force such a step; with max_grad >= 3 the ridge is the unique zero-cost path again)."""
    noise = np.concatenate([dp_results[tag, g][2][G[f"{tag}_family"] == FAMILIES.index("noise")] for tag, _, _, g in cases()])
    assert noise.size >= 48 and (~noise).sum() * 2 >= noise.size
    for tag, H, W, g in cases():
        fam, tied = G[f"{tag}_family"], dp_results[tag, g][2]
        for name in ("ridge_noise", "ridge_clean"):
            assert not tied[fam == FAMILIES.index(name)].any(), (tag, g, name)
        jump = fam == FAMILIES.index("ridge_jump3")
        if H >= 12:
            ridge_rows = G[f"{tag}_maps"][jump].argmax(axis=1).astype(np.int64)
            assert (np.abs(np.diff(ridge_rows, axis=1)).max(axis=1) == 3).all()
            if g <= 2:
                assert tied[jump].all(), (tag, g)
            else:
                assert not tied[jump].any(), (tag, g)
    # some tied maps do differ from the reference: the fallback is needed, not decoration
    differ = sum(int(((dp_results[tag, g][0] != G[f"{tag}_g{g}_rows"]).any(axis=1) & dp_results[tag, g][2]).sum())
                 for tag, _, _, g in cases())
    assert differ >= 1


def test_merge_with_host_ties_equals_segment_maps(dp_results):
    """The merge evaluate_model / predict use: untied maps keep the recurrence's rows, tied maps go through the host
    search (an inline SegmentPool here) -- rows and errors equal graph_search.segment_maps on ALL fixture maps."""
    ge.build()
    from oct_image_segmentation_models_amd.min_path_processing import graph_search
    from oct_image_segmentation_models_amd.min_path_processing.device_search import merge_ties
    from oct_image_segmentation_models_amd.min_path_processing.pool import SegmentPool
    assert graph_search._native() is not None, "liboct_minpath.so was not built"
    rng = np.random.default_rng(5)
    for tag, H, W, g in cases():
        maps = G[f"{tag}_maps"]
        n = maps.shape[0]
        rows, _, tied = dp_results[tag, g]
        truths = rng.integers(0, H + 1, (n, 1, W)).astype(np.float64)            # zeros exercise calc_errors' invalid rows
        sent = []
        with SegmentPool((H, W), g, workers=1) as pool:
            def segment(m, t):
                sent.append(m.shape[0])
                return pool.segment(m, t)
            got = merge_ties(maps[:, None], rows[:, None], tied[:, None], truths, segment, "host")
            dev = merge_ties(maps[:, None], rows[:, None], tied[:, None], None, None, "device")     # never calls segment
        assert sum(sent) == int(tied.sum())                                       # the tied maps, and only those
        graph = graph_search.create_graph_structure((W, H), g)
        for i in range(n):
            pred, err, _ = graph_search.segment_maps(np.transpose(maps[i:i + 1], (0, 2, 1)), truths[i], graph)
            assert np.array_equal(pred, G[f"{tag}_g{g}_rows"][i:i + 1])
            assert got[i][0].dtype == np.uint16 and np.array_equal(got[i][0], pred), (tag, g, i)
            assert np.array_equal(got[i][1], err, equal_nan=True), (tag, g, i)
            assert np.array_equal(dev[i][0], rows[i:i + 1]) and not dev[i][1].any()


def test_delineate_dp_rejects_bad_arguments():
    from oct_image_segmentation_models_amd.min_path_processing.device_search import delineate_dp, merge_ties
    m = np.zeros((1, 1, 4, 5), np.uint8)
    for g in (0, 17):
        with pytest.raises(ValueError):
            delineate_dp(m, g)
    with pytest.raises(TypeError):
        delineate_dp(m.astype(np.float64), 1)
    with pytest.raises(ValueError):
        merge_ties(m, np.zeros((1, 1, 5), np.uint16), np.zeros((1, 1), bool), None, None, "heap")


def test_parameter_classes_take_the_new_options():
    import inspect
    from oct_image_segmentation_models_amd.evaluation.evaluation_parameters import EvaluationParameters
    from oct_image_segmentation_models_amd.prediction.prediction_parameters import PredictionParams
    for cls in (EvaluationParameters, PredictionParams):
        p = inspect.signature(cls.__init__).parameters
        assert p["gs_device"].default is False and p["gs_device_ties"].default == "host"
