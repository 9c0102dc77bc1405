"""GPU tests of the boundary-weighted pixel loss: ``oct_edge_weight_map`` against the numpy restatement
``common.utils.edge_weight_reference`` bit for bit, the per-pixel weights in the three head kernel families
(``oct_unet_set_pixel_weights``) against ``oracle/unet_torch.forward`` in fp64 with the weighted loss differentiated by
autograd, and ``Model.fit`` with ``edge_weight`` against an engine stepped by hand.

The map is defined in integers, so every map comparison is on raw bytes.  The head parity cases reuse the seeds, helpers and
tolerances of tests/test_gpu_masked_loss.py (the map changes the loss, not the forward: the ReLU-margin seeds still hold, and
the margin is re-asserted): 1e-5 on losses, DICE_TOL on the coefficients, GRAD_RTOL through ``check_grads_vs_oracle``."""
import numpy as np
import pytest
import torch

from oracle import unet_numpy as on
from oracle import unet_torch as ot
from tests.helpers import relu_margin
from tests.test_gpu_any_size import _Batches, _cfg, _engine, _scans, _weights
from tests.test_gpu_bce_dice_loss import bce_terms
from tests.test_gpu_many_classes import C9, CLS_CASES, assert_cls_route
from tests.test_gpu_many_classes import make as make_cls
from tests.test_gpu_masked_loss import CASE_B, EPS, FOCAL, IGN, SEED_B, _cw, _make_with, frame_labels, select, step
from tests.test_gpu_parity import DICE_TOL, GRAD_RTOL, PROB_TOL, check_grads_vs_oracle, data, make, make_bf16
from tests.test_gpu_wide_head import SN40_C8, WIDE_CASES, assert_wide_route

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
# the tile of edge_weight_k (csrc/kernels_edge_weight.hpp EW_TH x EW_TW): one block owns 32 rows x 64 columns
TILE_H, TILE_W = 32, 64


def _utils():
    from oct_image_segmentation_models_amd.common import utils
    return utils


def _lut(R, profile="linear", weight=3.0, sigma=None):
    """Distinct values per index (linear in d), so that a wrong distance cannot hide behind an equal weight."""
    return _utils().edge_weight_lut(R, profile, weight, sigma)


def device_map(labels, n_cls, R, lut, out=None):
    from oct_image_segmentation_models_amd import _hip
    lab = torch.from_numpy(np.ascontiguousarray(labels)).to(DEV)
    B, H, W = labels.shape[:3]
    ld = torch.from_numpy(lut).to(DEV)
    out = torch.full((B, H, W), -7.0, dtype=torch.float32, device=DEV) if out is None else out
    _hip.call("oct_edge_weight_map", torch.device(DEV), lab.data_ptr(), B, H, W, n_cls, R, ld.data_ptr(), out.data_ptr(),
              _hip.stream_ptr(torch.device(DEV)))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def layered(B, H, W, n_cls, seed, noise=0.01, frame=(0, 0, 0, 0)):
    """(B,H,W) uint8: ``n_cls`` layers with a wavy border (another phase per image), ``noise`` of the pixels relabelled at
    random, a 255 frame (top, bottom, left, right)."""
    rng = np.random.default_rng(seed)
    y, x = np.arange(H)[None, :, None], np.arange(W)[None, None, :]
    ph = rng.uniform(0, 6.28, (B, 1, 1))
    rows = y + 2.0 * np.sin(x / 5.0 + ph) + rng.uniform(-1, 1, (B, 1, 1))
    lab = np.clip(np.floor(rows * n_cls / H), 0, n_cls - 1).astype(np.uint8)
    flip = rng.random(lab.shape) < noise
    lab[flip] = rng.integers(0, n_cls, int(flip.sum()))
    t, b, l, r = frame
    lab[:, :t] = 255; lab[:, H - b:] = 255; lab[:, :, :l] = 255; lab[:, :, W - r:] = 255
    return lab


def check_map(labels, n_cls, R, general=True, lut=None):
    u = _utils()
    lut = _lut(R) if lut is None else lut
    idx = u.edge_index_reference(labels, n_cls, R)
    if general:       # the reference itself holds an edge pixel, a far pixel and something between: a constant cannot pass
        assert (idx == 0).any() and (idx == R * R + 1).any() and ((idx > 0) & (idx <= R * R)).any(), np.unique(idx)
    want = u.edge_weight_reference(labels, n_cls, R, lut)
    got = device_map(labels, n_cls, R, lut)
    assert got.dtype == np.float32 and got.shape == want.shape
    bad = got.view(np.int32) != want.view(np.int32)
    assert not bad.any(), (int(bad.sum()), np.argwhere(bad)[:5], got[bad][:5], want[bad][:5])
    return idx, got


# ---- the map ----------------------------------------------------------------------------------------------------------------
def test_radius_beyond_the_image():
    check_map(layered(2, 16, 16, 3, 1, noise=0.0), 3, 32, general=False)
    idx, _ = check_map(layered(2, 16, 16, 3, 1, noise=0.0), 3, 32, general=False)
    assert (idx == 0).any() and idx.max() <= 32 * 32          # 16 x 16: nothing is farther than R


@pytest.mark.parametrize("H, W, R", [(20, 34, 3), (36, 68, 7)])
def test_sizes_that_divide_no_tile(H, W, R):
    check_map(layered(2, H, W, 4, 2), 4, R)


def test_edges_across_tile_seams():
    """72 x 136 with R = 5 (both exceed the tile edge + R: 37, 69): single pixels of another class beside the seams at row
    32 / column 64 and row 64 / column 128.  The pixel's own 4-neighbours are edge pixels too, so the edge pixel nearest
    to the seam sits at row 31 / column 63; pixels exactly R across the seam (horizontally, vertically, and by the (4, 3)
    diagonal: 16 + 9 = R^2) are in, one pixel further is far."""
    R, H, W = 5, 72, 136
    assert H > TILE_H + R and W > TILE_W + R
    lab = np.zeros((1, H, W), np.uint8)
    lab[0, 30, 62] = 1
    lab[0, 62, 126] = 2
    idx, _ = check_map(lab, 3, R)
    for y0, x0 in ((30, 62), (62, 126)):
        assert idx[0, y0 + 1, x0] == 0 and idx[0, y0, x0 + 1] == 0
        assert (y0 + 1) % TILE_H == TILE_H - 1 and (x0 + 1) % TILE_W == TILE_W - 1      # the last row / column of a tile
        assert idx[0, y0, x0 + 1 + R] == R * R and idx[0, y0, x0 + 2 + R] == R * R + 1          # horizontally
        assert idx[0, y0 + 1 + R, x0] == R * R and idx[0, y0 + 2 + R, x0] == R * R + 1          # vertically
        assert idx[0, y0 + 1 + 4, x0 + 3] == R * R and idx[0, y0 + 1 + 5, x0 + 4] == R * R + 1  # diagonally, from (y0 + 1, x0)
    # and the other way: sources behind the seam, targets in front of it
    lab = np.zeros((1, H, W), np.uint8)
    lab[0, 33, 65] = 1
    idx, _ = check_map(lab, 3, R)
    assert idx[0, 33, 64] == 0 and idx[0, 32, 65] == 0
    assert idx[0, 33, 64 - R] == R * R and idx[0, 33, 63 - R] == R * R + 1
    assert idx[0, 32 - R, 65] == R * R and idx[0, 31 - R, 65] == R * R + 1
    assert idx[0, 32 - 4, 65 - 3] == R * R and idx[0, 32 - 5, 65 - 4] == R * R + 1


def test_uniform_maps():
    R = 4
    one = np.full((1, 40, 70), 2, np.uint8)                       # a one-class image: all far
    idx, got = check_map(one, 3, R, general=False)
    assert (idx == R * R + 1).all() and (got == 1.0).all()
    yy, xx = np.mgrid[0:40, 0:70]
    board = ((yy + xx) % 2).astype(np.uint8)[None]                # a checkerboard: all edge
    idx, got = check_map(board, 2, R, general=False)
    assert (idx == 0).all() and (got == _lut(R)[0]).all()
    idx, got = check_map(np.full((2, 40, 70), 255, np.uint8), 3, R, general=False)       # nothing known: all 0.0
    assert (idx == -1).all() and (got.view(np.int32) == 0).all()


def test_frame_of_unequal_widths_makes_no_edge():
    lab = layered(2, 44, 75, 3, 3, frame=(5, 3, 4, 9))
    idx, got = check_map(lab, 3, 6)
    assert (got[lab == 255] == 0.0).all() and (idx[lab == 255] == -1).all()
    plain = np.full((1, 30, 40), 1, np.uint8)
    plain[:, :4] = 255; plain[:, :, 33:] = 255                    # one class inside a frame: the frame's border is no edge
    idx, _ = check_map(plain, 3, 6, general=False)
    assert set(np.unique(idx)) == {-1, 37}


def test_edge_pixels_in_the_first_and_last_row_and_column():
    lab = np.zeros((1, 37, 70), np.uint8)
    lab[0, 0, 10] = 1; lab[0, 36, 50] = 1; lab[0, 12, 0] = 2; lab[0, 20, 69] = 2
    idx, _ = check_map(lab, 3, 3)
    assert idx[0, 0, 10] == 0 and idx[0, 36, 50] == 0 and idx[0, 12, 0] == 0 and idx[0, 20, 69] == 0


@pytest.mark.parametrize("n_cls", [2, 16])
def test_class_counts(n_cls):
    lab = layered(1, 48, 80, n_cls, 4)
    lab[0, 5:9, 5:30] = 16                                        # 16 is unknown at both counts (and a class at neither)
    idx, _ = check_map(lab, n_cls, 5)
    assert (idx[lab == 16] == -1).all()


def test_three_different_images_and_a_trailing_axis():
    lab = np.concatenate([layered(1, 36, 68, 3, 5), layered(1, 36, 68, 3, 6, noise=0.05), layered(1, 36, 68, 3, 7, frame=(2, 0, 0, 3))])
    assert not np.array_equal(lab[0], lab[1]) and not np.array_equal(lab[1], lab[2])
    _, got3 = check_map(lab, 3, 7)
    _, got4 = check_map(lab[..., None], 3, 7)                     # (B,H,W,1) as given
    assert np.array_equal(got3.view(np.int32), got4.view(np.int32))
    for b in range(3):                                            # nothing depends on the batch: each image alone
        _, alone = check_map(lab[b:b + 1], 3, 7, general=False)
        assert np.array_equal(alone[0].view(np.int32), got3[b].view(np.int32))


def test_profiles_of_the_training_path():
    lab = layered(2, 40, 72, 3, 8)
    for R, profile, sigma in ((3, "box", None), (15, "gauss", 5.0), (15, "linear", None)):
        check_map(lab, 3, R, general=False, lut=_lut(R, profile, 10.0, sigma))      # (R = 15 leaves nothing far in 40 x 72)


def test_repeats_and_records_into_a_graph():
    from oct_image_segmentation_models_amd import _hip
    first, second = layered(2, 36, 68, 3, 9), layered(2, 36, 68, 3, 10)
    R, lut = 7, _lut(7)
    a, b = device_map(first, 3, R, lut), device_map(first, 3, R, lut)
    assert np.array_equal(a.view(np.int32), b.view(np.int32))
    lab = torch.from_numpy(first).to(DEV); ld = torch.from_numpy(lut).to(DEV)
    out = torch.full((2, 36, 68), -7.0, dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _hip.call("oct_edge_weight_map", torch.device(DEV), lab.data_ptr(), 2, 36, 68, 3, R, ld.data_ptr(), out.data_ptr(),
                  _hip.stream_ptr(torch.device(DEV)))
    for case in (first, second, first):
        lab.copy_(torch.from_numpy(case).to(DEV))
        out.fill_(-7.0)
        graph.replay()
        torch.cuda.synchronize()
        want = _utils().edge_weight_reference(case, 3, R, lut)
        assert np.array_equal(out.cpu().numpy().view(np.int32), want.view(np.int32))


def test_argument_errors():
    from oct_image_segmentation_models_amd import _hip
    lib = _hip.lib()
    lab = torch.zeros((1, 8, 8), dtype=torch.uint8, device=DEV)
    lut = torch.ones(32 * 32 + 2, dtype=torch.float32, device=DEV)
    out = torch.full((1, 8, 8), -7.0, dtype=torch.float32, device=DEV)
    p = lambda t: None if t is None else t.data_ptr()
    call = lambda l, B, H, W, n, R, t, o: lib.oct_edge_weight_map(p(l), B, H, W, n, R, p(t), p(o), None)
    with torch.cuda.device(0):
        for args, word in (((lab, 1, 8, 8, 3, 0, lut, out), "radius"), ((lab, 1, 8, 8, 3, 33, lut, out), "radius"),
                           ((None, 1, 8, 8, 3, 3, lut, out), "null"), ((lab, 1, 8, 8, 3, 3, None, out), "null"),
                           ((lab, 1, 8, 8, 3, 3, lut, None), "null"), ((lab, 0, 8, 8, 3, 3, lut, out), "positive"),
                           ((lab, 1, 8, 0, 3, 3, lut, out), "positive"), ((lab, 1, 8, 8, 0, 3, lut, out), "n_cls"),
                           ((lab, 1, 8, 8, 256, 3, lut, out), "n_cls"), ((lab, 70000, 8, 8, 3, 3, lut, out), "65535"),
                           ((lab, 1, 20000, 8, 3, 3, lut, out), "16384")):
            assert call(*args) < 0 and word in lib.oct_last_error().decode(), (args[1:6], lib.oct_last_error())
    torch.cuda.synchronize()
    assert (out == -7.0).all()                                    # nothing was launched


# ---- the head kernels ---------------------------------------------------------------------------------------------------------
def random_weights(shape, seed):
    """Values in {0} U [0.5, 4]: about one pixel in eight weighs nothing."""
    rng = np.random.default_rng(seed)
    w = rng.uniform(0.5, 4.0, shape).astype(np.float32)
    w[rng.random(shape) < 0.125] = 0.0
    return w


def weighted_loss_t(probs, labels, pw, C, kind, macro, ignore, cw=None, smooth=1e-5):
    """tests/test_gpu_masked_loss.py::masked_loss_t with the per-pixel weight ``pw`` (B,H,W) in the focal / BCE term only; the
    divisor stays the number of counted pixels."""
    lab = torch.as_tensor(labels[..., 0].astype(np.int64))
    keep = (lab != ignore) if ignore is not None else torch.ones_like(lab, dtype=torch.bool)
    m = keep.to(torch.float64)
    safe = torch.where(keep, lab, torch.zeros_like(lab))
    y = torch.nn.functional.one_hot(safe, C).to(torch.float64) * m[..., None]
    pm = probs * m[..., None]
    I = (y * pm).sum(dim=(1, 2)); D = y.sum(dim=(1, 2)) + pm.sum(dim=(1, 2))
    dice = 1.0 - ((2.0 * I + smooth) / (D + smooth)).mean() if macro else 1.0 - (2.0 * I.sum() + smooth) / (D.sum() + smooth)
    inv = 1.0 / float(m.sum())
    wpx = m * torch.as_tensor(pw.astype(np.float64))
    if kind == "focal":
        fw, gamma = FOCAL
        py = torch.gather(probs, -1, safe[..., None])[..., 0]
        wt = torch.ones_like(py) if cw is None else torch.tensor(np.asarray(cw, np.float64))[safe]
        term = (wpx * wt * (1.0 - py) ** gamma * -torch.log(torch.clamp(py, EPS, 1.0 - EPS))).sum() * inv
        return term, fw * term + (1.0 - fw) * dice
    term = (wpx[..., None] * bce_terms(y, probs)).sum() * (inv / C)
    return term, term + dice


def head_parity(case, seed, made, kind, ignore):
    """One training step with a random map against the fp64 oracle: loss vector and every gradient."""
    from oct_image_segmentation_models_amd.common.custom_losses import masked_loss_reference
    B, H, W, C, sn, P, L, ic = case
    cfg, eng, p64, s64 = made
    images, labels = data(B, H, W, C, ic, seed=seed)
    if ignore is not None:
        labels = frame_labels(labels, (2, 1, 3, 2), rects=((0, 6, 9, 10, 20),))
    macro = kind == "focal"
    cw = _cw(C) if kind == "focal" else None
    pw = random_weights((B, H, W), seed + 1)
    assert (pw == 0).any() and pw[pw > 0].min() >= 0.5 and pw.max() <= 4.0
    select(eng, kind, cw)
    eng.set_ignore_label(ignore)
    eng.set_pixel_weights(torch.from_numpy(pw).to(DEV))
    eng.profile_begin()
    probs, v, mask = step(eng, images, labels, kind, macro)
    kernels = {e["kernel"] for e in eng.profile_end()}
    _, cache = on.forward(cfg, p64, s64, on.preprocess_u8(images, np.float64), training=True, dropout_mask=mask)
    assert relu_margin(cfg, p64, cache) > 2e-5
    tp, ts = ot.to_torch(p64, s64, requires_grad=True)
    pr = ot.forward(cfg, tp, ts, torch.tensor(on.preprocess_u8(images, np.float64)), training=True, dropout_mask=torch.tensor(mask))
    term, loss = weighted_loss_t(pr, labels, pw, C, kind, macro, ignore, cw)
    (loss * 0.5).backward()
    grads = [{k: t.grad.numpy() for k, t in p.items()} for p in tp]
    ref = pr.detach().numpy()
    assert np.abs(probs.cpu().numpy() - ref).max() < PROB_TOL
    want = masked_loss_reference(labels, ref, C, ignore, kind, gamma=FOCAL[1], class_weight=cw, focal_loss_weight=FOCAL[0], pixel_weight=pw)
    plain = masked_loss_reference(labels, ref, C, ignore, kind, gamma=FOCAL[1], class_weight=cw, focal_loss_weight=FOCAL[0])
    term, loss = float(term.detach()), float(loss.detach())
    assert abs(term - want["term"]) < 1e-12 and abs(loss - want["loss_macro" if macro else "loss_micro"]) < 1e-12
    assert abs(want["term"] - plain["term"]) > 0.05 * plain["term"]           # the map does change the term
    print(f"{case} {kind} ignore={ignore}: out8 {v.tolist()} want term {term} loss {loss} (unweighted term {plain['term']})")
    # the Dice term and the metrics do not see the map
    assert abs(v[0] - plain["dice_loss_macro"]) < 1e-5 and abs(v[1] - plain["dice_loss_micro"]) < 1e-5
    assert abs(v[2] - plain["dice_coef_macro"]) < DICE_TOL and abs(v[3] - plain["dice_coef_micro"]) < DICE_TOL
    assert abs(v[4] - term) < 1e-5 * max(1.0, term)
    assert abs(v[5 if macro else 6] - loss) < 1e-5 * max(1.0, loss)
    worst = check_grads_vs_oracle(eng, grads)
    print(f"worst gradient piece error {worst:.3g} (GRAD_RTOL {GRAD_RTOL})")
    return kernels


FAMILIES = {
    "register": (CASE_B, SEED_B, lambda c: make(*c, training=True)),
    "channel-streaming": (SN40_C8, WIDE_CASES[SN40_C8], lambda c: make(*c, training=True)),
    "class-streaming": (C9, CLS_CASES[C9], lambda c: make_cls(*c, training=True)),
}


def assert_route(family, kernels, case, at="float"):
    C, sn = case[3], case[4]
    if family == "register":
        assert {f"head_fwd_k<{C},{sn},{at}>", f"head_bwd_k<{C},{sn},{at}>"} <= kernels, sorted(kernels)
    elif family == "channel-streaming":
        assert_wide_route(kernels, C, sn, at)
    else:
        assert_cls_route(kernels, C, sn, at)


@pytest.mark.parametrize("ignore", [None, IGN])
@pytest.mark.parametrize("kind", ["focal", "bce"])
@pytest.mark.parametrize("family", list(FAMILIES))
def test_weighted_step_matches_the_oracle(family, kind, ignore):
    case, seed, maker = FAMILIES[family]
    assert_route(family, head_parity(case, seed, maker(case), kind, ignore), case)


def _bits_of_step(eng, w0, images, labels, kind, macro, weights):
    eng.set_weights(w0)
    eng.set_pixel_weights(weights)
    _, v, _ = step(eng, images, labels, kind, macro)
    return v.copy(), eng.grads.clone().view(torch.int32), eng.state.clone().view(torch.int32)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("family", list(FAMILIES))
def test_ones_twos_and_plain_dice(family, dtype):
    """A map of ones against no map: loss vector, gradients and BN state as raw bytes, for focal (class weights, ignore label
    on) and BCE.  A map of twos: the focal / BCE mean ``out8[4]`` is exactly twice.  Plain Dice with a random map: the bits
    of the off path.  Both storage types."""
    case, seed, _ = FAMILIES[family]
    B, H, W, C, sn, P, L, ic = case
    if family == "class-streaming":
        cfg, eng, _, _ = make_cls(*case, training=True, dtype="bfloat16" if dtype == "bf16" else "float32")
    else:
        cfg, eng, _, _ = (make_bf16 if dtype == "bf16" else make)(B, H, W, C, sn, P, L, ic)
    w0 = eng.get_weights()
    images, labels = data(B, H, W, C, ic, seed=seed)
    framed = frame_labels(labels, (2, 1, 3, 2))
    ones = torch.ones((B, H, W), dtype=torch.float32, device=DEV)
    twos = torch.full((B, H, W), 2.0, dtype=torch.float32, device=DEV)
    rnd = torch.from_numpy(random_weights((B, H, W), 3)).to(DEV)
    for kind, macro, ignore, lab in (("focal", True, IGN, framed), ("focal", False, None, labels), ("bce", False, None, labels),
                                     ("bce", False, IGN, framed)):
        select(eng, kind, _cw(C) if kind == "focal" else None)
        eng.set_ignore_label(ignore)
        off = _bits_of_step(eng, w0, images, lab, kind, macro, None)
        one = _bits_of_step(eng, w0, images, lab, kind, macro, ones)
        assert np.array_equal(off[0].view(np.int32), one[0].view(np.int32)), (kind, off[0], one[0])
        assert torch.equal(off[1], one[1]) and torch.equal(off[2], one[2]), kind
        two = _bits_of_step(eng, w0, images, lab, kind, macro, twos)
        assert off[0][4] > 0 and two[0][4] == np.float32(2.0) * off[0][4], (kind, off[0], two[0])
        assert np.array_equal(two[0][:4].view(np.int32), off[0][:4].view(np.int32))      # the Dice outputs stay
        assert not torch.equal(two[1], off[1])
        eng.profile_begin()
        some = _bits_of_step(eng, w0, images, lab, kind, macro, rnd)
        assert_route(family, {e["kernel"] for e in eng.profile_end()}, case, "unsigned short" if dtype == "bf16" else "float")
        assert some[0][4] != off[0][4] and not torch.equal(some[1], off[1])
    select(eng, "dice")
    eng.set_ignore_label(None)
    off = _bits_of_step(eng, w0, images, labels, "dice", True, None)
    on_ = _bits_of_step(eng, w0, images, labels, "dice", True, rnd)
    assert np.array_equal(off[0].view(np.int32), on_[0].view(np.int32)) and torch.equal(off[1], on_[1]) and torch.equal(off[2], on_[2])


def test_setting_the_map_drops_a_pending_forward():
    from oct_image_segmentation_models_amd._hip import OctError
    case = CASE_B
    B, H, W, C, sn, P, L, ic = case
    cfg, eng, _, _ = make(*case, training=True)
    images, labels = data(B, H, W, C, ic, seed=SEED_B)
    x = torch.from_numpy(images).cuda(); lab = torch.from_numpy(labels[..., 0].copy()).cuda()
    w = torch.ones((B, H, W), dtype=torch.float32, device=DEV)
    eng.set_focal_dice(0.5, 2.0)
    eng.forward(x, training=True, labels=lab)
    eng.set_pixel_weights(w)
    with pytest.raises(OctError, match="forward"):
        eng.loss_focal_dice()
    eng.forward(x, training=True, labels=lab)
    eng.set_pixel_weights(w)                                      # the same map again: nothing is dropped
    eng.loss_focal_dice()
    eng.set_pixel_weights(None)
    with pytest.raises(OctError, match="forward"):
        eng.loss_focal_dice()
    for bad in (torch.ones((B, H, W + 1), dtype=torch.float32, device=DEV), torch.ones((B, H, W), dtype=torch.float64, device=DEV),
                torch.ones((B + 1, H, W), dtype=torch.float32, device=DEV)):
        with pytest.raises(OctError, match="pixel weights"):
            eng.set_pixel_weights(bad)
    assert eng.pixel_weights is None


# ---- the model ------------------------------------------------------------------------------------------------------------------
P3 = dict(pool_layers=3)
SPEC = {"radius": 3, "weight": 10.0, "profile": "gauss", "sigma": 1.5}


def _compiled(cfg, w0, loss_name, **loss_kw):
    from oct_image_segmentation_models_amd import optimizers
    from oct_image_segmentation_models_amd.common import custom_losses, custom_metrics
    from oct_image_segmentation_models_amd.models.engine_model import Model
    m = Model(name="unet", config=dict(cfg, seed=2))
    m.set_weights(w0)
    loss = custom_losses.custom_loss_objects[loss_name]["function"](num_classes=3, is_y_true_sparse=True, **loss_kw)
    metric = custom_metrics.training_monitor_metric_objects["dice_coef_macro"](True, 3)
    m.compile(optimizer=optimizers.Adam(learning_rate=2e-3), loss=loss, metrics=[metric], pad_mode="edge")
    return m


def _by_hand(w0, batches, kind, spec):
    """A native 40 x 72 engine stepped by hand over padded batches: (engine, mean loss vector)."""
    from oct_image_segmentation_models_amd import optimizers
    from oct_image_segmentation_models_amd.common.utils import edge_weight_lut, pad_reference
    native = _engine(_cfg(40, 72, **P3), w0, 2, training=True)
    native.set_ignore_label(IGN)
    if kind == "focal":
        native.set_focal_dice(0.5, 2.0)
    else:
        native.set_bce_dice(True)
    opt = optimizers.Adam(learning_rate=2e-3)
    wbuf = torch.empty((2, 40, 72), dtype=torch.float32, device=DEV)
    acc = None
    for x, lab in batches.items:
        xp = torch.from_numpy(pad_reference(x, 40, 72, 2, 2, "edge", 0)).cuda()
        lp = torch.from_numpy(pad_reference(lab, 40, 72, 2, 2, "constant", IGN)).cuda()
        if spec:
            lut = edge_weight_lut(spec["radius"], spec["profile"], spec["weight"], spec["sigma"])
            native.edge_weight_map(lp, spec["radius"], lut, out=wbuf)
            assert (wbuf[lp[..., 0] == IGN] == 0).all() and float(wbuf.max()) > 2.0
            native.set_pixel_weights(wbuf)
        native.forward(xp, training=True, labels=lp, want_probs=False)
        v = native.loss_focal_dice() if kind == "focal" else native.loss_bce_dice()
        native.backward(lp, macro=kind == "focal", loss_scale=1.0)
        opt.apply(native)
        acc = v.clone() if acc is None else acc + v
    torch.cuda.synchronize()
    return native, (acc / len(batches.items)).cpu().numpy()


@pytest.mark.parametrize("loss_name, kind", [("focal_dice_loss", "focal"), ("bce_dice_loss", "bce")])
def test_fit_with_edge_weight_equals_the_engine_stepped_by_hand(loss_name, kind):
    """``Model.fit`` with ``edge_weight`` for two steps on 36 x 68 padded to 40 x 72 against a native engine stepped by hand
    with ``edge_weight_map`` + ``set_pixel_weights``: parameters, moving statistics and the logged loss, bit for bit.  A
    second model without the keyword on the same engine then gives the bits of an engine that never had a map."""
    cfg = _cfg(32, 64, **P3)
    w0 = _weights(cfg, 5)
    tr = _scans(4, 36, 68, 31)
    model = _compiled(cfg, w0, loss_name, edge_weight=SPEC)
    hist = model.fit(_Batches(*tr, 2), epochs=1, verbose=0)
    torch.cuda.synchronize()
    eng = model._engines["train"]
    assert (eng.cfg.H, eng.cfg.W) == (40, 72) and eng.opt_step == 2 and eng.ignore_label == IGN
    assert eng.pixel_weights is not None and len(eng._edge_maps) == 1 and len(eng._edge_luts) == 1
    native, acc = _by_hand(w0, _Batches(*tr, 2), kind, SPEC)
    at = 5 if kind == "focal" else 6
    assert torch.equal(eng.params, native.params) and torch.equal(eng.state, native.state)
    assert hist.history["loss"][0] == float(acc[at]) and hist.history["dice_coef_macro"][0] == float(acc[2])
    plain_native, plain_acc = _by_hand(w0, _Batches(*tr, 2), kind, None)
    assert not torch.equal(plain_native.params, native.params) and float(plain_acc[at]) != float(acc[at])      # the map matters
    # a model without the keyword on the engine the weighted model left (evaluation: no dropout stream, no optimizer state
    # between the two): the bits of an engine that never had a map
    from oct_image_segmentation_models_amd.common.utils import pad_reference
    other = _compiled(cfg, w0, loss_name)
    eng.set_weights(w0)
    other._engines, other._engine, other._pending_weights = model._engines, eng, None
    va = _Batches(*_scans(2, 36, 68, 32), 2)
    got = other.evaluate(va)
    torch.cuda.synchronize()
    assert other._engine is eng and eng.pixel_weights is None
    fresh = _engine(_cfg(40, 72, **P3), w0, 2, training=True)
    fresh.set_ignore_label(IGN)
    fresh.set_focal_dice(0.5, 2.0) if kind == "focal" else fresh.set_bce_dice(True)
    xv, lv = va.items[0]
    fresh.forward(torch.from_numpy(pad_reference(xv, 40, 72, 2, 2, "edge", 0)).cuda(), training=False,
                  labels=torch.from_numpy(pad_reference(lv, 40, 72, 2, 2, "constant", IGN)).cuda(), want_probs=False)
    vv = (fresh.loss_focal_dice() if kind == "focal" else fresh.loss_bce_dice()).cpu().numpy()
    assert got[0] == float(vv[at]) and got[1] == float(vv[2])
    # ... while the weighted model's own evaluation differs from it
    model._engine = eng
    eng.set_weights(w0)
    assert model.evaluate(va)[0] != got[0] and eng.pixel_weights is not None
