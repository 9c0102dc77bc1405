"""The step's non-conv kernels at the shapes where their load pipelines can go wrong.

conv_dw_first_k walks its 8 x 128 image tiles with the next tile's image bytes parked in registers and two LDS buffers,
one barrier per tile, and requests a thread's dz / z quads two pixels ahead; head_fwd_k and head_bwd_k keep one chunk
requested ahead of the one in work; dice_finalize_k requests 32 partial rows at a time and hands the focal / BCE slot of
an image to a thread without a (b, c) pair.  conv_first_fwd_k kept its walk but runs the same cases.  What is checked:

* first layer: several tiles per block with unequal counts, a ragged right-hand tile, look-ahead across image boundaries
  and off the end (18 tiles on 4 blocks), one tile per block (cap 32 -- a strider's grid is min(tiles, cap), so this is
  the walk without any look-ahead), one tile in all; u8 and fp32 input, bf16 storage once.  Every stored tensor of the
  step goes through tests/layer_local.py at its own gates, enc0.conv0's z, record, dW and bias among them.
* head: 4 chunks with a ragged last one (nblk = 4: the finalize's tail loops only), 12 chunks (one group of 8 rows and a
  tail), 16 chunks on 16 blocks at B = 1, and B = 300 at 40 x 100 -- head_nblk is min(chunks, ceil(2048 / B)), so a block
  walks several chunks only beyond B = 128: 16 chunks on 7 blocks, 3 or 2 each, the request ahead running past the end.
  Losses against fp64 sums of the stored probabilities (1e-5; DICE_TOL for the coefficients), the head's dW / db and the
  last block's g' against torch-fp64 autograd from the engine's stored z and BN record (GRAD_RTOL on the scale of the
  tensor, elements within fp32 rounding of the ReLU kink excluded as layer_local does), for Dice macro and micro,
  focal-Dice and BCE-Dice, C = 3 and C = 8.
* more (b, c) pairs than threads: B = 33, C = 8, losses only (no idle thread: every owner forms its own slot sum)."""
import numpy as np
import pytest
import torch

from oracle import unet_numpy as on
from oracle import unet_torch as ot
from tests import layer_local as ll
from tests.test_gpu_bce_dice_loss import bce_terms
from tests.test_gpu_layer_local import _finish, _params_from_engine, ragged_scans
from tests.test_gpu_parity import DICE_TOL, GRAD_RTOL, PROB_TOL, data, make, make_bf16

pytestmark = pytest.mark.gpu

FOCAL = (0.35, 2.0)            # focal_loss_weight, gamma


# ---- first layer -------------------------------------------------------------------------------------------------------------

FIRST = [   # B, H, W, pool_layers, cap, storage, fp32 input
    (3, 24, 160, 1, 4, "f32", False), (3, 24, 160, 1, 4, "f32", True), (3, 24, 160, 1, 4, "bf16", False),
    (3, 24, 160, 2, 32, "f32", False), (3, 24, 160, 2, 32, "f32", True),
    (1, 8, 32, 1, 0, "f32", False),
]


@pytest.mark.parametrize("case", FIRST, ids=lambda c: f"{c[0]}x{c[1]}x{c[2]}-p{c[3]}-cap{c[4]}-{c[5]}-{'f32in' if c[6] else 'u8in'}")
def test_first_layer_tile_walk(case):
    import time
    from oct_image_segmentation_models_amd import _hip
    t0 = time.time()
    B, H, W, P, cap, mode, f32in = case
    cfg, eng, _, _ = (make_bf16 if mode == "bf16" else make)(B, H, W, 3, 8, P)
    if cap:
        eng.set_option("persistent_max_blocks", cap)
    tiles = B * ((H + 7) // 8) * ((W + 127) // 128)
    img, lab = ragged_scans(B, H, W, 21, 5)
    lut = (np.arange(256) / 255.0).astype(np.float32)
    x = torch.from_numpy(lut[img] if f32in else img).cuda()
    l = torch.from_numpy(lab[..., 0].copy()).cuda()
    eng.set_dropout_step(3)
    mask = eng.dropout_mask(B).double()
    eng.profile_begin()
    probs, _ = eng.forward(x, training=True, labels=l)
    eng.loss_dice()
    eng.backward(l, macro=True, loss_scale=1.0)
    ents = eng.profile_end()
    at = "unsigned short" if mode == "bf16" else "float"
    ran = {e["kernel"]: e for e in ents}
    assert f"conv_first_fwd_k<{at}>" in ran and f"conv_dw_first_k<{at}>" in ran, sorted(ran)
    # the grid that ran: statistic rows of enc0.conv0's forward finalize = min(tiles, cap, 2048)
    rows = [e["bytes"] / (2 * 8 * 4) for e in ents if e["kernel"] == "bn_fwd_finalize_k" and e["layer"] == "enc0.conv0"]
    assert rows == [min(tiles, cap or tiles)], (rows, tiles, cap)
    p64, _ = _params_from_engine(eng)
    S = ll.engine_stored(eng, B, probs)
    rep = ll.LayerLocal(cfg, p64, S, img, labels=lab[..., 0], dropout_mask=mask, mode=mode,
                        mfma_mode=_hip.get_option("mfma_mode"), device="cuda:0").run()
    assert {"z", "rec.mean", "rec.rstd", "dW", "bias"} <= set(rep.rows["enc0.conv0"]), rep.rows["enc0.conv0"]
    _finish(rep, t0, f"first layer {case}")


# ---- head and Dice finalize --------------------------------------------------------------------------------------------------

def _losses_from_probs(p, labels, C, kind, cw):
    """out4 / out8 of the finalize from fp64 sums of the stored probabilities."""
    y = on.one_hot(labels, C, np.float64)
    out = [on.dice_loss_macro(y, p), on.dice_loss_micro(y, p), on.dice_coef_macro(y, p), on.dice_coef_micro(y, p)]
    if kind == "focal":
        f = on.focal_loss_mean(labels, p, FOCAL[1], cw)
        out += [f, FOCAL[0] * f + (1 - FOCAL[0]) * out[0], FOCAL[0] * f + (1 - FOCAL[0]) * out[1], 0.0]
    if kind == "bce":
        b = float(bce_terms(torch.tensor(y), torch.tensor(p)).mean())
        out += [b, 0.0, b + out[1], 0.0]
    return out


def _check_losses(v, want):
    print("losses", [float(t) for t in v], "fp64", want)
    for j, w in enumerate(want):
        tol = DICE_TOL if j in (2, 3) else 1e-5 * max(1.0, abs(w))
        assert abs(float(v[j]) - w) < tol, (j, float(v[j]), w)


def _head_step(B, H, W, C, P, kind, macro, scale=0.5):
    """One training step; the losses, then head dW / db and the last block's g' against autograd over the head alone."""
    cfg, eng, p64, _ = make(B, H, W, C, 8, P)
    images, labels = data(B, H, W, C, seed=17)
    x = torch.from_numpy(images).cuda(); lab = torch.from_numpy(labels[..., 0].copy()).cuda()
    cw = tuple(0.5 + 0.25 * k for k in range(C))
    if kind == "focal":
        eng.set_focal_dice(FOCAL[0], FOCAL[1], cw)
    if kind == "bce":
        eng.set_bce_dice(True)
    eng.set_dropout_step(3)
    eng.profile_begin()
    probs, _ = eng.forward(x, training=True, labels=lab)
    v = {"dice": eng.loss_dice, "focal": eng.loss_focal_dice, "bce": eng.loss_bce_dice}[kind]().cpu().numpy()
    eng.backward(lab, macro=macro, loss_scale=scale)
    kernels = {e["kernel"] for e in eng.profile_end()}
    assert {f"head_fwd_k<{C},8,float>", f"head_bwd_k<{C},8,float>"} <= kernels, sorted(kernels)
    pst = probs.cpu().numpy().astype(np.float64)
    _check_losses(v, _losses_from_probs(pst, labels, C, kind, cw))
    # the head alone, from the engine's stored z and record of the last block
    li = len(eng.layers) - 2
    z = eng.debug_activation(li, 0)[:B].double().cpu()
    rec = eng.debug_bn_record(li).double().cpu()
    pre = rec[0] * z + rec[1]
    unsure = pre.abs() <= 2 * ll.U32 * ((rec[0] * z).abs() + rec[1].abs())
    act = torch.relu(pre).requires_grad_(True)
    w = torch.tensor(p64[-1]["kernel"].reshape(8, C), requires_grad=True)
    b = torch.tensor(p64[-1]["bias"], requires_grad=True)
    p = torch.softmax(act @ w + b, dim=-1)
    assert float((p.detach() - torch.tensor(pst)).abs().max()) < PROB_TOL
    lt = torch.tensor(labels[..., 0].astype(np.int64))
    y = torch.nn.functional.one_hot(lt, C).double()
    loss = ot.dice_loss(y, p, macro=macro)
    if kind == "focal":
        py = p.gather(-1, lt[..., None])[..., 0]
        foc = (torch.tensor(cw, dtype=torch.float64)[lt] * (1.0 - py) ** FOCAL[1] * -torch.log(py.clamp(on.FOCAL_EPS, 1.0 - on.FOCAL_EPS))).sum() / lt.numel()
        loss = FOCAL[0] * foc + (1.0 - FOCAL[0]) * loss
    if kind == "bce":
        loss = loss + bce_terms(y, p).mean()
    (loss * scale).backward()
    g = eng.grads.double().cpu().numpy()
    hd = eng.layers[-1]
    dw, db = w.grad.numpy().ravel(), b.grad.numpy()
    kscale = np.abs(dw).max()
    e_w = np.abs(g[hd["kernel_off"]:hd["kernel_off"] + dw.size] - dw).max() / kscale
    e_b = np.abs(g[hd["bias_off"]:hd["bias_off"] + C] - db).max() / max(np.abs(db).max(), kscale)
    gm = act.grad * (pre > 0)
    pred = gm if eng.debug_layer_fused(li) else rec[6] * gm + rec[7] * z + rec[8]
    got = eng.debug_activation(li, 1)[:B].double().cpu()
    err = torch.where(unsure, torch.zeros_like(pred), (got - pred).abs())
    e_g = float(err.max() / pred.abs().max())
    print(f"{kind} macro={macro} {B}x{H}x{W} C={C}: head dW err {e_w:.3g}, db err {e_b:.3g}, g' err {e_g:.3g} of the scale "
          f"(GRAD_RTOL {GRAD_RTOL}); {int(unsure.sum())} elements at the ReLU kink excluded")
    assert int(unsure.sum()) <= 1e-4 * unsure.numel()
    assert e_w < GRAD_RTOL and e_b < GRAD_RTOL and e_g < GRAD_RTOL


HEAD = [(3, 24, 40, 2), (3, 48, 64, 2), (1, 40, 100, 2)]
LOSSES = [("dice", True), ("dice", False), ("focal", True), ("focal", False), ("bce", False)]


@pytest.mark.parametrize("C", [3, 8])
@pytest.mark.parametrize("kind,macro", LOSSES, ids=[f"{k}-{'macro' if m else 'micro'}" for k, m in LOSSES])
@pytest.mark.parametrize("shape", HEAD, ids=lambda s: f"{s[0]}x{s[1]}x{s[2]}")
def test_head_chunks(shape, kind, macro, C):
    B, H, W, P = shape
    _head_step(B, H, W, C, P, kind, macro)


@pytest.mark.parametrize("kind,macro,C", [("dice", True, 3), ("focal", False, 8), ("bce", False, 3)])
def test_head_blocks_walk_several_chunks(kind, macro, C):
    """B = 300 at 40 x 100: nblk = ceil(2048 / 300) = 7 < 16 chunks, 3 or 2 chunks per block, the last one ragged."""
    assert min(-(-4000 // 256), -(-2048 // 300)) == 7
    _head_step(300, 40, 100, C, 1, kind, macro)


@pytest.mark.parametrize("kind", ["dice", "focal", "bce"])
def test_more_pairs_than_threads(kind):
    """B = 33, C = 8: 264 (b, c) pairs on 256 threads -- threads 0 .. 7 own two pairs each, and thread 0 two slot sums."""
    B, H, W, C = 33, 8, 32, 8
    cfg, eng, _, _ = make(B, H, W, C, 8, 1)
    images, labels = data(B, H, W, C, seed=23)
    x = torch.from_numpy(images).cuda(); lab = torch.from_numpy(labels[..., 0].copy()).cuda()
    cw = tuple(0.5 + 0.25 * k for k in range(C))
    if kind == "focal":
        eng.set_focal_dice(FOCAL[0], FOCAL[1], cw)
    if kind == "bce":
        eng.set_bce_dice(True)
    eng.set_dropout_step(3)
    probs, _ = eng.forward(x, training=True, labels=lab)
    v = {"dice": eng.loss_dice, "focal": eng.loss_focal_dice, "bce": eng.loss_bce_dice}[kind]().cpu().numpy()
    _check_losses(v, _losses_from_probs(probs.cpu().numpy().astype(np.float64), labels, C, kind, cw))
