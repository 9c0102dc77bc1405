"""GPU parity tests: the HIP path (through the C ABI) vs the CPU oracle on the same seeded inputs.

Tolerances (north_star): per-pixel probabilities within 1e-4 (fp32 path vs the fp64 oracle on fp32-rounded
weights), Dice within 1e-3; gradients within 2e-4 of the layer's largest gradient entry.
PARITY UNPINNED vs TensorFlow 2.9 itself -- see oracle/unet_numpy.py.
"""
import numpy as np
import pytest
import torch

from oracle import unet_numpy as on
from tests.helpers import dropout_keep_mask, relu_margin, stored_activation_view
# the bf16-mode rounding rules are shared with the full-size layer-local checks
from tests.layer_local import (bf16_dw_operands, bf16_dx_weights, bf16_fwd_operands, bf16_round, bf16_ulp,  # noqa: F401
                               upconv_dx_effective)

pytestmark = pytest.mark.gpu

PROB_TOL = 1e-4
DICE_TOL = 1e-3
GRAD_RTOL = 2e-4


def make(B, H, W, C, sn, P, L=2, in_ch=1, seed=0, training=True, max_batch=None):
    from oct_image_segmentation_models_amd.engine import UNetEngine
    cfg = on.UNetConfig(input_channels=in_ch, num_classes=C, start_neurons=sn, pool_layers=P, conv_layers=L)
    params, state = on.init_params(cfg, seed=seed, dtype=np.float32, randomize_bn=True)
    eng = UNetEngine(device="cuda:0", input_channels=in_ch, num_classes=C, image_height=H, image_width=W,
                     start_neurons=sn, pool_layers=P, conv_layers=L, max_batch=max_batch or B, training=training,
                     seed=seed + 100)
    eng.set_weights(on.keras_weight_list(params, state))
    p64 = [{k: v.astype(np.float64) for k, v in p.items()} for p in params]
    s64 = [{k: v.astype(np.float64) for k, v in s.items()} for s in state]
    return cfg, eng, p64, s64


def data(B, H, W, C, in_ch=1, seed=5):
    images, labels = on.synth_scans(B, H, W, C, seed=seed)
    if in_ch > 1:
        rng = np.random.default_rng(seed)
        images = rng.integers(0, 256, (B, H, W, in_ch)).astype(np.uint8)
    return images, labels


CASES = [
    # B, H, W, C, sn, P, L, in_ch
    (2, 32, 64, 3, 8, 2, 2, 1),
    (3, 16, 32, 4, 4, 2, 2, 1),
    (1, 48, 80, 3, 8, 3, 1, 3),     # ragged tiles (48x80 not multiples of the 8x32 thread tile), 3 input channels
    (1, 32, 64, 2, 16, 1, 3, 1),
    (1, 32, 64, 3, 8, 2, 2, 4),     # 4 input channels: the first layer's dW must take the image-typed (uint8 / f32) VALU path
    (1, 32, 64, 3, 32, 1, 2, 1),    # start_neurons 32: every conv but the first on the wide kernels, 32-channel head
    (1, 32, 64, 3, 12, 2, 2, 1),    # start_neurons 12 (12/24/48 channels): nothing divides by 8 or 32 -> the generic kernels
    # ragged geometries with conv_layers = 2: every kernel tiles pixels 32 wide and 4 / 8 / 16 rows high (8 x 64 for the
    # pixel-pair and VALU thin kernels); none of the sizes below divides them at any level
    (2, 36, 68, 3, 8, 2, 2, 1),     # 36x68, 18x34, 9x17: ragged 8 -> 8 layers (fused backward-weights, two-pixel form), odd bottleneck
    (1, 48, 80, 3, 8, 4, 2, 1),     # default depth: the 64- and 128-channel wide kernels on 6x10 and 3x5 images, up-conv backward from 3x5
    (3, 16, 16, 3, 8, 4, 2, 1),     # smallest legal image: 1x1 bottleneck (BN statistics over 3 values), W < 32 at every level
    (1, 80, 24, 3, 16, 2, 2, 1),    # tall and narrow: widths 24, 12, 6; start_neurons 16
    (2, 20, 34, 3, 4, 1, 2, 1),     # 8 -> 8 bottleneck 17 wide: the two-pixel form meets an odd width; 4-channel layers on the generic kernels
]
RAGGED = CASES[7:]
# Data seeds (found offline with the oracle alone) for which every BN pre-activation of the training
# forward stays > 2e-5 away from the ReLU kink: fp32-vs-fp64 rounding then cannot flip a ReLU mask, so the
# gradient comparison can use tight tolerances.  The margin is re-asserted inside the test.
# Margins of the ragged cases: 2.13e-5, 4.06e-5, 3.7e-5, 2.56e-5, 6.1e-5 (CASES[8]: tools/find_margin_seed.py over seeds 1 .. 12000).
# 2e-5 is not a guarantee for every variant: at |a z| of about 9 the "bt_one_px" summation order flipped the ReLU of an
# element 2.33e-5 from the kink (48x80 P=4, dec3.up), so prefer a seed with a wider margin where the search finds one.
MARGIN_SEED = {CASES[0]: 97, CASES[1]: 13, CASES[2]: 28, CASES[3]: 75, CASES[4]: 3, CASES[5]: 72, CASES[6]: 58,
               CASES[7]: 308, CASES[8]: 2743, CASES[9]: 2, CASES[10]: 38, CASES[11]: 2}   # tools/find_margin_seed.py
DROP_STEP = 3


@pytest.fixture(params=["tile_per_block", "persistent", "thin8_valu", "pair8_mfma", "pair8_mfma_111", "dw16_padded",
                        "bx_tall", "bx_tall_w4", "f32_pipe", "dwbt_all", "bt_one_px", "bn_apply_separate",
                        "bn_finalize_in_launch", "bx_one_block", "dw_thin_separate", "bn_apply16_separate", "fork_marker_grouped", "no_side_stream"])
def variant(request):
    """Run the same verified inputs through every conv kernel variant: for the thin layers the persistent
    software-pipelined, VALU and pixel-pair MFMA kernels (otherwise only chosen on large grids); for the wide layers the
    bf16-pipe split-product kernels with the short pixel tiles (default on these small grids), with the tall tiles
    ("bx_tall": tiles larger than the image, ragged everywhere) and the fp32-pipe kernels ("f32_pipe": mfma_mode 0)."""
    from oct_image_segmentation_models_amd import _hip
    v = request.param
    _hip.set_option("bx_min_blocks", 1 if v.startswith("bx_tall") else 256)
    _hip.set_option("bx_waves", 4 if v == "bx_tall_w4" else 8)
    # wide launches: one-image 4-wave blocks, two per CU (default) / the 8-wave double-buffered blocks, also in their tall-tile forms
    _hip.set_option("bx_two_blocks", 0 if v in ("bx_one_block", "bx_tall", "bx_tall_w4") else 1)
    _hip.set_option("mfma_mode", 0 if v == "f32_pipe" else 1)
    _hip.set_option("dwbt_f32_all", 1 if v == "dwbt_all" else 0)     # fp32 mode: every thin dW shape on the bf16 pipe
    _hip.set_option("bt_m2", 0 if v == "bt_one_px" else 1)           # thin kernel: 8-channel launches without the two-pixel form
    _hip.set_option("fuse_first_apply", 0 if v == "bn_apply_separate" else 1)   # bn_bwd_apply as its own pass: block 0 ...
    _hip.set_option("fuse_bn_apply", 0 if v == "bn_apply_separate" else 1)      # ... and every other block
    _hip.set_option("fuse_bn_finalize", 1 if v == "bn_finalize_in_launch" else 0)   # thin layers' BN records written by the last block of the producing launch
    _hip.set_option("fuse_dw_thin", 0 if v == "dw_thin_separate" else 1)   # 8-channel 3x3 layers: backward-weights as their own kernel
    _hip.set_option("fuse_bn_apply16", 0 if v == "bn_apply16_separate" else 1)   # 16 -> 16 thin layers: transform as its own pass
    # side-stream forks as recorded markers with a system fence, three blocks' backward-weights launches per fork
    _hip.set_option("fork_on_launch", 0 if v == "fork_marker_grouped" else 1)
    _hip.set_option("event_sysfence", 1 if v == "fork_marker_grouped" else 0)
    _hip.set_option("dw_fork_group", 3 if v == "fork_marker_grouped" else 1)
    _hip.set_option("dw_side_stream", 0 if v == "no_side_stream" else 1)       # everything on the caller's stream
    _hip.set_option("igemm_persistent_min_tiles", 1 if v == "persistent" else 1 << 30)
    _hip.set_option("thin8_min_tiles", 1 if v == "thin8_valu" or v.startswith("pair8") else 1 << 30)
    _hip.set_option("pair8_min_tiles", 1 if v.startswith("pair8") else 1 << 30)
    _hip.set_option("pair8_geometry", int(v[-3:]) if v[-3:].isdigit() else 221)
    _hip.set_option("dwpair8_enable", 0 if v == "dw16_padded" else 1)
    yield v
    _hip.set_option("bx_min_blocks", 256)
    _hip.set_option("bx_waves", 8)
    _hip.set_option("bx_two_blocks", 1)
    _hip.set_option("mfma_mode", 1)
    _hip.set_option("dwbt_f32_all", 0)
    _hip.set_option("bt_m2", 1)
    _hip.set_option("fuse_first_apply", 1)
    _hip.set_option("fuse_bn_apply", 1)
    _hip.set_option("fuse_bn_finalize", 0)
    _hip.set_option("fuse_dw_thin", 1)
    _hip.set_option("fuse_bn_apply16", 1)
    _hip.set_option("fork_on_launch", 1)
    _hip.set_option("event_sysfence", 0)
    _hip.set_option("dw_fork_group", 1)
    _hip.set_option("dw_side_stream", 1)
    _hip.set_option("dwpair8_enable", 1)
    _hip.set_option("igemm_persistent_min_tiles", 2048)
    _hip.set_option("thin8_min_tiles", 2048)
    _hip.set_option("pair8_min_tiles", 2048)
    _hip.set_option("pair8_geometry", 221)


# the variants under which the ragged cases assert, from the profile of the step itself, that the intricate edge code ran on
# them: the default routing at these grid sizes, and one variant that forces the thin-layer choices
PROFILED = ("tile_per_block", "thin8_valu")


def check_ragged_routing(case, variant, ents, training):
    """The ragged geometries reach what they were added for (asserted, not assumed): a conv_bt_k instantiation that also
    reduces the backward-weights (",dw>") on the 8 -> 8 3x3 layers of the start_neurons-8 cases, and the two-pixel form
    (",2px") on the 17-wide 8 -> 8 bottleneck of the last case, in its forward and its backward-data launch."""
    B, H, W, C, sn, P, L, ic = case
    bt = [(e["kernel"], e["layer"]) for e in ents if e["kernel"].startswith("conv_bt_k<")]
    if training and sn == 8:
        fused = {l for k, l in bt if k.endswith(",dw>")}
        assert {"enc0.conv1", f"dec{P - 1}.conv0", f"dec{P - 1}.conv1"} <= fused, (fused, bt)
    if case == CASES[11]:
        two = [k for k, l in bt if ",2px" in k and l == "mid.conv1"]              # conv_bt_k<KH,AMODE,EPI,...>: EPI 0 is the forward
        assert any(k.split(",")[2] == "0" for k in two), bt
        assert not training or any(k.split(",")[2] != "0" for k in two), bt


@pytest.mark.parametrize("case", CASES)
def test_inference_forward_matches_oracle(case, variant):
    B, H, W, C, sn, P, L, ic = case
    cfg, eng, p64, s64 = make(B, H, W, C, sn, P, L, ic, training=False)
    images, labels = data(B, H, W, C, ic)
    x = torch.from_numpy(images).cuda()
    profiled = case in RAGGED and variant in PROFILED
    if profiled:
        eng.profile_begin()
    probs, am = eng.forward(x, training=False, want_argmax=True)
    if profiled:
        check_ragged_routing(case, variant, eng.profile_end(), training=False)
    ref, cache = on.forward(cfg, p64, s64, on.preprocess_u8(images, np.float64), training=False)
    # layer-wise first: names the first diverging layer
    for li, spec in enumerate(on.build_plan(cfg)[:-1]):
        z = eng.debug_activation(li, 0)[:B].cpu().numpy()
        scale = max(1.0, np.abs(cache[li]["z"]).max())
        assert np.abs(z - cache[li]["z"]).max() / scale < 1e-4, f"layer {li} {spec.name} pre-BN output differs"
    assert np.abs(probs.cpu().numpy() - ref).max() < PROB_TOL
    ref_am = ref.argmax(-1)
    # identical argmax except at numerical ties
    diff = am.cpu().numpy() != ref_am
    if diff.any():
        srt = np.sort(ref, -1)
        assert (srt[..., -1] - srt[..., -2])[diff].max() < 1e-4
    # float32 input path gives the same result as the u8 path
    xf = torch.from_numpy(on.preprocess_u8(images, np.float32)).cuda()
    probs_f, _ = eng.forward(xf, training=False)
    assert torch.equal(probs_f, probs)


def training_step_vs_oracle(cfg, eng, p64, s64, case, images, labels, macro, variant):
    """One training step of ``eng`` on the case's own B images (the engine's max_batch may be larger) against the fp64
    oracle: layer-wise z, probabilities, the four loss values, layer-wise dz, every gradient piece, the moving
    statistics.  Returns (probabilities, loss vector) of the step."""
    B, H, W, C, sn, P, L, ic = case
    assert images.shape[0] == B
    x = torch.from_numpy(images).cuda()
    lab = torch.from_numpy(labels[..., 0].copy()).cuda()
    eng.set_dropout_step(DROP_STEP)
    mask = eng.dropout_mask(B).cpu().numpy()
    # the device dropout stream is the documented counter hash (seed = engine seed, step, element index)
    assert np.array_equal(mask, dropout_keep_mask(100, DROP_STEP, mask.shape).astype(np.uint8))
    mask = mask.astype(np.float64)
    assert 0.3 < mask.mean() < 0.7
    profiled = case in RAGGED and variant in PROFILED
    if profiled:
        eng.profile_begin()
    probs, _ = eng.forward(x, training=True, labels=lab)
    loss4_dev = eng.loss_dice()
    loss4 = loss4_dev.cpu().numpy()
    eng.backward(lab, macro=macro, loss_scale=0.5)
    torch.cuda.synchronize()
    if profiled:
        check_ragged_routing(case, variant, eng.profile_end(), training=True)

    xin = on.preprocess_u8(images, np.float64)
    ref, cache = on.forward(cfg, p64, s64, xin, training=True, dropout_mask=mask)
    assert relu_margin(cfg, p64, cache) > 2e-5, "test input lost its ReLU margin; re-run the seed search"
    plan = on.build_plan(cfg)
    worst = {"z": 0.0, "dz": 0.0}                       # worst err / bound per gate, printed at the end
    for li, spec in enumerate(plan[:-1]):
        z = eng.debug_activation(li, 0)[:B].cpu().numpy()
        scale = max(1.0, np.abs(cache[li]["z"]).max())
        worst["z"] = max(worst["z"], np.abs(z - cache[li]["z"]).max() / scale / 1e-4)
        assert np.abs(z - cache[li]["z"]).max() / scale < 1e-4, f"layer {li} {spec.name} pre-BN output differs"
    worst["probs"] = np.abs(probs.cpu().numpy() - ref).max() / PROB_TOL
    assert np.abs(probs.cpu().numpy() - ref).max() < PROB_TOL

    y = on.one_hot(labels, C, np.float64)
    assert abs(loss4[0] - on.dice_loss_macro(y, ref)) < 1e-5
    assert abs(loss4[1] - on.dice_loss_micro(y, ref)) < 1e-5
    assert abs(loss4[2] - on.dice_coef_macro(y, ref)) < DICE_TOL
    assert abs(loss4[3] - on.dice_coef_micro(y, ref)) < DICE_TOL

    loss, grads = on.backward(cfg, p64, cache, labels, macro=macro, loss_scale=0.5)
    # layer-wise dz from the last block backwards.  On the default route the BN-backward transform is applied by the
    # consumers of dz while they stage it and the buffer keeps the masked gradient g': debug_dz then forms
    # ga g' + gb z + gd from the stored tensors and the record's rows, which pins g', the coefficients and (through the
    # kernel / bias gradients below) what the stagers made of them; in the "bn_apply_separate" variant it is the buffer.
    n_fused = 0
    for li in range(len(plan) - 2, -1, -1):
        n_fused += eng.debug_layer_fused(li)
        dz = eng.debug_dz(li)[:B].cpu().numpy()
        ref_dz = cache[li]["dz"]
        scale = np.abs(ref_dz).max()
        worst["dz"] = max(worst["dz"], np.abs(dz - ref_dz).max() / scale / 5e-4)
        assert np.abs(dz - ref_dz).max() / scale < 5e-4, f"layer {li} {plan[li].name} dz differs"
    if variant == "bn_apply_separate":
        assert n_fused == 0
    elif variant == "f32_pipe":
        assert n_fused <= 1                               # (block 0's streaming backward-weights kernel is not an MFMA kernel)
    elif sn == 8 and ic == 1:
        # (every block but those behind the thin kernel's instantiations that would spill: 32 K channels, 16 K with 16 outputs)
        assert n_fused >= 4, n_fused
    worst["grads"] = check_grads_vs_oracle(eng, grads) / GRAD_RTOL

    # moving statistics (Bessel-corrected variance, momentum 0.99)
    new_state = on.flatten_state(on.updated_moving_stats(cfg, s64, cache))
    worst["state"] = np.abs(eng.state.cpu().numpy() - new_state).max() / 1e-5
    assert np.abs(eng.state.cpu().numpy() - new_state).max() < 1e-5
    worst["loss"] = max(abs(loss4[0] - on.dice_loss_macro(y, ref)), abs(loss4[1] - on.dice_loss_micro(y, ref))) / 1e-5
    print("worst err / bound:", ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    return probs, loss4_dev


def check_grads_vs_oracle(eng, grads):
    """Every gradient piece of every layer within GRAD_RTOL of the oracle's, on the scale of the piece; returns the
    worst relative error."""
    g = eng.grads.cpu().numpy()
    worst = 0.0
    for L_, gr in zip(eng.layers, grads):
        n = L_["kh"] * L_["kw"] * L_["cin"] * L_["cout"]; c = L_["cout"]
        pieces = [("kernel", L_["kernel_off"], n), ("bias", L_["bias_off"], c)]
        if L_["has_bn"]:
            pieces += [("gamma", L_["gamma_off"], c), ("beta", L_["beta_off"], c)]
        kscale = np.abs(gr["kernel"]).max()
        for key, off, cnt in pieces:
            refv = gr[key].ravel()
            # a conv bias ahead of a BN has an analytically zero gradient: judge it on the kernel's scale
            scale = max(np.abs(refv).max(), kscale if key == "bias" else 0.0, 1e-12)
            err = np.abs(g[off:off + cnt] - refv).max() / scale
            worst = max(worst, err)
            assert err < GRAD_RTOL, f"{L_['name']}.{key}: rel err {err}"
    return worst


@pytest.mark.parametrize("macro", [True, False])
@pytest.mark.parametrize("case", CASES)
def test_training_step_matches_oracle(case, macro, variant):
    B, H, W, C, sn, P, L, ic = case
    cfg, eng, p64, s64 = make(B, H, W, C, sn, P, L, ic, training=True)
    images, labels = data(B, H, W, C, ic, seed=MARGIN_SEED[case])
    training_step_vs_oracle(cfg, eng, p64, s64, case, images, labels, macro, variant)


GRAD_SENTINEL = 1e30


def dirty_engine(eng, B, seed, scale=64.0):
    """Make ``eng`` a USED engine before a step at B < max_batch: one full training step at max_batch on other scans
    (fed as float32, scaled up so that every stale row is large), then NaN in the tail rows [B:max_batch] of every
    layer's z and gradient buffer and a large finite sentinel in every gradient float.  The caller restores the weights
    (set_weights: parameters and moving statistics) afterwards."""
    mb, H, W, ic, C = eng.cfg.max_batch, eng.cfg.H, eng.cfg.W, eng.cfg.in_ch, eng.cfg.n_cls
    assert B < mb
    images, labels = data(mb, H, W, C, ic, seed=seed)
    x = torch.from_numpy(on.preprocess_u8(images, np.float32) * np.float32(scale)).cuda()
    lab = torch.from_numpy(labels[..., 0].copy()).cuda()
    eng.set_dropout_step(DROP_STEP + 1)
    eng.forward(x, training=True, labels=lab, want_probs=False)
    eng.loss_dice()
    eng.backward(lab, macro=True)
    torch.cuda.synchronize()
    nb = len(eng.layers) - 1
    for li in range(nb):
        for which in (0, 1):
            v = stored_activation_view(eng, li, which)
            assert bool((v[B:].float() != 0).any()), (li, which)     # the full step really left something behind
            v[B:] = float("nan")
    eng.grads.fill_(GRAD_SENTINEL)


def assert_tails_untouched(eng, B):
    """The NaN tails written by dirty_engine are still NaN everywhere (nothing wrote past image B - 1) and backward filled
    the whole gradient buffer."""
    for li in range(len(eng.layers) - 1):
        for which in (0, 1):
            assert bool(torch.isnan(stored_activation_view(eng, li, which)[B:]).all()), \
                f"{eng.layers[li]['name']} {'zg'[which]} buffer: rows past image {B - 1} were written"
    g = eng.grads
    assert bool(torch.isfinite(g).all())
    assert not bool((g.abs() >= 1e-3 * GRAD_SENTINEL).any()), "a gradient float still holds (part of) the sentinel"


def assert_same_as_fresh_engine(eng, fresh, B, probs, probs_f, loss4, loss4_f):
    """The partial step on the used engine against the same step on an engine created with max_batch = B: bit for bit."""
    for li, L_ in enumerate(eng.layers[:-1]):
        assert torch.equal(stored_activation_view(eng, li, 0)[:B], stored_activation_view(fresh, li, 0)[:B]), f"{L_['name']} z"
        assert torch.equal(eng.debug_bn_record(li), fresh.debug_bn_record(li)), f"{L_['name']} BN record"
    assert torch.equal(probs, probs_f) and torch.equal(loss4, loss4_f) and torch.equal(eng.state, fresh.state)
    # the backward-weights plan of a launch (kernel family, channel chunks, number of partial slabs) is a function of the
    # call's B; the slab count is only clamped by the rows allocated for max_batch, which are never fewer: same launches,
    # same summation order, equal gradients
    for L_ in eng.layers:
        lo, hi = L_["kernel_off"], (L_["beta_off"] if L_["has_bn"] else L_["bias_off"]) + L_["cout"]
        assert torch.equal(eng.grads[lo:hi], fresh.grads[lo:hi]), f"{L_['name']} gradients"


# (case, macro, max_batch): max_batch = B + 1 with the macro loss, 4 B with the micro loss, and one B = 1 step on an
# engine for 3 -- the committed margin seeds stay valid (the margin is a property of the B images and the (B, ...)
# dropout mask, not of max_batch)
PARTIAL = [(c, True, c[0] + 1) for c in CASES[:7]] + [(c, False, 4 * c[0]) for c in CASES[:7]] + [(CASES[5], True, 3)]
PARTIAL += [(c, True, c[0] + 1) for c in RAGGED] + [(c, False, 4 * c[0]) for c in RAGGED]     # (appended: the ids above stay)


@pytest.mark.parametrize("case,macro,max_batch", PARTIAL)
def test_partial_training_step_on_a_used_engine(case, macro, max_batch, variant):
    """A batch smaller than max_batch on an engine that has already run a full one (the ragged last batch of an epoch,
    a smaller validation batch, predict after fit: Model._ensure_engine reuses the engine).  The workspace is carved for
    max_batch and still holds the larger step; every launch must size itself by the call's B."""
    B, H, W, C, sn, P, L, ic = case
    cfg, eng, p64, s64 = make(B, H, W, C, sn, P, L, ic, training=True, max_batch=max_batch)
    weights = eng.get_weights()
    dirty_engine(eng, B, seed=MARGIN_SEED[case] + 1000)
    eng.set_weights(weights)
    images, labels = data(B, H, W, C, ic, seed=MARGIN_SEED[case])
    probs, loss4 = training_step_vs_oracle(cfg, eng, p64, s64, case, images, labels, macro, variant)
    assert bool(torch.isfinite(probs).all()) and bool(torch.isfinite(loss4).all()) and bool(torch.isfinite(eng.state).all())
    assert_tails_untouched(eng, B)

    # the same step on a fresh engine created with max_batch = B
    _, fresh, _, _ = make(B, H, W, C, sn, P, L, ic, training=True)
    x = torch.from_numpy(images).cuda(); lab = torch.from_numpy(labels[..., 0].copy()).cuda()
    fresh.set_dropout_step(DROP_STEP)
    probs_f, _ = fresh.forward(x, training=True, labels=lab)
    loss4_f = fresh.loss_dice()
    fresh.backward(lab, macro=macro, loss_scale=0.5)
    torch.cuda.synchronize()
    assert_same_as_fresh_engine(eng, fresh, B, probs, probs_f, loss4, loss4_f)

    # the validation path of Model._run_epoch on the same used training engine: inference forward with labels + Dice
    pv, _ = eng.forward(x, training=False, labels=lab)
    lv = eng.loss_dice().cpu().numpy()
    s_new = on.unflatten_state(cfg, eng.state.cpu().numpy().astype(np.float64))
    ref_v, _ = on.forward(cfg, p64, s_new, on.preprocess_u8(images, np.float64), training=False)
    assert np.abs(pv.cpu().numpy() - ref_v).max() < PROB_TOL
    y = on.one_hot(labels, C, np.float64)
    assert abs(lv[0] - on.dice_loss_macro(y, ref_v)) < 1e-5 and abs(lv[1] - on.dice_loss_micro(y, ref_v)) < 1e-5
    assert abs(lv[2] - on.dice_coef_macro(y, ref_v)) < DICE_TOL and abs(lv[3] - on.dice_coef_micro(y, ref_v)) < DICE_TOL
    for li in range(len(eng.layers) - 1):
        assert bool(torch.isnan(stored_activation_view(eng, li, 0)[B:]).all()), f"{eng.layers[li]['name']}: validation forward wrote past image {B - 1}"


def test_adam_and_sgd_steps_match_keras_formulas():
    B, H, W, C = 2, 32, 64, 3
    cfg, eng, p64, s64 = make(B, H, W, C, 8, 2)
    images, labels = data(B, H, W, C)
    x = torch.from_numpy(images).cuda(); lab = torch.from_numpy(labels[..., 0].copy()).cuda()
    theta = eng.params.cpu().numpy().astype(np.float64)
    m = np.zeros_like(theta); v = np.zeros_like(theta)
    for t in (1, 2, 3):
        eng.forward(x, training=True, labels=lab, want_probs=False)
        eng.loss_dice(); eng.backward(lab)
        g = eng.grads.cpu().numpy().astype(np.float64)
        eng.adam_step(lr=1e-3)
        theta, m, v = on.adam_step(theta, g, m, v, t)
        assert np.abs(eng.params.cpu().numpy() - theta).max() < 2e-6
    mom = np.zeros_like(theta)
    for _ in range(2):
        eng.forward(x, training=True, labels=lab, want_probs=False)
        eng.loss_dice(); eng.backward(lab)
        g = eng.grads.cpu().numpy().astype(np.float64)
        theta = eng.params.cpu().numpy().astype(np.float64)
        eng.sgd_step(lr=0.05, momentum=0.9)
        theta, mom = on.sgd_step(theta, g, mom, lr=0.05, momentum=0.9)
        assert np.abs(eng.params.cpu().numpy() - theta).max() < 2e-6


def test_training_reduces_loss_and_eval_mode_uses_moving_stats():
    B, H, W, C = 4, 32, 64, 3
    cfg, eng, _, _ = make(B, H, W, C, 8, 2, seed=1)
    images, labels = data(B, H, W, C, seed=2)
    x = torch.from_numpy(images).cuda(); lab = torch.from_numpy(labels[..., 0].copy()).cuda()
    losses = []
    for it in range(60):
        eng.set_dropout_step(it)
        eng.forward(x, training=True, labels=lab, want_probs=False)
        losses.append(eng.loss_dice()); eng.backward(lab); eng.adam_step(lr=5e-3)
    losses = torch.stack(losses).cpu().numpy()
    assert losses[-1, 0] < 0.6 * losses[0, 0], losses[:, 0]
    assert np.isfinite(eng.params.cpu().numpy()).all()


def test_partial_batch_and_graph_replay():
    B, H, W, C = 4, 32, 64, 3
    cfg, eng, p64, s64 = make(B, H, W, C, 8, 2, training=False, max_batch=B)
    images, _ = data(B, H, W, C)
    x = torch.from_numpy(images).cuda()
    full, _ = eng.forward(x, training=False)
    part, _ = eng.forward(x[:3].contiguous(), training=False)
    assert torch.equal(part, full[:3])  # per-scan results independent of batch composition in inference
    xb = x.clone()
    gp, gam = eng.graph_capture(xb, want_probs=True, want_argmax=True)
    eng.graph_launch(); torch.cuda.synchronize()
    assert torch.equal(gp, full) and torch.equal(gam.long(), full.argmax(-1))
    xb.copy_(torch.flip(x, dims=[0])); eng.graph_launch(); torch.cuda.synchronize()
    assert torch.equal(gp, torch.flip(full, dims=[0]))


def test_api_errors_are_loud():
    from oct_image_segmentation_models_amd._hip import OctError
    cfg, eng, _, _ = make(2, 32, 64, 3, 8, 2, training=False)
    x = torch.zeros((2, 32, 64, 1), dtype=torch.uint8, device="cuda")
    with pytest.raises(OctError):
        eng.forward(x, training=True)               # no training workspaces
    with pytest.raises(OctError):
        eng.forward(torch.zeros((3, 32, 64, 1), dtype=torch.uint8, device="cuda"))  # B > max_batch
    with pytest.raises(OctError):
        eng.forward(x.cpu())
    eng.forward(x)
    with pytest.raises(OctError):
        eng.loss_dice()                              # forward had no labels


def test_full_size_properties_config2():
    """BASELINE config[1] shape (256x512, P=4, C=3): size-independent properties at full size --
    probabilities sum to 1, batch-composition independence in inference, per-scan linearity of the
    macro-Dice batch loss (mean of single-scan losses), gradient buffer finite and non-trivial."""
    B, H, W, C = 4, 256, 512, 3
    cfg, eng, _, _ = make(B, H, W, C, 8, 4, training=True)
    images, labels = data(B, H, W, C, seed=9)
    x = torch.from_numpy(images).cuda(); lab = torch.from_numpy(labels[..., 0].copy()).cuda()
    probs, am = eng.forward(x, training=False, labels=lab, want_argmax=True)
    l_all = eng.loss_dice().cpu().numpy()
    assert torch.allclose(probs.sum(-1), torch.ones_like(probs[..., 0]), atol=1e-5)
    assert torch.equal(am.long(), probs.argmax(-1))
    singles = []
    for i in range(B):
        pi, _ = eng.forward(x[i:i + 1].contiguous(), training=False, labels=lab[i:i + 1].contiguous())
        # kernel variants are chosen by grid size, so batch-1 and batch-4 runs may differ in the last bits
        assert torch.allclose(pi[0], probs[i], atol=1e-6, rtol=0)
        singles.append(eng.loss_dice().cpu().numpy())
    assert abs(np.mean([s[0] for s in singles]) - l_all[0]) < 1e-6
    eng.forward(x, training=True, labels=lab, want_probs=False)
    eng.loss_dice(); eng.backward(lab)
    g = eng.grads.cpu().numpy()
    assert np.isfinite(g).all() and np.abs(g).max() > 1e-6


def test_config3_shape_runs_in_fp32():
    """BASELINE configs[2] shape (512x1024x1, pool_layers=5) in fp32 mode: a few training steps + inference at a
    reduced batch; finite, normalised, learning.  (The bf16-storage mode of that config: test_bf16_* below.)"""
    import ctypes
    from oct_image_segmentation_models_amd import _hip
    from oct_image_segmentation_models_amd.engine import UNetEngine, make_cfg
    B, H, W, C = 2, 512, 1024, 3
    # the full configuration (batch 64) is accepted by the config check
    make_cfg(input_channels=1, num_classes=3, image_height=H, image_width=W, pool_layers=5, max_batch=64, training=True)
    eng = UNetEngine(device="cuda:0", input_channels=1, num_classes=C, image_height=H, image_width=W, pool_layers=5,
                     max_batch=B, training=True, seed=3)
    assert eng.n_params == 1948267
    images, labels = data(B, H, W, C, seed=4)
    x = torch.from_numpy(images).cuda(); lab = torch.from_numpy(labels[..., 0].copy()).cuda()
    losses = []
    for _ in range(8):
        eng.forward(x, training=True, labels=lab, want_probs=False)
        losses.append(eng.loss_dice()); eng.backward(lab); eng.adam_step(lr=2e-3)
    losses = torch.stack(losses).cpu().numpy()
    assert np.isfinite(losses).all() and losses[-1, 0] < losses[0, 0]
    probs, am = eng.forward(x, training=False, want_argmax=True)
    assert torch.allclose(probs.sum(-1), torch.ones_like(probs[..., 0]), atol=1e-5) and torch.equal(am.long(), probs.argmax(-1))
    cfg = make_cfg(input_channels=1, num_classes=3, image_height=H, image_width=W, pool_layers=5)
    cfg.dtype = 7
    assert _hip.lib().oct_unet_cfg_check(ctypes.byref(cfg)) != 0 and b"dtype" in _hip.lib().oct_last_error()


def test_device_boundary_maps_match_reference_definition():
    """arg-max -> boundary maps on the device, bit-exact vs the numpy restatement of
    common/utils.py:115-168 (including the edge rows, where np.gradient is one-sided and the uint8 cast wraps)."""
    cfg, eng, _, _ = make(2, 32, 64, 4, 8, 2, training=False)
    rng = np.random.default_rng(0)
    _, smooth = on.synth_scans(3, 32, 64, 4, seed=6)
    cases = [smooth[..., 0], rng.integers(0, 4, (3, 32, 64)).astype(np.uint8)]
    edge = np.zeros((2, 32, 64), np.uint8); edge[0, 1:, :] = 1; edge[1, :-1, :] = 2; edge[1, -1, :] = 3   # steps at the first / last row
    cases.append(edge)
    for lab in cases:
        cat = np.transpose(np.eye(4, dtype=np.float32)[lab], (0, 3, 1, 2))
        for kw in (dict(bg_ilm=True, bg_csi=False), dict(bg_ilm=False, bg_csi=True), dict(bg_ilm=True, bg_csi=True)):
            with np.errstate(invalid="ignore"):
                ref = on.convert_predictions_to_maps_semantic(cat, **kw)
            got = eng.boundary_maps(torch.from_numpy(np.ascontiguousarray(lab)).cuda(), **kw).cpu().numpy()
            assert np.array_equal(got, ref), kw


@pytest.mark.parametrize("shape", [(3, 36, 68), (2, 496, 768)])
def test_device_boundary_maps_at_sizes_off_the_launch_grid(shape):
    """oct_boundary_maps at 36x68 and at the height of a real B-scan, 496x768 (B H W is no multiple of the block, and at
    the second size the grid-stride loop wraps), bit-exact against the same numpy definition: smooth layered maps, random
    maps, and steps at the first / last row and column."""
    B, H, W = shape
    cfg, eng, _, _ = make(1, 32, 64, 4, 8, 2, training=False)          # (the maps' size is the call's, not the engine's)
    rng = np.random.default_rng(1)
    _, smooth = on.synth_scans(B, H, W, 4, seed=8)
    edge = np.zeros((B, H, W), np.uint8); edge[0, 1:, :] = 1; edge[1, :-1, :] = 2; edge[1, -1, :] = 3
    edge[-1, :, 0] = 3; edge[-1, :, -1] = 1
    for lab in (smooth[..., 0], rng.integers(0, 4, (B, H, W)).astype(np.uint8), edge):
        cat = np.transpose(np.eye(4, dtype=np.float32)[lab], (0, 3, 1, 2))
        for kw in (dict(bg_ilm=True, bg_csi=False), dict(bg_ilm=False, bg_csi=True), dict(bg_ilm=True, bg_csi=True)):
            with np.errstate(invalid="ignore"):
                ref = on.convert_predictions_to_maps_semantic(cat, **kw)
            got = eng.boundary_maps(torch.from_numpy(np.ascontiguousarray(lab)).cuda(), **kw).cpu().numpy()
            assert got.shape == (B, 3, H, W) and np.array_equal(got, ref), kw


def test_hip_path_matches_committed_golden():
    """HIP path vs the COMMITTED fixture tests/golden/unet_golden.npz (fp64 oracle outputs; generating script
    committed next to it).  Tolerances as in the live-oracle tests."""
    import os
    from oct_image_segmentation_models_amd.engine import UNetEngine
    from tests.golden.make_unet_golden import CFG, B, H, W
    G = np.load(os.path.join(os.path.dirname(__file__), "golden", "unet_golden.npz"))
    cfg = on.UNetConfig(**CFG)
    eng = UNetEngine(device="cuda:0", input_channels=1, num_classes=3, image_height=H, image_width=W, start_neurons=4,
                     pool_layers=2, max_batch=B, training=True, seed=int(G["dropout_seed"]))
    eng.set_weights(on.keras_weight_list(on.unflatten_params(cfg, G["params_flat"]), on.unflatten_state(cfg, G["state_flat"])))
    x = torch.from_numpy(G["images"]).cuda(); lab = torch.from_numpy(G["labels"][..., 0].copy()).cuda()
    probs, _ = eng.forward(x, training=False)
    assert np.abs(probs.cpu().numpy() - G["probs_infer"]).max() < PROB_TOL
    for macro, key in ((True, "grads_macro"), (False, "grads_micro")):
        eng.set_weights(on.keras_weight_list(on.unflatten_params(cfg, G["params_flat"]), on.unflatten_state(cfg, G["state_flat"])))
        eng.set_dropout_step(int(G["dropout_step"]))
        probs, _ = eng.forward(x, training=True, labels=lab)
        m = eng.loss_dice().cpu().numpy()
        eng.backward(lab, macro=macro)
        assert np.abs(probs.cpu().numpy() - G["probs_train"]).max() < PROB_TOL
        assert np.abs(m[:2] - G["metrics_train"][:2]).max() < 1e-5 and np.abs(m[2:] - G["metrics_train"][2:]).max() < DICE_TOL
        g = eng.grads.cpu().numpy(); ref = G[key]
        assert np.abs(g - ref).max() / np.abs(ref).max() < GRAD_RTOL
        assert np.abs(eng.state.cpu().numpy() - G["state_after"]).max() < 1e-5


def test_full_size_parity_with_real_kernel_selection():
    """256x512 (BASELINE configs[1] geometry, batch 2): the grid sizes that select the thin VALU kernel, the persistent
    kernel and the wide MFMA shapes in production.  Forward compared tightly layer by layer; gradients with a metric
    that tolerates isolated ReLU-kink flips (a 2M-element layer cannot be kept 2e-5 away from zero everywhere):
    relative L2 error per tensor."""
    B, H, W, C = 2, 256, 512, 3
    cfg, eng, p64, s64 = make(B, H, W, C, 8, 4, training=True)
    images, labels = data(B, H, W, C, seed=21)
    x = torch.from_numpy(images).cuda(); lab = torch.from_numpy(labels[..., 0].copy()).cuda()
    # inference first (training forwards update the moving statistics)
    probs_i, am = eng.forward(x, training=False, want_argmax=True)
    ref_i, _ = on.forward(cfg, p64, s64, on.preprocess_u8(images, np.float64), training=False)
    assert np.abs(probs_i.cpu().numpy() - ref_i).max() < PROB_TOL
    eng.set_dropout_step(2)
    mask = eng.dropout_mask(B).cpu().numpy().astype(np.float64)
    probs, _ = eng.forward(x, training=True, labels=lab)
    loss4 = eng.loss_dice().cpu().numpy()
    eng.backward(lab, macro=True)
    g = eng.grads.cpu().numpy()
    ref, cache = on.forward(cfg, p64, s64, on.preprocess_u8(images, np.float64), training=True, dropout_mask=mask)
    for li, spec in enumerate(on.build_plan(cfg)[:-1]):
        z = eng.debug_activation(li, 0)[:B].cpu().numpy()
        assert np.abs(z - cache[li]["z"]).max() / max(1.0, np.abs(cache[li]["z"]).max()) < 1e-4, spec.name
    assert np.abs(probs.cpu().numpy() - ref).max() < PROB_TOL
    loss, grads = on.backward(cfg, p64, cache, labels, macro=True)
    assert abs(loss4[0] - loss) < 1e-5
    # vs the oracle: flip-tolerant bound.  With ~2M elements per layer some BN pre-activations are within fp32 rounding
    # of the ReLU kink (tools/debug_layers.py full: the first diverging layer has a handful of outliers, all with
    # |pre-activation| < 1e-5), and each flipped element perturbs everything upstream of it.
    for L_, gr in zip(eng.layers, grads):
        n = L_["kh"] * L_["kw"] * L_["cin"] * L_["cout"]
        gk = g[L_["kernel_off"]:L_["kernel_off"] + n]; rk = gr["kernel"].ravel()
        assert np.linalg.norm(gk - rk) / np.linalg.norm(rk) < 1e-2, L_["name"]
    # oracle-independent and flip-free: directional derivative through the engine's own (oracle-verified) forward vs
    # g.v from its backward, along v = g/|g| -- exercises the multi-tile dX / dW loops of the production kernel selection
    theta = eng.params.clone()
    gt = eng.grads.clone()
    v = gt / gt.norm()
    eps = 5e-4   # linear regime (loss in [0,1], |g| ~ 0.5) yet well above the fp32 loss resolution; the function is
                 # piecewise smooth (ReLU / max-pool kinks), so the central difference wobbles by ~1 % with the step
    vals = []
    for sgn in (+1.0, -1.0):
        eng.params.copy_(theta + sgn * eps * v)
        eng.set_dropout_step(2)
        eng.forward(x, training=True, labels=lab, want_probs=False)
        vals.append(float(eng.loss_dice()[0]))
    eng.params.copy_(theta)
    fd = (vals[0] - vals[1]) / (2 * eps)
    gv = float((gt * v).sum())
    assert abs(fd - gv) < 0.03 * abs(gv), (fd, gv)


@pytest.mark.parametrize("macro", [True, False])
@pytest.mark.parametrize("cw", [None, (0.5, 2.0, 1.25)])
def test_focal_dice_loss_and_gradients_match_oracle(macro, cw):
    """focal_dice_loss (reference custom_losses.py:98-178; third-party focal-loss formula restated -- parity unpinned):
    loss terms and every gradient tensor vs the fp64 oracle, with and without class weights."""
    case = CASES[0]
    B, H, W, C, sn, P, L, ic = case
    fw, gamma = 0.35, 2.0
    cfg, eng, p64, s64 = make(B, H, W, C, sn, P, L, ic, training=True)
    images, labels = data(B, H, W, C, ic, seed=MARGIN_SEED[case])
    x = torch.from_numpy(images).cuda(); lab = torch.from_numpy(labels[..., 0].copy()).cuda()
    eng.set_dropout_step(DROP_STEP)
    mask = eng.dropout_mask(B).cpu().numpy().astype(np.float64)
    eng.set_focal_dice(fw, gamma, cw)
    probs, _ = eng.forward(x, training=True, labels=lab)
    v = eng.loss_focal_dice().cpu().numpy()
    eng.backward(lab, macro=macro, loss_scale=0.5)
    ref, cache = on.forward(cfg, p64, s64, on.preprocess_u8(images, np.float64), training=True, dropout_mask=mask)
    assert relu_margin(cfg, p64, cache) > 2e-5
    assert np.abs(probs.cpu().numpy() - ref).max() < PROB_TOL
    y = on.one_hot(labels, C, np.float64)
    focal = on.focal_loss_mean(labels, ref, gamma, cw)
    assert abs(v[0] - on.dice_loss_macro(y, ref)) < 1e-5 and abs(v[1] - on.dice_loss_micro(y, ref)) < 1e-5
    assert abs(v[4] - focal) < 1e-5 * max(1.0, focal)
    assert abs(v[5] - on.focal_dice_loss(labels, ref, C, gamma, cw, fw, True)) < 1e-5
    assert abs(v[6] - on.focal_dice_loss(labels, ref, C, gamma, cw, fw, False)) < 1e-5
    loss, grads = on.backward(cfg, p64, cache, labels, macro=macro, loss_scale=0.5, focal=(fw, gamma, cw))
    g = eng.grads.cpu().numpy()
    for L_, gr in zip(eng.layers, grads):
        n = L_["kh"] * L_["kw"] * L_["cin"] * L_["cout"]; c = L_["cout"]
        pieces = [("kernel", L_["kernel_off"], n), ("bias", L_["bias_off"], c)]
        if L_["has_bn"]:
            pieces += [("gamma", L_["gamma_off"], c), ("beta", L_["beta_off"], c)]
        kscale = np.abs(gr["kernel"]).max()
        for key, off, cnt in pieces:
            refv = gr[key].ravel()
            scale = max(np.abs(refv).max(), kscale if key == "bias" else 0.0, 1e-12)
            assert np.abs(g[off:off + cnt] - refv).max() / scale < GRAD_RTOL, f"{L_['name']}.{key}"
    # w = 0 restores the plain Dice gradient bit for bit
    eng.set_focal_dice(0.0)
    eng.set_dropout_step(DROP_STEP)          # same dropout mask as the fresh engine below
    eng.forward(x, training=True, labels=lab); eng.loss_dice(); eng.backward(lab, macro=macro, loss_scale=0.5)
    g0 = eng.grads.clone()
    cfg2, eng2, _, _ = make(B, H, W, C, sn, P, L, ic, training=True)
    eng2.set_dropout_step(DROP_STEP)
    eng2.forward(x, training=True, labels=lab); eng2.loss_dice(); eng2.backward(lab, macro=macro, loss_scale=0.5)
    assert torch.equal(g0, eng2.grads)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("geo", [(3, 40, 96, 3, 8, 3), (2, 32, 64, 4, 16, 2), (2, 36, 68, 3, 8, 2)])   # last: ragged at every level
def test_bn_backward_on_load_equals_the_separate_pass(dtype, geo):
    """By default no block's dz is ever stored: the BN-backward transform dz = ga g' + gb z + gd is applied by the
    consumers of dz while they stage g' and z -- block 0 inside conv_dw_first_k (its only consumer; the image has no
    gradient), every other block inside its backward-weights kernel and its backward-data launches -- instead of by a
    bn_bwd_apply pass per block (3 tensor passes each).  Same two fmas, same rounding of dz to the storage type: every
    gradient must equal the separate-pass route BIT FOR BIT, in fp32 and in bf16 storage."""
    from oct_image_segmentation_models_amd import _hip
    from oct_image_segmentation_models_amd.engine import UNetEngine
    B, H, W, C, sn, P = geo                         # first: ragged against the 8 x 128 tile of the streaming kernel
    images, labels = data(B, H, W, C, 1, seed=21)
    x = torch.from_numpy(images).cuda(); lab = torch.from_numpy(labels[..., 0].copy()).cuda()
    got, applied = {}, {}
    try:
        _hip.set_option("fuse_dw_thin", 0)       # (same backward-weights kernels on both routes: this test is about dz)
        for fuse in (1, 0):
            _hip.set_option("fuse_first_apply", fuse); _hip.set_option("fuse_bn_apply", fuse)
            eng = UNetEngine(device="cuda:0", input_channels=1, num_classes=C, image_height=H, image_width=W,
                             start_neurons=sn, pool_layers=P, max_batch=B, training=True, seed=9, init_seed=4,
                             dtype="bfloat16" if dtype == "bf16" else "float32")
            eng.set_dropout_step(2)
            eng.profile_begin()
            eng.forward(x, training=True, labels=lab, want_probs=False); eng.loss_dice(); eng.backward(lab, macro=True)
            names = [(e["kernel"], e["layer"]) for e in eng.profile_end()]
            applied[fuse] = {l for k, l in names if k.startswith("bn_bwd_apply")}
            nb = len(eng.layers) - 1
            fused = {eng.layers[li]["name"] for li in range(nb) if eng.debug_layer_fused(li)}
            assert applied[fuse] | fused == {L["name"] for L in eng.layers[:nb]} and not (applied[fuse] & fused), names
            if fuse:       # the passes are really gone: at most the thin kernel's 32-channel backward-data layers keep theirs
                # (and block 0 where it is not the 1 -> 8 streaming kernel)
                assert len(applied[1]) <= len(eng.layers) // 2 and (sn != 8 or "enc0.conv0" in fused), applied[1]
                assert any(k.endswith(",gb>") for k, _ in names)
            else:
                assert not fused and not any(k.endswith(",gb>") for k, _ in names)
                assert eng.debug_activation(0, 1)[:B].float().abs().sum().item() > 0
            got[fuse] = eng.grads.clone()
    finally:
        _hip.set_option("fuse_first_apply", 1); _hip.set_option("fuse_bn_apply", 1); _hip.set_option("fuse_dw_thin", 1)
    assert torch.isfinite(got[1]).all() and got[1].abs().max() > 0
    assert torch.equal(got[0], got[1])


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_backward_weights_inside_the_backward_data_launch(dtype):
    """3x3 layers with 8 output channels (the full-resolution convs): by default their backward-data launches also reduce
    the layer's backward-weights (conv_bt_k FDW) -- no separate dW kernel, g', z and the producer's z read once.  Same
    products, another summation order: every gradient equals the separate-kernel route to fp32 accumulation accuracy (and
    both are checked against the oracle by the variant tests), the dW kernels of those layers are really gone, and
    everything else (backward-data results, BN statistics) is bit-identical."""
    backward_weights_fused_vs_separate(dtype, 3, 40, 96)          # ragged against the 8 x 32 tile


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_backward_weights_inside_the_backward_data_launch_at_36x68(dtype):
    """The same at 36 x 68, pool_layers 2: neither the rows nor the width of any level (36x68, 18x34, 9x17) divide the
    8 x 32 tile, so every block of the fused launches clamps its X loads into the image and masks its own pixels."""
    backward_weights_fused_vs_separate(dtype, 2, 36, 68)


def backward_weights_fused_vs_separate(dtype, B, H, W):
    from oct_image_segmentation_models_amd import _hip
    from oct_image_segmentation_models_amd.engine import UNetEngine
    C = 3
    images, labels = data(B, H, W, C, 1, seed=23)
    x = torch.from_numpy(images).cuda(); lab = torch.from_numpy(labels[..., 0].copy()).cuda()
    got, gbuf = {}, {}
    try:
        for fdw in (1, 0):
            _hip.set_option("fuse_dw_thin", fdw)
            eng = UNetEngine(device="cuda:0", input_channels=1, num_classes=C, image_height=H, image_width=W,
                             start_neurons=8, pool_layers=2, max_batch=B, training=True, seed=9, init_seed=4,
                             dtype="bfloat16" if dtype == "bf16" else "float32")
            eng.set_dropout_step(2)
            eng.profile_begin()
            eng.forward(x, training=True, labels=lab, want_probs=False); eng.loss_dice(); eng.backward(lab, macro=True)
            ents = eng.profile_end()
            fused = {e["layer"] for e in ents if e["kernel"].startswith("conv_bt_k") and e["kernel"].endswith(",dw>")}
            dwk = {e["layer"] for e in ents if e["kernel"].startswith("conv_dw") and not e["kernel"].startswith("conv_dw_first")}
            thin3 = {L["name"] for L in eng.layers if L["kh"] == 3 and L["cout"] == 8 and L["cin"] in (8, 16)}
            assert thin3 == {"enc0.conv1", "dec1.conv0", "dec1.conv1"}
            assert fused == (thin3 if fdw else set()) and not (fused & dwk) and (thin3 <= dwk or fdw), (fused, dwk)
            got[fdw] = eng.grads.clone()
            gbuf[fdw] = [eng.debug_activation(li, 1)[:B].clone() for li in range(len(eng.layers) - 1)]
    finally:
        _hip.set_option("fuse_dw_thin", 1)
    for a, b in zip(gbuf[1], gbuf[0]):               # masked gradients of every block: the dX results did not move
        assert torch.equal(a, b)
    g1, g0 = got[1].cpu().numpy().astype(np.float64), got[0].cpu().numpy().astype(np.float64)
    tol = 2e-2 if dtype == "bf16" else 1e-5          # (bf16 mode: the two routes round X / dz to bf16 identically, sums differ)
    for L in eng.layers:
        n = L["kh"] * L["kw"] * L["cin"] * L["cout"]
        a, b = g1[L["kernel_off"]:L["kernel_off"] + n], g0[L["kernel_off"]:L["kernel_off"] + n]
        assert np.abs(a - b).max() <= tol * max(np.abs(b).max(), 1e-30), L["name"]
        a, b = g1[L["bias_off"]:L["bias_off"] + L["cout"]], g0[L["bias_off"]:L["bias_off"] + L["cout"]]
        assert np.abs(a - b).max() <= tol * max(np.abs(g0[L["kernel_off"]:L["kernel_off"] + n]).max(), 1e-30), L["name"]


@pytest.mark.parametrize("clip_mod", [0, 1])
def test_focal_clip_modulation_switch(clip_mod):
    """The one focal-loss detail that cannot be verified here (does (1 - p_y)^gamma see the CLIPPED probability?) is a
    switch on both sides.  A saturated head (bias +12 / 0 / -12: p_y ~ e^-24 < 1e-7 on class-2 pixels, in range on the others) makes the clip
    active on most pixels; each setting must match the oracle run with the same setting -- and, the actual finding, the
    two settings agree with each other far below the test tolerances, because the softmax Jacobian multiplies the
    differing term by p_y < 1e-7."""
    from oct_image_segmentation_models_amd import _hip
    case = CASES[0]
    B, H, W, C, sn, P, L, ic = case
    fw, gamma, cw = 0.6, 2.0, (0.5, 2.0, 1.25)
    cfg, eng, p64, s64 = make(B, H, W, C, sn, P, L, ic, training=True)
    wl = eng.get_weights()
    wl[-1] = np.array([12.0, 0.0, -12.0], np.float32)            # head bias: p_2 ~ e^-24 (clipped), p_1 ~ e^-12 (in range)
    eng.set_weights(wl)
    p64[-1]["bias"] = wl[-1].astype(np.float64)
    images, labels = data(B, H, W, C, ic, seed=MARGIN_SEED[case])
    x = torch.from_numpy(images).cuda(); lab = torch.from_numpy(labels[..., 0].copy()).cuda()
    eng.set_dropout_step(DROP_STEP)
    mask = eng.dropout_mask(B).cpu().numpy().astype(np.float64)
    ref, cache = on.forward(cfg, p64, s64, on.preprocess_u8(images, np.float64), training=True, dropout_mask=mask)
    py = np.take_along_axis(ref, labels.astype(np.int64), axis=-1)
    assert (py < 1e-7).mean() > 0.2                                             # the clip really is active
    eng.set_option("focal_clip_modulation", clip_mod)        # per handle: the process-wide default stays 0
    assert eng.handle_option("focal_clip_modulation") == clip_mod and _hip.get_option("focal_clip_modulation") == 0
    eng.set_focal_dice(fw, gamma, cw)
    eng.forward(x, training=True, labels=lab, want_probs=False)
    v = eng.loss_focal_dice().cpu().numpy()
    eng.backward(lab, macro=True, loss_scale=1.0)
    g = eng.grads.cpu().numpy().astype(np.float64)
    focal = on.focal_loss_mean(labels, ref, gamma, cw, clip_modulation=bool(clip_mod))
    assert abs(v[4] - focal) < 2e-5 * max(1.0, focal), (v[4], focal)
    both = [on.backward(cfg, p64, cache, labels, macro=True, loss_scale=1.0, focal=(fw, gamma, cw),
                        focal_clip_modulation=m)[1] for m in (False, True)]
    gref = on.flatten_grads(both[clip_mod]); gother = on.flatten_grads(both[1 - clip_mod])
    scale = np.abs(gref).max()
    assert np.abs(g - gref).max() / scale < 2e-3       # saturated softmax: f32 cancellation in p*(dp - dot) limits this case
    assert np.abs(gref - gother).max() / scale < 1e-6  # the unverifiable choice cannot move the gradient


def test_config3_shape_in_its_own_dtype_bf16():
    """BASELINE configs[2] geometry (512x1024x1, pool_layers=5) IN bf16 (bf16 activations and MFMA operands, fp32
    accumulation / BN / parameters), reduced batch: the bf16 engine tracks an fp32 engine started from the same weights on
    the same data (first-forward probabilities, loss trajectory), stays finite and learns; the profiler shows the bf16-pipe
    kernels of every family (wide, thin, both backward-weights kernels) were the ones that ran.  The exact rounding model
    of this mode is pinned layer by layer at small sizes (test_bf16_storage_layer_local_rounding_is_exact)."""
    from oct_image_segmentation_models_amd.engine import UNetEngine
    B, H, W, C = 2, 512, 1024, 3
    kw = dict(device="cuda:0", input_channels=1, num_classes=C, image_height=H, image_width=W, pool_layers=5, max_batch=B,
              training=True, seed=3, init_seed=5, dropout_rate=0.0)
    e16 = UNetEngine(dtype="bfloat16", **kw)
    e32 = UNetEngine(dtype="float32", **kw)
    assert e16.n_params == 1948267 and e16.workspace.numel() < 0.75 * e32.workspace.numel()
    assert torch.equal(e16.params, e32.params)
    images, labels = data(B, H, W, C, seed=4)
    x = torch.from_numpy(images).cuda(); lab = torch.from_numpy(labels[..., 0].copy()).cuda()
    p16, _ = e16.forward(x, training=True, labels=lab); l16 = [e16.loss_dice().clone()]
    p32, _ = e32.forward(x, training=True, labels=lab); l32 = [e32.loss_dice().clone()]
    # 27 conv blocks of 2^-9 operand rounding through a random-init ReLU net with B=2 batch statistics: the per-pixel
    # deviation is large where the three classes are near a tie (measured mean 4e-2); the class maps must still agree
    d = (p16 - p32).abs()
    same = (p16.argmax(-1) == p32.argmax(-1)).float().mean()
    assert torch.isfinite(p16).all() and d.mean() < 8e-2 and same > 0.85, (float(d.mean()), float(d.max()), float(same))
    e16.profile_begin()
    e16.backward(lab); e16.adam_step(lr=2e-3)
    fams = {e["kernel"].split("<")[0] for e in e16.profile_end()}
    assert {"conv_bx_k", "conv_bt_k", "conv_dwbx_k", "conv_dwbt_k"} <= fams, fams
    assert not ({"conv_igemm_k", "conv_pair8_k", "conv_dw16_k", "conv_dw32_k", "conv_dwpair8_k"} & fams), fams
    e32.backward(lab); e32.adam_step(lr=2e-3)
    for _ in range(7):
        e16.forward(x, training=True, labels=lab, want_probs=False); l16.append(e16.loss_dice().clone()); e16.backward(lab); e16.adam_step(lr=2e-3)
        e32.forward(x, training=True, labels=lab, want_probs=False); l32.append(e32.loss_dice().clone()); e32.backward(lab); e32.adam_step(lr=2e-3)
    l16 = torch.stack(l16).cpu().numpy()[:, 0]; l32 = torch.stack(l32).cpu().numpy()[:, 0]
    assert np.isfinite(l16).all() and l16[-1] < l16[0] and l32[-1] < l32[0]
    assert np.abs(l16 - l32).max() < 0.05, (l16, l32)          # same trajectory within accumulated bf16 noise
    assert torch.isfinite(e16.params).all()


# ---- bf16 activation storage (BASELINE configs[2]: "bf16 with fp32 BN accum") ---------------------------------
# dtype=1 keeps every activation / activation-gradient tensor in HBM as bf16 (round-to-nearest-even at the store),
# while arithmetic, BN statistics, parameters and parameter gradients stay fp32.  Two kinds of gate:
#  (1) LAYER-LOCAL, tight: each layer's fp64 oracle output computed FROM THE HIP PATH'S OWN stored inputs must round
#      to the stored bf16 value -- within 1 bf16 ulp everywhere, identical on >= 99.5 % of the elements (the remainder
#      are rounding-boundary flips caused by fp32-vs-fp64 arithmetic); the BN record the consumers apply is read back.
#      A wrong half-word, a truncating conversion or a misaligned 8-byte access fails this at ~50 % of the elements.
#  (2) END-TO-END, loose: rounding noise of 2^-9 relative per stored tensor accumulates through the 2P(L+1)+L stored
#      tensors (measured with tools/bf16_layer_error.py: rms 1.7e-3 at the first layer, the store-only floor, rising
#      smoothly to 3e-2 at the last, the same growth profile the fp32 path shows at 1e-7 scale), so against the
#      unrounded oracle the gates are: probabilities 8e-2 max / 1.5e-2 mean, Dice 2e-2; gradients, which also see the
#      ReLU masks that the forward noise flips, cosine > 0.9 per kernel tensor and > 0.97 over the whole gradient
#      (the layer-local test above is the one that pins every backward kernel to one rounding).
BF16_CASES = [(2, 32, 64, 3, 8, 2, 2, 1), (1, 48, 80, 3, 8, 3, 1, 3), (1, 32, 64, 3, 8, 2, 2, 4), (1, 32, 64, 3, 32, 1, 2, 1),
              (1, 32, 64, 3, 12, 2, 2, 1),
              # the ragged geometries of CASES whose channel counts are multiples of 8 (bf16 MFMA operands on every layer but the first)
              (2, 36, 68, 3, 8, 2, 2, 1), (1, 48, 80, 3, 8, 4, 2, 1), (1, 80, 24, 3, 16, 2, 2, 1)]


def make_bf16(B, H, W, C, sn, P, L=2, in_ch=1, seed=0, max_batch=None):
    from oct_image_segmentation_models_amd.engine import UNetEngine
    cfg = on.UNetConfig(input_channels=in_ch, num_classes=C, start_neurons=sn, pool_layers=P, conv_layers=L)
    params, state = on.init_params(cfg, seed=seed, dtype=np.float32, randomize_bn=True)
    eng = UNetEngine(device="cuda:0", input_channels=in_ch, num_classes=C, image_height=H, image_width=W,
                     start_neurons=sn, pool_layers=P, conv_layers=L, max_batch=max_batch or B, training=True, seed=seed + 100,
                     dtype="bfloat16")
    eng.set_weights(on.keras_weight_list(params, state))
    p64 = [{k: v.astype(np.float64) for k, v in p.items()} for p in params]
    s64 = [{k: v.astype(np.float64) for k, v in s.items()} for s in state]
    return cfg, eng, p64, s64


@pytest.mark.parametrize("case", BF16_CASES)
def test_bf16_storage_layer_local_rounding_is_exact(case, variant):
    from oct_image_segmentation_models_amd import _hip
    _hip.set_option("fuse_first_apply", 0); _hip.set_option("fuse_bn_apply", 0)   # this test reads EVERY block's STORED dz (the fused
    B, H, W, C, sn, P, L, ic = case               # route is pinned bit for bit against this one by the test below)
    cfg, eng, p64, s64 = make_bf16(B, H, W, C, sn, P, L, ic)
    # the stored z and gradient tensor of every block are 2 bytes per element smaller; partial slabs, records and prepared
    # weights stay fp32
    ws16, ws32 = eng.workspace.numel(), make(B, H, W, C, sn, P, L, ic)[1].workspace.numel()
    act = sum(B * L_["out_h"] * L_["out_w"] * L_["cout"] for L_ in eng.layers[:-1])
    assert ws32 - ws16 >= 4 * act
    # (one geometry by name: on the 80 x 24 image with start_neurons 16 the stored activations are 4 act = 0.095 of an fp32
    #  workspace of 64-channel dW slabs and prepared weights; the ratio there is 0.805 and only the exact saving is asserted)
    assert ws16 < 0.8 * ws32 or case == (1, 80, 24, 3, 16, 2, 2, 1)
    images, labels = data(B, H, W, C, ic, seed=MARGIN_SEED.get(case, 5))
    bf16_step_layer_local(cfg, eng, p64, case, images, labels)


def bf16_step_layer_local(cfg, eng, p64, case, images, labels):
    """One training step of a bf16-storage engine on the case's own B images (max_batch may be larger), stand-alone
    BN-backward route: every stored tensor and every gradient against the fp64 recomputation from the engine's own stored
    inputs, one rounding each."""
    B, H, W, C, sn, P, L, ic = case
    x = torch.from_numpy(images).cuda(); lab = torch.from_numpy(labels[..., 0].copy()).cuda()
    eng.set_dropout_step(DROP_STEP)
    mask = eng.dropout_mask(B).cpu().numpy().astype(np.float64)
    probs, _ = eng.forward(x, training=True, labels=lab)
    plan = on.build_plan(cfg)
    zh = [eng.debug_activation(li, 0)[:B].cpu().numpy().astype(np.float64) for li in range(len(plan) - 1)]

    rec = [eng.debug_bn_record(li).cpu().numpy().astype(np.float64) for li in range(len(plan) - 1)]
    for li in range(len(plan) - 1):      # the record itself: a = gamma*rstd, b = beta - a*mean (its batch statistics: below)
        assert np.allclose(rec[li][0], p64[li]["gamma"] * rec[li][3], rtol=1e-5, atol=1e-7)
        assert np.allclose(rec[li][1], p64[li]["beta"] - rec[li][0] * rec[li][2], rtol=1e-5, atol=1e-6)

    def act(li):      # what a consumer computes from the STORED tensor: relu(a*z + b) (+dropout after the bottleneck)
        y = on.relu(rec[li][0] * zh[li] + rec[li][1])
        if plan[li].name == f"mid.conv{L - 1}":
            y = y * mask / (1.0 - cfg.dropout_rate)
        return y

    from oct_image_segmentation_models_amd import _hip
    mm = _hip.get_option("mfma_mode")
    inps = {}
    for li, spec in enumerate(plan):
        if spec.src == "input":
            inp = on.preprocess_u8(images, np.float64)
        elif spec.src in ("prev", "head"):
            inp = act(li - 1)
        elif spec.src == "pool":
            inp = bf16_round(on.maxpool2x2(act(li - 1)))          # the pooled tensor is itself stored in bf16
        elif spec.src == "up":
            inp = on.upsample2x(act(li - 1))
        else:
            inp = np.concatenate([act(li - 1), act(spec.skip_from)], axis=-1)
        inps[li] = inp
        if bf16_fwd_operands(plan, li, cfg, mm):      # bf16 MFMA operands: activation and weights rounded, fp32 accumulate
            z = on.conv2d_same(bf16_round(inp), bf16_round(p64[li]["kernel"]), p64[li]["bias"])
        else:
            z = on.conv2d_same(inp, p64[li]["kernel"], p64[li]["bias"])
        if spec.has_bn:
            # the record's batch statistics: the engine takes them of its fp32 accumulators BEFORE it rounds z for the store,
            # so they are those of this unrounded recomputation, not of the stored roundings (the two differ by the mean of
            # N rounding errors: nothing at a full-size layer, 2x this bound over the 15 pixels of a 3 x 5 bottleneck, where
            # a defect-free model of the engine misses it too -- tests/layer_local.py has the same rule)
            _, mean, var, rstd, _ = on.batchnorm_train(z, p64[li]["gamma"], p64[li]["beta"], cfg.bn_eps)
            assert np.allclose(rec[li][2], mean, atol=2e-4 * np.abs(zh[li]).max()) and np.allclose(rec[li][3], rstd, rtol=2e-3), spec.name
            err = np.abs(zh[li] - bf16_round(z))
            # + an absolute floor for cancelling sums near zero (the statistics differ by ~1e-5 relative)
            bound = 1.001 * bf16_ulp(z) + 5e-5 * np.abs(z).max()
            # an operand whose fp32 activation sits on a bf16 rounding boundary may round the other way than this fp64
            # model (a few per 1e5 elements): such an element moves its 9*cout outputs by up to |w| * ulp(x)
            loose = bound + 2.0 ** -7 * np.abs(inp).max() * np.abs(p64[li]["kernel"]).max()
            assert (err <= loose).all(), (spec.name, (err / loose).max())
            assert (err <= bound).mean() > 0.999, (spec.name, (err <= bound).mean())
            assert (err == 0).mean() > 0.99, (spec.name, (err == 0).mean())
        else:
            assert np.abs(probs.cpu().numpy() - on.softmax(z)).max() < 2e-4      # head arithmetic is fp32, unrounded

    # ---- backward, layer-local: every stored dz and every parameter gradient recomputed in fp64 from the HIP path's
    # own stored tensors, with the storage roundings of backward_impl (oct_unet.hip): masked g' rounded at the store
    # (statistics before rounding), raw skip / pooled gradients rounded, dz = round(gamma*rstd*(g' - c1 - xhat*c2)).
    eng.loss_dice()
    eng.backward(lab, macro=True)
    g = eng.grads.cpu().numpy().astype(np.float64)
    nb = len(plan) - 1
    dzh = [eng.debug_activation(li, 1)[:B].cpu().numpy().astype(np.float64) for li in range(nb)]
    rec = [eng.debug_bn_record(li).cpu().numpy().astype(np.float64) for li in range(nb)]
    skipraw = {}
    for li in range(nb - 1, -1, -1):
        spec, Lh = plan[li], eng.layers[li]
        wq = bf16_dx_weights(plan, li, mm)
        gx, _, db = on._conv_backward(inps[li], bf16_round(p64[li]["kernel"]) if wq else p64[li]["kernel"], dzh[li])
        _, dk, _ = on._conv_backward(bf16_round(inps[li]) if bf16_dw_operands(plan, li, mm) else inps[li], p64[li]["kernel"], dzh[li])
        gk = g[Lh["kernel_off"]:Lh["kernel_off"] + dk.size].reshape(dk.shape)
        assert np.linalg.norm(gk - dk) <= 1e-4 * np.linalg.norm(dk) + 1e-9, spec.name            # dW: fp32 accumulation
        gb = g[Lh["bias_off"]:Lh["bias_off"] + spec.cout]
        assert np.abs(gb - db).max() <= 1e-5 * np.abs(dzh[li]).sum(axis=(0, 1, 2)).max() + 1e-7, spec.name
        N = dzh[li].shape[0] * dzh[li].shape[1] * dzh[li].shape[2]
        assert np.allclose(g[Lh["beta_off"]:Lh["beta_off"] + spec.cout], rec[li][4] * N, rtol=1e-4, atol=1e-6)
        assert np.allclose(g[Lh["gamma_off"]:Lh["gamma_off"] + spec.cout], rec[li][5] * N, rtol=1e-4, atol=1e-6)
        if spec.src == "input":
            break
        pi = li - 1
        alive = (rec[pi][0] * zh[pi] + rec[pi][1]) > 0
        if spec.src == "prev":
            gq = bf16_round(alive * gx)
        elif spec.src == "up":
            gy = upconv_dx_effective(dzh[li], p64[li]["kernel"], wq)
            if plan[pi].name == f"mid.conv{L - 1}":
                gy = gy * mask / (1.0 - cfg.dropout_rate)
            gq = bf16_round(alive * gy)
        elif spec.src == "concat":
            C0 = plan[pi].cout
            skipraw[spec.skip_from] = bf16_round(gx[..., C0:])
            gq = bf16_round(alive * gx[..., :C0])
        else:   # pool: raw gradient of the pooled tensor (stored), routed to the first maximum, + the skip half
            routed = on._maxpool_backward(on.relu(rec[pi][0] * zh[pi] + rec[pi][1]), bf16_round(gx))
            gq = bf16_round(alive * (routed + skipraw[pi]))
        a_, mean_, rstd_, c1_, c2_ = rec[pi][0], rec[pi][2], rec[pi][3], rec[pi][4], rec[pi][5]
        gr = p64[pi]["gamma"] * rstd_
        pred = gr * (gq - c1_ - (zh[pi] - mean_) * rstd_ * c2_)
        err = np.abs(dzh[pi] - bf16_round(pred))
        bound = 1.001 * bf16_ulp(pred) + np.abs(gr) * bf16_ulp(gq) * (gq != 0) + 5e-5 * np.abs(pred).max()
        assert (err <= bound).mean() > 0.999, (plan[pi].name, (err <= bound).mean())
        assert (err <= 4 * bound).all(), (plan[pi].name, (err / bound).max())
        assert (err == 0).mean() > 0.99, (plan[pi].name, (err == 0).mean())
    return probs


@pytest.mark.parametrize("case,max_batch", [(BF16_CASES[0], 3), (BF16_CASES[1], 4), (BF16_CASES[5], 3), (BF16_CASES[6], 4),
                                            (BF16_CASES[7], 2)])
def test_bf16_partial_training_step_on_a_used_engine(case, max_batch):
    """test_partial_training_step_on_a_used_engine in bf16 storage, default kernel selection: the partial step after a
    full one, held to the one-rounding checks of test_bf16_storage_layer_local_rounding_is_exact."""
    from oct_image_segmentation_models_amd import _hip
    B, H, W, C, sn, P, L, ic = case
    try:
        _hip.set_option("fuse_first_apply", 0); _hip.set_option("fuse_bn_apply", 0)     # (every block's dz is stored)
        cfg, eng, p64, s64 = make_bf16(B, H, W, C, sn, P, L, ic, max_batch=max_batch)
    finally:
        _hip.set_option("fuse_first_apply", 1); _hip.set_option("fuse_bn_apply", 1)
    weights = eng.get_weights()
    dirty_engine(eng, B, seed=MARGIN_SEED.get(case, 5) + 1000)
    eng.set_weights(weights)
    images, labels = data(B, H, W, C, ic, seed=MARGIN_SEED.get(case, 5))
    probs = bf16_step_layer_local(cfg, eng, p64, case, images, labels)
    assert bool(torch.isfinite(probs).all()) and bool(torch.isfinite(eng.state).all())
    assert_tails_untouched(eng, B)


@pytest.mark.parametrize("case", BF16_CASES[:2])     # (the 4-channel case feeds uniform noise images: its gradient is dominated
def test_bf16_storage_mode_end_to_end_within_accumulated_rounding(case):   # by flipped ReLU masks -- layer-local test only)
    B, H, W, C, sn, P, L, ic = case
    cfg, eng, p64, s64 = make_bf16(B, H, W, C, sn, P, L, ic)
    images, labels = data(B, H, W, C, ic, seed=MARGIN_SEED.get(case, 5))
    x = torch.from_numpy(images).cuda(); lab = torch.from_numpy(labels[..., 0].copy()).cuda()
    xin = on.preprocess_u8(images, np.float64)
    probs, am = eng.forward(x, training=False, want_argmax=True)
    ref_i, _ = on.forward(cfg, p64, s64, xin, training=False)
    e = np.abs(probs.cpu().numpy() - ref_i)
    assert e.max() < 8e-2 and e.mean() < 1.5e-2
    assert (am.cpu().numpy() == ref_i.argmax(-1)).mean() > 0.95
    eng.set_dropout_step(DROP_STEP)
    mask = eng.dropout_mask(B).cpu().numpy().astype(np.float64)
    probs, _ = eng.forward(x, training=True, labels=lab)
    loss4 = eng.loss_dice().cpu().numpy()
    eng.backward(lab, macro=True)
    ref, cache = on.forward(cfg, p64, s64, xin, training=True, dropout_mask=mask)
    e = np.abs(probs.cpu().numpy() - ref)
    assert e.max() < 8e-2 and e.mean() < 1.5e-2
    y = on.one_hot(labels, C, np.float64)
    assert abs(loss4[0] - on.dice_loss_macro(y, ref)) < 2e-2 and abs(loss4[1] - on.dice_loss_micro(y, ref)) < 2e-2
    loss, grads = on.backward(cfg, p64, cache, labels, macro=True)
    g = eng.grads.cpu().numpy()
    assert np.isfinite(g).all()
    worst, allg, allr = 1.0, [], []
    for L_, gr in zip(eng.layers, grads):
        n = L_["kh"] * L_["kw"] * L_["cin"] * L_["cout"]
        gk = g[L_["kernel_off"]:L_["kernel_off"] + n].astype(np.float64); rk = gr["kernel"].ravel()
        cos = gk @ rk / (np.linalg.norm(gk) * np.linalg.norm(rk))
        worst = min(worst, cos); allg.append(gk); allr.append(rk)
        assert cos > 0.9, (L_["name"], cos)
    allg, allr = np.concatenate(allg), np.concatenate(allr)
    total = allg @ allr / (np.linalg.norm(allg) * np.linalg.norm(allr))
    print("bf16 kernel-gradient cosine vs unrounded oracle: worst tensor", worst, "whole gradient", total)
    assert total > 0.97
    new_state = on.flatten_state(on.updated_moving_stats(cfg, s64, cache))
    assert np.abs(eng.state.cpu().numpy() - new_state).max() < 1e-3    # BN statistics accumulate in fp32


def test_bf16_training_converges_like_fp32():
    B, H, W, C = 4, 64, 128, 3
    images, labels = data(B, H, W, C, seed=2)
    x = torch.from_numpy(images).cuda(); lab = torch.from_numpy(labels[..., 0].copy()).cuda()
    finals = {}
    for name, mk in (("f32", lambda: make(B, H, W, C, 8, 3, seed=1)), ("bf16", lambda: make_bf16(B, H, W, C, 8, 3, seed=1))):
        cfg, eng, _, _ = mk()
        ls = []
        for it in range(80):
            eng.set_dropout_step(it)
            eng.forward(x, training=True, labels=lab, want_probs=False)
            ls.append(eng.loss_dice()); eng.backward(lab); eng.adam_step(lr=5e-3)
        ls = torch.stack(ls).cpu().numpy()[:, 0]
        assert np.isfinite(ls).all() and ls[-1] < 0.6 * ls[0]
        finals[name] = ls[-10:].mean()
    assert abs(finals["bf16"] - finals["f32"]) < 0.1, finals
