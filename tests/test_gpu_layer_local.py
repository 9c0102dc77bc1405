"""Layer-local fp64 checks of every layer at the benched batch sizes (BASELINE configs[1], [2], [4]), default options.

Each test runs one step of the production route, reads back what the engine stored (pre-BN outputs, BN records, gradient
buffers, probabilities, gradients) and recomputes every layer in fp64 FROM THOSE STORED INPUTS with tests/layer_local.py:
an element is held to the rounding of its own kernel, not to what an upstream mask flip made of it.  The kernel
instantiations the step ran are asserted first, so a routing change cannot silently move what these checks cover.

fp32 gates (tests/layer_local.py): z, g' and dz per element within GAMMA = 2^-17 of the same conv on absolute values
(128 fp32 roundings of the largest possible accumulation; the 3-term split products of the bf16 pipe carry 2^-24 per
product) and within 1e-6 relative L2 per tensor; dW, bias, gamma, beta within 2e-5 of the tensor's
scale; record rows within 1e-5.  Measured margins: >= 7x on the per-element, parameter and record gates; 1.8x - 2.1x on
the relative L2 gate at the widest layers, which is what fp32 accumulation predicts there (the arithmetic is at REL_L2
in tests/layer_local.py).  Elements whose ReLU mask or pool route is decided within fp32 rounding are excluded and
counted (<= 1e-5 of the elements).  bf16 gates: the one-rounding bounds of test_bf16_storage_layer_local_rounding_is_exact
per layer and image.  Each test prints its per-layer table (worst err / bound per gate) and its wall time.

Two tests run a batch SMALLER than max_batch on an engine that has already run a full one (the ragged last batch of an
epoch on the engine Model._ensure_engine reuses): the workspace is carved for max_batch and still holds the larger step,
while every launch sizes its grid, its statistic rows and its kernel family by the call's B."""
import time

import numpy as np
import pytest
import torch

from oracle import unet_numpy as on
from tests import layer_local as ll

pytestmark = pytest.mark.gpu

C = 3

# kernel instantiations of one training step at configs[1] (B=32, 256x512, fp32) and configs[2] (B=64, 512x1024, P=5,
# bf16) on the default route, and of the configs[4] inference forward (B=128) -- profiles/r03_*launch_table.json
CONV_B32 = {
    "conv_bt_k<2,1,0,16,3,float,2px>", "conv_bt_k<2,1,0,32,3,float>", "conv_bt_k<3,0,0,16,3,float,2px>",
    "conv_bt_k<3,0,0,16,3,float>", "conv_bt_k<3,0,0,32,3,float>", "conv_bt_k<3,0,0,8,3,float,2px>",
    "conv_bt_k<3,0,0,8,3,float>", "conv_bt_k<3,0,1,16,3,float,2px,gb>", "conv_bt_k<3,0,1,16,3,float,gb>",
    "conv_bt_k<3,0,1,32,3,float>", "conv_bt_k<3,0,1,8,3,float,2px,gb,dw>", "conv_bt_k<3,0,2,16,3,float,gb>",
    "conv_bt_k<3,0,2,8,3,float,2px,gb,dw>", "conv_bt_k<3,2,2,8,3,float,gb>", "conv_bx_k<2,1,0,8,32,3,4,float,1img>",
    "conv_bx_k<2,1,0,8,64,3,8,float>", "conv_bx_k<3,0,0,4,64,3,4,float,1img>", "conv_bx_k<3,0,0,8,32,3,4,float,1img>",
    "conv_bx_k<3,0,1,4,64,3,4,float,gb,1img>", "conv_bx_k<3,0,1,8,32,3,4,float,gb,1img>",
    "conv_bx_k<3,0,2,4,64,3,4,float,gb,1img>", "conv_bx_k<3,0,2,8,32,3,4,float,gb,1img>",
    "conv_bx_k<3,2,2,4,32,3,4,float,gb>", "conv_bx_k<3,2,2,4,64,3,4,float,gb>", "conv_dw16_k<2,16,true,float,gb,dz8>",
    "conv_dw16_k<2,16,true,float,gb>", "conv_dw_first_k<float>", "conv_dwbt_k<3,false,16,16,3,float,gb>",
    "conv_dwbt_k<3,false,16,32,3,float>", "conv_dwbt_k<3,false,32,16,3,float,gb>", "conv_dwbt_k<3,false,8,16,3,float,gb>",
    "conv_dwbx_k<2,true,3,float,gb>", "conv_dwbx_k<3,false,3,float,gb>", "conv_first_fwd_k<float>",
    "head_bwd_k<3,8,float>", "head_fwd_k<3,8,float>", "pool_bwd_flat_k<float>", "pool_fwd_k<float>",
    "bn_bwd_apply_k<float>"}
CONV_CFG2 = {
    "conv_bt_k<2,1,0,16,1,unsigned short,2px>", "conv_bt_k<2,1,0,32,1,unsigned short>",
    "conv_bt_k<3,0,0,16,1,unsigned short,2px>", "conv_bt_k<3,0,0,16,1,unsigned short>",
    "conv_bt_k<3,0,0,32,1,unsigned short>", "conv_bt_k<3,0,0,8,1,unsigned short,2px>", "conv_bt_k<3,0,0,8,1,unsigned short>",
    "conv_bt_k<3,0,1,16,1,unsigned short,2px,gb>", "conv_bt_k<3,0,1,16,1,unsigned short,gb>",
    "conv_bt_k<3,0,1,32,1,unsigned short>", "conv_bt_k<3,0,1,8,1,unsigned short,2px,gb,dw>",
    "conv_bt_k<3,0,2,16,1,unsigned short,gb>", "conv_bt_k<3,0,2,8,1,unsigned short,2px,gb,dw>",
    "conv_bt_k<3,2,2,8,1,unsigned short,gb>", "conv_bx_k<2,1,0,4,64,1,4,unsigned short,1img>",
    "conv_bx_k<2,1,0,8,32,1,4,unsigned short,1img>", "conv_bx_k<2,1,0,8,64,1,8,unsigned short>",
    "conv_bx_k<3,0,0,4,64,1,4,unsigned short,1img>", "conv_bx_k<3,0,0,8,32,1,4,unsigned short,1img>",
    "conv_bx_k<3,0,1,4,64,1,4,unsigned short,gb,1img>", "conv_bx_k<3,0,1,8,32,1,4,unsigned short,gb,1img>",
    "conv_bx_k<3,0,2,4,64,1,4,unsigned short,gb,1img>", "conv_bx_k<3,0,2,8,32,1,4,unsigned short,gb,1img>",
    "conv_bx_k<3,2,2,4,32,1,4,unsigned short,gb>", "conv_bx_k<3,2,2,4,64,1,4,unsigned short,gb>",
    "conv_dw_first_k<unsigned short>", "conv_dwbt_k<2,true,16,8,1,unsigned short,gb>",
    "conv_dwbt_k<2,true,32,16,1,unsigned short,gb>", "conv_dwbt_k<3,false,16,16,1,unsigned short,gb>",
    "conv_dwbt_k<3,false,16,32,1,unsigned short>", "conv_dwbt_k<3,false,32,16,1,unsigned short,gb>",
    "conv_dwbt_k<3,false,8,16,1,unsigned short,gb>", "conv_dwbx_k<2,true,1,unsigned short,gb>",
    "conv_dwbx_k<3,false,1,unsigned short,gb>", "conv_first_fwd_k<unsigned short>", "head_bwd_k<3,8,unsigned short>",
    "head_fwd_k<3,8,unsigned short>", "pool_bwd_flat_k<unsigned short,8>", "pool_fwd_k<unsigned short>",
    "bn_bwd_apply8_bf16_k"}
CONV_INFER = {"conv_bt_k<2,1,0,16,3,float,2px>", "conv_bt_k<2,1,0,32,3,float>", "conv_bt_k<3,0,0,16,3,float>",
              "conv_bt_k<3,0,0,16,3,float,2px>", "conv_bt_k<3,0,0,32,3,float>", "conv_bt_k<3,0,0,8,3,float>",
              "conv_bt_k<3,0,0,8,3,float,2px>", "conv_bx_k<2,1,0,4,64,3,4,float,1img>",
              "conv_bx_k<2,1,0,8,32,3,4,float,1img>", "conv_bx_k<3,0,0,4,64,3,4,float,1img>",
              "conv_bx_k<3,0,0,8,32,3,4,float,1img>", "conv_first_fwd_k<float>", "head_fwd_k<3,8,float>",
              "pool_fwd_k<float>"}


# the partial steps on used engines: fp32 B = 7 on a max_batch-32 engine, bf16 B = 5 on a max_batch-8 engine (512x1024, P=5)
# (routing depends on the call's B: at these batch sizes the up-conv forward of the widest level leaves the 8-wave
# double-buffered blocks for the 4-wave two-image ones; everything else is the full-batch set)
CONV_B7_OF_32 = (CONV_B32 - {"conv_bx_k<2,1,0,8,64,3,8,float>"}) | {"conv_bx_k<2,1,0,4,64,3,4,float>"}
CONV_B5_OF_8 = (CONV_CFG2 - {"conv_bx_k<2,1,0,8,64,1,8,unsigned short>"}) | {"conv_bx_k<2,1,0,4,64,1,4,unsigned short>"}


def _compute_kernels(ents):
    return {e["kernel"] for e in ents if e["kernel"].startswith(("conv_", "head_", "pool_", "bn_bwd_apply"))}


def _check_routing(ents, expected):
    got = _compute_kernels(ents)
    print("kernel instantiations:", sorted(got))
    assert got == expected, ("missing", sorted(expected - got), "unexpected", sorted(got - expected))


def _finish(rep, t0, title):
    print(f"\n{title}: per-layer worst err / bound (fp32 and bf16 gates), share of elements not bit-identical "
          f"(bf16 '!=0' columns), relative L2 ('.L2')")
    print(rep.table())
    print(f"{title}: wall time {time.time() - t0:.1f} s")
    assert not rep.failures, "\n".join(rep.failures[:20])


def _params_from_engine(eng):
    """The engine's weights as oracle structures in fp64 (params, BN moving state)."""
    wl, params, state, k = eng.get_weights(), [], [], 0
    for L in eng.layers:
        p = {"kernel": wl[k].astype(np.float64), "bias": wl[k + 1].astype(np.float64)}
        k += 2
        if L["has_bn"]:
            p["gamma"], p["beta"] = wl[k].astype(np.float64), wl[k + 1].astype(np.float64)
            state.append({"moving_mean": wl[k + 2].astype(np.float64), "moving_var": wl[k + 3].astype(np.float64)})
            k += 4
        params.append(p)
    return params, state


def test_configs1_fp32_batch_32_every_layer_every_element():
    """configs[1] as bench.py times it: 256x512, P=4, fp32, batch 32 -- the inputs of
    test_bench_configuration_matches_the_fp64_oracle (randomised BN parameters, 32 distinct scans, dropout step 3)."""
    from oct_image_segmentation_models_amd.engine import UNetEngine
    from tests.test_gpu_fullsize import scans
    t0 = time.time()
    B, H, W, P = 32, 256, 512, 4
    cfg = on.UNetConfig(num_classes=C, start_neurons=8, pool_layers=P)
    params, state = on.init_params(cfg, seed=7, dtype=np.float32, randomize_bn=True)
    eng = UNetEngine(device="cuda:0", input_channels=1, num_classes=C, image_height=H, image_width=W, max_batch=B,
                     training=True, seed=5, init_seed=1)
    eng.set_weights(on.keras_weight_list(params, state))
    img, lab = scans(B, 31)
    for k in range(B):
        img[k] = np.roll(img[k], 5 * k, axis=1); lab[k] = np.roll(lab[k], 5 * k, axis=1)
    x = torch.from_numpy(img).cuda(); l = torch.from_numpy(lab[..., 0].copy()).cuda()
    eng.set_dropout_step(3)
    mask = eng.dropout_mask(B).double()
    eng.profile_begin()
    probs, _ = eng.forward(x, training=True, labels=l)
    eng.loss_dice()
    eng.backward(l, macro=True, loss_scale=1.0)
    _check_routing(eng.profile_end(), CONV_B32)
    p64, _ = _params_from_engine(eng)
    S = ll.engine_stored(eng, B, probs)
    rep = ll.LayerLocal(cfg, p64, S, img, labels=lab[..., 0], dropout_mask=mask, mode="f32", device="cuda:0").run()
    _finish(rep, t0, "configs[1] fp32 B=32 256x512")


def test_configs2_bf16_batch_64_every_layer_every_image():
    """configs[2]: 512x1024, P=5, bf16 storage, batch 64, on the fused route (the BN-backward transform applied by the
    consumers on load: dz of a fused layer is reconstructed from its stored g', z and record).  Then the existing
    small-shape equality at size, on identical inputs: with the same backward-weights kernels on both routes
    (fuse_dw_thin = 0, as test_bn_backward_on_load_equals_the_separate_pass), the two routes' gradients are equal bit for
    bit against the stand-alone BN-backward route (fuse_first_apply = fuse_bn_apply = 0).  (With the default
    fuse_dw_thin = 1 the fused route reduces three layers' dW inside their backward-data launches -- another summation
    order -- and the last bits of the BN-backward means then move every gradient below.)"""
    from oct_image_segmentation_models_amd import _hip
    from oct_image_segmentation_models_amd.common.synthetic import make_scans
    from oct_image_segmentation_models_amd.engine import UNetEngine
    t0 = time.time()
    B, H, W, P = 64, 512, 1024, 5
    cfg = on.UNetConfig(num_classes=C, start_neurons=8, pool_layers=P)
    params, state = on.init_params(cfg, seed=11, dtype=np.float32, randomize_bn=True)
    kw = dict(device="cuda:0", input_channels=1, num_classes=C, image_height=H, image_width=W, max_batch=B,
              training=True, seed=5, init_seed=2, pool_layers=P, dtype="bfloat16")
    img8, lab8 = make_scans(8, H, W, C, seed=41)
    img = np.concatenate([np.roll(img8, 9 * k, axis=2) for k in range(B // 8)])
    lab = np.concatenate([np.roll(lab8, 9 * k, axis=2) for k in range(B // 8)])
    x = torch.from_numpy(img).cuda(); l = torch.from_numpy(lab[..., 0].copy()).cuda()

    def engine(fuse=1, fuse_dw_thin=1):
        try:
            _hip.set_option("fuse_first_apply", fuse); _hip.set_option("fuse_bn_apply", fuse)
            _hip.set_option("fuse_dw_thin", fuse_dw_thin)
            eng = UNetEngine(**kw)
        finally:
            _hip.set_option("fuse_first_apply", 1); _hip.set_option("fuse_bn_apply", 1); _hip.set_option("fuse_dw_thin", 1)
        eng.set_weights(on.keras_weight_list(params, state))
        eng.set_dropout_step(2)
        eng.profile_begin()
        probs, _ = eng.forward(x, training=True, labels=l)
        eng.loss_dice()
        eng.backward(l, macro=True)
        return eng, probs, eng.profile_end()

    def check(eng, probs):
        p64, _ = _params_from_engine(eng)
        S = ll.engine_stored(eng, B, probs)
        return ll.LayerLocal(cfg, p64, S, img, labels=lab[..., 0], dropout_mask=eng.dropout_mask(B).double(), mode="bf16",
                             mfma_mode=_hip.get_option("mfma_mode"), device="cuda:0").run()

    eng, probs, ents = engine()
    _check_routing(ents, CONV_CFG2)
    assert {e["layer"] for e in ents if e["kernel"] == "conv_dwbt_k<2,true,16,8,1,unsigned short,gb>"} == {"dec4.up"}
    assert {e["layer"] for e in ents if e["kernel"] == "bn_bwd_apply8_bf16_k"} == {"enc2.conv0"}
    assert {e["layer"] for e in ents if e["kernel"].endswith(",dw>")} == {"enc0.conv1", f"dec{P - 1}.conv0", f"dec{P - 1}.conv1"}
    nb = len(eng.layers) - 1
    assert sum(eng.debug_layer_fused(li) for li in range(nb)) >= nb - 4
    rep = check(eng, probs)
    del eng
    eng1, _, ents1 = engine(fuse=0, fuse_dw_thin=0)
    assert not any(eng1.debug_layer_fused(li) for li in range(nb))
    assert not any(",gb" in e["kernel"] for e in ents1)
    g_sep = eng1.grads.clone()
    del eng1
    eng2, _, ents2 = engine(fuse=1, fuse_dw_thin=0)
    assert not any(e["kernel"].endswith(",dw>") for e in ents2) and any(",gb" in e["kernel"] for e in ents2)
    differ = [L["name"] for L in eng2.layers if not torch.equal(eng2.grads[L["kernel_off"]:L["beta_off" if L["has_bn"] else "bias_off"] + L["cout"]],
                                                                  g_sep[L["kernel_off"]:L["beta_off" if L["has_bn"] else "bias_off"] + L["cout"]])]
    _finish(rep, t0, "configs[2] bf16 B=64 512x1024 P=5")
    assert not differ, f"fused and stand-alone BN-backward routes differ at configs[2] in {differ}"


def _used_engine_partial_step(eng, cfg, img_full, lab_full, img, lab, mode):
    """One full step at max_batch on ``img_full``, then the step under test on the B < max_batch scans ``img``: returns
    the layer-local report of the partial step and the profile entries of its launches."""
    from oct_image_segmentation_models_amd import _hip
    weights = eng.get_weights()
    x = torch.from_numpy(img_full).cuda(); l = torch.from_numpy(lab_full[..., 0].copy()).cuda()
    eng.set_dropout_step(2)
    eng.forward(x, training=True, labels=l, want_probs=False)
    eng.loss_dice()
    eng.backward(l, macro=True, loss_scale=1.0)
    eng.set_weights(weights)                      # (the moving statistics of the full step are not part of the check)
    B = img.shape[0]
    assert B < eng.cfg.max_batch
    x = torch.from_numpy(img).cuda(); l = torch.from_numpy(lab[..., 0].copy()).cuda()
    eng.set_dropout_step(3)
    mask = eng.dropout_mask(B).double()
    eng.profile_begin()
    probs, _ = eng.forward(x, training=True, labels=l)
    eng.loss_dice()
    eng.backward(l, macro=True, loss_scale=1.0)
    ents = eng.profile_end()
    p64, _ = _params_from_engine(eng)
    S = ll.engine_stored(eng, B, probs)
    rep = ll.LayerLocal(cfg, p64, S, img, labels=lab[..., 0], dropout_mask=mask, mode=mode,
                        mfma_mode=_hip.get_option("mfma_mode"), device="cuda:0").run()
    return rep, ents


def test_configs1_fp32_batch_7_on_an_engine_used_at_32():
    """configs[1] geometry, fp32, max_batch 32: one full B = 32 step, then B = 7 on other scans (the ragged last batch of
    an epoch on the reused engine).  The workspace still holds the larger step; routing depends on the call's B."""
    from oct_image_segmentation_models_amd.engine import UNetEngine
    from tests.test_gpu_fullsize import scans
    t0 = time.time()
    MB, B, H, W, P = 32, 7, 256, 512, 4
    cfg = on.UNetConfig(num_classes=C, start_neurons=8, pool_layers=P)
    params, state = on.init_params(cfg, seed=7, dtype=np.float32, randomize_bn=True)
    eng = UNetEngine(device="cuda:0", input_channels=1, num_classes=C, image_height=H, image_width=W, max_batch=MB,
                     training=True, seed=5, init_seed=1)
    eng.set_weights(on.keras_weight_list(params, state))
    img, lab = scans(MB, 31)
    for k in range(MB):
        img[k] = np.roll(img[k], 5 * k, axis=1); lab[k] = np.roll(lab[k], 5 * k, axis=1)
    img7, lab7 = scans(B, 57)
    for k in range(B):
        img7[k] = np.roll(img7[k], 11 * k + 3, axis=1); lab7[k] = np.roll(lab7[k], 11 * k + 3, axis=1)
    rep, ents = _used_engine_partial_step(eng, cfg, img, lab, img7, lab7, "f32")
    _check_routing(ents, CONV_B7_OF_32)
    _finish(rep, t0, "configs[1] fp32 B=7 of max_batch 32, 256x512")


def test_configs2_bf16_batch_5_on_an_engine_used_at_8():
    """configs[2] geometry (512x1024, P=5), bf16 storage, max_batch 8: one full step, then B = 5 on other scans."""
    from oct_image_segmentation_models_amd.common.synthetic import make_scans
    from oct_image_segmentation_models_amd.engine import UNetEngine
    t0 = time.time()
    MB, B, H, W, P = 8, 5, 512, 1024, 5
    cfg = on.UNetConfig(num_classes=C, start_neurons=8, pool_layers=P)
    params, state = on.init_params(cfg, seed=11, dtype=np.float32, randomize_bn=True)
    eng = UNetEngine(device="cuda:0", input_channels=1, num_classes=C, image_height=H, image_width=W, max_batch=MB,
                     training=True, seed=5, init_seed=2, pool_layers=P, dtype="bfloat16")
    eng.set_weights(on.keras_weight_list(params, state))
    img, lab = make_scans(MB, H, W, C, seed=41)
    img5, lab5 = make_scans(B, H, W, C, seed=67)
    rep, ents = _used_engine_partial_step(eng, cfg, img, lab, img5, lab5, "bf16")
    _check_routing(ents, CONV_B5_OF_8)
    _finish(rep, t0, "configs[2] bf16 B=5 of max_batch 8, 512x1024 P=5")


def test_configs4_inference_batch_128_every_layer():
    """configs[4]: inference, fp32, batch 128, randomised moving statistics (those of
    test_inference_at_batch_128_graph_replay_equals_chunked_forwards): every layer's z with the BN coefficients taken
    from the parameters, the probabilities from the stored head input, the arg-max away from ties."""
    from oct_image_segmentation_models_amd.engine import UNetEngine
    from tests.test_gpu_fullsize import scans
    t0 = time.time()
    B, H, W = 128, 256, 512
    cfg = on.UNetConfig(num_classes=C, start_neurons=8, pool_layers=4)
    eng = UNetEngine(device="cuda:0", input_channels=1, num_classes=C, image_height=H, image_width=W, max_batch=B,
                     training=False, seed=5, init_seed=1)
    rng = np.random.default_rng(0)
    wl = eng.get_weights()
    i = 0
    for L in eng.layers:
        i += 2
        if L["has_bn"]:
            c = L["cout"]
            wl[i] = rng.uniform(0.5, 1.5, c).astype(np.float32); wl[i + 1] = rng.normal(0, 0.1, c).astype(np.float32)
            wl[i + 2] = rng.normal(0, 0.1, c).astype(np.float32); wl[i + 3] = rng.uniform(0.5, 1.5, c).astype(np.float32)
            i += 4
    eng.set_weights(wl)
    img, _ = scans(B, 21)
    for k in range(B):
        img[k] = np.roll(img[k], 3 * k, axis=1)
    x = torch.from_numpy(img).cuda()
    eng.profile_begin()
    probs, am = eng.forward(x, training=False, want_argmax=True)
    _check_routing(eng.profile_end(), CONV_INFER)
    p64, s64 = _params_from_engine(eng)
    S = ll.engine_stored(eng, B, probs, training=False, argmax=am)
    rep = ll.LayerLocal(cfg, p64, S, img, training=False, state=s64, mode="f32", device="cuda:0").run()
    _finish(rep, t0, "configs[4] fp32 inference B=128 256x512")


# ---- production routing at real, non-power-of-two sizes ---------------------------------------------------------------
# OCT B-scans are 496 rows high.  Every conv kernel tiles pixels 32 wide and 4, 8 or 16 rows high and the thin persistent
# kernel walks B * cdiv(W, 32) * cdiv(H, 8) tiles with at most 256 * per_cu blocks: at the sizes below blocks loop over
# many tiles of which some are ragged (the last tile row at 496 = 62 x 8 is full, at 124 and 62 it is not; 432 and 48 are
# no multiples of 32), levels have odd heights (31, 17, 15) and odd widths (27, 23), and the statistic rows of a launch
# count cdiv(H, 2) * cdiv(W, 32) per image.  Same model, gates and default options as the tests above.  Their printed tables:
# profiles/r05_layer_local_ragged.txt.

# Scan seeds.  EXCLUDE_MAX (1e-5 of the elements) caps what the fp32 mask / route exclusions may remove; that the inputs alone
# stay inside it is checked on the CPU by tools/check_exclusions.py: the same LayerLocal on the tensors of a defect-free
# engine (tests/test_layer_local.perfect_engine: the oracle's primitives, same weights, scans, rolls and dropout bits) at
# the tests' own batches reports no failure and excludes 46 of 4.72e8 elements at 496x768 (B = 8), 9 of 1.46e8 at 272x432
# (B = 8), 2 of 5.5e7 for the partial step's scans (B = 3); bf16 480x736 (B = 8): no failure (that mode has no exclusions).
# The inference check excludes nothing by construction.
SCAN_SEED = {(496, 768): 31, (272, 432): 43, (272, 432, "partial"): 57, (480, 736): 41, (496, 768, "infer"): 21}


# Kernel instantiations of these steps (from their first passing run; a tripwire for routing changes, not a correctness
# gate).  At batch 8 / 3 every one is the set of the partial steps above: the routing depends on the kernel shapes and the
# call's B, not on whether the image divides the tiles.
CONV_496x768 = CONV_272x432 = CONV_272x432_B3_OF_8 = CONV_B7_OF_32
CONV_480x736_BF16 = CONV_B5_OF_8
CONV_INFER_496x768 = CONV_INFER


def ragged_scans(n, H, W, seed, step):
    """n synthetic scans at H x W (8 distinct ones, tiled), image k rolled by step * k columns -- labels alongside."""
    from oct_image_segmentation_models_amd.common.synthetic import make_scans
    img8, lab8 = make_scans(8, H, W, C, seed=seed)
    reps = (n + 7) // 8
    img, lab = np.tile(img8, (reps, 1, 1, 1))[:n], np.tile(lab8, (reps, 1, 1, 1))[:n]
    for k in range(n):
        img[k] = np.roll(img[k], step * k, axis=1); lab[k] = np.roll(lab[k], step * k, axis=1)
    return img, lab


def _cdiv(a, b):
    return (a + b - 1) // b


def _check_routing_rules(ents, P, B, H, W):
    """What the routing rules predict at any size (the pinned sets above and below are tripwires, these are the claims):
    the full-resolution 8 -> 8 layers reduce their backward-weights inside their conv_bt_k backward-data launches, and the
    wide kernel and both bf16-pipe backward-weights kernels ran.  That the persistent thin kernel's blocks loop is not
    observable (a profile entry carries no grid): the last line is arithmetic on the test's own constants, a comment that
    the size was chosen so, not a check."""
    dw = {e["layer"] for e in ents if e["kernel"].startswith("conv_bt_k<") and e["kernel"].endswith(",dw>")}
    assert dw == {"enc0.conv1", f"dec{P - 1}.conv0", f"dec{P - 1}.conv1"}, dw
    fams = {e["kernel"].split("<")[0] for e in ents}
    assert {"conv_bt_k", "conv_bx_k", "conv_dwbx_k", "conv_dwbt_k"} <= fams, fams
    # launch_bt: grid = min(B * tiles, 256 * per_cu), per_cu <= 3
    assert B * _cdiv(W, 32) * _cdiv(H, 8) > 256 * 3


def _train_step_layer_local(H, W, P, B, mode, scan_seed, expected, title):
    """One default-route training step at batch B of H x W against the layer-local fp64 model."""
    from oct_image_segmentation_models_amd import _hip
    from oct_image_segmentation_models_amd.engine import UNetEngine
    t0 = time.time()
    cfg = on.UNetConfig(num_classes=C, start_neurons=8, pool_layers=P)
    params, state = on.init_params(cfg, seed=7, dtype=np.float32, randomize_bn=True)
    eng = UNetEngine(device="cuda:0", input_channels=1, num_classes=C, image_height=H, image_width=W, max_batch=B,
                     training=True, seed=5, init_seed=1, pool_layers=P, dtype="bfloat16" if mode == "bf16" else "float32")
    eng.set_weights(on.keras_weight_list(params, state))
    img, lab = ragged_scans(B, H, W, scan_seed, 5)
    x = torch.from_numpy(img).cuda(); l = torch.from_numpy(lab[..., 0].copy()).cuda()
    eng.set_dropout_step(3)
    mask = eng.dropout_mask(B).double()
    eng.profile_begin()
    probs, _ = eng.forward(x, training=True, labels=l)
    eng.loss_dice()
    eng.backward(l, macro=True, loss_scale=1.0)
    ents = eng.profile_end()
    _check_routing(ents, expected)
    _check_routing_rules(ents, P, B, H, W)
    p64, _ = _params_from_engine(eng)
    S = ll.engine_stored(eng, B, probs)
    rep = ll.LayerLocal(cfg, p64, S, img, labels=lab[..., 0], dropout_mask=mask, mode=mode,
                        mfma_mode=_hip.get_option("mfma_mode"), device="cuda:0").run()
    _finish(rep, t0, title)


def test_fp32_batch_8_at_496x768():
    """496x768 (a real B-scan height), P=4, fp32, batch 8: levels 496x768, 248x384, 124x192, 62x96, bottleneck 31x48 --
    rows ragged from 124 down, the width ragged at 48, the bottleneck height odd."""
    _train_step_layer_local(496, 768, 4, 8, "f32", SCAN_SEED[496, 768], CONV_496x768, "fp32 B=8 496x768")


def test_fp32_batch_8_at_272x432():
    """272x432, P=4, fp32, batch 8: bottleneck 17x27; 432 = 13.5 x 32, so every persistent conv_bt_k block walks ragged
    tiles at full resolution, and every level below has a ragged width too (216, 108, 54, 27)."""
    _train_step_layer_local(272, 432, 4, 8, "f32", SCAN_SEED[272, 432], CONV_272x432, "fp32 B=8 272x432")


def test_fp32_batch_3_at_272x432_on_an_engine_used_at_8():
    """272x432, fp32, max_batch 8: one full step, then B = 3 on other scans; the workspace rows were carved for 8."""
    from oct_image_segmentation_models_amd.engine import UNetEngine
    t0 = time.time()
    MB, B, H, W, P = 8, 3, 272, 432, 4
    cfg = on.UNetConfig(num_classes=C, start_neurons=8, pool_layers=P)
    params, state = on.init_params(cfg, seed=7, dtype=np.float32, randomize_bn=True)
    eng = UNetEngine(device="cuda:0", input_channels=1, num_classes=C, image_height=H, image_width=W, max_batch=MB,
                     training=True, seed=5, init_seed=1)
    eng.set_weights(on.keras_weight_list(params, state))
    img, lab = ragged_scans(MB, H, W, SCAN_SEED[272, 432], 5)
    img3, lab3 = ragged_scans(B, H, W, SCAN_SEED[272, 432, "partial"], 11)
    rep, ents = _used_engine_partial_step(eng, cfg, img, lab, img3, lab3, "f32")
    _check_routing(ents, CONV_272x432_B3_OF_8)
    _check_routing_rules(ents, P, B, H, W)
    _finish(rep, t0, "fp32 B=3 of max_batch 8, 272x432")


def test_bf16_batch_8_at_480x736():
    """480x736, P=5, bf16 storage, batch 8, on the fused route (the default): levels down to a 15x23 bottleneck, odd
    heights and widths from 30x46 down."""
    _train_step_layer_local(480, 736, 5, 8, "bf16", SCAN_SEED[480, 736], CONV_480x736_BF16, "bf16 B=8 480x736 P=5")


def test_inference_batch_16_at_496x768_and_graph_replay():
    """Inference, fp32, batch 16 at 496x768, randomised moving statistics: every layer's z, the probabilities, the
    arg-max away from ties; then the same forward captured into a hipGraph and replayed, bit-equal to the direct call."""
    from oct_image_segmentation_models_amd.engine import UNetEngine
    t0 = time.time()
    B, H, W = 16, 496, 768
    cfg = on.UNetConfig(num_classes=C, start_neurons=8, pool_layers=4)
    eng = UNetEngine(device="cuda:0", input_channels=1, num_classes=C, image_height=H, image_width=W, max_batch=B,
                     training=False, seed=5, init_seed=1)
    rng = np.random.default_rng(0)
    wl = eng.get_weights()
    i = 0
    for L in eng.layers:
        i += 2
        if L["has_bn"]:
            c = L["cout"]
            wl[i] = rng.uniform(0.5, 1.5, c).astype(np.float32); wl[i + 1] = rng.normal(0, 0.1, c).astype(np.float32)
            wl[i + 2] = rng.normal(0, 0.1, c).astype(np.float32); wl[i + 3] = rng.uniform(0.5, 1.5, c).astype(np.float32)
            i += 4
    eng.set_weights(wl)
    img, _ = ragged_scans(B, H, W, SCAN_SEED[496, 768, "infer"], 3)
    x = torch.from_numpy(img).cuda()
    eng.profile_begin()
    probs, am = eng.forward(x, training=False, want_argmax=True)
    ents = eng.profile_end()
    _check_routing(ents, CONV_INFER_496x768)
    assert {"conv_bt_k", "conv_bx_k"} <= {e["kernel"].split("<")[0] for e in ents}
    assert B * _cdiv(W, 32) * _cdiv(H, 8) > 256 * 3          # (a comment, as in _check_routing_rules: the size makes the thin kernel's blocks loop)
    probs, am = probs.clone(), am.clone()
    p64, s64 = _params_from_engine(eng)
    S = ll.engine_stored(eng, B, probs, training=False, argmax=am)
    rep = ll.LayerLocal(cfg, p64, S, img, training=False, state=s64, mode="f32", device="cuda:0").run()
    xb = x.clone()
    gp, gam = eng.graph_capture(xb, want_probs=True, want_argmax=True)
    for _ in range(2):
        gp.zero_(); gam.zero_()
        eng.graph_launch(); torch.cuda.synchronize()
        assert torch.equal(gp, probs) and torch.equal(gam, am)
    _finish(rep, t0, "fp32 inference B=16 496x768")
