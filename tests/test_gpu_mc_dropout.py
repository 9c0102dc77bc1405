"""GPU tests of the Monte-Carlo dropout prediction: ``oct_mc_update`` against its numpy restatement, one stochastic sample
of ``oct_unet_infer`` (kind MC) against the fp64 oracle with the replayed mask, the reuse of the encoder across samples, the
absence of side effects on the handle, the known answer without dropout, and ``predict`` with ``mc_samples``."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest
import torch

from oracle import unet_numpy as on
from tests.helpers import save_untrained_model, tree_equal
from tests.mc_cases import ENTROPY_TOL, forward_mc_oracle, softmax_stack

pytestmark = pytest.mark.gpu


def _utils():
    from oct_image_segmentation_models_amd.common import utils as cu
    return cu


def make(B, H, W, Cn, sn, P, training=False, max_batch=None, dtype="float32", dropout_rate=0.5, seed=0):
    from oct_image_segmentation_models_amd.engine import UNetEngine
    cfg = on.UNetConfig(num_classes=Cn, start_neurons=sn, pool_layers=P, dropout_rate=dropout_rate)
    params, state = on.init_params(cfg, seed=seed, dtype=np.float32, randomize_bn=True)
    eng = UNetEngine(device="cuda:0", input_channels=1, num_classes=Cn, image_height=H, image_width=W, start_neurons=sn,
                     pool_layers=P, max_batch=max_batch or B, training=training, seed=seed + 100, dtype=dtype,
                     dropout_rate=dropout_rate)
    eng.set_weights(on.keras_weight_list(params, state))
    p64 = [{k: v.astype(np.float64) for k, v in p.items()} for p in params]
    s64 = [{k: v.astype(np.float64) for k, v in s.items()} for s in state]
    return cfg, eng, p64, s64


def scans(B, H, W, Cn, seed=5):
    images, _ = on.synth_scans(B, H, W, Cn, seed=seed)
    return images, torch.from_numpy(images).cuda()


def mc(eng, x, T, step0, mean=True):
    """``forward_mc`` -> host copies (the engine's buffers are refilled by the next call)."""
    out = eng.forward_mc(x, T, step0=step0, want_mean_probs=mean)
    return {k: v.cpu().numpy().copy() for k, v in out.items()}


@pytest.fixture(scope="module")
def small_engine():
    return make(1, 16, 32, 3, 8, 2)[1]


# ---- the reduction kernel against numpy --------------------------------------------------------------------------------
def run_sequence(eng, stack):
    """``oct_mc_update`` over the samples of ``stack`` in order -> the four maps on the host."""
    from oct_image_segmentation_models_amd import _hip
    T, B, H, W, Cn = stack.shape
    dev = eng.device
    ws = torch.empty(int(_hip.lib().oct_mc_workspace_bytes(B, H, W, Cn)), dtype=torch.uint8, device=dev)
    ws.fill_(0xFF)                                          # NaN patterns: sample 0 must assign, never add
    outs = dict(mean_probs=torch.zeros((B, H, W, Cn), dtype=torch.float32, device=dev),
                argmax=torch.full((B, H, W), 255, dtype=torch.uint8, device=dev),
                entropy=torch.full((B, H, W), -1.0, dtype=torch.float32, device=dev),
                mutual_info=torch.full((B, H, W), -1.0, dtype=torch.float32, device=dev))
    dstack = torch.from_numpy(stack).to(dev)
    for t in range(T):
        eng.mc_update(dstack[t], t, T, ws, **outs)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in outs.items()}


@pytest.mark.parametrize("shape", [(3, 5, 7, 3, 1), (1, 16, 32, 2, 2), (2, 9, 13, 8, 5), (1, 3, 1031, 32, 3)],
                         ids=lambda s: "x".join(map(str, s)))
def test_mc_update_equals_the_numpy_restatement(small_engine, shape):
    """(B,H,W,C,T): pixel counts that divide no block or vector width; the float4 path with whole items (16x32x2) and with a
    tail (2x9x13x8: 234 pixels), the per-pixel path for C = 3 at an odd count and for C = 32."""
    B, H, W, Cn, T = shape
    stack = softmax_stack((T, B, H, W, Cn), seed=sum(shape))
    assert (stack == 0).any() and (stack == 1).any()
    got = run_sequence(small_engine, stack)
    m32, a32, _, _ = _utils().mc_reduce_reference(stack, np.float32)
    _, _, e64, i64 = _utils().mc_reduce_reference(stack, np.float64)
    assert np.array_equal(got["mean_probs"].view(np.uint32), m32.view(np.uint32))          # bit for bit
    assert np.array_equal(got["argmax"], a32)
    e_err, i_err = np.abs(got["entropy"] - e64).max(), np.abs(got["mutual_info"] - i64).max()
    print(f"{shape}: entropy err {e_err:.3e}, mutual_info err {i_err:.3e}")
    assert e_err <= ENTROPY_TOL and i_err <= ENTROPY_TOL
    assert (got["mutual_info"] >= 0).all()
    again = run_sequence(small_engine, stack)
    for k in got:
        assert got[k].tobytes() == again[k].tobytes(), k


def test_mc_update_writes_only_the_maps_that_are_asked_for(small_engine):
    stack = softmax_stack((2, 1, 8, 16, 3), seed=4)
    full = run_sequence(small_engine, stack)
    dev = small_engine.device
    from oct_image_segmentation_models_amd import _hip
    ws = torch.empty(int(_hip.lib().oct_mc_workspace_bytes(1, 8, 16, 3)), dtype=torch.uint8, device=dev)
    ent = torch.empty((1, 8, 16), dtype=torch.float32, device=dev)
    d = torch.from_numpy(stack).to(dev)
    small_engine.mc_update(d[0], 0, 2, ws)
    small_engine.mc_update(d[1], 1, 2, ws, entropy=ent)
    assert np.array_equal(ent.cpu().numpy(), full["entropy"])


# ---- one stochastic sample against the oracle --------------------------------------------------------------------------
PARITY = [
    # B, H, W, C, sn, P, training, max_batch          layer k = the up-conv behind the bottleneck: sn 2^P -> sn 2^(P-1) channels
    (3, 16, 32, 3, 8, 2, False, 4),      # 32 -> 16: fp32-pipe tile kernel (the thin bf16-pipe kernel applies no dropout); partial batch
    (2, 20, 36, 2, 4, 2, False, None),   # 16 -> 8: the 8-output-channel route; ragged 20x36, 10x18, 5x9
    (1, 16, 32, 8, 16, 2, False, None),  # 64 -> 32: the wide bf16-pipe kernel in its dropout form
    (1, 20, 36, 8, 16, 2, False, None),
    (1, 20, 36, 3, 40, 2, False, None),  # 160 -> 80 and the channel-streaming head
    (2, 16, 32, 3, 40, 2, False, None),
    (2, 16, 32, 3, 8, 1, False, None),   # pool_layers 1: 16 -> 8 at full resolution
    (2, 20, 36, 3, 8, 2, True, None),    # a training handle
    (2, 16, 32, 2, 16, 2, True, None),
]


@pytest.mark.parametrize("case", PARITY, ids=lambda c: "-".join(map(str, c)))
def test_one_sample_equals_the_oracle_with_the_replayed_mask(case):
    B, H, W, Cn, sn, P, training, max_batch = case
    cfg, eng, p64, s64 = make(B, H, W, Cn, sn, P, training=training, max_batch=max_batch)
    images, x = scans(B, H, W, Cn)
    xin = on.preprocess_u8(images, np.float64)
    for step in (3, 1 << 40):
        got = mc(eng, x, 1, step)                                   # T = 1: m = p * 1.0f, the mean IS the sample
        eng.set_dropout_step(step)
        mask = eng.dropout_mask(B).cpu().numpy()
        assert 0.3 < mask.mean() < 0.7
        ref = forward_mc_oracle(cfg, p64, s64, xin, mask)
        err = float(np.abs(got["mean_probs"] - ref).max())
        print(f"{case} step {step}: probs err {err:.3e}")
        assert err < 1e-4                                           # the project's tolerance on probabilities
        assert (got["argmax"] == got["mean_probs"].argmax(-1)).all()
        assert (got["mutual_info"] == 0).all()
    plain, _ = on.forward(cfg, p64, s64, xin, training=False)
    assert np.abs(got["mean_probs"] - plain).max() > 1e-3           # and the dropout did something


def test_one_sample_in_bf16_storage():
    """The tolerance of the bf16 cases of tests/test_gpu_parity.py on probabilities (max < 8e-2, mean < 1.5e-2)."""
    B, H, W, Cn, sn, P = 2, 32, 64, 3, 8, 2
    cfg, eng, p64, s64 = make(B, H, W, Cn, sn, P, training=True, dtype="bfloat16")
    images, x = scans(B, H, W, Cn, seed=97)
    got = mc(eng, x, 1, 3)
    eng.set_dropout_step(3)
    mask = eng.dropout_mask(B).cpu().numpy()
    e = np.abs(got["mean_probs"] - forward_mc_oracle(cfg, p64, s64, on.preprocess_u8(images, np.float64), mask))
    print(f"bf16: probs err max {e.max():.3e} mean {e.mean():.3e}")
    assert e.max() < 8e-2 and e.mean() < 1.5e-2


# ---- the encoder is reused, exactly --------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [(3, 16, 32, 3, 8, 2), (2, 20, 36, 8, 16, 2)], ids=lambda c: "-".join(map(str, c)))
def test_three_samples_equal_three_single_samples_reduced(case):
    B, H, W, Cn, sn, P = case
    _, eng, _, _ = make(B, H, W, Cn, sn, P, max_batch=B + 1)
    _, x = scans(B, H, W, Cn)
    s = 7
    singles = np.stack([mc(eng, x, 1, s + t)["mean_probs"] for t in range(3)])
    assert not np.array_equal(singles[0], singles[1])
    got = mc(eng, x, 3, s)
    m32, a32, _, _ = _utils().mc_reduce_reference(singles, np.float32)
    _, _, e64, i64 = _utils().mc_reduce_reference(singles, np.float64)
    assert np.array_equal(got["mean_probs"].view(np.uint32), m32.view(np.uint32)) and np.array_equal(got["argmax"], a32)
    assert np.abs(got["entropy"] - e64).max() <= ENTROPY_TOL and np.abs(got["mutual_info"] - i64).max() <= ENTROPY_TOL
    assert got["mutual_info"].max() > 1e-4


# ---- no side effects --------------------------------------------------------------------------------------------------
def test_forward_mc_leaves_the_handle_as_it_was():
    B, H, W, Cn = 2, 16, 32, 3
    _, eng, _, _ = make(B, H, W, Cn, 8, 2, training=True)
    _, x = scans(B, H, W, Cn)
    eng.set_dropout_step(5)
    mask0 = eng.dropout_mask(B).clone()
    probs0 = eng.forward(x, training=False)[0].clone()
    params0, state0 = eng.params.clone(), eng.state.clone()
    mc(eng, x, 3, 11)
    assert torch.equal(eng.dropout_mask(B), mask0)
    assert torch.equal(eng.params, params0) and torch.equal(eng.state, state0)
    assert torch.equal(eng.forward(x, training=False)[0], probs0)
    # a training step still draws step 5's mask first (set_dropout_step, then the first forward does not advance)
    lab = torch.zeros((B, H, W), dtype=torch.uint8, device=eng.device)
    p_a = eng.forward(x, training=True, labels=lab)[0].clone()
    eng.state.copy_(state0)
    eng.set_dropout_step(5)
    assert torch.equal(eng.forward(x, training=True, labels=lab)[0], p_a)
    # the Dice sums of a forward are dropped by forward_mc: the loss needs a new forward
    from oct_image_segmentation_models_amd._hip import OctError
    mc(eng, x, 1, 0)
    with pytest.raises(OctError, match="forward with io.labels"):
        eng.loss_dice()


def test_forward_mc_argument_errors_launch_nothing():
    from oct_image_segmentation_models_amd import _hip
    B, H, W, Cn = 2, 16, 32, 3
    _, eng, _, _ = make(B, H, W, Cn, 8, 2)
    _, x = scans(B, H, W, Cn)
    b = eng._mc_buffers(B)
    for k in ("mean_probs", "entropy", "mutual_info"):
        b[k].fill_(-7.0)
    out = _hip.McOut(b["mean_probs"].data_ptr(), b["argmax"].data_ptr(), b["entropy"].data_ptr(), b["mutual_info"].data_ptr())
    lib, need = _hip.lib(), b["ws"].numel()
    assert need == lib.oct_mc_workspace_bytes(B, H, W, Cn)

    def call(x_ptr=x.data_ptr(), Bn=B, T=4, scratch=b["scratch"].data_ptr(), ws=b["ws"].data_ptr(), ws_bytes=need, o=out):
        d = _hip.Infer(x_dev=x_ptr, x_is_u8=1, B=Bn, kind=_hip.INFER_MC, T=T, step0=0, probs_scratch_dev=scratch, ws_dev=ws,
                       ws_bytes=ws_bytes, H=H, W=W, out=o or _hip.McOut())      # the maps are in the descriptor: "no out" is no map
        return lib.oct_unet_infer(eng._h, C.byref(d), None), lib.oct_last_error().decode()

    for kw, msg in ((dict(x_ptr=None), "null"), (dict(scratch=None), "null"), (dict(ws=None), "null"), (dict(o=None), "null"),
                    (dict(Bn=0), "B out of range"), (dict(Bn=3), "B out of range"), (dict(T=0), "T out of range"),
                    (dict(T=65), "T out of range"), (dict(ws_bytes=need - 1), "workspace too small"),
                    (dict(scratch=b["mean_probs"].data_ptr()), "overlaps")):
        rc, err = call(**kw)
        assert rc < 0 and msg in err, (kw, rc, err)
    torch.cuda.synchronize()
    assert all((b[k] == -7.0).all() for k in ("mean_probs", "entropy", "mutual_info"))
    with pytest.raises(_hip.OctError, match="samples"):
        eng.forward_mc(x, 65)
    assert call()[0] == 0


# ---- known answer -----------------------------------------------------------------------------------------------------
def test_without_dropout_the_samples_are_the_plain_prediction():
    """p + p, 2p + p (+ p) and 4p * 0.25 return p exactly (a tie of 3p rounds to the even 4p): the mean is the plain inference
    output bit for bit, and the mutual information is rounding alone."""
    B, H, W, Cn = 2, 20, 36, 3
    _, eng, _, _ = make(B, H, W, Cn, 8, 2, dropout_rate=0.0)
    _, x = scans(B, H, W, Cn)
    probs, am = eng.forward(x, training=False, want_argmax=True)
    got = mc(eng, x, 4, 2)
    assert np.array_equal(got["mean_probs"].view(np.uint32), probs.cpu().numpy().view(np.uint32))
    assert np.array_equal(got["argmax"], am.cpu().numpy())
    assert got["mutual_info"].max() <= ENTROPY_TOL and (got["mutual_info"] >= 0).all()
    _, _, e64, _ = _utils().mc_reduce_reference(probs.cpu().numpy()[None], np.float64)
    assert np.abs(got["entropy"] - e64).max() <= ENTROPY_TOL


# ---- Model.predict_mc and the workflow ------------------------------------------------------------------------------------
N_IMG, H_, W_, CC, SN, P_, BATCH = 5, 16, 32, 3, 8, 2, 2


def test_predict_mc_equals_forward_mc_per_batch():
    from oct_image_segmentation_models_amd.models.engine_model import Model
    images, _ = on.synth_scans(N_IMG, H_, W_, CC, seed=21)
    cfg = on.UNetConfig(num_classes=CC, start_neurons=SN, pool_layers=P_)
    model = Model(name="unet", config=dict(input_channels=1, num_classes=CC, image_height=H_, image_width=W_, start_neurons=SN,
                                           pool_layers=P_))
    model.set_weights(on.keras_weight_list(*on.init_params(cfg, seed=3, dtype=np.float32, randomize_bn=True)))
    mean, ent, mi = model.predict_mc(images, 4, batch_size=BATCH, step0=6)
    assert mean.shape == (N_IMG, H_, W_, CC) and ent.shape == mi.shape == (N_IMG, H_, W_)
    assert mean.dtype == ent.dtype == mi.dtype == np.float32
    eng = model._engine
    for lo in range(0, N_IMG, BATCH):
        got = mc(eng, torch.from_numpy(images[lo:lo + BATCH]).cuda(), 4, 6)
        assert np.array_equal(mean[lo:lo + BATCH], got["mean_probs"]) and np.array_equal(ent[lo:lo + BATCH], got["entropy"])
        assert np.array_equal(mi[lo:lo + BATCH], got["mutual_info"])
    # float input already in [0,1] is the same prediction as the raw bytes, as for predict
    mean_f, _, _ = model.predict_mc(on.preprocess_u8(images, np.float32), 4, batch_size=BATCH, step0=6)
    assert np.array_equal(mean_f, mean)
    labels, maps, e2, i2 = model.predict_labels(images, batch_size=BATCH, want_maps=True, mc_samples=4, mc_step0=6)
    assert np.array_equal(e2, ent) and np.array_equal(i2, mi) and np.array_equal(labels, mean.argmax(-1))


@pytest.mark.parametrize("soft", [False, True])
def test_both_pipeline_sources_carry_the_mean_prediction_and_the_maps(tmp_path, soft):
    """``BatchedPredictor`` (uint8 images, the fixed input buffer, pinned double buffers over three batches) and
    ``host_batches`` (float images) against ``forward_mc`` on the same batches; with ``soft_maps`` the boundary maps are
    those of the mean probabilities."""
    from oct_image_segmentation_models_amd.evaluation.pipeline import InferenceRun
    from oct_image_segmentation_models_amd.models.engine_model import load_model
    images, _ = on.synth_scans(N_IMG, H_, W_, CC, seed=21)
    model = load_model(save_untrained_model(tmp_path, H_, W_, CC, SN, P_))
    with InferenceRun(model, images, BATCH, CC, soft_maps=soft, mc_samples=3, mc_step0=2) as run:
        dev = list(run)
    with InferenceRun(model, images.astype(np.float32), BATCH, CC, soft_maps=soft, mc_samples=3, mc_step0=2) as run:
        host = list(run)
    with InferenceRun(model, images, BATCH, CC, soft_maps=soft) as run:
        plain = list(run)
    assert [(b.lo, b.hi) for b in dev] == [(b.lo, b.hi) for b in host] == [(0, 2), (2, 4), (4, 5)]
    eng = model._ensure_engine(BATCH, False)
    fimg = images.astype(np.float32) / np.float32(255.0)                        # what host_batches hands the engine
    for b, h, p in zip(dev, host, plain):
        for rec, x in ((b, images[b.lo:b.hi]), (h, fimg[b.lo:b.hi])):
            got = mc(eng, torch.from_numpy(np.ascontiguousarray(x)).cuda(), 3, 2)
            maps = (eng.boundary_maps_soft(torch.from_numpy(got["mean_probs"]).cuda()) if soft
                    else eng.boundary_maps(torch.from_numpy(got["argmax"]).cuda())).cpu().numpy()
            assert rec.entropy.dtype == np.float32 and rec.entropy.shape == (b.hi - b.lo, H_, W_)
            assert np.array_equal(rec.entropy, got["entropy"]) and np.array_equal(rec.mutual_info, got["mutual_info"])
            assert np.array_equal(rec.labels, got["argmax"]) and np.array_equal(rec.maps, maps)
        assert p.entropy is None and p.mutual_info is None and len(p) == len(b)


def test_predict_with_mc_samples(tmp_path):
    from oct_image_segmentation_models_amd.common import h5io, png, utils as cu
    from oct_image_segmentation_models_amd.common.dataset import Dataset
    from oct_image_segmentation_models_amd.models.engine_model import load_model
    from oct_image_segmentation_models_amd.prediction import predict
    from oct_image_segmentation_models_amd.prediction.prediction_parameters import PredictionParams, PredictionSaveParams
    images, _ = on.synth_scans(N_IMG, H_, W_, CC, seed=21)
    save_untrained_model(tmp_path, H_, W_, CC, SN, P_)

    def run(name, **kw):
        ds = Dataset(images, [Path(f"volume_{i}.tiff") for i in range(N_IMG)], [tmp_path / name / f"image_{i}" for i in range(N_IMG)])
        pp = PredictionParams(model_path=tmp_path / "model" / "model.npz", mlflow_tracking_uri=None, mlflow_run_uuid=None,
                              dataset=ds, config_output_dir=tmp_path / name, save_params=PredictionSaveParams(),
                              graph_search=True, batch_size=BATCH, **kw)
        pp.gs_workers = 1
        return predict(pp)

    outs = run("mc", mc_samples=4, mc_step0=6, png_plots=True)
    # the same numbers from the model itself: batches of BATCH in order, the same steps for every batch
    mean, ent, mi = load_model(tmp_path / "model" / "model.npz").predict_mc(images, 4, batch_size=BATCH, step0=6)
    assert len(outs) == N_IMG
    for i, o in enumerate(outs):
        f = h5io.load(o.image_output_dir / "prediction_info.hdf5")
        for k in ("predictive_entropy", "mutual_information"):
            assert f[k].dtype == np.float32 and f[k].shape == (H_, W_), k
        e, m = f["predictive_entropy"], f["mutual_information"]
        assert np.array_equal(e, ent[i]) and np.array_equal(m, mi[i])
        assert np.array_equal(o.predictive_entropy, e) and np.array_equal(o.mutual_information, m)
        assert (e >= 0).all() and (e <= np.log(CC) + ENTROPY_TOL).all() and (m >= 0).all() and (m <= e + ENTROPY_TOL).all()
        assert int(f["attr:mc_samples"]) == 4
        assert np.array_equal(f["predicted_labels"], mean[i].argmax(-1)) and np.array_equal(o.predicted_labels, mean[i].argmax(-1))
        binary = cu.convert_predictions_to_maps_semantic(cu.labels_to_categorical(o.predicted_labels[None], CC))[0]
        assert np.array_equal(o.boundary_maps, binary)               # everything behind the arg-max works on the mean prediction
        assert o.gs_pred_segs.shape == (CC - 1, W_)
        pic = png.read_rgba(o.image_output_dir / "uncertainty_map.png")
        want = cu.entropy_to_u8(e, CC)
        assert pic.shape == (H_, W_, 4) and (pic[..., 3] == 255).all()
        assert all(np.array_equal(pic[..., c], want) for c in range(3))
        assert (o.image_output_dir / "segmentation_map.png").exists()
    assert ent.max() > 0.05 and mi.max() > 1e-3
    cfg = h5io.load(tmp_path / "mc" / "prediction_params.hdf5")
    assert int(cfg["attr:mc_samples"]) == 4 and int(cfg["attr:mc_step0"]) == 6

    # mc_samples=0 is the deterministic path: the same files as a run that never names the parameter, nothing new in them
    plain, zero = run("plain"), run("zero", mc_samples=0)
    tree_equal(tmp_path / "plain", tmp_path / "zero", ["prediction_info.hdf5", "graph_search_prediction_info.hdf5"])
    labels = load_model(tmp_path / "model" / "model.npz").predict_labels(images, batch_size=BATCH)
    for i, (a, b) in enumerate(zip(plain, zero)):
        assert a.predictive_entropy is None and b.predictive_entropy is None and b.mutual_information is None
        assert np.array_equal(b.predicted_labels, labels[i])
        f = h5io.load(b.image_output_dir / "prediction_info.hdf5")
        assert sorted(k for k in f if not k.startswith("attr:")) == ["boundary_maps", "predicted_labels", "raw_image"]
        assert "attr:mc_samples" not in f and not (b.image_output_dir / "uncertainty_map.png").exists()
    for name in ("plain", "zero"):
        cfg = h5io.load(tmp_path / name / "prediction_params.hdf5")
        assert "attr:mc_samples" not in cfg and "attr:mc_step0" not in cfg
