"""GPU tests of test-time augmentation: ``oct_flip_batch`` and ``oct_tta_update`` against their numpy restatements and against
``oct_mc_update``, ``forward_tta`` and its captured graph against the per-view forwards, the padded variant against the native
engine of the padded size, and the switch through ``InferenceRun``, ``predict`` and ``evaluate_model``."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest
import torch

from oracle import unet_numpy as on
from tests.helpers import save_untrained_model, tree_equal
from tests.mc_cases import ENTROPY_TOL, softmax_stack

pytestmark = pytest.mark.gpu

MAPS = ("mean_probs", "argmax", "entropy", "mutual_info")
NAMES = ("identity", "flip_lr", "flip_ud", "flip_both")


def _utils():
    from oct_image_segmentation_models_amd.common import utils as cu
    return cu


def _up(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()            # a copy: the shared stacks are read only


def make(B, H, W, Cn, sn, P, training=False, dtype="float32", seed=0):
    from oct_image_segmentation_models_amd.engine import UNetEngine
    cfg = on.UNetConfig(num_classes=Cn, start_neurons=sn, pool_layers=P)
    params, state = on.init_params(cfg, seed=seed, dtype=np.float32, randomize_bn=True)
    eng = UNetEngine(device="cuda:0", input_channels=1, num_classes=Cn, image_height=H, image_width=W, start_neurons=sn,
                     pool_layers=P, max_batch=B, training=training, seed=seed + 100, dtype=dtype)
    eng.set_weights(on.keras_weight_list(params, state))
    return eng


def host(d):
    """A dict of device maps -> host copies (the engine's buffers are refilled by the next call)."""
    torch.cuda.synchronize()
    return {k: v.cpu().numpy().copy() for k, v in d.items()}


def same_bytes(a, b, keys=MAPS):
    for k in keys:
        assert a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), k


@pytest.fixture(scope="module")
def small_engine():
    return make(1, 16, 32, 3, 8, 2)


# ---- 1. oct_flip_batch ---------------------------------------------------------------------------------------------------------
FLIP_CASES = [(3, 5, 7, 1), (2, 8, 16, 1), (1, 16, 36, 4), (2, 9, 13, 12), (1, 3, 1031, 32), (2, 1, 8, 4), (2, 8, 1, 4)]


@pytest.mark.parametrize("case", FLIP_CASES, ids=lambda c: "x".join(map(str, c)))
def test_flip_batch_equals_flip_reference(small_engine, case):
    """(B,H,W,pixel_bytes): rows that are and are not whole dwords, one-byte, 12-byte and 32-byte pixels, a single row, a
    single column, a row longer than one block.  Aligned buffers take the dword path where the rows allow it; the same
    buffers offset by one byte take the byte path.  Sentinel bytes around the output stay."""
    from oct_image_segmentation_models_amd import _hip
    B, H, W, pb = case
    n = B * H * W * pb
    src = np.random.default_rng(sum(case)).integers(0, 256, (B, H, W, pb), dtype=np.uint8)
    lib, stream = _hip.lib(), C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for off in (0, 1):
        s_arena = torch.zeros(n + 32, dtype=torch.uint8, device="cuda")
        s_arena[16 + off:16 + off + n] = _up(src.reshape(-1))
        for view in range(4):
            d_arena = torch.full((n + 64,), 0x5A, dtype=torch.uint8, device="cuda")
            rc = lib.oct_flip_batch(s_arena.data_ptr() + 16 + off, B, H, W, pb, view, d_arena.data_ptr() + 32 + off, stream)
            assert rc == 0, lib.oct_last_error()
            got = d_arena.cpu().numpy()
            want = _utils().flip_reference(src, view)
            assert np.array_equal(got[32 + off:32 + off + n], want.reshape(-1)), (off, view)
            assert (got[:32 + off] == 0x5A).all() and (got[32 + off + n:] == 0x5A).all(), (off, view)


def test_flip_of_tensors_by_name(small_engine):
    eng, cu = small_engine, _utils()
    rng = np.random.default_rng(3)
    for a in (rng.integers(0, 256, (2, 6, 10, 1), dtype=np.uint8), rng.normal(size=(2, 6, 10, 3)).astype(np.float32),
              rng.normal(size=(3, 5, 7)).astype(np.float32), rng.integers(0, 9, (1, 4, 9), dtype=np.uint8)):
        for v, name in enumerate(NAMES):
            assert np.array_equal(eng.flip(_up(a), name).cpu().numpy(), cu.flip_reference(a, v))
            assert np.array_equal(eng.flip(_up(a), v).cpu().numpy(), cu.flip_reference(a, v))
    from oct_image_segmentation_models_amd._hip import OctError
    t = _up(np.zeros((1, 4, 4), np.uint8))
    with pytest.raises(OctError, match="unknown view"):
        eng.flip(t, "rot90")
    with pytest.raises(OctError, match="overlaps"):
        eng.flip(t, 1, out=t)


def test_flip_batch_argument_errors_launch_nothing():
    from oct_image_segmentation_models_amd import _hip
    lib, stream = _hip.lib(), C.c_void_p(torch.cuda.current_stream().cuda_stream)
    B, H, W, pb = 2, 4, 8, 4
    n = B * H * W * pb
    arena = torch.full((4 * n,), 0x5A, dtype=torch.uint8, device="cuda")
    src, dst = arena.data_ptr(), arena.data_ptr() + 2 * n

    def call(src=src, B=B, H=H, W=W, pb=pb, view=3, dst=dst):
        return lib.oct_flip_batch(src, B, H, W, pb, view, dst, stream)

    for kw in (dict(src=None), dict(dst=None), dict(B=0), dict(H=-1), dict(W=0), dict(pb=3), dict(pb=64), dict(view=4), dict(view=-1),
               dict(dst=src), dict(dst=src + n - 1), dict(dst=src + 1)):
        assert call(**kw) < 0 and b"flip_batch" in lib.oct_last_error(), kw
    torch.cuda.synchronize()
    assert bool((arena == 0x5A).all())
    arena[:n] = _up(np.arange(n, dtype=np.uint8))
    assert call() == 0
    torch.cuda.synchronize()
    assert bool((arena[n:2 * n] == 0x5A).all()) and bool((arena[3 * n:] == 0x5A).all()) and not bool((arena[2 * n:3 * n] == 0x5A).all())


# ---- 2. oct_tta_update ------------------------------------------------------------------------------------------------------------
def run_sequence(eng, stack, views=None, only=MAPS):
    """``oct_tta_update`` (``views`` given) or ``oct_mc_update`` over the samples of ``stack`` in order -> the maps on the host."""
    from oct_image_segmentation_models_amd import _hip
    T, B, H, W, Cn = stack.shape
    dev = eng.device
    ws = torch.empty(int(_hip.lib().oct_mc_workspace_bytes(B, H, W, Cn)), dtype=torch.uint8, device=dev)
    ws.fill_(0xFF)                                          # NaN patterns: sample 0 must assign, never add
    outs = dict(mean_probs=torch.zeros((B, H, W, Cn), dtype=torch.float32, device=dev),
                argmax=torch.full((B, H, W), 255, dtype=torch.uint8, device=dev),
                entropy=torch.full((B, H, W), -1.0, dtype=torch.float32, device=dev),
                mutual_info=torch.full((B, H, W), -1.0, dtype=torch.float32, device=dev))
    given = {k: outs[k] for k in only}
    dstack = _up(stack)
    for t in range(T):
        if views is None:
            eng.mc_update(dstack[t], t, T, ws, **given)
        else:
            eng.tta_update(dstack[t], views[t], t, T, ws, **given)
    return host(outs)


TTA_SHAPES = [(3, 1, 5, 7, 3), (4, 2, 16, 32, 2), (4, 1, 6, 36, 3), (2, 5, 9, 13, 8), (2, 3, 1, 1031, 32)]


@pytest.fixture(scope="module")
def stacks():
    """The softmax stacks of TTA_SHAPES, made once and shared (read only)."""
    out = {s: softmax_stack(s, seed=sum(s)) for s in TTA_SHAPES}
    for a in out.values():
        a.setflags(write=False)
    return out


@pytest.mark.parametrize("shape", TTA_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_tta_update_equals_the_numpy_restatement(small_engine, stacks, shape):
    """(T,B,H,W,C): the float4 path (W % 4 == 0 and C <= 8: 16x32x2, 6x36x3 with its 9 items per row) and the per-pixel path
    (odd W, C = 32, a single row longer than a block), the view codes cycling through 0..3 from a different start each."""
    T = shape[0]
    stack = stacks[shape]
    for start in range(4):
        views = [(start + t) % 4 for t in range(T)]
        got = run_sequence(small_engine, stack, views)
        m32, a32, _, _ = _utils().tta_reduce_reference(stack, views, np.float32)
        _, _, e64, i64 = _utils().tta_reduce_reference(stack, views, np.float64)
        assert np.array_equal(got["mean_probs"].view(np.uint32), m32.view(np.uint32)), views         # bit for bit
        assert np.array_equal(got["argmax"], a32), views
        e_err, i_err = np.abs(got["entropy"] - e64).max(), np.abs(got["mutual_info"] - i64).max()
        print(f"{shape} views {views}: entropy err {e_err:.3e}, mutual_info err {i_err:.3e}")
        assert e_err <= ENTROPY_TOL and i_err <= ENTROPY_TOL
        assert (got["mutual_info"] >= 0).all()


@pytest.mark.parametrize("shape", TTA_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_tta_update_against_mc_update(small_engine, stacks, shape):
    """With every view 0 the four maps are ``oct_mc_update``'s byte for byte; for each view, folding the flipped samples under
    that view is ``oct_mc_update`` on the samples themselves, byte for byte."""
    T = shape[0]
    stack = stacks[shape]
    want = run_sequence(small_engine, stack)
    same_bytes(run_sequence(small_engine, stack, [0] * T), want)
    for v in range(1, 4):
        flipped = np.stack([_utils().flip_reference(stack[t], v) for t in range(T)])
        same_bytes(run_sequence(small_engine, flipped, [v] * T), want)


def test_tta_update_writes_only_the_maps_that_are_asked_for(small_engine):
    stack = softmax_stack((2, 1, 8, 16, 3), seed=4)
    full = run_sequence(small_engine, stack, [1, 2])
    for k in MAPS:
        got = run_sequence(small_engine, stack, [1, 2], only=(k,))
        assert got[k].tobytes() == full[k].tobytes()
        fresh = dict(mean_probs=0.0, argmax=255, entropy=-1.0, mutual_info=-1.0)
        assert all((got[o] == fresh[o]).all() for o in MAPS if o != k), k


def test_tta_update_argument_errors_launch_nothing(small_engine):
    from oct_image_segmentation_models_amd import _hip
    lib, stream = _hip.lib(), C.c_void_p(torch.cuda.current_stream().cuda_stream)
    B, H, W, Cn = 1, 4, 8, 3
    npx = B * H * W
    need = lib.oct_mc_workspace_bytes(B, H, W, Cn)
    arena = torch.full((8 * need,), 0x5A, dtype=torch.uint8, device="cuda")       # workspace and outputs with a sentinel
    base = arena.data_ptr()
    probs = _up(softmax_stack((1, B, H, W, Cn), seed=2)[0])
    ws, o = base, base + 2 * need
    out = _hip.McOut(o, o + need, o + 2 * need, o + 3 * need)

    def call(probs=probs.data_ptr(), Cn=Cn, view=1, t=0, T=1, ws=ws, ws_bytes=need, out=out):
        return lib.oct_tta_update(probs, B, H, W, Cn, view, t, T, ws, ws_bytes, None if out is None else C.byref(out), stream)

    for kw in (dict(view=4), dict(view=-1), dict(T=5), dict(T=0), dict(probs=None), dict(ws=None), dict(out=None), dict(Cn=1), dict(Cn=33),
               dict(t=1), dict(t=-1), dict(ws_bytes=need - 1), dict(ws=base + 2), dict(out=_hip.McOut(ws, None, None, None)),
               dict(out=_hip.McOut(o, None, o + 4, None)), dict(out=_hip.McOut(probs.data_ptr(), None, None, None))):
        assert call(**kw) < 0 and b"tta_update" in lib.oct_last_error(), kw
    torch.cuda.synchronize()
    assert bool((arena == 0x5A).all())
    assert call() == 0
    torch.cuda.synchronize()
    got = arena.cpu().numpy()
    assert (got[:2 * need] == 0x5A).all()                       # T == 1: first and last, the sums stay in registers
    assert not (got[2 * need:2 * need + npx * Cn * 4] == 0x5A).all() and (got[2 * need + npx * Cn * 4:3 * need] == 0x5A).all()
    assert (got[6 * need:] == 0x5A).all()


# ---- 3. the engine call and its graph -------------------------------------------------------------------------------------------
ENGINE_CASES = [(3, 16, 32, 3, 8, 2), (2, 20, 36, 8, 16, 2)]


def scans(B, H, W, Cn, seed=5):
    return _up(on.synth_scans(B, H, W, Cn, seed=seed)[0])


def per_view(eng, x, views):
    """The definition with the stand-alone pieces: ``forward(flip(x, v))`` per view -> the stack and its ``tta_update`` fold."""
    stack = np.stack([eng.forward(eng.flip(x, v) if v != "identity" else x, training=False)[0].cpu().numpy() for v in views])
    return stack, run_sequence(eng, stack, [NAMES.index(v) for v in views])


@pytest.mark.parametrize("case", ENGINE_CASES, ids=lambda c: "-".join(map(str, c)))
def test_forward_tta_equals_the_per_view_forwards_folded(case):
    B, H, W, Cn, sn, P = case
    eng = make(B, H, W, Cn, sn, P)
    x = scans(B, H, W, Cn)
    plain = eng.forward(x, training=False, want_argmax=True)
    plain = [t.cpu().numpy().copy() for t in plain]
    for views in (NAMES, ("flip_ud", "identity"), ("flip_both", "flip_lr", "flip_ud")):
        stack, want = per_view(eng, x, views)
        got = host(eng.forward_tta(x, views, want_mean_probs=True))
        same_bytes(got, want)
        codes = [NAMES.index(v) for v in views]
        m32, a32, _, _ = _utils().tta_reduce_reference(stack, codes)
        assert np.array_equal(got["mean_probs"].view(np.uint32), m32.view(np.uint32)) and np.array_equal(got["argmax"], a32)
        assert not np.array_equal(stack[0], _utils().flip_reference(stack[1], codes[0] ^ codes[1]))    # the net is not mirror-symmetric
    # one view, the identity: the plain forward, and nothing to disagree about
    one = host(eng.forward_tta(x, ("identity",), want_mean_probs=True))
    assert np.array_equal(one["mean_probs"].view(np.uint32), plain[0].view(np.uint32)) and np.array_equal(one["argmax"], plain[1])
    assert (one["mutual_info"] == 0).all()
    assert set(eng.forward_tta(x, ("flip_lr",))) == {"argmax", "entropy", "mutual_info"}
    # a plain forward afterwards gives what it gave before
    again = eng.forward(x, training=False, want_argmax=True)
    assert np.array_equal(again[0].cpu().numpy(), plain[0]) and np.array_equal(again[1].cpu().numpy(), plain[1])


@pytest.mark.parametrize("case", ENGINE_CASES, ids=lambda c: "-".join(map(str, c)))
def test_captured_tta_graph_replays_the_eager_call(case):
    B, H, W, Cn, sn, P = case
    eng = make(B, H, W, Cn, sn, P)
    views = ("identity", "flip_lr", "flip_both")
    xa, xb = scans(B, H, W, Cn, seed=5), scans(B, H, W, Cn, seed=6)
    want = [host(eng.forward_tta(x, views, want_mean_probs=True)) for x in (xa, xb)]
    assert not np.array_equal(want[0]["mean_probs"], want[1]["mean_probs"])
    x_fix = torch.zeros_like(xa)
    outs = eng.graph_capture_tta(x_fix, views, want_mean_probs=True)
    for x, w in ((xa, want[0]), (xb, want[1]), (xa, want[0])):
        x_fix.copy_(x)
        eng.graph_launch()
        same_bytes(host(outs), w)


def test_forward_tta_on_a_training_handle_in_bf16_storage():
    """A training handle with bf16 activations: the same equalities, and the handle is left as ``forward_mc`` leaves it."""
    B, H, W, Cn = 2, 16, 32, 3
    eng = make(B, H, W, Cn, 8, 2, training=True, dtype="bfloat16")
    x = scans(B, H, W, Cn, seed=9)
    eng.set_dropout_step(5)
    mask0, params0, state0 = eng.dropout_mask(B).clone(), eng.params.clone(), eng.state.clone()
    views = ("flip_lr", "identity", "flip_ud")
    _, want = per_view(eng, x, views)
    same_bytes(host(eng.forward_tta(x, views, want_mean_probs=True)), want)
    assert torch.equal(eng.dropout_mask(B), mask0) and torch.equal(eng.params, params0) and torch.equal(eng.state, state0)
    from oct_image_segmentation_models_amd._hip import OctError
    lab = torch.zeros((B, H, W), dtype=torch.uint8, device=eng.device)
    eng.forward(x, training=True, labels=lab)
    eng.forward_tta(x, views)
    with pytest.raises(OctError, match="forward with io.labels"):       # a pending Dice sum is dropped
        eng.loss_dice()


def test_forward_tta_argument_errors_launch_nothing():
    from oct_image_segmentation_models_amd import _hip
    B, H, W, Cn = 2, 16, 32, 3
    eng = make(B, H, W, Cn, 8, 2)
    x = scans(B, H, W, Cn)
    b = eng._tta_buffers(B, x)
    for k in ("mean_probs", "entropy", "mutual_info"):
        b[k].fill_(-7.0)
    b["x_view"].fill_(0x5A)
    out = _hip.McOut(b["mean_probs"].data_ptr(), b["argmax"].data_ptr(), b["entropy"].data_ptr(), b["mutual_info"].data_ptr())
    lib, need = _hip.lib(), b["ws"].numel()

    def call(x_ptr=x.data_ptr(), Bn=B, views=(0, 1), T=2, xv=b["x_view"].data_ptr(), scratch=b["scratch"].data_ptr(),
             ws=b["ws"].data_ptr(), ws_bytes=need, o=out):
        # the views are an array inside the descriptor (there is no views pointer to be null); "no out" is no map asked for
        d = _hip.Infer(x_dev=x_ptr, x_is_u8=1, B=Bn, kind=_hip.INFER_TTA, T=T, views=(C.c_int * 4)(*views[:4]), x_view_dev=xv,
                       probs_scratch_dev=scratch, ws_dev=ws, ws_bytes=ws_bytes, H=H, W=W, out=o or _hip.McOut())
        return lib.oct_unet_infer(eng._h, C.byref(d), None), lib.oct_last_error().decode()

    for kw, msg in ((dict(x_ptr=None), "null"), (dict(scratch=None), "null"), (dict(ws=None), "null"),
                    (dict(o=None), "null"), (dict(Bn=0), "B out of range"), (dict(Bn=3), "B out of range"), (dict(T=0), "T out of range"),
                    (dict(views=(0, 1, 2, 3, 0), T=5), "T out of range"), (dict(views=(0, 4)), "outside 0..3"),
                    (dict(views=(-1, 0)), "outside 0..3"), (dict(xv=None), "x_view_dev"), (dict(xv=x.data_ptr()), "overlaps"),
                    (dict(ws_bytes=need - 1), "workspace too small"), (dict(scratch=b["mean_probs"].data_ptr()), "overlaps")):
        rc, err = call(**kw)
        assert rc < 0 and msg in err, (kw, rc, err)
    torch.cuda.synchronize()
    assert all((b[k] == -7.0).all() for k in ("mean_probs", "entropy", "mutual_info")) and bool((b["x_view"] == 0x5A).all())
    assert call(views=(0, 0), xv=None)[0] == 0                      # identity views need no second input buffer
    for bad in ((), ("flip_lr", "flip_lr"), ("spin",), NAMES + ("identity",)):
        with pytest.raises(_hip.OctError, match="tta"):
            eng.forward_tta(x, bad)
    assert call()[0] == 0


@pytest.mark.parametrize("mode", ["edge", "reflect"])
def test_padded_tta_graph_equals_the_native_engine_on_the_padded_batch(mode):
    """18x30 scans on a 20x32 engine (top 1, left 1): the views are flips of the PADDED batch, the fold runs at the padded size and
    the crop comes last -- the native engine's ``forward_tta`` on ``pad_reference(x)``, cropped."""
    cu = _utils()
    B, H, W, Cn = 2, 18, 30, 3
    Hp, Wp, top, left = cu.padded_geometry(H, W, 2)
    assert (Hp, Wp, top, left) == (20, 32, 1, 1)
    eng = make(B, Hp, Wp, Cn, 8, 2)
    x = on.synth_scans(B, H, W, Cn, seed=13)[0]
    views = ("identity", "flip_lr", "flip_ud")
    native = host(eng.forward_tta(_up(cu.pad_reference(x, Hp, Wp, top, left, mode)), views, want_mean_probs=True))
    want = {k: cu.crop_reference(v, H, W, top, left) for k, v in native.items()}
    x_fix = torch.zeros((B, H, W, 1), dtype=torch.uint8, device="cuda")
    outs = eng.graph_capture_tta(x_fix, views, want_mean_probs=True, pad=(top, left, mode, 0))
    for _ in range(2):
        x_fix.copy_(_up(x))
        eng.graph_launch()
        same_bytes(host(outs), want)
    assert outs["argmax"].shape == (B, H, W) and outs["mean_probs"].shape == (B, H, W, Cn)


# ---- 4. the pipeline, predict and evaluate_model --------------------------------------------------------------------------------
N_IMG, H_, W_, CC, SN, P_, BATCH = 5, 16, 32, 3, 8, 2, 3
VIEWS = ("identity", "flip_lr", "flip_ud")


@pytest.fixture(scope="module")
def images():
    return on.synth_scans(N_IMG, H_, W_, CC, seed=21)


@pytest.mark.parametrize("soft", [False, True])
def test_both_pipeline_sources_carry_predict_tta(tmp_path, images, soft):
    """``BatchedPredictor`` (uint8 images: the captured TTA graph over the fixed input buffer, two batches of 3 and 2) and
    ``host_batches`` (float images) against ``Model.predict_tta``; with ``soft_maps`` the boundary maps are those of the mean
    probabilities."""
    from oct_image_segmentation_models_amd.evaluation.pipeline import InferenceRun
    from oct_image_segmentation_models_amd.models.engine_model import load_model
    imgs = images[0]
    model = load_model(save_untrained_model(tmp_path, H_, W_, CC, SN, P_))
    with InferenceRun(model, imgs, BATCH, CC, soft_maps=soft, tta=VIEWS) as run:
        dev = list(run)
    with InferenceRun(model, imgs.astype(np.float32), BATCH, CC, soft_maps=soft, tta=VIEWS) as run:
        hst = list(run)
    with InferenceRun(model, imgs, BATCH, CC, soft_maps=soft) as run:
        plain = list(run)
    assert [(b.lo, b.hi) for b in dev] == [(b.lo, b.hi) for b in hst] == [(0, 3), (3, 5)]
    eng = model._ensure_engine(BATCH, False)
    fimg = imgs.astype(np.float32) / np.float32(255.0)                          # what host_batches hands the engine
    mean, am, ent, mi = model.predict_tta(imgs, VIEWS, batch_size=BATCH)
    for got, want in zip(model.predict_tta(fimg, VIEWS, batch_size=2), (mean, am, ent, mi)):
        assert got.dtype == want.dtype and np.array_equal(got, want)            # float input in [0,1]; no batch dependence
    assert mean.shape == (N_IMG, H_, W_, CC) and am.dtype == np.uint8 and ent.dtype == mi.dtype == np.float32
    assert mi.max() > 1e-4 and not np.array_equal(am, np.concatenate([p.labels for p in plain]))
    for b, h, p in zip(dev, hst, plain):
        s = slice(b.lo, b.hi)
        maps = (eng.boundary_maps_soft(_up(mean[s])) if soft else eng.boundary_maps(_up(am[s]))).cpu().numpy()
        for rec in (b, h):
            assert rec.entropy.dtype == np.float32 and rec.entropy.shape == (b.hi - b.lo, H_, W_)
            assert np.array_equal(rec.entropy, ent[s]) and np.array_equal(rec.mutual_info, mi[s])
            assert np.array_equal(rec.labels, am[s]) and np.array_equal(rec.maps, maps)
        assert p.entropy is None and p.mutual_info is None and len(p) == len(b)
    labels, maps, e2, i2 = model.predict_labels(imgs, batch_size=BATCH, want_maps=True, tta=VIEWS)
    assert np.array_equal(labels, am) and np.array_equal(e2, ent) and np.array_equal(i2, mi)
    with pytest.raises(ValueError, match="mc_samples"):
        model.predict_labels(imgs, tta=VIEWS, mc_samples=2)


def test_predict_with_tta(tmp_path, images):
    from oct_image_segmentation_models_amd.common import h5io, png, utils as cu
    from oct_image_segmentation_models_amd.common.dataset import Dataset
    from oct_image_segmentation_models_amd.models.engine_model import load_model
    from oct_image_segmentation_models_amd.prediction import predict
    from oct_image_segmentation_models_amd.prediction.prediction_parameters import PredictionParams, PredictionSaveParams
    imgs = images[0]
    save_untrained_model(tmp_path, H_, W_, CC, SN, P_)

    def run(name, **kw):
        ds = Dataset(imgs, [Path(f"volume_{i}.tiff") for i in range(N_IMG)], [tmp_path / name / f"image_{i}" for i in range(N_IMG)])
        pp = PredictionParams(model_path=tmp_path / "model" / "model.npz", mlflow_tracking_uri=None, mlflow_run_uuid=None,
                              dataset=ds, config_output_dir=tmp_path / name, save_params=PredictionSaveParams(),
                              graph_search=True, batch_size=BATCH, **kw)
        pp.gs_workers = 1
        return predict(pp)

    outs = run("tta", tta=VIEWS, png_plots=True)
    _, am, ent, mi = load_model(tmp_path / "model" / "model.npz").predict_tta(imgs, VIEWS, batch_size=BATCH)
    assert len(outs) == N_IMG
    for i, o in enumerate(outs):
        f = h5io.load(o.image_output_dir / "prediction_info.hdf5")
        e, m = f["predictive_entropy"], f["mutual_information"]
        assert e.dtype == m.dtype == np.float32 and np.array_equal(e, ent[i]) and np.array_equal(m, mi[i])
        assert np.array_equal(o.predictive_entropy, e) and np.array_equal(o.mutual_information, m)
        assert bytes(f["attr:tta_views"]).decode().rstrip("\x00") == "identity,flip_lr,flip_ud" and "attr:mc_samples" not in f
        assert np.array_equal(f["predicted_labels"], am[i]) and np.array_equal(o.predicted_labels, am[i])
        binary = cu.convert_predictions_to_maps_semantic(cu.labels_to_categorical(o.predicted_labels[None], CC))[0]
        assert np.array_equal(o.boundary_maps, binary)               # everything behind the arg-max works on the mean prediction
        pic = png.read_rgba(o.image_output_dir / "uncertainty_map.png")
        want = cu.entropy_to_u8(e, CC)
        assert pic.shape == (H_, W_, 4) and all(np.array_equal(pic[..., c], want) for c in range(3))
    cfg = h5io.load(tmp_path / "tta" / "prediction_params.hdf5")
    assert bytes(cfg["attr:tta_views"]).decode().rstrip("\x00") == "identity,flip_lr,flip_ud"

    # unset: the same files as a run that never names the parameter, and nothing new in them
    plain, off = run("plain"), run("off", tta=())
    tree_equal(tmp_path / "plain", tmp_path / "off", ["prediction_info.hdf5", "graph_search_prediction_info.hdf5"])
    for b in off:
        f = h5io.load(b.image_output_dir / "prediction_info.hdf5")
        assert sorted(k for k in f if not k.startswith("attr:")) == ["boundary_maps", "predicted_labels", "raw_image"]
        assert "attr:tta_views" not in f and b.predictive_entropy is None
        assert not (b.image_output_dir / "uncertainty_map.png").exists()
    assert "attr:tta_views" not in h5io.load(tmp_path / "off" / "prediction_params.hdf5")


def test_evaluate_model_with_tta(tmp_path, images):
    """Every metric comes from the mean prediction: the Dice of the result files is ``dice_from_counts`` of the confusion of
    ``predict_tta``'s arg-max against the ground truth, on the host path and with ``metrics_device``."""
    from oct_image_segmentation_models_amd.common import h5io
    from oct_image_segmentation_models_amd.evaluation import dice_device as dd, eval_model
    from oct_image_segmentation_models_amd.evaluation.evaluation_parameters import EvaluationParameters, EvaluationSaveParams
    from oct_image_segmentation_models_amd.models.engine_model import load_model
    imgs, labels = images
    metrics = ["dice_coef_classes", "dice_coef_macro", "dice_coef_micro"]
    save_untrained_model(tmp_path, H_, W_, CC, SN, P_)
    h5io.save(tmp_path / "data.hdf5", {"test_images": imgs, "test_labels": labels})
    _, am, _, _ = load_model(tmp_path / "model" / "model.npz").predict_tta(imgs, VIEWS, batch_size=BATCH)

    def evaluate(name, **kw):
        ep = EvaluationParameters(model_path=tmp_path / "model" / "model.npz", mlflow_tracking_uri=None, mlflow_run_uuid=None,
                                  test_dataset_path=tmp_path / "data.hdf5", save_foldername=tmp_path / name,
                                  save_params=EvaluationSaveParams(), graph_search=False, metrics=metrics, batch_size=BATCH,
                                  gs_workers=1, **kw)
        return eval_model(ep)

    plain = evaluate("plain")
    differs = False
    for name, kw in (("host", {}), ("device", dict(metrics_device=True))):
        outs = evaluate(name, tta=VIEWS, **kw)
        assert len(outs) == N_IMG
        for i, o in enumerate(outs):
            f = h5io.load(o.image_output_dir / "evaluation_results.hdf5")
            gt = labels[i, :, :, 0]
            assert np.array_equal(f["predicted_segmentation_map"], am[i])
            counts = dd.counts_matrix(dd.confusion_counts_reference(am[i][None], gt[None], CC), CC)[0]
            dc, dm, dmi = dd.dice_from_counts(counts, metrics)
            assert np.array_equal(f["dice_coef_classes"], np.squeeze(dc).astype(np.float64))
            assert np.array_equal(f["dice_coef_macro"], np.expand_dims(dm, 0).astype(np.float64))
            assert np.array_equal(f["dice_coef_micro"], np.expand_dims(dmi, 0).astype(np.float64))
            assert bytes(f["attr:tta_views"]).decode().rstrip("\x00") == "identity,flip_lr,flip_ud"
            p = h5io.load(plain[i].image_output_dir / "evaluation_results.hdf5")
            differs |= not np.array_equal(p["predicted_segmentation_map"], am[i])
            assert "attr:tta_views" not in p
        assert bytes(h5io.load(tmp_path / name / "eval_params.hdf5")["attr:tta_views"]).decode().rstrip("\x00") == "identity,flip_lr,flip_ud"
    assert differs
    assert "attr:tta_views" not in h5io.load(tmp_path / "plain" / "eval_params.hdf5")
