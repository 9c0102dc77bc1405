"""GPU tests of the optimizer family (``oct_opt_step``): every kind and flag combination against the fp64 restatement
``optimizers.reference_step`` on flat buffers of awkward sizes and alignments; gradient clipping on an engine's real
variable table and on a synthetic one with odd offsets; bit-equivalence with ``oct_adam_step`` / ``oct_sgd_step``;
``train_model`` with ``RMSprop(momentum, clipnorm)`` and the slot carry-over across an engine rebuild."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
STEPS = 5
PAD = 4          # floats in front of a test buffer: [PAD, PAD + n) of a fresh torch allocation is 16-byte aligned

from oct_image_segmentation_models_amd import _hip, optimizers as O  # noqa: E402

N, A, C_ = _hip.OPT_NESTEROV, _hip.OPT_AMSGRAD, _hip.OPT_CENTERED
# every kind and flag combination: (name, kind, hyper-parameters).  Learning rates keep each update below 0.05.
CONFIGS = [
    ("sgd", _hip.OPT_SGD, dict(lr=0.01)),
    ("sgd_momentum", _hip.OPT_SGD, dict(lr=0.01, momentum=0.9)),
    ("sgd_nesterov", _hip.OPT_SGD, dict(lr=0.01, momentum=0.9, flags=N)),
    ("adam", _hip.OPT_ADAM, dict(lr=0.01)),
    ("adam_amsgrad", _hip.OPT_ADAM, dict(lr=0.01, flags=A)),
    ("adamax", _hip.OPT_ADAMAX, dict(lr=0.01)),
    ("rmsprop", _hip.OPT_RMSPROP, dict(lr=0.003)),
    ("rmsprop_momentum", _hip.OPT_RMSPROP, dict(lr=0.003, momentum=0.9)),
    ("rmsprop_centered", _hip.OPT_RMSPROP, dict(lr=0.003, flags=C_)),
    ("rmsprop_centered_momentum", _hip.OPT_RMSPROP, dict(lr=0.002, momentum=0.9, flags=C_)),
    ("adagrad", _hip.OPT_ADAGRAD, dict(lr=0.02)),
    ("adadelta", _hip.OPT_ADADELTA, dict(lr=1.0, rho=0.95)),
]
DEFAULTS = dict(lr=0.0, beta_1=0.9, beta_2=0.999, rho=0.9, momentum=0.0, epsilon=1e-7, flags=0)


def f32(x):
    """The value the ABI's float field carries."""
    return float(np.float32(x))


def hyper(kw):
    """Hyper-parameters as the device receives them: rounded to float."""
    h = dict(DEFAULTS, **kw)
    return {k: (v if k == "flags" else f32(v)) for k, v in h.items()}


def inputs(n, seed):
    """|w| <= 0.7; fresh gradients per step with 0.2 <= |g| <= 1 (centered RMSprop then keeps rms - mg^2 >= rho^t * rms > 1e-3)."""
    rng = np.random.default_rng(seed)
    w = rng.uniform(-0.7, 0.7, n).astype(np.float32)
    gs = [(rng.uniform(0.2, 1.0, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32) for _ in range(STEPS)]
    return w, gs


class Flat:
    """A caller of the raw ABI: params, grads and 3 state buffers as views at `shift` floats into padded allocations
    (shift = PAD: 16-byte aligned base; PAD + 1: 4-byte aligned only), guard values on both sides."""
    GUARD = 123.25

    def __init__(self, n, shift):
        self.n, self.shift = n, shift
        self.full = [torch.full((n + 2 * PAD + 4,), self.GUARD, dtype=torch.float32, device="cuda") for _ in range(5)]
        self.p, self.g, *self.s = [t[shift:shift + n] for t in self.full]
        assert self.p.data_ptr() % 16 == 4 * (shift - PAD)

    def load(self, w, slots):
        self.p.copy_(torch.from_numpy(w))
        for t, v in zip(self.s, slots):
            t.copy_(torch.from_numpy(np.asarray(v, np.float32)))

    def step(self, kind, t, g, h, clip_mode=0, clip=0.0, var_off=None, scratch=None, n_slots=3):
        self.g.copy_(torch.from_numpy(g))
        d = _hip.OptDesc(kind, h["flags"], clip_mode, clip, h["lr"], h["beta_1"], h["beta_2"], h["rho"], h["momentum"], h["epsilon"])
        ptrs = (C.c_void_p * 3)(*[s.data_ptr() for s in self.s[:n_slots]])
        _hip.check(_hip.lib().oct_opt_step(
            C.byref(d), self.p.data_ptr(), self.g.data_ptr(), ptrs, self.n, t, var_off.data_ptr() if var_off is not None else None,
            (var_off.numel() - 1) if var_off is not None else 0, scratch.data_ptr() if scratch is not None else None,
            C.c_void_p(torch.cuda.current_stream().cuda_stream)), "oct_opt_step")

    def guards_intact(self):
        return all(bool((t[:self.shift] == self.GUARD).all()) and bool((t[self.shift + self.n:] == self.GUARD).all()) for t in self.full)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    return _hip.lib()


def reference_run(kind, kw, w, gs, centered_margin=True, **clip):
    """fp64 reference of STEPS steps: [(w, slots)] after every step; asserts the premise of the gates: |w| <= 1, updates
    <= 0.05 and, on the flat buffers, rms - mg^2 > 1e-4 for centered RMSprop."""
    h = hyper(kw)
    names = O.slot_names(kind, momentum=h["momentum"], flags=h["flags"])
    s = {k: np.full(w.size, f32(0.1) if kind == _hip.OPT_ADAGRAD else 0.0) for k in names}
    w = w.astype(np.float64)
    out = []
    for t, g in enumerate(gs, 1):
        w1, s = O.reference_step(kind, w, g.astype(np.float64), s, t, **h, **clip)
        assert np.abs(w1 - w).max() <= 0.05 and np.abs(w1).max() <= 1.0
        if centered_margin and h["flags"] & C_ and kind == _hip.OPT_RMSPROP:
            assert (s["rms"] - s["mg"] ** 2).min() > 1e-4
        w = w1
        out.append((w, s))
    return names, out


# ---- raw ABI on flat buffers ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", [PAD, PAD + 1], ids=["aligned16", "aligned4"])
@pytest.mark.parametrize("n", [1, 3, 5, 1027, 65537])
def test_every_kind_matches_the_fp64_restatement(lib, n, shift):
    """Gates: parameters within 2e-6 absolute (the gate of test_adam_and_sgd_steps_match_keras_formulas), every slot within
    2e-6 * max(1, max|ref|): at most 4 fp32 roundings per element and step x 5 steps x 2^-24 ~ 1.2e-6."""
    buf = Flat(n, shift)
    w0, gs = inputs(n, seed=n + shift)
    for name, kind, kw in CONFIGS:
        names, ref = reference_run(kind, kw, w0, gs)
        assert lib.oct_opt_slot_count(C.byref(_hip.OptDesc(kind=kind, flags=kw.get("flags", 0), momentum=kw.get("momentum", 0.0)))) == len(names)
        buf.load(w0, [np.full(n, 0.1 if kind == _hip.OPT_ADAGRAD else 0.0)] * 3)
        h = hyper(kw)
        for t, g in enumerate(gs, 1):
            buf.step(kind, t, g, h)
            assert np.array_equal(buf.g.cpu().numpy(), g), name
            wr, sr = ref[t - 1]
            err = np.abs(buf.p.cpu().numpy().astype(np.float64) - wr).max()
            assert err < 2e-6, (name, t, err)
            for k, sn in enumerate(names):
                serr = np.abs(buf.s[k].cpu().numpy().astype(np.float64) - sr[sn]).max()
                assert serr < 2e-6 * max(1.0, np.abs(sr[sn]).max()), (name, t, sn, serr)
        for k in range(len(names), 3):      # buffers past the slot count are not touched
            assert bool((buf.s[k] == (0.1 if kind == _hip.OPT_ADAGRAD else 0.0)).all()), name
        assert buf.guards_intact(), name


@pytest.mark.parametrize("shift", [PAD, PAD + 1], ids=["aligned16", "aligned4"])
def test_buffers_of_different_alignment_take_the_scalar_path(lib, shift):
    """Params at one alignment, the state buffers at another: no common float4 boundary, same results."""
    n = 1027
    buf = Flat(n, shift)
    other = Flat(n, PAD + 2)
    buf.s = other.s
    w0, gs = inputs(n, seed=77)
    for name, kind, kw in (CONFIGS[4], CONFIGS[9]):
        names, ref = reference_run(kind, kw, w0, gs)
        buf.load(w0, [np.zeros(n)] * 3)
        for t, g in enumerate(gs, 1):
            buf.step(kind, t, g, hyper(kw))
        assert np.abs(buf.p.cpu().numpy() - ref[-1][0]).max() < 2e-6, name
        for k, sn in enumerate(names):
            assert np.abs(buf.s[k].cpu().numpy() - ref[-1][1][sn]).max() < 2e-6 * max(1.0, np.abs(ref[-1][1][sn]).max()), (name, sn)
        assert buf.guards_intact() and other.guards_intact()


@pytest.mark.parametrize("shift", [PAD, PAD + 1], ids=["aligned16", "aligned4"])
def test_clipping_on_a_table_of_odd_pieces(lib, shift):
    """Variables of lengths down to 2 at offsets that are no multiples of 4; some above the threshold, some below, one
    all zero.  clipnorm, global_clipnorm and clipvalue against the restatement; the gradient buffer stays untouched and a
    second run gives the same bits."""
    lens = [2, 3, 5, 7, 2, 1027, 4, 301, 2, 4099, 3]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    n = int(off[-1])
    w0, gs = inputs(n, seed=9)
    for g in gs:
        g[off[4]:off[5]] = 0.0                              # an all-zero variable: scale 1, no NaN
        g[off[6]:off[7]] *= 0.05                            # norm 0.1 .. 0.2: below the threshold
        g[off[0]:off[1]] *= 0.1
    var_off = torch.from_numpy(off).cuda()
    scratch = torch.empty(lib.oct_opt_scratch_bytes(len(lens), n), dtype=torch.uint8, device="cuda")
    buf = Flat(n, shift)
    name, kind, kw = CONFIGS[7]                              # RMSprop with momentum
    for mode, thr in ((_hip.CLIP_NORM, 0.5), (_hip.CLIP_GLOBAL_NORM, 2.0), (_hip.CLIP_VALUE, 0.4)):
        names, ref = reference_run(kind, kw, w0, gs, clip_mode=mode, clip=f32(thr), var_off=off)
        runs = []
        for _ in range(2):
            buf.load(w0, [np.zeros(n)] * 3)
            for t, g in enumerate(gs, 1):
                buf.step(kind, t, g, hyper(kw), mode, thr, var_off, scratch)
                assert np.array_equal(buf.g.cpu().numpy(), g)
            runs.append([buf.p.cpu().numpy()] + [s.cpu().numpy() for s in buf.s[:len(names)]])
        assert all(np.array_equal(a, b) for a, b in zip(*runs)), mode
        assert np.abs(runs[0][0] - ref[-1][0]).max() < 2e-6, mode
        for k, sn in enumerate(names):
            assert np.abs(runs[0][1 + k] - ref[-1][1][sn]).max() < 2e-6 * max(1.0, np.abs(ref[-1][1][sn]).max()), (mode, sn)
        assert np.isfinite(runs[0][0]).all() and buf.guards_intact()


@pytest.mark.parametrize("shift", [PAD, PAD + 1], ids=["aligned16", "aligned4"])
@pytest.mark.parametrize("n", [5, 1027, 65537])
def test_generic_adam_and_sgd_equal_the_dedicated_entry_points_bit_for_bit(lib, n, shift):
    a, b = Flat(n, shift), Flat(n, shift)
    w0, gs = inputs(n, seed=3 * n)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for kind, kw in ((_hip.OPT_ADAM, dict(lr=0.01)), (_hip.OPT_SGD, dict(lr=0.01, momentum=0.9))):
        h = hyper(kw)
        for x in (a, b):
            x.load(w0, [np.zeros(n)] * 3)
        for t, g in enumerate(gs[:3], 1):
            a.step(kind, t, g, h)
            b.g.copy_(torch.from_numpy(g))
            if kind == _hip.OPT_ADAM:
                _hip.check(lib.oct_adam_step(b.p.data_ptr(), b.g.data_ptr(), b.s[0].data_ptr(), b.s[1].data_ptr(), n, h["lr"],
                                             h["beta_1"], h["beta_2"], h["epsilon"], t, st), "oct_adam_step")
            else:
                _hip.check(lib.oct_sgd_step(b.p.data_ptr(), b.g.data_ptr(), b.s[0].data_ptr(), n, h["lr"], h["momentum"], st),
                           "oct_sgd_step")
            assert torch.equal(a.p, b.p) and torch.equal(a.s[0], b.s[0]) and torch.equal(a.s[1], b.s[1]), (kind, t)
    # plain SGD as well
    for x in (a, b):
        x.load(w0, [np.zeros(n)] * 3)
    a.step(_hip.OPT_SGD, 1, gs[0], hyper(dict(lr=0.01)))
    b.g.copy_(torch.from_numpy(gs[0]))
    _hip.check(lib.oct_sgd_step(b.p.data_ptr(), b.g.data_ptr(), None, n, f32(0.01), 0.0, st), "oct_sgd_step")
    assert torch.equal(a.p, b.p)


def test_amsgrad_equals_adam_while_v_grows(lib):
    """Gradients whose magnitude grows every step: v is non-decreasing, vhat = v, and amsgrad is Adam bit for bit."""
    n = 1027
    a, b = Flat(n, PAD), Flat(n, PAD + 1)
    w0, gs = inputs(n, seed=12)
    gs = [(gs[0] * (1.0 + 0.2 * t)).astype(np.float32) for t in range(STEPS)]
    for x in (a, b):
        x.load(w0, [np.zeros(n)] * 3)
    for t, g in enumerate(gs, 1):
        a.step(_hip.OPT_ADAM, t, g, hyper(dict(lr=0.01)))
        b.step(_hip.OPT_ADAM, t, g, hyper(dict(lr=0.01, flags=A)))
        assert torch.equal(a.p, b.p) and torch.equal(a.s[1], b.s[1]) and torch.equal(b.s[2], b.s[1]), t


def test_bad_descriptors_are_refused(lib):
    buf = Flat(8, PAD)
    g = np.zeros(8, np.float32)
    with pytest.raises(_hip.OctError, match="kind"):
        buf.step(17, 1, g, hyper({}))
    with pytest.raises(_hip.OctError, match="step"):
        buf.step(_hip.OPT_SGD, 0, g, hyper(dict(lr=0.1)))
    with pytest.raises(_hip.OctError, match="scratch"):
        buf.step(_hip.OPT_SGD, 1, g, hyper(dict(lr=0.1)), _hip.CLIP_GLOBAL_NORM, 1.0)
    with pytest.raises(_hip.OctError, match="threshold"):
        buf.step(_hip.OPT_SGD, 1, g, hyper(dict(lr=0.1)), _hip.CLIP_VALUE, -1.0)
    sc = torch.empty(lib.oct_opt_scratch_bytes(1, 8), dtype=torch.uint8, device="cuda")
    with pytest.raises(_hip.OctError, match="variable table"):
        buf.step(_hip.OPT_SGD, 1, g, hyper(dict(lr=0.1)), _hip.CLIP_NORM, 1.0, None, sc)


# ---- on an engine: the real variable table ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def eng(lib):
    from oct_image_segmentation_models_amd.engine import UNetEngine
    return UNetEngine(device="cuda:0", input_channels=1, num_classes=3, image_height=16, image_width=32, start_neurons=4,
                      pool_layers=1, conv_layers=1, max_batch=2, training=True, seed=1)


def engine_run(eng, w0, gs, kind, kw, mode=_hip.CLIP_NONE, thr=0.0):
    """STEPS steps of UNetEngine.optimizer_step from fresh state on given gradients: (params, {slot: values})."""
    eng.params.copy_(torch.from_numpy(w0)); eng._opt.clear(); eng.opt_step = 0
    h = dict(kw); lr = h.pop("lr")
    for g in gs:
        eng.grads.copy_(torch.from_numpy(g))
        before = eng.grads.clone()
        eng.optimizer_step(kind, lr=lr, clip_mode=mode, clip=thr, **h)
        assert torch.equal(eng.grads, before)               # clipping happens on the fly: the buffer keeps its bits
    names = [k for k in eng._opt if not k.startswith("clip.")]
    return eng.params.cpu().numpy(), {k: eng._opt[k].cpu().numpy() for k in names}


def engine_inputs(eng, seed=4):
    off = eng.var_offsets().astype(np.int64)
    assert off[0] == 0 and off[-1] == eng.n_params and (np.diff(off) > 0).all()
    assert eng.n_params % 4 and np.diff(off).min() <= 4         # the head's 3 biases end the buffer
    assert len(off) - 1 == sum(4 if L["has_bn"] else 2 for L in eng.layers)
    w0, gs = inputs(eng.n_params, seed)
    for g in gs:        # every variable's norm to 0.3 (below the thresholds used here) ...
        for lo, hi in zip(off[:-1], off[1:]):
            g[lo:hi] *= 0.3 / np.sqrt(np.sum(g[lo:hi].astype(np.float64) ** 2))
    return off, w0, gs


ENGINE_KINDS = [(_hip.OPT_SGD, dict(lr=0.01, momentum=0.9, flags=N), ["mom"]),
                (_hip.OPT_RMSPROP, dict(lr=0.002, momentum=0.9, flags=C_), ["rmsprop.rms", "rmsprop.mom", "rmsprop.mg"])]
REF_NAMES = {"mom": "v", "rmsprop.rms": "rms", "rmsprop.mom": "mom", "rmsprop.mg": "mg"}


def check_against_reference(eng, got, kind, kw, w0, gs, **clip):
    names, ref = reference_run(kind, kw, w0, gs, centered_margin=False, **clip)
    p, slots = got
    assert np.abs(p - ref[-1][0]).max() < 2e-6
    assert sorted(REF_NAMES[k] for k in slots) == sorted(names)
    for k, v in slots.items():
        r = ref[-1][1][REF_NAMES[k]]
        assert np.abs(v - r).max() < 2e-6 * max(1.0, np.abs(r).max()), k


@pytest.mark.parametrize("case", [0, 1], ids=["sgd_nesterov", "rmsprop_centered_momentum"])
def test_engine_clipnorm_scales_only_the_variable_above_the_threshold(eng, case):
    kind, kw, _ = ENGINE_KINDS[case]
    off, w0, gs = engine_inputs(eng)
    big = 5                                               # one variable of the second conv: norm 0.3 -> 3.0
    for g in gs:
        g[off[big]:off[big + 1]] *= 10.0
    plain = engine_run(eng, w0, gs, kind, kw)
    clipped = engine_run(eng, w0, gs, kind, kw, _hip.CLIP_NORM, 1.0)
    again = engine_run(eng, w0, gs, kind, kw, _hip.CLIP_NORM, 1.0)
    check_against_reference(eng, clipped, kind, kw, w0, gs, clip_mode=_hip.CLIP_NORM, clip=1.0, var_off=off)
    keep = np.ones(eng.n_params, bool); keep[off[big]:off[big + 1]] = False
    assert np.array_equal(clipped[0][keep], plain[0][keep])             # the others move exactly as without clipping
    assert not np.array_equal(clipped[0][~keep], plain[0][~keep])
    for k in plain[1]:
        assert np.array_equal(clipped[1][k][keep], plain[1][k][keep]), k
    assert np.array_equal(clipped[0], again[0]) and all(np.array_equal(clipped[1][k], again[1][k]) for k in again[1])


@pytest.mark.parametrize("case", [0, 1], ids=["sgd_nesterov", "rmsprop_centered_momentum"])
def test_engine_global_clipnorm_above_and_below_the_threshold(eng, case):
    kind, kw, _ = ENGINE_KINDS[case]
    off, w0, gs = engine_inputs(eng)
    gnorm = 0.3 * np.sqrt(len(off) - 1)                   # every variable has norm 0.3
    plain = engine_run(eng, w0, gs, kind, kw)
    below = engine_run(eng, w0, gs, kind, kw, _hip.CLIP_GLOBAL_NORM, 2.0 * gnorm)
    assert np.array_equal(below[0], plain[0]) and all(np.array_equal(below[1][k], plain[1][k]) for k in plain[1])
    above = engine_run(eng, w0, gs, kind, kw, _hip.CLIP_GLOBAL_NORM, 0.5 * gnorm)
    again = engine_run(eng, w0, gs, kind, kw, _hip.CLIP_GLOBAL_NORM, 0.5 * gnorm)
    check_against_reference(eng, above, kind, kw, w0, gs, clip_mode=_hip.CLIP_GLOBAL_NORM, clip=f32(0.5 * gnorm))
    assert not np.array_equal(above[0], plain[0])
    assert np.array_equal(above[0], again[0]) and all(np.array_equal(above[1][k], again[1][k]) for k in again[1])


def test_engine_clipvalue(eng):
    kind, kw, _ = ENGINE_KINDS[1]
    off, w0, gs = engine_inputs(eng)
    thr = float(np.median(np.abs(gs[0])))                  # about half of the elements are clipped
    got = engine_run(eng, w0, gs, kind, kw, _hip.CLIP_VALUE, thr)
    check_against_reference(eng, got, kind, kw, w0, gs, clip_mode=_hip.CLIP_VALUE, clip=f32(thr))
    assert not np.array_equal(got[0], engine_run(eng, w0, gs, kind, kw)[0])


@pytest.mark.parametrize("mode", [_hip.CLIP_NORM, _hip.CLIP_GLOBAL_NORM], ids=["clipnorm", "global_clipnorm"])
def test_engine_zero_gradients_leave_finite_unchanged_parameters(eng, mode):
    off, w0, _ = engine_inputs(eng)
    zeros = [np.zeros(eng.n_params, np.float32)] * 2
    for kind, kw, _ in ENGINE_KINDS:
        p, slots = engine_run(eng, w0, zeros, kind, kw, mode, 1.0)
        assert np.isfinite(p).all() and np.array_equal(p, w0)
        assert all(np.isfinite(v).all() for v in slots.values())


def test_optimizer_objects_drive_the_engine(eng):
    """optimizers.X.apply(engine): the decayed learning rate of each step, Adagrad's initial accumulator, and the lazily
    created state buffers."""
    off, w0, gs = engine_inputs(eng)
    opt = O.Adagrad(learning_rate=0.02, initial_accumulator_value=0.25, decay=0.5, clipnorm=1.0)
    eng.params.copy_(torch.from_numpy(w0)); eng._opt.clear(); eng.opt_step = 0
    w, s = w0.astype(np.float64), {"a": np.full(eng.n_params, 0.25)}
    for t, g in enumerate(gs, 1):
        eng.grads.copy_(torch.from_numpy(g))
        opt.apply(eng)
        w, s = O.reference_step(_hip.OPT_ADAGRAD, w, g, s, t, lr=f32(0.02 / (1 + 0.5 * (t - 1))), epsilon=f32(1e-7),
                                clip_mode=_hip.CLIP_NORM, clip=1.0, var_off=off)
    assert eng.opt_step == STEPS and set(eng._opt) == {"adagrad.a", "clip.var_off", "clip.scratch"}
    assert np.abs(eng.params.cpu().numpy() - w).max() < 2e-6
    assert np.abs(eng._opt["adagrad.a"].cpu().numpy() - s["a"]).max() < 2e-6 * max(1.0, s["a"].max())


# ---- workflow ---------------------------------------------------------------------------------------------------------------
def test_train_model_with_rmsprop_momentum_and_clipnorm(tmp_path):
    from oct_image_segmentation_models_amd.common import h5io
    from oct_image_segmentation_models_amd.training.training import train_model
    from oct_image_segmentation_models_amd.training.training_parameters import TrainingParams
    tp = TrainingParams(model_architecture="unet", training_dataset_path=ROOT / "tests" / "golden" / "dataset_small.hdf5",
                        initial_model=None, results_location=tmp_path / "results", opt_con=O.RMSprop,
                        opt_params={"learning_rate": 1e-3, "momentum": 0.9, "clipnorm": 1.0}, loss="dice_loss_macro",
                        metric="dice_coef_macro", epochs=2, batch_size=2, model_hyperparameters={"pool_layers": 2}, seed=3)
    res = train_model(tp, None)
    h = res.history
    assert all(len(v) == 2 and np.isfinite(v).all() for v in h.values()) and "loss" in h and "val_loss" in h
    attrs = h5io.load(Path(res.save_foldername) / "training_params.hdf5")
    assert bytes(attrs["attr:optimizer"]).rstrip(b"\x00") == b"RMSprop"
    assert float(attrs["attr:opt_param: rho"]) == 0.9 and float(attrs["attr:opt_param: momentum"]) == 0.9
    assert float(attrs["attr:opt_param: clipnorm"]) == 1.0 and float(attrs["attr:opt_param: learning_rate"]) == 1e-3


def test_fit_keeps_the_slots_across_an_engine_rebuild():
    """A second fit with a larger batch rebuilds the engine; the Adagrad accumulator goes on from where it was:
    after the one step of the second fit it is exactly the old accumulator + g^2 of that step."""
    from oracle import unet_numpy as on
    from oct_image_segmentation_models_amd.common import custom_losses, custom_metrics
    from oct_image_segmentation_models_amd.common.data_generator import DataGenerator
    from oct_image_segmentation_models_amd.models import get_model_class
    cfg = dict(input_channels=1, num_classes=3, image_height=32, image_width=64, start_neurons=8, pool_layers=2)
    model = get_model_class("unet")(**cfg).build_model()
    model.config["seed"] = 3
    loss = custom_losses.custom_loss_objects["dice_loss_macro"]["function"](num_classes=3, is_y_true_sparse=True)
    metric = custom_metrics.training_monitor_metric_objects["dice_coef_macro"](True, 3)
    model.compile(optimizer=O.Adagrad(learning_rate=0.01), loss=loss, metrics=[metric])
    images, labels = on.synth_scans(6, 32, 64, 3, seed=5)
    model.fit(x=DataGenerator(images[:4], labels[:4], 2, [], "none", (), True, None, seed=8), epochs=1, verbose=0)
    e1 = model.engine
    assert e1.opt_step == 2 and e1.cfg.max_batch == 2
    acc1 = e1._opt["adagrad.a"].clone()
    assert float(acc1.min()) >= np.float32(0.1) and float(acc1.max()) > 0.1
    model.fit(x=DataGenerator(images[:3], labels[:3], 3, [], "none", (), True, None, seed=8), epochs=1, verbose=0)
    e2 = model.engine
    assert e2 is not e1 and e2.cfg.max_batch == 3 and e2.opt_step == 3
    g = e2.grads
    assert torch.equal(e2._opt["adagrad.a"], acc1 + g * g)
