"""CPU tests of the optimizer family: the fp64 restatement of every update (``optimizers.reference_step``, what the GPU
tests hold the kernels to) against hand-computed first steps and against ``torch.optim`` in fp64 where the two forms
coincide, and the Keras constructor contract (defaults, ``lr=``, ``get_config`` keys, clipping options, schedules)."""
import math

import numpy as np
import pytest
import torch

from oct_image_segmentation_models_amd import _hip, optimizers as O


def zeros(kind, n, **kw):
    return {k: np.full(n, 0.1 if kind == _hip.OPT_ADAGRAD else 0.0) for k in O.slot_names(kind, **kw)}


# ---- hand-computed first steps ------------------------------------------------------------------------------------------
def test_adagrad_first_step_from_accumulator_0p1():
    w, s = O.reference_step(_hip.OPT_ADAGRAD, [1.0], [0.5], {"a": [0.1]}, 1, lr=0.1, epsilon=1e-7)
    assert s["a"][0] == pytest.approx(0.35, abs=1e-15)
    assert w[0] == pytest.approx(1.0 - 0.1 * 0.5 / (math.sqrt(0.35) + 1e-7), abs=1e-15)


def test_adadelta_first_step_from_zeros():
    w, s = O.reference_step(_hip.OPT_ADADELTA, [1.0], [0.5], {"a": [0.0], "b": [0.0]}, 1, lr=1.0, rho=0.95, epsilon=1e-7)
    a = 0.05 * 0.25
    u = 0.5 * math.sqrt(1e-7) / math.sqrt(a + 1e-7)
    assert s["a"][0] == pytest.approx(a, rel=1e-14) and s["b"][0] == pytest.approx(0.05 * u * u, rel=1e-13)
    assert w[0] == pytest.approx(1.0 - u, abs=1e-15)
    assert 1e-3 < u < 2e-3          # the first Adadelta step is ~ sqrt(eps / (1 - rho)): tiny, whatever the gradient


def test_rmsprop_first_steps_place_epsilon_outside_and_inside_the_root():
    eps, lr = 1e-2, 0.1             # an epsilon large enough to tell the two placements apart
    rms = 0.1 * 0.25
    w0, s0 = O.reference_step(_hip.OPT_RMSPROP, [1.0], [0.5], {"rms": [0.0]}, 1, lr=lr, rho=0.9, epsilon=eps)
    assert s0["rms"][0] == pytest.approx(rms, rel=1e-14)
    assert w0[0] == pytest.approx(1.0 - lr * 0.5 / (math.sqrt(rms) + eps), abs=1e-15)
    w1, s1 = O.reference_step(_hip.OPT_RMSPROP, [1.0], [0.5], {"rms": [0.0], "mom": [0.0]}, 1, lr=lr, rho=0.9, momentum=0.9,
                              epsilon=eps)
    mom = lr * 0.5 / math.sqrt(rms + eps)
    assert s1["mom"][0] == pytest.approx(mom, rel=1e-14) and w1[0] == pytest.approx(1.0 - mom, abs=1e-15)
    assert abs((1.0 - w0[0]) - (1.0 - w1[0])) > 1e-2       # 0.2974 (eps outside) against 0.2673 (eps inside)
    # second step with momentum: the velocity carries over
    w2, s2 = O.reference_step(_hip.OPT_RMSPROP, w1, [0.5], s1, 2, lr=lr, rho=0.9, momentum=0.9, epsilon=eps)
    rms2 = 0.9 * rms + 0.1 * 0.25
    assert s2["mom"][0] == pytest.approx(0.9 * mom + lr * 0.5 / math.sqrt(rms2 + eps), rel=1e-14)


def test_centered_rmsprop_subtracts_the_squared_mean_gradient():
    w, s = O.reference_step(_hip.OPT_RMSPROP, [1.0], [0.5], {"rms": [0.0], "mg": [0.0]}, 1, lr=0.1, rho=0.9, epsilon=1e-7,
                            flags=_hip.OPT_CENTERED)
    assert s["mg"][0] == pytest.approx(0.05, rel=1e-14)
    assert w[0] == pytest.approx(1.0 - 0.1 * 0.5 / (math.sqrt(0.025 - 0.0025) + 1e-7), abs=1e-15)


def test_sgd_nesterov_amsgrad_adamax_first_steps():
    w, s = O.reference_step(_hip.OPT_SGD, [1.0], [0.5], {"v": [0.2]}, 1, lr=0.1, momentum=0.9, flags=_hip.OPT_NESTEROV)
    v = 0.9 * 0.2 - 0.05
    assert s["v"][0] == pytest.approx(v) and w[0] == pytest.approx(1.0 + 0.9 * v - 0.05, abs=1e-15)
    # amsgrad: vhat keeps the larger second moment
    w, s = O.reference_step(_hip.OPT_ADAM, [1.0], [0.1], {"m": [0.0], "v": [0.0], "vhat": [0.5]}, 1, lr=0.01,
                            flags=_hip.OPT_AMSGRAD)
    assert s["vhat"][0] == 0.5 and s["v"][0] == pytest.approx(1e-5, rel=1e-9)
    lr_t = 0.01 * math.sqrt(1 - 0.999) / (1 - 0.9)
    assert w[0] == pytest.approx(1.0 - lr_t * 0.01 / (math.sqrt(0.5) + 1e-7), abs=1e-15)
    w, s = O.reference_step(_hip.OPT_ADAMAX, [1.0], [-0.5], {"m": [0.0], "u": [0.0]}, 1, lr=0.01)
    assert s["u"][0] == 0.5 and s["m"][0] == pytest.approx(-0.05)
    assert w[0] == pytest.approx(1.0 + 0.01 / 0.1 * 0.05 / (0.5 + 1e-7), abs=1e-15)


def test_clipping_restatement():
    g = np.array([3.0, 4.0, 0.3, 0.4, 0.0, 0.0])
    off = [0, 2, 4, 6]
    c = O.clip_gradient(g, _hip.CLIP_NORM, 1.0, off)
    assert np.allclose(c[:2], [0.6, 0.8]) and np.array_equal(c[2:], g[2:])      # |.|=5 scaled, |.|=0.5 and 0 untouched
    assert np.allclose(O.clip_gradient(g, _hip.CLIP_GLOBAL_NORM, 1.0), g / np.sqrt(25.25))
    assert np.array_equal(O.clip_gradient(g, _hip.CLIP_GLOBAL_NORM, 10.0), g)
    assert np.array_equal(O.clip_gradient(np.zeros(4), _hip.CLIP_GLOBAL_NORM, 1.0), np.zeros(4))
    assert np.array_equal(O.clip_gradient([-2.0, 0.5, 2.0], _hip.CLIP_VALUE, 1.0), [-1.0, 0.5, 1.0])


# ---- 5 steps against torch.optim in fp64, where the forms coincide ---------------------------------------------------------
def run_torch(make, w0, grads):
    p = torch.nn.Parameter(torch.tensor(w0, dtype=torch.float64))
    opt = make([p])
    out = []
    for g in grads:
        p.grad = torch.tensor(g, dtype=torch.float64)
        opt.step()
        out.append(p.detach().numpy().copy())
    return out


TORCH_CASES = {
    "adagrad": (_hip.OPT_ADAGRAD, dict(lr=0.05, epsilon=1e-7),
                lambda ps: torch.optim.Adagrad(ps, lr=0.05, initial_accumulator_value=0.1, eps=1e-7)),
    "adadelta": (_hip.OPT_ADADELTA, dict(lr=0.7, rho=0.95, epsilon=1e-6),
                 lambda ps: torch.optim.Adadelta(ps, lr=0.7, rho=0.95, eps=1e-6)),
    "sgd_nesterov": (_hip.OPT_SGD, dict(lr=0.03, momentum=0.9, flags=_hip.OPT_NESTEROV),
                     lambda ps: torch.optim.SGD(ps, lr=0.03, momentum=0.9, nesterov=True)),
    "rmsprop": (_hip.OPT_RMSPROP, dict(lr=0.01, rho=0.9, epsilon=1e-7),
                lambda ps: torch.optim.RMSprop(ps, lr=0.01, alpha=0.9, eps=1e-7)),
    "rmsprop_centered": (_hip.OPT_RMSPROP, dict(lr=0.01, rho=0.9, epsilon=1e-7, flags=_hip.OPT_CENTERED),
                         lambda ps: torch.optim.RMSprop(ps, lr=0.01, alpha=0.9, eps=1e-7, centered=True)),
}


@pytest.mark.parametrize("case", sorted(TORCH_CASES))
def test_five_steps_match_torch_optim_fp64(case):
    kind, kw, make = TORCH_CASES[case]
    rng = np.random.default_rng(5)
    w = rng.uniform(-1, 1, 37)
    grads = [rng.normal(0, 1, 37) for _ in range(5)]
    ref = run_torch(make, w, grads)
    s = zeros(kind, 37, momentum=kw.get("momentum", 0.0), flags=kw.get("flags", 0))
    for t, g in enumerate(grads, 1):
        w, s = O.reference_step(kind, w, g, s, t, **kw)
        assert np.abs(w - ref[t - 1]).max() < 1e-13, (case, t)
    if case == "sgd_nesterov":      # v = -lr * buf: five steps of the torch recurrence buf <- mu*buf + g
        buf = np.zeros(37)
        for g in grads:
            buf = 0.9 * buf + g
        assert np.abs(s["v"] + 0.03 * buf).max() < 1e-14


# ---- constructor contract ------------------------------------------------------------------------------------------------
def test_keras_defaults():
    assert (O.SGD().learning_rate, O.SGD().momentum, O.SGD().nesterov) == (0.01, 0.0, False)
    a = O.Adam()
    assert (a.learning_rate, a.beta_1, a.beta_2, a.epsilon, a.amsgrad) == (1e-3, 0.9, 0.999, 1e-7, False)
    a = O.Adamax()
    assert (a.learning_rate, a.beta_1, a.beta_2, a.epsilon) == (1e-3, 0.9, 0.999, 1e-7)
    r = O.RMSprop()
    assert (r.learning_rate, r.rho, r.momentum, r.epsilon, r.centered) == (1e-3, 0.9, 0.0, 1e-7, False)
    g = O.Adagrad()
    assert (g.learning_rate, g.initial_accumulator_value, g.epsilon) == (1e-3, 0.1, 1e-7)
    d = O.Adadelta()
    assert (d.learning_rate, d.rho, d.epsilon) == (1e-3, 0.95, 1e-7)
    for o in (O.SGD(), a, r, g, d):
        assert o.decay == 0.0 and o.clipnorm is None and o.clipvalue is None and o.global_clipnorm is None


@pytest.mark.parametrize("cls", [O.SGD, O.Adam, O.Adamax, O.RMSprop, O.Adagrad, O.Adadelta])
def test_lr_alias_and_unknown_keyword(cls):
    assert cls(lr=0.25).learning_rate == 0.25
    assert cls(learning_rate=0.5, lr=0.25).learning_rate == 0.25        # Keras: `lr` wins
    with pytest.raises(TypeError, match="bogus"):
        cls(bogus=1)


def test_get_config_keys():
    shared = {"name", "learning_rate", "decay"}
    assert set(O.SGD().get_config()) == shared | {"momentum", "nesterov"}
    assert set(O.Adam().get_config()) == shared | {"beta_1", "beta_2", "epsilon", "amsgrad"}
    assert set(O.Adamax().get_config()) == shared | {"beta_1", "beta_2", "epsilon"}
    assert set(O.RMSprop().get_config()) == shared | {"rho", "momentum", "epsilon", "centered"}
    assert set(O.Adagrad().get_config()) == shared | {"initial_accumulator_value", "epsilon"}
    assert set(O.Adadelta().get_config()) == shared | {"rho", "epsilon"}
    cfg = O.RMSprop(learning_rate=1e-3, momentum=0.9, clipnorm=1.0).get_config()
    assert (cfg["name"], cfg["rho"], cfg["momentum"], cfg["clipnorm"]) == ("RMSprop", 0.9, 0.9, 1.0)
    assert "clipvalue" not in cfg and "global_clipnorm" not in cfg       # Keras lists only the option that is set
    assert O.SGD(nesterov=True, clipvalue=0.5).get_config()["clipvalue"] == 0.5
    assert O.Adam(amsgrad=True, global_clipnorm=2.0).get_config()["global_clipnorm"] == 2.0
    assert O.Adam(amsgrad=True).get_config()["amsgrad"] is True


@pytest.mark.parametrize("pair", [dict(clipnorm=1.0, clipvalue=0.5), dict(clipnorm=1.0, global_clipnorm=2.0),
                                  dict(clipvalue=0.5, global_clipnorm=2.0)])
def test_two_clip_options_raise(pair):
    with pytest.raises(ValueError, match="at most one"):
        O.Adam(**pair)
    with pytest.raises(ValueError, match="at most one"):
        O.RMSprop(**pair)


def test_clip_thresholds_are_checked_and_mapped():
    with pytest.raises(ValueError):
        O.SGD(clipnorm=0.0)
    with pytest.raises(ValueError):
        O.SGD(global_clipnorm=-1.0)
    assert O.SGD().clip() == (_hip.CLIP_NONE, 0.0)
    assert O.SGD(clipvalue=0.5).clip() == (_hip.CLIP_VALUE, 0.5)
    assert O.SGD(clipnorm=1.5).clip() == (_hip.CLIP_NORM, 1.5)
    assert O.SGD(global_clipnorm=2.5).clip() == (_hip.CLIP_GLOBAL_NORM, 2.5)


@pytest.mark.parametrize("name", ["Nadam", "Ftrl"])
def test_unimplemented_optimizers_are_refused_by_name(name):
    cls = getattr(O, name)
    assert cls.__name__ == name
    with pytest.raises(NotImplementedError, match=name):
        cls(learning_rate=1e-3)


def test_decay_and_schedule_give_the_learning_rate_sequence():
    o = O.Adam(learning_rate=0.1, decay=0.5)
    assert [o.lr_at(t) for t in (1, 2, 3, 5)] == [0.1, 0.1 / 1.5, 0.1 / 2.0, 0.1 / 3.0]
    seen = []

    def schedule(step):
        seen.append(step)
        return 0.1 * 0.5 ** (step // 2)

    o = O.RMSprop(learning_rate=schedule)
    assert [o.lr_at(t) for t in (1, 2, 3, 4, 5)] == [0.1, 0.1, 0.05, 0.05, 0.025] and seen == [0, 1, 2, 3, 4]
    assert o.get_config()["learning_rate"]["class_name"] == "function"
    with pytest.raises(ValueError):
        O.SGD(decay=-0.1)


class FakeEngine:
    """Records what an optimizer asks of the engine (no GPU): the three step methods of UNetEngine."""
    def __init__(self):
        self.opt_step, self.calls = 0, []

    def adam_step(self, **kw):
        self.opt_step += 1; self.calls.append(("adam_step", kw))

    def sgd_step(self, **kw):
        self.opt_step += 1; self.calls.append(("sgd_step", kw))

    def optimizer_step(self, kind, **kw):
        self.opt_step += 1; self.calls.append(("optimizer_step", kind, kw))


def test_plain_adam_and_sgd_keep_their_entry_points_and_options_take_the_generic_one():
    e = FakeEngine()
    O.Adam(learning_rate=2e-3).apply(e)
    O.SGD(learning_rate=0.1, momentum=0.9).apply(e)
    assert e.calls == [("adam_step", dict(lr=2e-3, beta_1=0.9, beta_2=0.999, epsilon=1e-7)),
                       ("sgd_step", dict(lr=0.1, momentum=0.9))]
    for opt, kind in ((O.Adam(amsgrad=True), _hip.OPT_ADAM), (O.Adam(clipnorm=1.0), _hip.OPT_ADAM),
                      (O.Adam(decay=1e-3), _hip.OPT_ADAM), (O.Adam(learning_rate=lambda s: 1e-3), _hip.OPT_ADAM),
                      (O.SGD(momentum=0.9, nesterov=True), _hip.OPT_SGD), (O.SGD(clipvalue=0.1), _hip.OPT_SGD),
                      (O.Adamax(), _hip.OPT_ADAMAX), (O.RMSprop(), _hip.OPT_RMSPROP), (O.Adagrad(), _hip.OPT_ADAGRAD),
                      (O.Adadelta(), _hip.OPT_ADADELTA)):
        e = FakeEngine()
        opt.apply(e)
        assert e.calls[0][0] == "optimizer_step" and e.calls[0][1] == kind
    e = FakeEngine()
    o = O.RMSprop(learning_rate=0.1, decay=1.0, momentum=0.5, centered=True, global_clipnorm=3.0)
    o.apply(e); o.apply(e)
    assert [c[2]["lr"] for c in e.calls] == [0.1, 0.05]
    assert e.calls[0][2] == dict(lr=0.1, clip_mode=_hip.CLIP_GLOBAL_NORM, clip=3.0, rho=0.9, momentum=0.5, epsilon=1e-7,
                                 flags=_hip.OPT_CENTERED)


def test_descriptor_slot_counts():
    """oct_opt_slot_count agrees with the restatement's slot lists for every kind and flag combination (host only)."""
    import ctypes as C
    import __graft_entry__ as ge
    ge.build()
    lib = _hip.lib()
    for kind, mom, flags in [(_hip.OPT_SGD, 0.0, 0), (_hip.OPT_SGD, 0.9, 0), (_hip.OPT_SGD, 0.9, _hip.OPT_NESTEROV),
                             (_hip.OPT_SGD, 0.0, _hip.OPT_NESTEROV), (_hip.OPT_ADAM, 0.0, 0), (_hip.OPT_ADAM, 0.0, _hip.OPT_AMSGRAD),
                             (_hip.OPT_ADAMAX, 0.0, 0), (_hip.OPT_RMSPROP, 0.0, 0), (_hip.OPT_RMSPROP, 0.9, 0),
                             (_hip.OPT_RMSPROP, 0.0, _hip.OPT_CENTERED), (_hip.OPT_RMSPROP, 0.9, _hip.OPT_CENTERED),
                             (_hip.OPT_ADAGRAD, 0.0, 0), (_hip.OPT_ADADELTA, 0.0, 0)]:
        d = _hip.OptDesc(kind=kind, flags=flags, momentum=mom)
        assert lib.oct_opt_slot_count(C.byref(d)) == len(O.slot_names(kind, momentum=mom, flags=flags)), (kind, mom, flags)
    assert lib.oct_opt_slot_count(C.byref(_hip.OptDesc(kind=17))) == -1
    assert lib.oct_opt_scratch_bytes(90, 487403) >= 90 * 8 * 8 + 90 * 4
    assert lib.oct_opt_scratch_bytes(0, 1) >= 8 + 4
