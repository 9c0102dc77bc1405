"""Optimizer constructors a caller passes as ``TrainingParams.opt_con`` (the reference receives a Keras
optimizer class there, training/training.py:190-193): the Keras 2.9 ``optimizer_v2`` signatures, defaults and
``get_config`` keys of SGD, Adam, Adamax, RMSprop, Adagrad and Adadelta, with the shared keywords ``clipnorm``,
``clipvalue``, ``global_clipnorm``, ``decay`` and ``lr``.  The update itself runs on the device: plain Adam / SGD in
``adam_k`` / ``sgd_k``, everything else in ``opt_k`` behind ``oct_opt_step`` (formulas and the
clipping reduction: DESIGN.md section 13).  ``reference_step`` restates every formula in fp64 numpy."""
from __future__ import annotations

import numpy as np

from . import _hip

_SHARED_KWARGS = ("clipnorm", "clipvalue", "global_clipnorm", "decay", "lr")


class Optimizer:
    kind: int = -1

    def _init_shared(self, name: str, learning_rate, kwargs: dict) -> None:
        bad = sorted(k for k in kwargs if k not in _SHARED_KWARGS)
        if bad:
            raise TypeError(f"unsupported {type(self).__name__} arguments: {bad}")
        if "lr" in kwargs:
            learning_rate = kwargs["lr"]
        self.name = name
        self.learning_rate = learning_rate        # a float, or a schedule: any callable of the 0-based step
        self.decay = float(kwargs.get("decay", 0.0))
        if self.decay < 0:
            raise ValueError(f"decay cannot be less than 0: {self.decay}")
        self.clipnorm, self.clipvalue, self.global_clipnorm = (kwargs.get(k) for k in ("clipnorm", "clipvalue", "global_clipnorm"))
        given = [k for k in ("clipnorm", "clipvalue", "global_clipnorm") if getattr(self, k) is not None]
        if len(given) > 1:
            raise ValueError(f"at most one of clipnorm, clipvalue, global_clipnorm can be set, got {given}")
        for k in given:
            v = float(getattr(self, k))
            if not np.isfinite(v) or v < 0 or (v == 0 and k != "clipvalue"):
                raise ValueError(f"{k} must be positive, got {v}")

    # ---- what a step needs ---------------------------------------------------------------------------
    def lr_at(self, step: int) -> float:
        """Learning rate of the 1-based ``step``, in double on the host: a schedule is called with ``step - 1``; a
        constant is divided by ``1 + decay * (step - 1)`` (Keras ``_decayed_lr``)."""
        if callable(self.learning_rate):
            return float(self.learning_rate(step - 1))
        return float(self.learning_rate) / (1.0 + self.decay * (step - 1))

    def clip(self):
        """(``oct_opt_desc.clip_mode``, threshold)."""
        if self.clipvalue is not None:
            return _hip.CLIP_VALUE, float(self.clipvalue)
        if self.clipnorm is not None:
            return _hip.CLIP_NORM, float(self.clipnorm)
        if self.global_clipnorm is not None:
            return _hip.CLIP_GLOBAL_NORM, float(self.global_clipnorm)
        return _hip.CLIP_NONE, 0.0

    def _plain(self) -> bool:
        """No clipping, decay or schedule: the learning rate is one constant and the gradient is used as it is."""
        return self.clip()[0] == _hip.CLIP_NONE and self.decay == 0.0 and not callable(self.learning_rate)

    def hyper(self) -> dict:
        """Keyword arguments of ``UNetEngine.optimizer_step`` besides kind, lr and the clipping."""
        raise NotImplementedError

    def apply(self, engine) -> None:
        mode, thr = self.clip()
        engine.optimizer_step(self.kind, lr=self.lr_at(engine.opt_step + 1), clip_mode=mode, clip=thr, **self.hyper())

    # ---- Keras get_config ------------------------------------------------------------------------------
    def _config(self, **own) -> dict:
        cfg = {"name": self.name}
        for k in ("clipnorm", "clipvalue", "global_clipnorm"):       # Keras lists only the one that is set
            if getattr(self, k) is not None:
                cfg[k] = getattr(self, k)
        lr = self.learning_rate
        if callable(lr):    # Keras serializes a schedule as {"class_name", "config"}
            lr = {"class_name": type(lr).__name__, "config": lr.get_config() if hasattr(lr, "get_config") else {}}
        cfg.update({"learning_rate": lr, "decay": self.decay}, **own)
        return cfg

    def get_config(self) -> dict:
        raise NotImplementedError


class SGD(Optimizer):
    kind = _hip.OPT_SGD

    def __init__(self, learning_rate=0.01, momentum: float = 0.0, nesterov: bool = False, name: str = "SGD", **kwargs):
        self._init_shared(name, learning_rate, kwargs)
        if not 0 <= momentum <= 1:
            raise ValueError("`momentum` must be between [0, 1].")
        self.momentum, self.nesterov = momentum, bool(nesterov)

    def get_config(self) -> dict:
        return self._config(momentum=self.momentum, nesterov=self.nesterov)

    def hyper(self) -> dict:
        return dict(momentum=self.momentum, flags=_hip.OPT_NESTEROV if self.nesterov else 0)

    def apply(self, engine) -> None:
        if self._plain() and not self.nesterov:
            engine.sgd_step(lr=self.learning_rate, momentum=self.momentum)
        else:
            super().apply(engine)


class Adam(Optimizer):
    kind = _hip.OPT_ADAM

    def __init__(self, learning_rate=1e-3, beta_1: float = 0.9, beta_2: float = 0.999, epsilon: float = 1e-7,
                 amsgrad: bool = False, name: str = "Adam", **kwargs):
        self._init_shared(name, learning_rate, kwargs)
        self.beta_1, self.beta_2, self.epsilon, self.amsgrad = beta_1, beta_2, epsilon, bool(amsgrad)

    def get_config(self) -> dict:
        return self._config(beta_1=self.beta_1, beta_2=self.beta_2, epsilon=self.epsilon, amsgrad=self.amsgrad)

    def hyper(self) -> dict:
        return dict(beta_1=self.beta_1, beta_2=self.beta_2, epsilon=self.epsilon, flags=_hip.OPT_AMSGRAD if self.amsgrad else 0)

    def apply(self, engine) -> None:
        if self._plain() and not self.amsgrad:
            engine.adam_step(lr=self.learning_rate, beta_1=self.beta_1, beta_2=self.beta_2, epsilon=self.epsilon)
        else:
            super().apply(engine)


class Adamax(Optimizer):
    kind = _hip.OPT_ADAMAX

    def __init__(self, learning_rate=1e-3, beta_1: float = 0.9, beta_2: float = 0.999, epsilon: float = 1e-7,
                 name: str = "Adamax", **kwargs):
        self._init_shared(name, learning_rate, kwargs)
        self.beta_1, self.beta_2, self.epsilon = beta_1, beta_2, epsilon

    def get_config(self) -> dict:
        return self._config(beta_1=self.beta_1, beta_2=self.beta_2, epsilon=self.epsilon)

    def hyper(self) -> dict:
        return dict(beta_1=self.beta_1, beta_2=self.beta_2, epsilon=self.epsilon)


class RMSprop(Optimizer):
    kind = _hip.OPT_RMSPROP

    def __init__(self, learning_rate=1e-3, rho: float = 0.9, momentum: float = 0.0, epsilon: float = 1e-7,
                 centered: bool = False, name: str = "RMSprop", **kwargs):
        self._init_shared(name, learning_rate, kwargs)
        if not 0 <= momentum <= 1:
            raise ValueError("`momentum` must be between [0, 1].")
        self.rho, self.momentum, self.epsilon, self.centered = rho, momentum, epsilon, bool(centered)

    def get_config(self) -> dict:
        return self._config(rho=self.rho, momentum=self.momentum, epsilon=self.epsilon, centered=self.centered)

    def hyper(self) -> dict:
        return dict(rho=self.rho, momentum=self.momentum, epsilon=self.epsilon, flags=_hip.OPT_CENTERED if self.centered else 0)


class Adagrad(Optimizer):
    kind = _hip.OPT_ADAGRAD

    def __init__(self, learning_rate=1e-3, initial_accumulator_value: float = 0.1, epsilon: float = 1e-7,
                 name: str = "Adagrad", **kwargs):
        self._init_shared(name, learning_rate, kwargs)
        if initial_accumulator_value < 0.0:
            raise ValueError(f"initial_accumulator_value must be non-negative: {initial_accumulator_value}")
        self.initial_accumulator_value, self.epsilon = initial_accumulator_value, epsilon

    def get_config(self) -> dict:
        return self._config(initial_accumulator_value=self.initial_accumulator_value, epsilon=self.epsilon)

    def hyper(self) -> dict:
        return dict(epsilon=self.epsilon, initial_accumulator_value=self.initial_accumulator_value)


class Adadelta(Optimizer):
    kind = _hip.OPT_ADADELTA

    def __init__(self, learning_rate=1e-3, rho: float = 0.95, epsilon: float = 1e-7, name: str = "Adadelta", **kwargs):
        self._init_shared(name, learning_rate, kwargs)
        self.rho, self.epsilon = rho, epsilon

    def get_config(self) -> dict:
        return self._config(rho=self.rho, epsilon=self.epsilon)

    def hyper(self) -> dict:
        return dict(rho=self.rho, epsilon=self.epsilon)


def _not_implemented(name: str):
    class _Refused(Optimizer):
        def __init__(self, *args, **kwargs):
            raise NotImplementedError(f"the {name} optimizer is not implemented by the HIP engine "
                                      "(available: SGD, Adam, Adamax, RMSprop, Adagrad, Adadelta)")
    _Refused.__name__ = _Refused.__qualname__ = name
    return _Refused


Nadam = _not_implemented("Nadam")
Ftrl = _not_implemented("Ftrl")


# ---- fp64 restatement of every update (what the tests hold the kernels to) --------------------------------------------
def slot_names(kind: int, *, momentum: float = 0.0, flags: int = 0):
    """The state buffers of a configuration, in the order ``oct_opt_step`` takes them."""
    if kind == _hip.OPT_SGD:
        return ["v"] if momentum != 0.0 else []
    if kind == _hip.OPT_ADAM:
        return ["m", "v"] + (["vhat"] if flags & _hip.OPT_AMSGRAD else [])
    if kind == _hip.OPT_ADAMAX:
        return ["m", "u"]
    if kind == _hip.OPT_RMSPROP:
        return ["rms"] + (["mom"] if momentum != 0.0 else []) + (["mg"] if flags & _hip.OPT_CENTERED else [])
    if kind == _hip.OPT_ADAGRAD:
        return ["a"]
    if kind == _hip.OPT_ADADELTA:
        return ["a", "b"]
    raise ValueError(f"unknown optimizer kind {kind}")


def clip_gradient(g: np.ndarray, clip_mode: int, clip: float, var_off=None) -> np.ndarray:
    """clipvalue: min(max(g, -c), c); clipnorm: g * c / max(||g_var||, c) per variable [var_off[k], var_off[k+1]);
    global_clipnorm: the same with the norm of the whole buffer.  A zero norm gives scale 1."""
    g = np.asarray(g, np.float64)
    if clip_mode == _hip.CLIP_NONE:
        return g
    if clip_mode == _hip.CLIP_VALUE:
        return np.minimum(np.maximum(g, -clip), clip)
    if clip_mode == _hip.CLIP_GLOBAL_NORM:
        return g * (clip / max(float(np.sqrt(np.sum(g * g))), clip))
    out = g.copy()
    for lo, hi in zip(var_off[:-1], var_off[1:]):
        lo, hi = int(lo), int(hi)
        out[lo:hi] *= clip / max(float(np.sqrt(np.sum(g[lo:hi] ** 2))), clip)
    return out


def reference_step(kind: int, w, g, slots: dict, step: int, *, lr: float, beta_1: float = 0.9, beta_2: float = 0.999,
                   rho: float = 0.9, momentum: float = 0.0, epsilon: float = 1e-7, flags: int = 0,
                   clip_mode: int = _hip.CLIP_NONE, clip: float = 0.0, var_off=None):
    """One step in fp64 numpy: returns (w, slots) with ``slots`` a dict keyed by ``slot_names``.  ``step`` is 1-based,
    ``lr`` the learning rate of this step (``Optimizer.lr_at``).  An Adagrad accumulator starts at
    ``initial_accumulator_value``, every other buffer at zero."""
    w = np.asarray(w, np.float64)
    g = clip_gradient(g, clip_mode, clip, var_off)
    s = {k: np.asarray(v, np.float64) for k, v in slots.items()}
    t, mu = step, momentum
    if kind == _hip.OPT_SGD:
        if mu == 0.0:
            return w - lr * g, s
        v = mu * s["v"] - lr * g
        return (w + mu * v - lr * g if flags & _hip.OPT_NESTEROV else w + v), {"v": v}
    if kind == _hip.OPT_ADAM:
        lr_t = lr * np.sqrt(1.0 - beta_2 ** t) / (1.0 - beta_1 ** t)
        m = beta_1 * s["m"] + (1.0 - beta_1) * g
        v = beta_2 * s["v"] + (1.0 - beta_2) * g * g
        if flags & _hip.OPT_AMSGRAD:
            vh = np.maximum(s["vhat"], v)
            return w - lr_t * m / (np.sqrt(vh) + epsilon), {"m": m, "v": v, "vhat": vh}
        return w - lr_t * m / (np.sqrt(v) + epsilon), {"m": m, "v": v}
    if kind == _hip.OPT_ADAMAX:
        m = beta_1 * s["m"] + (1.0 - beta_1) * g
        u = np.maximum(beta_2 * s["u"], np.abs(g))
        return w - lr / (1.0 - beta_1 ** t) * m / (u + epsilon), {"m": m, "u": u}
    if kind == _hip.OPT_RMSPROP:
        out = {"rms": rho * s["rms"] + (1.0 - rho) * g * g}
        d = out["rms"]
        if flags & _hip.OPT_CENTERED:
            out["mg"] = rho * s["mg"] + (1.0 - rho) * g
            d = d - out["mg"] ** 2
        if mu == 0.0:
            return w - lr * g / (np.sqrt(d) + epsilon), out
        out["mom"] = mu * s["mom"] + lr * g / np.sqrt(d + epsilon)      # the fused-op form: epsilon inside the root
        return w - out["mom"], out
    if kind == _hip.OPT_ADAGRAD:
        a = s["a"] + g * g
        return w - lr * g / (np.sqrt(a) + epsilon), {"a": a}
    if kind == _hip.OPT_ADADELTA:
        a = rho * s["a"] + (1.0 - rho) * g * g
        u = g * np.sqrt(s["b"] + epsilon) / np.sqrt(a + epsilon)
        return w - lr * u, {"a": a, "b": rho * s["b"] + (1.0 - rho) * u * u}
    raise ValueError(f"unknown optimizer kind {kind}")
