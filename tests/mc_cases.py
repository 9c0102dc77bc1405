"""Shared by the Monte-Carlo dropout tests: the fp64 oracle of ONE stochastic inference forward, and the random softmax
stacks the reduction kernel is held to."""
import numpy as np

from oracle import unet_numpy as on


def forward_mc_oracle(cfg, params, state, x, mask):
    """Softmax output of an INFERENCE forward (BN from the moving statistics) with the dropout keep-``mask``
    (B, H/2^P, W/2^P, start_neurons*2^P) of {0,1} applied, times 1 / (1 - rate), behind the bottleneck -- what one sample
    of ``oct_unet_infer`` (kind MC) computes.  ``oracle.unet_numpy.forward`` applies the mask only when ``training`` (which also
    switches BN to batch statistics), so the combination is composed here from its layer functions, walking ``build_plan``
    exactly as it does.  fp64 throughout: ``params`` / ``state`` / ``x`` are float64."""
    plan = on.build_plan(cfg)
    out_of, cur, bn_idx, probs = {}, x, 0, None
    for li, spec in enumerate(plan):
        p = params[li]
        if spec.src in ("input", "prev", "head"):
            inp = cur
        elif spec.src == "pool":
            inp = on.maxpool2x2(cur)
        elif spec.src == "up":
            inp = on.upsample2x(cur)
        elif spec.src == "concat":
            inp = np.concatenate([cur, out_of[spec.skip_from]], axis=-1)
        else:
            raise AssertionError(spec.src)
        z = on.conv2d_same(inp, p["kernel"], p["bias"])
        if not spec.has_bn:
            probs = on.softmax(z)
            continue
        st = state[bn_idx]; bn_idx += 1
        cur = on.relu(on.batchnorm_infer(z, p["gamma"], p["beta"], st["moving_mean"], st["moving_var"], cfg.bn_eps))
        out_of[li] = cur
        if spec.name == f"mid.conv{cfg.conv_layers - 1}" and cfg.dropout_rate > 0:
            assert mask.shape == cur.shape, (mask.shape, cur.shape)
            cur = cur * (mask.astype(np.float64) / (1.0 - cfg.dropout_rate))
    return probs


def softmax_stack(shape, seed):
    """(T, B, H, W, C) float32 softmax outputs of random logits with a spread that saturates some of them, with exact
    zeros and ones injected: every 7th pixel of every sample is a one-hot (a 1.0 and C-1 zeros), every 11th has one class
    zeroed (the rest no longer sums to 1: the kernel does not care)."""
    T, B, H, W, C = shape
    rng = np.random.default_rng(seed)
    z = rng.normal(0.0, 4.0, shape)
    z -= z.max(-1, keepdims=True)
    p = np.exp(z); p /= p.sum(-1, keepdims=True)
    p = p.astype(np.float32).reshape(T, -1, C)
    hot = np.zeros((T, p.shape[1], C), np.float32)
    hot[np.arange(T)[:, None], np.arange(p.shape[1])[None, :], rng.integers(0, C, (T, p.shape[1]))] = 1.0
    p[:, ::7] = hot[:, ::7]
    p[:, 3::11, rng.integers(0, C)] = 0.0
    return np.ascontiguousarray(p.reshape(shape))


# entropy / mutual information against the fp64 restatement: logf is ~1 ulp, so a p ln p term is off by <= ~1e-7; a class sum
# of <= 32 terms of <= ln 32 adds a few 1e-6; the sequential sum over T <= 64 of values <= ln C carries <= T 2^-24 relative,
# ~8e-6 after the division
ENTROPY_TOL = 2e-5
