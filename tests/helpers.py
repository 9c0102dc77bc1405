"""Shared test helpers (CPU side): numpy replica of the engine's counter-based dropout stream and a
ReLU-boundary margin check that justifies tight fp32-vs-fp64 tolerances; a writable view of an engine's stored tensors;
the untrained model and the result-tree comparison of the workflow tests."""
import json
from pathlib import Path

import numpy as np

from oracle import unet_numpy as on


def drop_hash(seed: int, step: int, idx: np.ndarray) -> np.ndarray:
    """Replica of oct::drop_hash (csrc/common.hpp)."""
    with np.errstate(over="ignore"):
        x = np.uint64(seed) ^ (np.uint64(step) * np.uint64(0x9E3779B97F4A7C15)) \
            ^ (idx.astype(np.uint64) * np.uint64(0xD1B54A32D192ED03))
        x ^= x >> np.uint64(33); x *= np.uint64(0xff51afd7ed558ccd)
        x ^= x >> np.uint64(33); x *= np.uint64(0xc4ceb9fe1a85ec53)
        x ^= x >> np.uint64(33)
    return (x >> np.uint64(32)).astype(np.uint32)


def dropout_keep_mask(seed: int, step: int, shape, rate: float = 0.5) -> np.ndarray:
    n = int(np.prod(shape))
    thresh = min(4294967295, int(np.floor(rate * 4294967296.0)))
    return (drop_hash(seed, step, np.arange(n, dtype=np.uint32)) >= np.uint32(thresh)).reshape(shape)


def relu_margin(cfg, params, cache) -> float:
    """Smallest |gamma*xhat+beta| over all BN blocks of a training forward: if it is well above the fp32
    rounding of the device path, no ReLU mask (and no pool arg-max among positive values) can flip."""
    m = np.inf
    for li, spec in enumerate(on.build_plan(cfg)):
        if spec.has_bn:
            yb = params[li]["gamma"] * cache[li]["xhat"] + params[li]["beta"]
            m = min(m, float(np.abs(yb).min()))
    return m


def stored_activation_view(eng, layer: int, which: int = 0):
    """A layer's saved pre-BN output (which=0) or gradient buffer (which=1) as a WRITABLE (max_batch, H, W, cout) view
    of the engine's workspace in its storage type (float32, or bfloat16 where ``debug_activation`` returns a copy)."""
    import torch
    L = eng.layers[layer]
    shape = (eng.cfg.max_batch, L["out_h"], L["out_w"], L["cout"])
    n = shape[0] * shape[1] * shape[2] * shape[3]
    bf = eng.cfg.dtype == 1
    ref = eng.debug_activation(layer, which)          # (raises for a layer without such a buffer)
    if not bf:
        return ref
    # bf16 storage: find the buffer's offset the way debug_activation does
    from oct_image_segmentation_models_amd import _hip
    off = _hip.lib().oct_unet_debug_activation(eng._h, layer, which) - eng.workspace.data_ptr()
    return eng.workspace[off:off + 2 * n].view(torch.bfloat16).view(shape)


def save_untrained_model(root: Path, H: int, W: int, num_classes: int, start_neurons: int, pool_layers: int):
    """An untrained ``unet`` of that geometry (oracle weights of seed 3, randomised BN) saved as ``root/model/model.npz``
    beside its ``model_config.json``; returns the path of the weights."""
    from oct_image_segmentation_models_amd.models.engine_model import Model
    config = dict(input_channels=1, num_classes=num_classes, image_height=H, image_width=W, start_neurons=start_neurons,
                  pool_layers=pool_layers)
    cfg = on.UNetConfig(num_classes=num_classes, start_neurons=start_neurons, pool_layers=pool_layers)
    params, state = on.init_params(cfg, seed=3, dtype=np.float32, randomize_bn=True)
    m = Model(name="unet", config=config)
    m.set_weights(on.keras_weight_list(params, state))
    (root / "model").mkdir()
    path = m.save(root / "model" / "model.npz")
    with open(root / "model" / "model_config.json", "w") as fh:
        json.dump(config, fh)
    return path


def datasets_equal(a: dict, b: dict, where=None):
    """Two loaded result files hold the same datasets: names, dtypes, shapes and values (NaN equal to NaN)."""
    keys = sorted(k for k in a if not k.startswith("attr:"))
    assert keys == sorted(k for k in b if not k.startswith("attr:")), where
    for k in keys:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.dtype == y.dtype and x.shape == y.shape, (where, k)
        assert np.array_equal(x, y, equal_nan=x.dtype.kind == "f"), (where, k)


def tree_equal(a: Path, b: Path, h5_names):
    """Every file under ``a`` has its twin under ``b``: hdf5 datasets identical (attributes carry the times; ``b`` may
    carry attributes ``a`` lacks), CSV and text files byte for byte."""
    from oct_image_segmentation_models_amd.common import h5io
    fa, fb = (sorted(p.relative_to(r) for p in r.rglob("*") if p.is_file()) for r in (a, b))
    assert fa == fb and fa
    seen = set()
    for rel in fa:
        if ".hdf5" in rel.suffixes:                                            # (foo.hdf5.npz without an HDF5 backend)
            x, y = h5io.load(a / rel), h5io.load(b / rel)
            datasets_equal(x, y, rel)
            for k in {k for k in x if k.startswith("attr:")} - {"attr:graph_time", "attr:predict_time", "attr:convert_time",
                                                                "attr:timestamp"}:
                assert np.array_equal(np.asarray(x[k]), np.asarray(y[k])), (rel, k)
            seen.add(rel.name.replace(".npz", ""))
        else:
            assert (a / rel).read_bytes() == (b / rel).read_bytes(), rel
    assert set(h5_names) <= seen
