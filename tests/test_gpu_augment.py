"""GPU tests of ``oct_augment_batch`` (include/oct_unet.h) and of the training path that uses it, against the numpy
restatement ``common.augmentation.device_aug_reference``.

Flips, no-op and salt-and-pepper are exact.  Gaussian / speckle are compared with the float64 restatement under
``|out - ref| <= 1e-5 sigma + 2^-23`` on EVERY element: |z| <= sqrt(-2 ln 2^-24) = 5.77; logf, sqrtf and cos a few ulp
each give |dz| of order 1e-6 (the fp32 numpy evaluation of the same formula differs from float64 by 1.6e-6 at most over
2^23 draws); scaled by sigma (times img <= 1 for speckle), plus one fp32 rounding (2^-24) of a value <= 1 for each of the
two final operations.  Clipping to [0, 1] cannot increase a difference, so elements at a clip edge are compared too."""
import ctypes as C
import os
import socket
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from oct_image_segmentation_models_amd.common import augmentation as A
from test_augment_device import check_distribution, distribution_inputs

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
SHAPES = [(32, 256, 512, 1), (3, 6, 10, 1), (2, 16, 32, 3)]
SEED = (0x1234ABCD << 32) | 0x9E3779B9


@pytest.fixture(scope="module")
def eng():
    from oct_image_segmentation_models_amd.engine import UNetEngine
    return UNetEngine(device="cuda:0", input_channels=1, num_classes=3, image_height=16, image_width=32, start_neurons=8,
                      pool_layers=2, max_batch=1, training=False)


def _batch(shape, seed=0):
    rng = np.random.default_rng(seed)
    B, H, W, _ = shape
    return rng.integers(0, 256, shape, dtype=np.uint8), rng.integers(0, 4, (B, H, W), dtype=np.uint8)


def _ops(kinds, p0=0.0, p1=0.0, first_id=100):
    ops = np.zeros(len(kinds), dtype=A.AUG_OP_DTYPE)
    ops["kind"], ops["p0"], ops["p1"] = kinds, p0, p1
    ops["noise_id"] = first_id + np.arange(len(kinds)) + (np.arange(len(kinds), dtype=np.uint64) << np.uint64(33))
    return ops


def _run(eng, x, lab, ops, seed=SEED):
    xo, lo = eng.augment(torch.from_numpy(x).cuda(), None if lab is None else torch.from_numpy(lab).cuda(), ops, seed)
    torch.cuda.synchronize()
    return xo.cpu().numpy(), None if lo is None else lo.cpu().numpy()


@pytest.mark.parametrize("shape", SHAPES)
def test_exact_kinds(eng, shape):
    """none, both flips, s&p, salt, pepper, mixed inside one batch: images AND labels bit-identical."""
    B = shape[0]
    x, lab = _batch(shape, seed=1)
    cycle = [(0, 0, 0), (1, 0, 0), (2, 0, 0), (5, 0.05, 0.5), (5, 0.2, 1.0), (5, 0.2, 0.0)]
    rows = [cycle[b % len(cycle)] for b in range(B)]
    ops = _ops([r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows])
    ref_x, ref_l = A.device_aug_reference(x, lab, ops, SEED)
    out_x, out_l = _run(eng, x, lab, ops)
    assert out_x.dtype == np.float32 and np.array_equal(out_x, ref_x)
    assert np.array_equal(out_l, ref_l)
    if B >= len(cycle):       # every kind did something: flips moved pixels, s&p flipped some
        for b, (kind, _, _) in enumerate(rows[:len(cycle)]):
            same = np.array_equal(out_x[b], A.device_aug_reference(x[b:b + 1], None, _ops([0]), SEED)[0][0])
            assert same == (kind == 0)
    # without labels nothing but the images is written
    only_x, none = _run(eng, x, None, ops)
    assert none is None and np.array_equal(only_x, ref_x)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("sigma", [0.1, 0.3])
def test_gaussian_and_speckle_against_float64(eng, shape, sigma):
    B = shape[0]
    x, lab = _batch(shape, seed=2)
    kinds = [A.AUG_GAUSSIAN if b % 2 == 0 else A.AUG_SPECKLE for b in range(B)]
    ops = _ops(kinds, [0.0 if b % 4 < 2 else 0.05 for b in range(B)], sigma)
    ref_x, ref_l = A.device_aug_reference(x, lab, ops, SEED)
    out_x, out_l = _run(eng, x, lab, ops)
    err = float(np.abs(out_x.astype(np.float64) - ref_x.astype(np.float64)).max())
    print(f"shape {shape} sigma {sigma}: max |out - ref| = {err:.3e}, bound {1e-5 * sigma + 2.0 ** -23:.3e}")
    assert err <= 1e-5 * sigma + 2.0 ** -23
    assert out_x.min() >= 0.0 and out_x.max() <= 1.0 and np.array_equal(out_l, lab) and np.array_equal(ref_l, lab)
    assert np.abs(out_x - A.device_aug_reference(x, None, _ops([0] * B), SEED)[0]).mean() > 0.1 * sigma * 0.3   # noise was added


def test_distribution_on_the_device(eng):
    x, ops = distribution_inputs()
    out, _ = _run(eng, x, None, ops, seed=2024)
    check_distribution(out[:2, ..., 0], out[2, ..., 0], 128 / 255.0, 0.1, 0.05, 0.5)


def test_determinism_and_geometry_independence(eng):
    shape = (32, 64, 128, 1)
    x, lab = _batch(shape, seed=3)
    ops = _ops([3, 4, 5, 1, 2, 0, 3, 5] * 4, [0.0, 0.0, 0.1, 0, 0, 0, 0.02, 0.05] * 4, [0.1, 0.2, 0.5, 0, 0, 0, 0.05, 0.3] * 4)
    a = _run(eng, x, lab, ops)
    b = _run(eng, x, lab, ops)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    halves = [_run(eng, x[lo:lo + 16], lab[lo:lo + 16], ops[lo:lo + 16]) for lo in (0, 16)]
    assert np.array_equal(np.concatenate([h[0] for h in halves]), a[0])
    assert np.array_equal(np.concatenate([h[1] for h in halves]), a[1])
    one = _run(eng, x[6:7], lab[6:7], ops[6:7])
    assert np.array_equal(one[0][0], a[0][6]) and np.array_equal(one[1][0], a[1][6])
    # the noise follows noise_id and the seed, not the batch position
    moved = ops[[6, 0]].copy()
    swapped = _run(eng, x[[6, 0]], lab[[6, 0]], moved)
    assert np.array_equal(swapped[0][0], a[0][6]) and np.array_equal(swapped[0][1], a[0][0])
    assert not np.array_equal(_run(eng, x[:1], lab[:1], ops[:1], seed=SEED + 1)[0], a[0][:1])


def test_argument_errors_launch_nothing(eng):
    from oct_image_segmentation_models_amd import _hip
    lib = _hip.lib()
    B, H, W, Cn = 2, 8, 16, 1
    n = B * H * W * Cn
    x = torch.zeros(n, dtype=torch.uint8, device="cuda")
    lab = torch.zeros(B * H * W, dtype=torch.uint8, device="cuda")
    ops = torch.from_numpy(_ops([1, 3], 0.0, 0.1).view(np.uint8).copy()).cuda()
    arena = torch.full((8 * n,), 0x5A, dtype=torch.uint8, device="cuda")       # outputs with a sentinel
    out, lab_out = arena[:4 * n], arena[4 * n:4 * n + B * H * W]
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: None if t is None else t.data_ptr()

    def call(x_=x, lab_=lab, ops_=ops, dims=(B, H, W, Cn), out_=out, lab_out_=lab_out):
        return lib.oct_augment_batch(p(x_), p(lab_), p(ops_), *dims, 1, p(out_), p(lab_out_), stream)

    bad = [dict(x_=None), dict(ops_=None), dict(out_=None), dict(dims=(0, H, W, Cn)), dict(dims=(B, -1, W, Cn)),
           dict(dims=(B, H, 0, Cn)), dict(dims=(B, H, W, 0)), dict(lab_=None),                # labels_out without labels
           dict(out_=arena[4 * n - 4:8 * n - 4]),                                               # out overlaps labels_out
           dict(x_=arena[:n]), dict(lab_=arena[16:16 + B * H * W]), dict(x_=arena[4 * n:5 * n])]
    for kw in bad:
        rc = call(**kw)
        assert rc < 0 and b"augment_batch" in lib.oct_last_error(), kw
    torch.cuda.synchronize()
    assert bool((arena == 0x5A).all())
    assert call() == 0
    torch.cuda.synchronize()
    assert not bool((arena[:4 * n + B * H * W] == 0x5A).all())
    # the Python binding validates descriptors before upload
    from oct_image_segmentation_models_amd._hip import OctError
    with pytest.raises(OctError, match="kind"):
        eng.augment(x.view(B, H, W, Cn), lab.view(B, H, W), _ops([1, 6]), 1)


def _compiled_model(cfg, seed):
    from oct_image_segmentation_models_amd import optimizers
    from oct_image_segmentation_models_amd.common import custom_losses, custom_metrics
    from oct_image_segmentation_models_amd.models import get_model_class
    model = get_model_class("unet")(**cfg).build_model()
    model.config["seed"] = seed
    nc = cfg["num_classes"]
    loss = custom_losses.custom_loss_objects["dice_loss_macro"]["function"](num_classes=nc, is_y_true_sparse=True)
    metric = custom_metrics.training_monitor_metric_objects["dice_coef_macro"](True, nc)
    model.compile(optimizer=optimizers.Adam(learning_rate=2e-3), loss=loss, metrics=[metric])
    return model


FIT_CFG = dict(input_channels=1, num_classes=3, image_height=32, image_width=64, start_neurons=8, pool_layers=2)
FLIPS = [(A.flip_aug, {"flip_type": "up-down"}), (A.flip_aug, {"flip_type": "left-right"}), (A.no_aug, {})]


def test_fit_with_flips_equals_the_host_path():
    """Mode "all" with flips only: 2 epochs x 2 steps of batch 3 over 2 images x 3 augmentations; the device path feeds
    the network the bits the host path feeds it, so the parameters end bit-identical."""
    from oracle import unet_numpy as on
    from oct_image_segmentation_models_amd.common.data_generator import DataGenerator
    images, labels = on.synth_scans(2, 32, 64, 3, seed=5)
    got = []
    for device_aug in (False, True):
        model = _compiled_model(FIT_CFG, seed=3)
        gen = DataGenerator(images, labels, 3, FLIPS, "all", (), True, None, seed=8, device_aug=device_aug)
        assert gen.oct_device_aug == device_aug and len(gen) == 2
        hist = model.fit(x=gen, epochs=2, verbose=0)
        torch.cuda.synchronize()
        got.append((model.engine.params.cpu().numpy(), model.engine.state.cpu().numpy(), hist.history["loss"]))
    assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1]) and got[0][2] == got[1][2]
    assert np.isfinite(got[0][0]).all() and len(got[0][2]) == 2


def test_train_model_end_to_end_with_device_augmentation(tmp_path):
    from oct_image_segmentation_models_amd import optimizers
    from oct_image_segmentation_models_amd.common import h5io
    from oct_image_segmentation_models_amd.training.training import train_model
    from oct_image_segmentation_models_amd.training.training_parameters import TrainingParams
    tp = TrainingParams(model_architecture="unet", training_dataset_path=ROOT / "tests" / "golden" / "dataset_small.hdf5",
                        initial_model=None, results_location=tmp_path / "results", opt_con=optimizers.Adam,
                        opt_params={"learning_rate": 4e-3}, loss="dice_loss_macro", metric="dice_coef_macro", epochs=2,
                        batch_size=2, model_hyperparameters={"pool_layers": 2}, seed=3,
                        augmentations=[{"name": "add_noise", "arguments": {"mode": "gaussian", "variance": 0.01}},
                                       {"name": "flip", "arguments": {"flip_type": "left-right"}}],
                        aug_mode="one", aug_probs=(0.5, 0.5), aug_fly=True, aug_val=True, aug_device=True)
    res = train_model(tp, None)
    h = res.history
    assert set(h) == {"loss", "dice_coef_macro", "val_loss", "val_dice_coef_macro"}
    assert all(len(v) == 2 and np.isfinite(v).all() for v in h.values())
    assert len(res.checkpoints) >= 1 and all(Path(p).exists() for p in res.checkpoints)
    attrs = h5io.load(Path(res.save_foldername) / "training_params.hdf5")
    assert bool(attrs["attr:aug_device"]) is True and bytes(attrs["attr:aug_mode"]).rstrip(b"\x00") == b"one"


# ---- 2-rank data parallelism on one GPU (pattern of tests/test_gpu_dp.py: gloo between two processes on cuda:0) ----
DP_AUGS = [(A.add_noise_aug, {"mode": "gaussian"}), (A.flip_aug, {"flip_type": "left-right"}),
           (A.add_noise_aug, {"mode": "s&p"}), (A.add_noise_aug, {"mode": "speckle"})]
G = 6


def _augmented_batches(rank, world):
    """What Model._run_epoch feeds the engine for the first 3 global batches: this rank's augmented slice."""
    from oracle import unet_numpy as on
    from oct_image_segmentation_models_amd.common.data_generator import DataGenerator
    images, labels = on.synth_scans(9, 32, 64, 3, seed=21)
    model = _compiled_model(FIT_CFG, seed=1)
    gen = DataGenerator(images, labels, G, DP_AUGS, "one", (0.4, 0.2, 0.2, 0.2), True, None, seed=77, device_aug=True)
    outs = []
    for i in range(3):
        b = model.feed.upload(model.feed.host_batch(gen, i, rank, world), i % 3)
        torch.cuda.current_stream().wait_event(b.ready)
        e = model._ensure_engine(b.x.shape[0], True)
        xa, la = model.feed.augment(e, gen.oct_aug_seed, b)
        torch.cuda.synchronize()
        outs.append((xa.cpu().numpy().copy(), la.cpu().numpy().copy()))
        if i == 0:
            gen.on_epoch_end()
    return np.stack([o[0] for o in outs]), np.stack([o[1] for o in outs])


def _dp_worker(rank, world, port, tmpdir):
    os.environ.update(RANK=str(rank), LOCAL_RANK="0", WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    from oct_image_segmentation_models_amd import parallel
    parallel.init("gloo")
    torch.cuda.set_device(0)
    x, lab = _augmented_batches(rank, world)
    np.savez(os.path.join(tmpdir, f"aug{rank}.npz"), x=x, lab=lab)
    torch.distributed.destroy_process_group()


def test_two_rank_slices_equal_the_one_rank_batch(tmp_path):
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    mp.spawn(_dp_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    r0, r1 = np.load(tmp_path / "aug0.npz"), np.load(tmp_path / "aug1.npz")
    x, lab = _augmented_batches(0, 1)
    assert r0["x"].shape == (3, G // 2, 32, 64, 1) and x.shape == (3, G, 32, 64, 1)
    assert np.array_equal(np.concatenate([r0["x"], r1["x"]], axis=1), x)
    assert np.array_equal(np.concatenate([r0["lab"], r1["lab"]], axis=1), lab)
