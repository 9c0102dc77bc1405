"""CPU tests of the device augmentation's host side: the Philox restatement, the descriptor walk of
``BatchGenerator.next_batch_aug`` against ``get_batch_list`` and the fall-backs.  No GPU, no library call.

The image of the distribution tests is constant uint8 128 = float32(128/255) = 0.50196: the input of
``oct_augment_batch`` is uint8, so exactly 0.5 does not exist; every bound is taken about that value."""
import numpy as np
import pytest

from oct_image_segmentation_models_amd.common import augmentation as A
from oct_image_segmentation_models_amd.common.data_generator import DataGenerator

FLIPS = [(A.flip_aug, {"flip_type": "up-down"}), (A.no_aug, {}), (A.flip_aug, {"flip_type": "left-right"})]
MODES = [("one", (0.2, 0.5, 0.3)), ("all", ())]


def _data(n=7, h=6, w=10, c=1, seed=0):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (n, h, w, c), dtype=np.uint8), rng.integers(0, 3, (n, h, w, 1), dtype=np.uint8)


def _words(*vals):
    return [int(v, 16) for v in vals]


@pytest.mark.parametrize("ctr, key, want", [
    (["0"] * 4, ["0"] * 2, ["6627e8d5", "e169c58d", "bc57ac4c", "9b00dbd8"]),
    (["ffffffff"] * 4, ["ffffffff"] * 2, ["408f276d", "41c83b0e", "a20bc7c6", "6d5451fd"]),
    (["243f6a88", "85a308d3", "13198a2e", "03707344"], ["a4093822", "299f31d0"],
     ["d16cfe09", "94fdcceb", "5001e420", "24126ea1"]),
])
def test_philox_known_answers(ctr, key, want):
    """Random123 kat_vectors, philox4x32 with 10 rounds."""
    out = A.philox4x32_10(_words(*ctr), _words(*key))
    assert out.dtype == np.uint32 and out.tolist() == _words(*want)


def test_philox_is_vectorised():
    ctr = np.array([_words("0", "0", "0", "0"), _words("243f6a88", "85a308d3", "13198a2e", "03707344")], dtype=np.uint32)
    key = np.array([_words("0", "0"), _words("a4093822", "299f31d0")], dtype=np.uint32)
    out = A.philox4x32_10(ctr, key)
    assert out.shape == (2, 4)
    assert out[0].tolist() == _words("6627e8d5", "e169c58d", "bc57ac4c", "9b00dbd8")
    assert out[1].tolist() == _words("d16cfe09", "94fdcceb", "5001e420", "24126ea1")
    # element e of a sample owns words 2(e&1), 2(e&1)+1 of the block with counter (e >> 1, 0, noise_id)
    w0, w1 = A.device_aug_words(5, noise_id=(7 << 32) | 9, seed=(3 << 32) | 2)
    for e in range(5):
        blk = A.philox4x32_10([e >> 1, 0, 9, 7], [2, 3])
        assert (w0[e], w1[e]) == (blk[2 * (e & 1)], blk[2 * (e & 1) + 1])


def test_descriptor_layout_and_templates():
    assert A.AUG_OP_DTYPE.itemsize == 32 and A.AUG_OP_DTYPE.fields["noise_id"][1] == 16
    ops = A.aug_ops_from(FLIPS + [(A.add_noise_aug, {"mode": "gaussian", "mean": 0.1, "variance": 0.04}),
                                  (A.add_noise_aug, {"mode": "speckle"}), (A.add_noise_aug, {"mode": "s&p", "amount": 0.1}),
                                  (A.add_noise_aug, {"mode": "salt"}), (A.add_noise_aug, {"mode": "pepper"})])
    assert ops["kind"].tolist() == [1, 0, 2, 3, 4, 5, 5, 5]
    assert ops["p0"][3] == np.float32(0.1) and ops["p1"][3] == np.float32(0.2) and ops["p1"][4] == np.float32(0.1)
    assert ops["p0"][5:].tolist() == [np.float32(0.1), np.float32(0.05), np.float32(0.05)]
    assert ops["p1"][5:].tolist() == [0.5, 1.0, 0.0]
    assert A.aug_ops_from([(lambda i, m, a: (i, m), {})]) is None
    assert A.aug_ops_from([(A.add_noise_aug, {"mode": "poisson"})]) is None
    assert A.aug_ops_from([(A.flip_aug, {"flip_type": "diagonal"})]) is None


@pytest.mark.parametrize("mode, probs", MODES)
@pytest.mark.parametrize("fly", [True, False])
def test_state_equivalence_with_host_path(mode, probs, fly):
    """Same seed, deterministic augmentations: the device walk hands out the (image, augmentation) pairs of
    ``__getitem__``, batch by batch, over 2 epochs with N not a multiple of the batch."""
    im, lb = _data()
    dev = DataGenerator(im, lb, 4, FLIPS, mode, probs, fly, None, seed=3, device_aug=True)
    host = DataGenerator(im, lb, 4, FLIPS, mode, probs, fly, None, seed=3)
    assert dev.oct_device_aug and not host.oct_device_aug and len(dev) == len(host) > 0
    assert dev.batch_gen.images is None        # no float copy of the dataset on the host
    for _ in range(2):
        for i in range(len(dev)):
            x, lab = A.device_aug_reference(*dev.next_batch_aug(), seed=1)
            X, y = host[i]
            assert x.dtype == np.float32 and np.array_equal(x, X) and np.array_equal(lab, y[..., 0])
            for k in ("full_counter", "aug_counter", "batch_counter"):
                assert getattr(dev.batch_gen, k) == getattr(host.batch_gen, k)
        dev.on_epoch_end(); host.on_epoch_end()


@pytest.mark.parametrize("mode, probs", MODES)
@pytest.mark.parametrize("fly", [True, False])
def test_shard_invariance(mode, probs, fly):
    im, lb = _data(n=9)
    augs = FLIPS[:2] + [(A.add_noise_aug, {"mode": "gaussian"})]
    whole, r0, r1 = (DataGenerator(im, lb, 6, augs, mode, probs, fly, None, seed=5, device_aug=True) for _ in range(3))
    for _ in range(2):
        for _ in range(len(whole)):
            x, lab, ops = whole.next_batch_aug()
            parts = [r0.next_batch_aug(shard=(0, 3)), r1.next_batch_aug(shard=(3, 6))]
            assert np.array_equal(np.concatenate([p[0] for p in parts]), x)
            assert np.array_equal(np.concatenate([p[1] for p in parts]), lab)
            assert np.concatenate([p[2] for p in parts]).tobytes() == ops.tobytes() and ops.dtype == A.AUG_OP_DTYPE
        for g in (whole, r0, r1):
            g.on_epoch_end()


def test_noise_id_rules():
    im, lb = _data(n=7)
    augs = [(A.add_noise_aug, {"mode": "gaussian"}), (A.add_noise_aug, {"mode": "speckle"})]
    # aug_fly: a running count of the samples drawn -> no id twice within 3 epochs
    g = DataGenerator(im, lb, 4, augs, "all", (), True, None, seed=2, device_aug=True)
    ids = []
    for _ in range(3):
        for _ in range(len(g)):
            ids.append(g.next_batch_aug()[2]["noise_id"])
        g.on_epoch_end()
    ids = np.concatenate(ids)
    assert ids.tolist() == list(range(len(ids))) and len(ids) == 3 * 3 * 4
    # pre-computed set: image_index * n_augs + j, the same for a pair in every epoch
    for mode, probs in (("all", ()), ("one", (0.5, 0.5))):
        g = DataGenerator(im, lb, 3, augs, mode, probs, False, None, seed=2, device_aug=True)
        seen = {}
        for _ in range(3):
            for _ in range(len(g)):
                x, _, ops = g.next_batch_aug()
                for xb, op in zip(x, ops):
                    idx = [i for i in range(len(im)) if np.array_equal(im[i], xb)]
                    assert len(idx) == 1
                    j = int(op["kind"]) - A.AUG_GAUSSIAN
                    assert int(op["noise_id"]) == idx[0] * 2 + j
                    seen[(idx[0], j)] = seen.get((idx[0], j), 0) + 1
            g.on_epoch_end()
        assert max(seen.values()) >= 2          # pairs recur across epochs, with their id


N_STAT = 1 << 23


def _lag1(a):
    """Correlation of horizontally adjacent elements of a (H, W) array."""
    a = a - a.mean()
    return float((a[:, :-1] * a[:, 1:]).mean() / a.var())


def check_distribution(gauss, sp, img, sigma, amount, svp):
    """Shared with the GPU test: ``gauss`` (2, H, W) gaussian output of two noise ids on the constant image ``img``,
    ``sp`` (H, W) salt-and-pepper output.  n = H*W = 2^23 per sample."""
    n = gauss[0].size
    assert n == N_STAT
    g = gauss.astype(np.float64)
    for s in g:
        assert abs(s.mean() - img) <= 5 * sigma / np.sqrt(n), s.mean() - img
        assert abs(s.var() / sigma ** 2 - 1) <= 0.01, s.var()
        assert abs(_lag1(s)) <= 5 / np.sqrt(n), _lag1(s)
    a, b = g[0] - g[0].mean(), g[1] - g[1].mean()
    cross = float((a * b).mean() / np.sqrt(a.var() * b.var()))
    assert abs(cross) <= 5 / np.sqrt(n), cross
    flipped = sp != np.float32(img)
    k = int(flipped.sum())
    assert abs(k - n * amount) <= 5 * np.sqrt(n * amount * (1 - amount)), k / n
    salted = int((sp[flipped] == 1).sum())
    assert np.all((sp[flipped] == 0) | (sp[flipped] == 1))
    assert abs(salted - k * svp) <= 5 * np.sqrt(k * svp * (1 - svp)), salted / k


def distribution_inputs():
    h, w = 2048, 4096
    ops = np.zeros(3, dtype=A.AUG_OP_DTYPE)
    ops["kind"] = [A.AUG_GAUSSIAN, A.AUG_GAUSSIAN, A.AUG_SP]
    ops["p0"], ops["p1"] = [0.0, 0.0, 0.05], [0.1, 0.1, 0.5]
    ops["noise_id"] = [11, 12, 13]
    return np.full((3, h, w, 1), 128, dtype=np.uint8), ops


def test_distribution_of_the_restatement():
    x, ops = distribution_inputs()
    out, _ = A.device_aug_reference(x, None, ops, seed=2024)
    check_distribution(out[:2, ..., 0], out[2, ..., 0], 128 / 255.0, 0.1, 0.05, 0.5)


def test_fp32_restatement_is_close_to_fp64():
    x, ops = _data(n=4, h=64, w=64)[0], np.zeros(4, dtype=A.AUG_OP_DTYPE)
    ops["kind"] = [A.AUG_GAUSSIAN, A.AUG_SPECKLE, A.AUG_SP, A.AUG_FLIP_LR]
    ops["p0"], ops["p1"], ops["noise_id"] = [0.0, 0.0, 0.05, 0], [0.1, 0.1, 0.5, 0], [1, 2, 3, 4]
    a, _ = A.device_aug_reference(x, None, ops, seed=9)
    b, _ = A.device_aug_reference(x, None, ops, seed=9, dtype=np.float32)
    assert np.abs(a[:2] - b[:2]).max() <= 1e-5 * 0.1 + 2.0 ** -23 and np.array_equal(a[2:], b[2:])
    assert a.min() >= 0 and a.max() <= 1


def test_fallbacks_keep_the_host_path():
    im, lb = _data()
    custom = [(lambda image, mask, args, desc_only=False: (image * 0.5, mask), {})]
    noise = [(A.add_noise_aug, {"mode": "gaussian"}), (A.flip_aug, {"flip_type": "up-down"})]
    cases = [(im, custom, True), (im.astype(np.float32), noise, True), (im, noise, False)]
    for images, augs, flag in cases:
        for fly in (True, False):
            A.seed(17)
            new = DataGenerator(images, lb, 3, augs, "all", (), fly, None, seed=4, device_aug=flag)
            got = [new[i] for i in range(len(new))]
            A.seed(17)
            old = DataGenerator(images, lb, 3, augs, "all", (), fly, None, seed=4)
            want = [old[i] for i in range(len(old))]
            assert not new.oct_device_aug and not old.oct_device_aug
            with pytest.raises(TypeError):
                new.next_batch_aug()
            for (x, y), (X, Y) in zip(got, want):
                assert np.array_equal(x, X) and np.array_equal(y, Y)
    # un-augmented generators keep the uint8 fast path whatever the keyword says
    g = DataGenerator(im, lb, 3, [], "none", (), False, None, seed=4, device_aug=True)
    assert g.oct_fast_path and not g.oct_device_aug


def test_training_params_carry_aug_device(tmp_path):
    from oct_image_segmentation_models_amd import optimizers
    from oct_image_segmentation_models_amd.training.training_parameters import TrainingParams
    kw = dict(model_architecture="unet", training_dataset_path=tmp_path / "d.hdf5", initial_model=None,
              results_location=tmp_path, opt_con=optimizers.Adam, loss="dice_loss_macro", metric="dice_coef_macro",
              epochs=1, batch_size=2)
    assert TrainingParams(**kw).aug_device is False and TrainingParams(aug_device=True, **kw).aug_device is True
