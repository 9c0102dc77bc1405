"""The ignore label off the GPU: ``masked_loss_reference`` against the unmasked restatements and
against a literal torch-fp64 masked loss, its defined edge cases, the public switches (``TrainingParams``, ``compile``, the
class count and the balanced weights of ``train_model``), the placement of padded labels, and the new ABI symbol in header
and binding."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 1e-7
IGN = 255


def _probs(shape, seed):
    z = np.random.default_rng(seed).normal(size=shape) * 3.0
    p = np.exp(z) / np.exp(z).sum(-1, keepdims=True)
    C = shape[-1]
    sat = np.full(C, 1e-9); sat[1] = 1.0 - (C - 1) * 1e-9       # saturated pixels: both clips of the focal / BCE terms active
    p[0, 6, 8:12] = sat
    p[0, 7, 8:12] = np.roll(sat, 1)
    return p


def _labels(shape, seed, frame=(5, 3, 4, 6)):
    """Random labels under a 255 frame (top, bottom, left, right), two ignored blobs inside; the LAST image is all 255."""
    B, H, W, C = shape
    lab = np.random.default_rng(seed).integers(0, C, (B, H, W)).astype(np.uint8)
    t, b, l, r = frame
    lab[:, :t] = IGN; lab[:, H - b:] = IGN; lab[:, :, :l] = IGN; lab[:, :, W - r:] = IGN
    lab[0, 8:12, 10:17] = IGN; lab[1 % B, 14:16, 5:9] = IGN
    lab[B - 1] = IGN
    return lab


def masked_loss_torch(lab, p, C, ignore, kind, smooth=1e-5, gamma=2.0, cw=None, w=0.5, inner_eps=True):
    """The definition written out with a mask tensor: every sum runs over the pixels whose label is not ``ignore``."""
    lab = torch.as_tensor(lab.astype(np.int64)); p = torch.as_tensor(p, dtype=torch.float64)
    m = (lab != ignore).to(torch.float64)
    y = torch.nn.functional.one_hot(torch.where(lab != ignore, lab, torch.zeros_like(lab)), C).to(torch.float64) * m[..., None]
    pm = p * m[..., None]
    I = (y * pm).sum(dim=(1, 2)); D = y.sum(dim=(1, 2)) + pm.sum(dim=(1, 2))
    macro = 1.0 - ((2.0 * I + smooth) / (D + smooth)).mean()
    micro = 1.0 - (2.0 * I.sum() + smooth) / (D.sum() + smooth)
    ph = (p > 0.5).to(torch.float64) * m[..., None]
    Ih = (y * ph).sum(dim=(1, 2)); Dh = y.sum(dim=(1, 2)) + ph.sum(dim=(1, 2))
    out = dict(dice_loss_macro=float(macro), dice_loss_micro=float(micro),
               dice_coef_macro=float(((2.0 * Ih + 1e-5) / (Dh + 1e-5)).mean()), dice_coef_micro=float(2.0 * Ih.sum() / Dh.sum()))
    n = m.sum()
    inv = 1.0 / n if n > 0 else torch.tensor(0.0, dtype=torch.float64)
    if kind == "focal":
        py = torch.clamp((p * torch.nn.functional.one_hot(torch.where(lab != ignore, lab, torch.zeros_like(lab)), C)).sum(-1), EPS, 1 - EPS)
        wt = torch.ones_like(py) if cw is None else torch.as_tensor(np.asarray(cw, np.float64))[torch.where(lab != ignore, lab, torch.zeros_like(lab))]
        term = float((m * wt * (1.0 - py) ** gamma * -torch.log(py)).sum() * inv)
        out.update(term=term, loss_macro=w * term + (1 - w) * out["dice_loss_macro"], loss_micro=w * term + (1 - w) * out["dice_loss_micro"])
    elif kind == "bce":
        e = EPS if inner_eps else 0.0
        pc = torch.clamp(p, EPS, 1 - EPS); qc = torch.clamp(1.0 - p, EPS, 1 - EPS)
        term = float((m[..., None] * -(y * torch.log(pc + e) + (1.0 - y) * torch.log(qc + e))).sum() * inv / C)
        out.update(term=term, loss_micro=term + out["dice_loss_micro"])
    return out


SHAPE = (3, 24, 40, 3)
CW = (0.5, 2.0, 1.25)


def test_without_an_ignored_pixel_it_is_the_unmasked_restatements():
    from oct_image_segmentation_models_amd.common import custom_losses as cl, custom_metrics as cm
    C = SHAPE[-1]
    p = _probs(SHAPE, 1)
    lab = np.random.default_rng(2).integers(0, C, SHAPE[:3]).astype(np.uint8)
    for ignore in (None, IGN):                                   # off, and on without a pixel of that value
        d = cl.masked_loss_reference(lab, p, C, ignore, "dice")
        assert abs(d["dice_loss_macro"] - cl.dice_loss_macro(is_y_true_sparse=True, num_classes=C)(lab, p)) < 1e-12
        assert abs(d["dice_loss_micro"] - cl.dice_loss_micro(is_y_true_sparse=True, num_classes=C)(lab, p)) < 1e-12
        assert d["loss_macro"] == d["dice_loss_macro"] and d["loss_micro"] == d["dice_loss_micro"] and d["term"] == 0.0
        assert abs(d["dice_coef_macro"] - cm.dice_coef_macro(True, C)(lab, p)) < 1e-6       # (the metrics' own sums are fp32)
        assert abs(d["dice_coef_micro"] - cm.dice_coef_micro(True, C)(lab, p)) < 1e-6
        for macro in (True, False):
            f = cl.masked_loss_reference(lab, p, C, ignore, "focal", gamma=2.0, class_weight=CW, focal_loss_weight=0.35)
            ref = cl.focal_dice_loss(num_classes=C, gamma=2.0, class_weight=CW, focal_loss_weight=0.35, dice_macro=macro)(lab, p)
            assert abs(f["loss_macro" if macro else "loss_micro"] - ref) < 1e-12
        for inner in (True, False):
            b = cl.masked_loss_reference(lab, p, C, ignore, "bce", bce_inner_eps=inner)
            assert abs(b["loss_micro"] - cl.bce_dice_loss(num_classes=C, bce_inner_eps=inner)(lab, p)) < 1e-12
            assert b["loss_macro"] is None
    with pytest.raises(ValueError, match="kind"):
        cl.masked_loss_reference(lab, p, C, None, "hinge")


@pytest.mark.parametrize("kind,kw", [("dice", {}), ("focal", dict(gamma=2.0, class_weight=CW, focal_loss_weight=0.35)),
                                     ("focal", dict(gamma=1.5)), ("bce", {}), ("bce", dict(bce_inner_eps=False))])
def test_frame_and_blobs_match_the_torch_masked_loss(kind, kw):
    from oct_image_segmentation_models_amd.common import custom_losses as cl
    C = SHAPE[-1]
    p, lab = _probs(SHAPE, 3), _labels(SHAPE, 4)
    assert (lab[-1] == IGN).all() and (lab[0] != IGN).any() and (lab[0, 8:12, 10:17] == IGN).all()
    got = cl.masked_loss_reference(lab[..., None], p, C, IGN, kind, **kw)             # (B,H,W,1) labels, as the generators hold them
    ref = masked_loss_torch(lab, p, C, IGN, kind, gamma=kw.get("gamma", 2.0), cw=kw.get("class_weight"),
                            w=kw.get("focal_loss_weight", 0.5), inner_eps=kw.get("bce_inner_eps", True))
    for k, v in ref.items():
        assert abs(got[k] - v) < 1e-12, (k, got[k], v)
    # the frame really is left out: other probabilities under it change nothing ...
    q = p.copy(); q[lab == IGN] = np.roll(q[lab == IGN], 1, axis=-1)
    assert cl.masked_loss_reference(lab, q, C, IGN, kind, **kw) == cl.masked_loss_reference(lab, p, C, IGN, kind, **kw)
    # ... whereas without the ignore label the 255 pixels count in P and Ph (an all-zero one-hot row)
    assert cl.masked_loss_reference(lab, p, C, None, kind, **kw)["dice_loss_micro"] != got["dice_loss_micro"]


@pytest.mark.parametrize("kind", ["dice", "focal", "bce"])
def test_a_batch_that_is_ignored_everywhere_has_the_defined_values(kind):
    from oct_image_segmentation_models_amd.common import custom_losses as cl
    C = SHAPE[-1]
    p = _probs(SHAPE, 5)
    lab = np.full(SHAPE[:3], IGN, np.uint8)
    d = cl.masked_loss_reference(lab, p, C, IGN, kind)
    assert d["dice_loss_macro"] == 0.0 and d["dice_loss_micro"] == 0.0 and d["term"] == 0.0 and d["loss_micro"] == 0.0
    assert d["loss_macro"] in (0.0, None)
    assert d["dice_coef_macro"] == 1.0 and np.isnan(d["dice_coef_micro"])
    # one image ignored everywhere: its per-class macro scores are s / s = 1
    lab2 = _labels(SHAPE, 6)
    one = cl.masked_loss_reference(lab2[-1:], p[-1:], C, IGN, "dice")
    assert one["dice_loss_macro"] == 0.0
    rest = cl.masked_loss_reference(lab2[:-1], p[:-1], C, IGN, "dice")
    both = cl.masked_loss_reference(lab2, p, C, IGN, "dice")
    B = SHAPE[0]
    assert abs((1.0 - both["dice_loss_macro"]) - ((B - 1) * (1.0 - rest["dice_loss_macro"]) + 1.0) / B) < 1e-12


def _params(**kw):
    from oct_image_segmentation_models_amd import optimizers
    from oct_image_segmentation_models_amd.training.training_parameters import TrainingParams
    return TrainingParams(model_architecture="unet", training_dataset_path="data.hdf5", initial_model=None, results_location="results",
                          opt_con=optimizers.Adam, loss="dice_loss_macro", metric="dice_coef_macro", epochs=1, batch_size=2, **kw)


def test_training_params_carry_the_three_switches():
    tp = _params()
    assert (tp.pad_mode, tp.pad_value, tp.ignore_label) == (None, 0, None)
    tp = _params(pad_mode="reflect", pad_value=7, ignore_label=200)
    assert (tp.pad_mode, tp.pad_value, tp.ignore_label) == ("reflect", 7, 200)


def test_class_count_and_balanced_weights_skip_the_ignore_label():
    from oct_image_segmentation_models_amd.training.training import _balanced_class_weight, _count_classes
    lab = np.array([0, 0, 0, 1, 2, 2, 255, 255, 255, 255], np.uint8).reshape(1, 2, 5, 1)
    assert _count_classes(lab) == 4 and _count_classes(lab, 255) == 3
    assert _count_classes(lab, 200) == 4                          # a value that does not occur takes nothing away
    w = _balanced_class_weight(lab, 255)
    assert np.allclose(w, 6.0 / (3 * np.array([3.0, 1.0, 2.0])))
    assert np.array_equal(_balanced_class_weight(lab[lab != 255]), w)
    assert len(_balanced_class_weight(lab)) == 4                  # unchanged without it


def test_compile_validates_and_keeps_the_ignore_label():
    from oct_image_segmentation_models_amd._hip import OctError
    from oct_image_segmentation_models_amd.models.engine_model import Model
    m = Model("unet", dict(input_channels=1, num_classes=3, image_height=16, image_width=32))
    assert m.ignore_label is None and m.pad_mode is None
    m.compile(ignore_label=255); assert m.ignore_label == 255
    m.compile(ignore_label=3); assert m.ignore_label == 3
    m.compile(); assert m.ignore_label is None
    for bad in (2, 0, -1, 256, 3.5):
        with pytest.raises(OctError, match="ignore_label"):
            m.compile(ignore_label=bad)
    # padded training is chosen at compile time; the attributes alone (inference) do not switch it on
    assert m._pad_fit is False
    m.pad_mode = "edge"; m.compile(); assert m._pad_fit is False and m.pad_mode == "edge"
    m.compile(pad_mode="constant", pad_value=7); assert m._pad_fit and (m.pad_mode, m.pad_value) == ("constant", 7.0)
    m.compile(); assert m._pad_fit is False and m.pad_mode == "constant"
    with pytest.raises(OctError, match="pad_mode"):
        m.compile(pad_mode="mirror")


class _HostEngine:
    """What ``Model._pad_batch`` needs of an engine, on host tensors: the geometry and ``pad`` (= its numpy restatement)."""

    def __init__(self, H, W):
        self.cfg = SimpleNamespace(H=H, W=W)
        self.calls, self._pad_bufs = [], {}

    def pad(self, x, Hp, Wp, top, left, mode, value=0, out=None):
        from oct_image_segmentation_models_amd.common.utils import pad_reference
        self.calls.append((tuple(x.shape), str(x.dtype), Hp, Wp, top, left, mode, value))
        out.copy_(torch.from_numpy(pad_reference(x.numpy(), Hp, Wp, top, left, mode, value)))
        return out


@pytest.mark.parametrize("labels_4d", [True, False])
def test_labels_are_placed_where_the_images_are(labels_4d):
    from oct_image_segmentation_models_amd.common.utils import pad_reference, padded_geometry
    from oct_image_segmentation_models_amd.models.engine_model import Model
    m = Model("unet", dict(input_channels=1, num_classes=3, image_height=32, image_width=64, pool_layers=3))
    geom, at = m._geometry((36, 68), "edge")
    assert (geom + at) == padded_geometry(36, 68, 3) == (40, 72, 2, 2)
    rng = np.random.default_rng(0)
    x = rng.random((2, 36, 68, 1)).astype(np.float32)
    lab = rng.integers(0, 3, (2, 36, 68, 1) if labels_4d else (2, 36, 68)).astype(np.uint8)
    eng = _HostEngine(*geom)
    xp, lp = m._pad_batch(eng, torch.from_numpy(x), torch.from_numpy(lab), at, "edge", 0.0, 255)
    assert np.array_equal(xp.numpy(), pad_reference(x, 40, 72, 2, 2, "edge"))
    lp_t, lp = lp, lp.numpy()
    assert lp.shape == (2, 40, 72, 1) and np.array_equal(lp[:, 2:38, 2:70, 0], lab.reshape(2, 36, 68))
    frame = np.ones((40, 72), bool); frame[2:38, 2:70] = False
    assert (lp[:, frame] == 255).all() and frame.sum() == 40 * 72 - 36 * 68
    assert eng.calls[1][2:] == (40, 72, 2, 2, "constant", 255)    # same placement, byte-generic kernel, constant mode
    # the pair belongs to the engine and is made once per batch size
    xp2, lp2 = m._pad_batch(eng, torch.from_numpy(x), torch.from_numpy(lab), at, "edge", 0.0, 255)
    assert xp2 is xp and lp2 is lp_t
    assert len(eng._pad_bufs) == 1
    m._pad_batch(eng, torch.from_numpy(x[:1]), torch.from_numpy(lab[:1]), at, "edge", 0.0, 255)
    assert len(eng._pad_bufs) == 2


def test_header_and_binding_declare_the_new_symbol():
    from oct_image_segmentation_models_amd import _hip
    hdr = open(os.path.join(ROOT, "include", "oct_unet.h")).read()
    bound = {s[0]: s for s in _hip.SYMBOLS}
    m = re.search(r"\bint\s+oct_unet_set_ignore_label\s*\(([^)]*)\)\s*;", hdr)
    assert m, "oct_unet_set_ignore_label not declared in include/oct_unet.h"
    assert len(m.group(1).split(",")) == 2
    assert "oct_unet_set_ignore_label" in bound and len(bound["oct_unet_set_ignore_label"][2]) == 2
    from oct_image_segmentation_models_amd.engine import UNetEngine
    assert callable(getattr(UNetEngine, "set_ignore_label", None))
