"""bce_dice_loss off the GPU: the registry factory against a literal torch-fp64 restatement of the definition
(DESIGN.md section 11), the two new ABI symbols in header and binding, and the register guard of the four head-kernel
instantiations the benched configurations run (the BCE branch shares those kernels: it must not make them spill)."""
import glob
import os
import re
import sys
import tempfile

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

EPS = 1e-7


def bce_dice_torch(y, p, inner_eps=True):
    """keras.losses.binary_crossentropy(y, p) + dice_loss_micro(y, p) written out: mean over the class axis, then
    SUM_OVER_BATCH_SIZE over (B, H, W)."""
    y = torch.as_tensor(y, dtype=torch.float64); p = torch.as_tensor(p, dtype=torch.float64)
    e = EPS if inner_eps else 0.0
    pc = torch.clamp(p, EPS, 1.0 - EPS); qc = torch.clamp(1.0 - p, EPS, 1.0 - EPS)
    bce = -(y * torch.log(pc + e) + (1.0 - y) * torch.log(qc + e))
    per_px = bce.mean(dim=-1)
    bce_mean = per_px.sum() / per_px.numel()
    yf, pf = y.reshape(-1), p.reshape(-1)
    dice = 1.0 - (2.0 * (yf * pf).sum() + 1e-5) / (yf.sum() + pf.sum() + 1e-5)
    return float(bce_mean + dice)


@pytest.mark.parametrize("shape", [(2, 8, 16, 3), (1, 8, 16, 8)])
def test_factory_matches_the_definition(shape):
    from oct_image_segmentation_models_amd.common import custom_losses as cl
    entry = cl.custom_loss_objects["bce_dice_loss"]
    assert entry["takes_sparse"] is False
    C = shape[-1]
    fn = entry["function"](num_classes=C, is_y_true_sparse=False)          # as training.train_model calls it
    assert fn.oct_loss == "bce_dice_loss"
    rng = np.random.default_rng(shape[-1])
    z = rng.normal(size=shape) * 3.0
    p = np.exp(z) / np.exp(z).sum(-1, keepdims=True)
    # saturated pixels: one class above 1 - eps, the others below eps (both clips active)
    sat = np.full(C, 1e-9); sat[1] = 1.0 - (C - 1) * 1e-9
    p[0, 0, :5] = sat
    p[0, 1, :5] = np.roll(sat, 1)
    assert (p < EPS).any() and (p > 1.0 - EPS).any()
    lab = rng.integers(0, C, shape[:3] + (1,)).astype(np.uint8)
    lab[0, 0, :5, 0] = [1, 0, 1, 2, 1]                                     # saturated towards the right and the wrong class
    y = np.eye(C)[lab[..., 0]]
    ref = bce_dice_torch(y, p)
    assert abs(fn(y, p) - ref) < 1e-12                                     # dense one-hot, as the reference feeds it
    assert abs(fn(lab, p) - ref) < 1e-12 and abs(fn(lab[..., 0], p) - ref) < 1e-12     # sparse labels
    fn0 = entry["function"](num_classes=C, is_y_true_sparse=False, bce_inner_eps=False)
    ref0 = bce_dice_torch(y, p, inner_eps=False)
    assert abs(fn0(y, p) - ref0) < 1e-12 and ref0 != ref


def test_the_other_two_registry_names_still_raise():
    from oct_image_segmentation_models_amd.common import custom_losses as cl
    with pytest.raises(NotImplementedError, match="cannot be called through the registry"):
        cl.custom_loss_objects["bce_focal_loss"]["function"](num_classes=3, is_y_true_sparse=False)
    with pytest.raises(NotImplementedError):
        cl.custom_loss_objects["focal_loss"]["function"](num_classes=3, is_y_true_sparse=True)


def test_compile_accepts_the_tag():
    from oct_image_segmentation_models_amd.common import custom_losses as cl
    from oct_image_segmentation_models_amd.models.engine_model import Model
    m = Model("unet", dict(input_channels=1, num_classes=3, image_height=16, image_width=32))
    m.compile(loss=cl.custom_loss_objects["bce_dice_loss"]["function"](num_classes=3, is_y_true_sparse=False))
    assert m._loss_name == "bce_dice_loss" and m._focal is None


def test_header_and_binding_declare_the_new_symbols():
    from oct_image_segmentation_models_amd import _hip
    hdr = open(os.path.join(ROOT, "include", "oct_unet.h")).read()
    bound = {s[0]: s for s in _hip.SYMBOLS}
    for name, nargs in (("oct_unet_set_bce_dice", 2), ("oct_unet_loss_bce_dice", 4)):
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, hdr)
        assert m, f"{name} not declared in include/oct_unet.h"
        assert len(m.group(1).split(",")) == nargs
        assert name in bound and len(bound[name][2]) == nargs
    assert '"bce_inner_eps"' in hdr


HEAD_HOT = [   # the head kernels of configs[1] (fp32) and of the bf16 configurations: 3 classes, start_neurons 8
    "head_fwd_k<3, 8, float>", "head_fwd_k<3, 8, unsigned short>",
    "head_bwd_k<3, 8, float>", "head_bwd_k<3, 8, unsigned short>",
]


def test_benched_head_instantiations_do_not_spill():
    import kernel_resources as kr
    objs = sorted(glob.glob(os.path.join(ROOT, "oct-image-segmentation-models_amd", "csrc", "build", "*.o")))
    if not objs:
        pytest.skip("csrc/build/*.o not present (run __graft_entry__.build())")
    found = {}
    with tempfile.TemporaryDirectory() as tmp:
        for o in objs:
            co = kr.code_objects(o, tmp)
            if not co:
                continue
            for k in kr.kernels(co):
                for h in HEAD_HOT:
                    if h in k["name"]:
                        found[h] = k
    if not found:
        pytest.skip("no gfx950 code objects could be read from csrc/build/*.o (llvm tools missing?)")
    missing = [h for h in HEAD_HOT if h not in found]
    assert not missing, f"instantiations not found in the build: {missing}"
    spilled = {h: (k["spill"], k["scratch"]) for h, k in found.items() if k["spill"] not in ("0", 0)}
    assert not spilled, f"register spills in the benched head kernels (vgpr_spill_count, scratch bytes): {spilled}"
