#!/usr/bin/env python3
"""20 training steps at the default configuration (256x512, 487 403 parameters) per optimizer kind, to be run under
`rocprofv3 --kernel-trace --stats` (a run of its own, no counters): the per-launch times of adam_k / sgd_k, of every opt_k
instantiation and of the two norm kernels end up in the trace's kernel_stats.csv.
Usage: rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python3 tools/profile_optimizers.py [WHICH]
  kinds (default): every kind and flag combination, unclipped (plain Adam / SGD through oct_adam_step / oct_sgd_step)
  clipnorm | global_clipnorm | clipvalue: RMSprop(momentum=0.9) with that option (the norm kernels carry one name in both
  norm modes: one run per mode keeps their times apart)"""
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from oct_image_segmentation_models_amd import optimizers as O  # noqa: E402
from oct_image_segmentation_models_amd.common.synthetic import make_scans  # noqa: E402
from oct_image_segmentation_models_amd.engine import UNetEngine  # noqa: E402

KINDS = [O.Adam(), O.SGD(momentum=0.9), O.SGD(), O.SGD(momentum=0.9, nesterov=True), O.SGD(decay=1e-4), O.Adam(amsgrad=True),
         O.Adam(decay=1e-4), O.Adamax(), O.RMSprop(), O.RMSprop(momentum=0.9), O.RMSprop(centered=True),
         O.RMSprop(momentum=0.9, centered=True), O.Adagrad(), O.Adadelta()]


def main():
    which = sys.argv[1] if len(sys.argv) > 1 else "kinds"
    B, H, W, C = 2, 256, 512, 3
    eng = UNetEngine(device="cuda:0", input_channels=1, num_classes=C, image_height=H, image_width=W, max_batch=B,
                     training=True, seed=1)
    assert eng.n_params == 487403
    images, labels = make_scans(B, H, W, C, seed=3)
    x = torch.from_numpy(images).cuda()
    lab = torch.from_numpy(labels[..., 0].copy()).cuda()
    for opt in (KINDS if which == "kinds" else [O.RMSprop(momentum=0.9, **{which: 0.01})]):
        for _ in range(20):
            eng.forward(x, training=True, labels=lab, want_probs=False)
            eng.loss_dice()
            eng.backward(lab)
            opt.apply(eng)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(eng.params).all()), type(opt).__name__
        print(type(opt).__name__, opt.get_config(), "ok", flush=True)


if __name__ == "__main__":
    main()
