"""Generate tests/golden/quantiles.npz: seeded inputs and the outputs of the REAL reference's extremes metric
(utils/weighted_acc_rmse.py: top_quantiles_error_torch on [n, c, h, w], the numpy top_quantiles_error on pred[0], target[0]) on the CPU.

    python tests/golden/make_golden_quantiles.py PATH/TO/reference

The reference file is imported by path at generation time only; the fixture is data (arrays, a few KB) and nothing of the
reference's text enters this repository.  The tests read the .npz and never need the reference.
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))


def main(ref_root):
    spec = importlib.util.spec_from_file_location("ref_weighted_acc_rmse", os.path.join(ref_root, "utils", "weighted_acc_rmse.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    g = torch.Generator().manual_seed(20241019)
    shape = (2, 3, 9, 16)
    # the prediction is a damped truth plus noise: its upper quantiles sit below the truth's, so the error is clearly negative
    target = torch.randn(shape, generator=g).float()
    pred = (0.8 * target + 0.3 * torch.randn(shape, generator=g)).float()
    out = {"pred": pred.numpy(), "target": target.numpy(),
           "top_quantiles_error_torch": ref.top_quantiles_error_torch(pred, target).numpy(),
           "top_quantiles_error": ref.top_quantiles_error(pred[0].numpy(), target[0].numpy()),
           # the levels as the reference forms them
           "levels": (1. - torch.logspace(-3, -0.1, steps=100)).numpy()}
    np.savez(os.path.join(HERE, "quantiles.npz"), **out)
    for k, v in out.items():
        print(k, v.shape, v.dtype)


if __name__ == "__main__":
    main(sys.argv[1])
