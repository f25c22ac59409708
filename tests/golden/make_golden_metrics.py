"""Generate tests/golden/metrics.npz: seeded inputs and the outputs of the REAL reference's torch metrics
(utils/weighted_acc_rmse.py: weighted_rmse_torch_channels, weighted_rmse_torch, weighted_acc_torch_channels, weighted_acc_torch,
unweighted_acc_torch_channels, unweighted_acc_torch) on the CPU.

    python tests/golden/make_golden_metrics.py PATH/TO/reference

The reference file is imported by path at generation time only; the fixture is data (fp32 arrays, a few KB) and nothing of the
reference's text enters this repository.  The tests read the .npz and never need the reference.
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = ("weighted_rmse_torch_channels", "weighted_rmse_torch", "weighted_acc_torch_channels", "weighted_acc_torch",
         "unweighted_acc_torch_channels", "unweighted_acc_torch")


def main(ref_root):
    spec = importlib.util.spec_from_file_location("ref_weighted_acc_rmse", os.path.join(ref_root, "utils", "weighted_acc_rmse.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    g = torch.Generator().manual_seed(20240607)
    shape = (2, 3, 9, 16)
    # a smooth "climatology" plus N(0, 1): the anomalies correlate, so ACC is neither 0 nor 1
    base = torch.randn(shape, generator=g)
    pred = (base + 0.5 * torch.randn(shape, generator=g)).float()
    target = (base + 0.5 * torch.randn(shape, generator=g)).float()
    out = {"pred": pred.numpy(), "target": target.numpy()}
    for n in NAMES:
        out[n] = getattr(ref, n)(pred, target).numpy()
    # the reference's own row weights, as its functions form them (the test pins latitude_weights to these bit for bit)
    j = torch.arange(start=0, end=shape[2])
    s = torch.sum(torch.cos(3.1416 / 180. * ref.lat(j, shape[2])))
    out["weights"] = ref.latitude_weighting_factor_torch(j, shape[2], s).numpy()
    np.savez(os.path.join(HERE, "metrics.npz"), **out)
    for k, v in out.items():
        print(k, v.shape, v.dtype)


if __name__ == "__main__":
    main(sys.argv[1])
