#!/usr/bin/env python3
"""Generate the l1 loss fixtures under tests/golden/ by importing the REAL reference on CPU, as make_golden.py does for the l2 strings
(run in the build container only, where the reference exists; `ref_shims.py` provides the missing third-party imports):

    python tests/golden/make_golden_l1.py

Writes loss_l1_values.json and loss_l1_aux.npz with the layout of loss_values.json / loss_aux.npz: H, W, C = 24, 48, 73, the channel
names and the statistics arrays of the l2 fixture, seeded randn prediction / target (seed 1 + n_future, the SAME fields for every
string, so that strings the reference treats alike give the same number), the reference's value and the gradient subsample
[:, ::9, ::5, ::7].  Every string with n_future in {0, 1}, train and eval; eval with n_future = 1 raises in the reference itself (chw
[1, C] against norms [B, 2 C]) and is recorded as such.  p = 1 with the 'naive' rule needs nothing from torch_harmonics.
"""
import json
import os
import sys
import tempfile
from types import SimpleNamespace

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import ref_shims  # noqa: E402

_, _, ls = ref_shims.import_reference()
assert ls is not None, "reference losses failed to import"

LOSSES = ["l1", "geometric l1", "squared geometric l1", "absolute l1", "weighted absolute temp-std geometric l1",
          "weighted relative temp-std squared geometric l1"]
CHANNEL_NAMES = (["u10m", "v10m", "u100m", "v100m", "t2m", "sp", "msl", "tcwv"] +
                 [f"{v}{l}" for v in "uvztq" for l in (50, 100, 150, 200, 250, 300, 400, 500, 600, 700, 850, 925, 1000)])


def main():
    torch.set_num_threads(8)
    H, W, C = 24, 48, 73
    l2 = np.load(os.path.join(HERE, "loss_aux.npz"))
    arrs = {"global_stds": l2["global_stds"], "time_diff_stds": l2["time_diff_stds"]}
    tmp = tempfile.mkdtemp()
    np.save(tmp + "/gs.npy", arrs["global_stds"])
    np.save(tmp + "/td.npy", arrs["time_diff_stds"])
    res = {}
    for li, loss in enumerate(LOSSES):
        for nf in (0, 1):
            params = SimpleNamespace(n_future=nf, img_shape_x=H, img_shape_y=W, loss=loss, channel_weights="auto", n_out_channels=C,
                                     channel_names=CHANNEL_NAMES, out_channels=np.arange(C), global_stds_path=tmp + "/gs.npy",
                                     time_diff_stds_path=tmp + "/td.npy", dt=1, model_grid_type="equiangular")
            lh = ls.LossHandler(params)
            seed = 1 + nf
            torch.manual_seed(seed)
            prd = torch.randn(2, C * (nf + 1), H, W, requires_grad=True)
            tar = torch.randn(2, C * (nf + 1), H, W)
            for mode in ("train", "eval"):
                lh.train(mode == "train")
                key = f"{li}_{nf}_{mode}"
                case = {"loss": loss, "n_future": nf, "mode": mode, "seed": seed}
                try:
                    val = lh(prd, tar, None)
                except RuntimeError as e:
                    case["raises"] = True
                    print(f"loss['{loss}', nf={nf}, {mode}] raises in the reference: {str(e).splitlines()[0]}")
                    res[key] = case
                    continue
                case["value"] = float(val)
                print(f"loss['{loss}', nf={nf}, {mode}] ref {float(val):.7f}")
                prd.grad = None
                val.backward()
                g = prd.grad.numpy().astype(np.float32)
                case["grad_zeros"] = int((g == 0).sum())
                arrs[f"gprd_{key}"] = g[:, ::9, ::5, ::7]
                res[key] = case
    with open(os.path.join(HERE, "loss_l1_values.json"), "w") as f:
        json.dump({"H": H, "W": W, "C": C, "cases": res}, f, indent=1)
    path = os.path.join(HERE, "loss_l1_aux.npz")
    np.savez_compressed(path, **arrs)
    print(f"wrote loss_l1_values.json and loss_l1_aux.npz ({os.path.getsize(path) / 1024:.0f} KB)")


if __name__ == "__main__":
    main()
