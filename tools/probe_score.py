#!/usr/bin/env python3
"""Time swv2_score_sums against swv2_loss_sums (the same read stream over prediction and truth; its two launches, sums and fold, timed as one).  GPU box.

One process, device events around every launch, warm-up first, the kernels ALTERNATING launch by launch (loss_sums, score_sums without
climatology, score_sums with climatology, swv2_score_finalize), --launches each per repeat, the whole measurement --repeats times for
the spread.  At B * C = 146 planes of 720 x 1440 (two samples of the 73-variable model).  Writes a JSON report (default
profiles/score_probe.json) and prints one line for LABNOTES.md.

Bytes come from the shapes.  TB/s are UNIQUE bytes over the median time: 2 B C H W 4 for loss_sums and score_sums without climatology,
(2 B + 1) C H W 4 with it (the climatology is one [C, H, W] array shared by the B samples).  The algorithm's reads, 3 B C H W 4 with the
climatology counted once per sample, are reported beside them as `algorithmic_*`: they are not memory traffic."""
import argparse, json, os, statistics, sys
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
from swin_v2_weather_amd import _lib as L, ops

ap = argparse.ArgumentParser()
ap.add_argument("--launches", type=int, default=200)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--warmup", type=int, default=20)
ap.add_argument("--batch", type=int, default=2)
ap.add_argument("--channels", type=int, default=73)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "score_probe.json"))
a = ap.parse_args()
assert torch.cuda.is_available(), "the probe measures on an MI355X: no GPU, no number"
dev = torch.device("cuda:0")
B, C, H, W = a.batch, a.channels, 720, 1440
g = torch.Generator(device=dev).manual_seed(0)
prd, tar = torch.randn(B, C, H, W, device=dev, generator=g), torch.randn(B, C, H, W, device=dev, generator=g)
clim = torch.randn(C, H, W, device=dev, generator=g)
from swin_v2_weather_amd.utils.weighted_acc_rmse import latitude_weights
w = latitude_weights(H, dev)
loss_out = torch.empty(B, C, 2, device=dev)
ws, loss_ws = ops.score_workspace(B * C, H, W, dev), ops.loss_workspace(B * C, H, W, dev)
kernels = {
    "loss_sums": lambda: ops.loss_sums(prd, tar, w, loss_out, loss_ws),
    "score_sums": lambda: ops.score_sums(prd, tar, w, ws),
    "score_sums_clim": lambda: ops.score_sums(prd, tar, w, ws, clim),
    "score_finalize": lambda: ops.score_finalize(ws, B, C, H, W),
}
plane_bytes = B * C * H * W * 4
algo_bytes = {"loss_sums": 2 * plane_bytes, "score_sums": 2 * plane_bytes, "score_sums_clim": 3 * plane_bytes, "score_finalize": ws.numel() * 4}
# bytes that have to come from memory at least once: the climatology is one [C, H, W] array, whichever sample reads it
unique_bytes = dict(algo_bytes, score_sums_clim=2 * plane_bytes + C * H * W * 4)
for _ in range(a.warmup):
    for f in kernels.values():
        f()
torch.cuda.synchronize()
report = {"shape": [B, C, H, W], "slices": ops.score_slices(B * C, H, W), "launches": a.launches, "device": torch.cuda.get_device_name(0),
          "source_hash": L.source_hash(), "algorithmic_bytes": algo_bytes, "unique_bytes": unique_bytes, "repeats": []}
for r in range(a.repeats):
    ev = {k: [] for k in kernels}
    for _ in range(a.launches):
        for k, f in kernels.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); f(); e1.record()
            ev[k].append((e0, e1))
    torch.cuda.synchronize()
    rep = {}
    for k, pairs in ev.items():
        us = [e0.elapsed_time(e1) * 1e3 for e0, e1 in pairs]
        rep[k] = {"median_us": statistics.median(us), "mean_us": statistics.fmean(us), "min_us": min(us),
                  "tb_per_s_median": unique_bytes[k] / statistics.median(us) / 1e6,
                  "algorithmic_tb_per_s_median": algo_bytes[k] / statistics.median(us) / 1e6}
    report["repeats"].append(rep)
summary = {k: {"median_us": [rep[k]["median_us"] for rep in report["repeats"]], "tb_per_s": [rep[k]["tb_per_s_median"] for rep in report["repeats"]]}
           for k in kernels}
report["summary"] = summary
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    json.dump(report, f, indent=1)
fmt = lambda k: "/".join(f"{v:.1f}" for v in summary[k]["median_us"]) + " us (" + "/".join(f"{v:.2f}" for v in summary[k]["tb_per_s"]) + " TB/s)"
print(f"LABNOTES: score probe B*C={B * C} 720x1440, {a.launches} launches x {a.repeats} repeats, medians: loss_sums {fmt('loss_sums')}; "
      f"score_sums {fmt('score_sums')}; with clim {fmt('score_sums_clim')}; finalize " + "/".join(f"{v:.1f}" for v in summary['score_finalize']['median_us']) + " us")
