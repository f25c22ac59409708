#!/usr/bin/env python3
"""Time the l1 loss kernels against their l2 neighbours (the same bytes over the same plan).  GPU box.

One process, device events around every launch, warm-up first, the kernels ALTERNATING launch by launch (swv2_score_sums without
climatology, swv2_l1_sums, swv2_loss_grad, swv2_l1_grad, swv2_l1_finalize), --launches each per repeat, the whole measurement --repeats
times for the spread.  At B * C = 146 planes of 720 x 1440 (two samples of the 73-variable model).  Writes a JSON report (default
profiles/l1_probe.json) and prints one line for LABNOTES.md.

Bytes come from the shapes: 2 B C H W 4 read by the two sums kernels, 3 B C H W 4 moved by the two gradient kernels (prediction and
target read, the gradient written).  TB/s are those bytes over the median time.  `ratio` is the l1 kernel's median over its l2
neighbour's in the same repeat; the expectation is within 10 % (same bytes, same plan)."""
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "l1_probe.json"))
a = ap.parse_args()
assert torch.cuda.is_available(), "the probe measures on an MI355X: no GPU, no number"
dev = torch.device("cuda:0")
B, C, H, W = a.batch, a.channels, 720, 1440
g = torch.Generator(device=dev).manual_seed(0)
prd, tar = torch.randn(B, C, H, W, device=dev, generator=g), torch.randn(B, C, H, W, device=dev, generator=g)
from swin_v2_weather_amd.utils.grids import naive_quadrature_weights
w = naive_quadrature_weights(H, W, True).to(dev)
coef = torch.rand(B, C, device=dev, generator=g) + 0.5
dprd = torch.empty_like(prd)
ws_score, ws_l1 = ops.score_workspace(B * C, H, W, dev), ops.l1_workspace(B * C, H, W, dev)
chw = torch.full((C,), 1.0 / C, device=dev)
kernels = {
    "score_sums": lambda: ops.score_sums(prd, tar, w, ws_score),
    "l1_sums": lambda: ops.l1_sums(prd, tar, w, ws_l1),
    "loss_grad": lambda: ops.loss_grad(prd, tar, w, coef, dprd),
    "l1_grad": lambda: ops.l1_grad(prd, tar, w, coef, dprd),
    "l1_finalize": lambda: ops.l1_finalize(ws_l1, B, C, H, W, chw, False),
}
neighbour = {"l1_sums": "score_sums", "l1_grad": "loss_grad"}
plane_bytes = B * C * H * W * 4
nbytes = {"score_sums": 2 * plane_bytes, "l1_sums": 2 * plane_bytes, "loss_grad": 3 * plane_bytes, "l1_grad": 3 * plane_bytes,
          "l1_finalize": ws_l1.numel() * 4}
for _ in range(a.warmup):
    for f in kernels.values():
        f()
torch.cuda.synchronize()
report = {"shape": [B, C, H, W], "slices": ops.score_slices(B * C, H, W), "launches": a.launches, "device": torch.cuda.get_device_name(0),
          "source_hash": L.source_hash(), "bytes": nbytes, "repeats": []}
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
                  "tb_per_s_median": nbytes[k] / statistics.median(us) / 1e6}
    for k, nb in neighbour.items():
        rep[k]["ratio_to_" + nb] = rep[k]["median_us"] / rep[nb]["median_us"]
    report["repeats"].append(rep)
summary = {k: {"median_us": [rep[k]["median_us"] for rep in report["repeats"]], "tb_per_s": [rep[k]["tb_per_s_median"] for rep in report["repeats"]]}
           for k in kernels}
for k, nb in neighbour.items():
    summary[k]["ratio_to_" + nb] = [rep[k]["ratio_to_" + nb] for rep in report["repeats"]]
report["summary"] = summary
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    json.dump(report, f, indent=1)
fmt = lambda k: "/".join(f"{v:.1f}" for v in summary[k]["median_us"]) + " us (" + "/".join(f"{v:.2f}" for v in summary[k]["tb_per_s"]) + " TB/s)"
rat = lambda k, nb: "/".join(f"{v:.3f}" for v in summary[k]["ratio_to_" + nb])
print(f"LABNOTES: l1 probe B*C={B * C} 720x1440, {a.launches} launches x {a.repeats} repeats, medians: score_sums {fmt('score_sums')}; "
      f"l1_sums {fmt('l1_sums')} = {rat('l1_sums', 'score_sums')} of it; loss_grad {fmt('loss_grad')}; l1_grad {fmt('l1_grad')} = "
      f"{rat('l1_grad', 'loss_grad')} of it; l1_finalize " + "/".join(f"{v:.1f}" for v in summary['l1_finalize']['median_us']) + " us")
