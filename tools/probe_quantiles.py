#!/usr/bin/env python3
"""Time the extremes metric on the HIP radix select against torch.quantile on the same device tensors.  GPU box.

One process, device events around every call, warm-up first, the contenders ALTERNATING call by call, --launches each per repeat, the
whole measurement --repeats times for the spread.  At B * C = 146 planes of 720 x 1440 (two samples of the 73-variable model), on three
inputs: N(0, 1) fields, fields that are 98 % exact zeros (precipitation-like: heavy ties), constant fields (every element in one counter
at every level).  Contenders, all returning the [B, C] error of prediction against truth:

    kernels   utils.weighted_acc_rmse.top_quantiles_error_torch: the stateless call (ranks built on the CPU, a fresh workspace, twice
              swv2_plane_order_stats = 2 x (memset + 5 count + 5 resolve launches), gather + lerp + mean in torch)
    scorer    ForecastScorer.quantile_error: the same with the ranks and the workspace made once
    torch     the reference's formula: torch.quantile(x.view(n, c, h w), q, dim=-1) for both operands, mean of the difference

Writes a JSON report (default profiles/quantile_probe.json) and prints one line for LABNOTES.md.  GB/s are the bytes of both operands
read once (2 B C H W 4) over the median time: the select reads them five times, so its memory rate is five times that figure."""
import argparse, json, os, statistics, sys
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
from swin_v2_weather_amd import _lib as L
from swin_v2_weather_amd.utils import weighted_acc_rmse as M

ap = argparse.ArgumentParser()
ap.add_argument("--launches", type=int, default=10)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--batch", type=int, default=2)
ap.add_argument("--channels", type=int, default=73)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "quantile_probe.json"))
a = ap.parse_args()
assert torch.cuda.is_available(), "the probe measures on an MI355X: no GPU, no number"
dev = torch.device("cuda:0")
B, C, H, W = a.batch, a.channels, 720, 1440
g = torch.Generator(device=dev).manual_seed(0)


def make(kind):
    if kind == "normal":
        return torch.randn(B, C, H, W, device=dev, generator=g)
    if kind == "zeros98":
        u = torch.rand(B, C, H, W, device=dev, generator=g)
        return torch.where(u < 0.98, torch.zeros_like(u), 50.0 * (u - 0.98))
    return torch.full((B, C, H, W), 1.5, device=dev)


def torch_quantile_error(pred, target):
    q = M.quantile_levels().to(pred.device)
    n, c, h, w = pred.shape
    return torch.mean(torch.quantile(pred.view(n, c, h * w), q, dim=-1) - torch.quantile(target.view(n, c, h * w), q, dim=-1), dim=0)


scorer = M.ForecastScorer(H, W, C, dev)
contenders = {"kernels": M.top_quantiles_error_torch, "scorer": scorer.quantile_error, "torch": torch_quantile_error}
report = {"shape": [B, C, H, W], "launches": a.launches, "device": torch.cuda.get_device_name(0), "source_hash": L.source_hash(),
          "ranks": int(M.quantile_ranks(H * W, M.quantile_levels())[0].numel()), "operand_bytes": 2 * B * C * H * W * 4, "inputs": {}}
for kind in ("normal", "zeros98", "constant"):
    pred, target = make(kind), make(kind)
    assert M._quantiles_on_kernels(pred)
    results = {k: f(pred, target) for k, f in contenders.items()}
    for _ in range(a.warmup):
        for f in contenders.values():
            f(pred, target)
    torch.cuda.synchronize()
    entry = {"max_abs_difference_kernels_vs_torch": float((results["kernels"] - results["torch"]).abs().max()),
             "scorer_equals_kernels": bool(torch.equal(results["kernels"], results["scorer"])), "repeats": []}
    for r in range(a.repeats):
        ev = {k: [] for k in contenders}
        for _ in range(a.launches):
            for k, f in contenders.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(); f(pred, target); e1.record()
                ev[k].append((e0, e1))
        torch.cuda.synchronize()
        rep = {}
        for k, pairs in ev.items():
            us = [e0.elapsed_time(e1) * 1e3 for e0, e1 in pairs]
            rep[k] = {"median_us": statistics.median(us), "mean_us": statistics.fmean(us), "min_us": min(us), "max_us": max(us),
                      "operand_gb_per_s_median": report["operand_bytes"] / statistics.median(us) / 1e3}
        entry["repeats"].append(rep)
    entry["median_us"] = {k: [rep[k]["median_us"] for rep in entry["repeats"]] for k in contenders}
    entry["torch_over_kernels"] = [rep["torch"]["median_us"] / rep["kernels"]["median_us"] for rep in entry["repeats"]]
    entry["torch_over_scorer"] = [rep["torch"]["median_us"] / rep["scorer"]["median_us"] for rep in entry["repeats"]]
    report["inputs"][kind] = entry
    print(f"{kind}: median us {entry['median_us']}", file=sys.stderr, flush=True)
    del pred, target, results
    torch.cuda.empty_cache()
base = statistics.median(report["inputs"]["normal"]["median_us"]["kernels"])
for kind, entry in report["inputs"].items():
    entry["kernels_time_over_normal"] = statistics.median(entry["median_us"]["kernels"]) / base
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    json.dump(report, f, indent=1)
fmt = lambda v: "/".join(f"{x:.0f}" for x in v)
print(f"LABNOTES: quantile probe B*C={B * C} 720x1440, {report['ranks']} ranks, {a.launches} calls x {a.repeats} repeats, median us "
      "(kernels; scorer; torch.quantile; torch / kernels): " +
      "; ".join(f"{kind} {fmt(e['median_us']['kernels'])}; {fmt(e['median_us']['scorer'])}; {fmt(e['median_us']['torch'])}; " +
                "/".join(f"{x:.1f}x" for x in e["torch_over_kernels"]) for kind, e in report["inputs"].items()))
