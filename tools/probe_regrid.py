#!/usr/bin/env python3
"""Time the regridding kernel against its yardsticks.  GPU box.

One process, device events around every launch, warm-up first, the items ALTERNATING launch by launch, --launches each per repeat, the
whole measurement --repeats times for the spread; medians.  On two samples of 73 x 720 x 1440 (B * C = 146 planes), for the 1.5 degree
(121 x 240) and the 5.625 degree (32 x 64) targets:

    regrid          swv2_regrid, prediction -> coarse buffer                        unique bytes B C (H W + Hd Wd) 4
    score_sums      swv2_score_sums without climatology on the same tensors         2 B C H W 4: the read-once plane kernel to compare with
    regrid_torch    the statement, two dense matmuls, on the same tensor
    scorer_coarse   RegriddedScorer.score (two regrids, sums and finalize on the coarse grid)
    scorer_native   ForecastScorer.score on the model's grid

Writes a JSON report (default profiles/regrid_probe.json) and prints one line for LABNOTES.md.  `rate_ratio_to_score_sums` is the
kernel's TB/s of unique bytes over swv2_score_sums' TB/s in the same repeat; `speedup_over_torch` is regrid_torch's median over the
kernel's."""
import argparse, json, os, statistics, sys
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
from swin_v2_weather_amd import _lib as L, ops
from swin_v2_weather_amd.utils import regrid as G
from swin_v2_weather_amd.utils.weighted_acc_rmse import ForecastScorer, RegriddedScorer, latitude_weights

ap = argparse.ArgumentParser()
ap.add_argument("--launches", type=int, default=50)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--batch", type=int, default=2)
ap.add_argument("--channels", type=int, default=73)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "regrid_probe.json"))
a = ap.parse_args()
assert torch.cuda.is_available(), "the probe measures on an MI355X: no GPU, no number"
dev = torch.device("cuda:0")
B, C, H, W = a.batch, a.channels, 720, 1440
g = torch.Generator(device=dev).manual_seed(0)
prd, tar = torch.randn(B, C, H, W, device=dev, generator=g), torch.randn(B, C, H, W, device=dev, generator=g)
w = latitude_weights(H, dev)
ws_score = ops.score_workspace(B * C, H, W, dev)
native = ForecastScorer(H, W, C, dev)
src = G.model_grid(H, W)
plane_bytes = B * C * H * W * 4
report = {"shape": [B, C, H, W], "launches": a.launches, "device": torch.cuda.get_device_name(0), "source_hash": L.source_hash(), "targets": {}}
lines = []
for deg in (1.5, 5.625):
    dst = G.grid_for_degrees(deg)
    rg = G.Regridder(src, dst, dev)
    Hd, Wd = dst.shape
    coarse = torch.empty(B, C, Hd, Wd, device=dev)
    A, Bm = rg._matrices(torch.float32, dev)
    scorer = RegriddedScorer(rg, C)
    items = {
        "regrid": lambda: rg(prd, out=coarse),
        "score_sums": lambda: ops.score_sums(prd, tar, w, ws_score),
        "regrid_torch": lambda: G.regrid_torch(prd, A, Bm),
        "scorer_coarse": lambda: scorer.score(prd, tar),
        "scorer_native": lambda: native.score(prd, tar),
    }
    nbytes = {"regrid": B * C * (H * W + Hd * Wd) * 4, "score_sums": 2 * plane_bytes}
    for _ in range(a.warmup):
        for f in items.values():
            f()
    torch.cuda.synchronize()
    reps = []
    for r in range(a.repeats):
        ev = {k: [] for k in items}
        for _ in range(a.launches):
            for k, f in items.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(); f(); e1.record()
                ev[k].append((e0, e1))
        torch.cuda.synchronize()
        rep = {}
        for k, pairs in ev.items():
            us = [e0.elapsed_time(e1) * 1e3 for e0, e1 in pairs]
            rep[k] = {"median_us": statistics.median(us), "mean_us": statistics.fmean(us), "min_us": min(us)}
            if k in nbytes:
                rep[k]["tb_per_s_median"] = nbytes[k] / statistics.median(us) / 1e6
        rep["regrid"]["rate_ratio_to_score_sums"] = rep["regrid"]["tb_per_s_median"] / rep["score_sums"]["tb_per_s_median"]
        rep["regrid"]["speedup_over_torch"] = rep["regrid_torch"]["median_us"] / rep["regrid"]["median_us"]
        rep["scorer_coarse"]["ratio_to_native"] = rep["scorer_coarse"]["median_us"] / rep["scorer_native"]["median_us"]
        reps.append(rep)
    summary = {k: {"median_us": [rep[k]["median_us"] for rep in reps]} for k in items}
    for k in nbytes:
        summary[k]["tb_per_s"] = [rep[k]["tb_per_s_median"] for rep in reps]
    summary["regrid"]["rate_ratio_to_score_sums"] = [rep["regrid"]["rate_ratio_to_score_sums"] for rep in reps]
    summary["regrid"]["speedup_over_torch"] = [rep["regrid"]["speedup_over_torch"] for rep in reps]
    summary["scorer_coarse"]["ratio_to_native"] = [rep["scorer_coarse"]["ratio_to_native"] for rep in reps]
    report["targets"][str(deg)] = {"grid": [Hd, Wd], "bands": [int(rg.band_counts[0].max()), int(rg.band_counts[1].max())], "bytes": nbytes,
                                   "repeats": reps, "summary": summary}
    j = lambda v, f="{:.1f}": "/".join(f.format(e) for e in v)          # noqa: E731
    lines.append(f"{deg} deg ({Hd}x{Wd}): regrid {j(summary['regrid']['median_us'])} us ({j(summary['regrid']['tb_per_s'], '{:.2f}')} TB/s unique, "
                 f"{j(summary['regrid']['rate_ratio_to_score_sums'], '{:.2f}')} of score_sums' {j(summary['score_sums']['tb_per_s'], '{:.2f}')} TB/s), "
                 f"torch statement {j(summary['regrid_torch']['median_us'])} us ({j(summary['regrid']['speedup_over_torch'])}x), "
                 f"RegriddedScorer.score {j(summary['scorer_coarse']['median_us'])} us vs ForecastScorer.score {j(summary['scorer_native']['median_us'])} us")
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    json.dump(report, f, indent=1)
print(f"LABNOTES: regrid probe B*C={B * C} 720x1440, {a.launches} launches x {a.repeats} repeats, medians: " + "; ".join(lines))
