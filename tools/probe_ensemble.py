#!/usr/bin/env python3
"""Time the ensemble scores on the HIP kernels against the plain-torch composition on the same device tensors.  GPU box.

The method of DESIGN 4j: one process, HIP event pairs around every call, warm-up first, the contenders ALTERNATING call by call,
--launches each per repeat, the whole measurement --repeats times for the spread, medians.  At B = 1, C = 73, 720 x 1440 (one sample
of the 73-variable model) and M = 16 and M = 50 members, N(0, 1) fields around a common signal.  Contenders, all returning
EnsembleScores for the same members and truth:

    scorer    ForecastScorer.ensemble_score: swv2_ens_sums + swv2_ens_finalize, the workspace made once
    torch     utils.weighted_acc_rmse.ensemble_scores_torch: sort over the member axis, member-sized temporaries
    stream    the yardstick for the byte rate: ForecastScorer.score (swv2_score_sums) over two tensors of M planes per channel, the
              same number of planes as the members -- 8 B per element in one pass

Writes a JSON report (default profiles/ensemble_probe.json) and prints one line for LABNOTES.md.  GB/s are the bytes the pass has to
read once -- (M + 1) B C H W 4 for the ensemble scores, 2 M B C H W 4 for the yardstick -- over the median time."""
import argparse, json, os, statistics, sys
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
from swin_v2_weather_amd import _lib as L
from swin_v2_weather_amd.utils import weighted_acc_rmse as M

ap = argparse.ArgumentParser()
ap.add_argument("--launches", type=int, default=8)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--members", type=int, nargs="+", default=[16, 50])
ap.add_argument("--channels", type=int, default=73)
ap.add_argument("--height", type=int, default=720)
ap.add_argument("--width", type=int, default=1440)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ensemble_probe.json"))
a = ap.parse_args()
assert torch.cuda.is_available(), "the probe measures on an MI355X: no GPU, no number"
dev = torch.device("cuda:0")
B, C, H, W = 1, a.channels, a.height, a.width
g = torch.Generator(device=dev).manual_seed(0)
report = {"shape": [B, C, H, W], "launches": a.launches, "repeats": a.repeats, "device": torch.cuda.get_device_name(0),
          "source_hash": L.source_hash(), "members": {}}
for m in a.members:
    signal = torch.randn(B, C, H, W, device=dev, generator=g)
    ens = signal.unsqueeze(0) + torch.randn(m, B, C, H, W, device=dev, generator=g)
    tar = signal + torch.randn(B, C, H, W, device=dev, generator=g)
    other = torch.randn(m, C, H, W, device=dev, generator=g)          # the yardstick's second operand
    del signal
    scorer, stream = M.ForecastScorer(H, W, C, dev), M.ForecastScorer(H, W, C, dev)
    from swin_v2_weather_amd import ops
    assert ops.ens_members_ok(ens), "the members must take the kernel path"
    contenders = {"scorer": lambda: scorer.ensemble_score(ens, tar, m), "torch": lambda: M.ensemble_scores_torch(ens, tar, scorer.w),
                  "stream": lambda: stream.score(ens.view(m * B, C, H, W), other)}
    res = {k: f() for k, f in contenders.items() if k != "stream"}
    torch.cuda.synchronize()
    rel = lambda x, y: float(((x - y).abs() / y.abs().clamp_min(1e-30)).max())      # noqa: E731
    entry = {"ensemble_bytes": (m + 1) * B * C * H * W * 4, "stream_bytes": 2 * m * B * C * H * W * 4,
             "max_rel_difference_scorer_vs_torch": {k: rel(getattr(res["scorer"], k), getattr(res["torch"], k)) for k in ("crps", "fair_crps", "spread", "ens_rmse")},
             "hist_equal": bool(torch.equal(res["scorer"].hist, res["torch"].hist)), "repeats": []}
    del res
    for _ in range(a.warmup):
        for f in contenders.values():
            f()
    torch.cuda.synchronize()
    for r in range(a.repeats):
        ev = {k: [] for k in contenders}
        for _ in range(a.launches):
            for k, f in contenders.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(); f(); e1.record()
                ev[k].append((e0, e1))
        torch.cuda.synchronize()
        rep = {}
        for k, pairs in ev.items():
            us = [e0.elapsed_time(e1) * 1e3 for e0, e1 in pairs]
            nbytes = entry["stream_bytes"] if k == "stream" else entry["ensemble_bytes"]
            rep[k] = {"median_us": statistics.median(us), "mean_us": statistics.fmean(us), "min_us": min(us), "max_us": max(us),
                      "gb_per_s_median": nbytes / statistics.median(us) / 1e3}
        entry["repeats"].append(rep)
    entry["median_us"] = {k: [rep[k]["median_us"] for rep in entry["repeats"]] for k in contenders}
    entry["gb_per_s"] = {k: [rep[k]["gb_per_s_median"] for rep in entry["repeats"]] for k in contenders}
    entry["torch_over_scorer"] = [rep["torch"]["median_us"] / rep["scorer"]["median_us"] for rep in entry["repeats"]]
    entry["scorer_rate_over_stream_rate"] = [rep["scorer"]["gb_per_s_median"] / rep["stream"]["gb_per_s_median"] for rep in entry["repeats"]]
    report["members"][str(m)] = entry
    print(f"M = {m}: median us {entry['median_us']}", file=sys.stderr, flush=True)
    del ens, tar, other, scorer, stream, contenders
    torch.cuda.empty_cache()
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    json.dump(report, f, indent=1)
fmt = lambda v, p=0: "/".join(f"{x:.{p}f}" for x in v)      # noqa: E731
print(f"LABNOTES: ensemble probe B={B} C={C} {H}x{W}, {a.launches} calls x {a.repeats} repeats, median us (scorer; torch; torch / scorer; "
      "scorer GB/s; score_sums GB/s): " +
      "; ".join(f"M={m} {fmt(e['median_us']['scorer'])}; {fmt(e['median_us']['torch'])}; {fmt(e['torch_over_scorer'], 1)}x; "
                f"{fmt(e['gb_per_s']['scorer'])}; {fmt(e['gb_per_s']['stream'])}" for m, e in report["members"].items()))
