#!/usr/bin/env python3
"""Time the forecast-event scores on the HIP kernels (csrc/events.hip) against their yardsticks on the same device tensors.  GPU box.

The method of DESIGN 4j (tools/probe_score.py, tools/probe_ensemble.py): one process, HIP event pairs around every call, warm-up first,
the contenders ALTERNATING call by call, --launches each per repeat, the whole measurement --repeats times, medians.  Two samples of
73 x 720 x 1440, N(0, 1) fields around a common signal.

  deterministic   events     ForecastScorer.event_score at K = 1, 4, 8, without and with a base field (thresholds near the median): the
                             two launches AND the fp64 scores formed from the table by some sixty small torch kernels
                  kernels    swv2_event_sums + swv2_event_finalize alone (ops.event_sums / event_finalize): what the yardstick compares with
                  stream     the yardstick: ForecastScorer.score (swv2_score_sums) on the same tensors -- the same bytes, 8 B / element
                             (12 with the climatology as the base field)
                  torch      utils.events.event_table_torch on the same tensors
  ensemble        kernels    swv2_event_ens_sums + swv2_event_ens_finalize alone
                  events     ForecastScorer.ensemble_event_score at M = 16, 50 and K = 1, 4; once on thresholds near the median
                             ("spread": the counts fall into many bins) and once on thresholds no value exceeds ("one_bin": every point
                             in the bin (n = 0, o = 0), which the kernel derives instead of counting)
                  stream     swv2_score_sums over the same number of planes as the members: the byte-rate yardstick
                  crps       ForecastScorer.ensemble_score (swv2_ens_sums) on the same members
                  torch      utils.events.ensemble_event_sums_torch

Writes a JSON report (default profiles/event_probe.json): median time, unique bytes / time, the ratio of the byte rates to the
yardstick's, torch / kernels."""
import argparse, json, os, statistics, sys
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
from swin_v2_weather_amd import _lib as L, ops
from swin_v2_weather_amd.utils import weighted_acc_rmse as S

ap = argparse.ArgumentParser()
ap.add_argument("--launches", type=int, default=6)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--members", type=int, nargs="+", default=[16, 50])
ap.add_argument("--batch", type=int, default=2)
ap.add_argument("--channels", type=int, default=73)
ap.add_argument("--height", type=int, default=720)
ap.add_argument("--width", type=int, default=1440)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "event_probe.json"))
a = ap.parse_args()
assert torch.cuda.is_available(), "the probe measures on an MI355X: no GPU, no number"
dev = torch.device("cuda:0")
B, C, H, W = a.batch, a.channels, a.height, a.width
N = B * C * H * W * 4
g = torch.Generator(device=dev).manual_seed(0)


def measure(contenders, nbytes):
    """contenders: name -> callable; nbytes: name -> unique bytes of one call -> {name: {median_us [repeats], gb_per_s [repeats]}}"""
    for _ in range(a.warmup):
        for f in contenders.values():
            f()
    torch.cuda.synchronize()
    out = {k: {"median_us": [], "gb_per_s": []} for k in contenders}
    for _ in range(a.repeats):
        ev = {k: [] for k in contenders}
        for _ in range(a.launches):
            for k, f in contenders.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(); f(); e1.record()
                ev[k].append((e0, e1))
        torch.cuda.synchronize()
        for k, pairs in ev.items():
            med = statistics.median(e0.elapsed_time(e1) * 1e3 for e0, e1 in pairs)
            out[k]["median_us"].append(med)
            out[k]["gb_per_s"].append(nbytes[k] / med / 1e3)
    return out


def ratios(res, yard="stream"):
    res["events_rate_over_stream_rate"] = [x / y for x, y in zip(res["events"]["gb_per_s"], res[yard]["gb_per_s"])]
    res["kernels_rate_over_stream_rate"] = [x / y for x, y in zip(res["kernels"]["gb_per_s"], res[yard]["gb_per_s"])]
    if "torch" in res:
        res["torch_over_events"] = [x / y for x, y in zip(res["torch"]["median_us"], res["events"]["median_us"])]
    return res


report = {"shape": [B, C, H, W], "launches": a.launches, "repeats": a.repeats, "device": torch.cuda.get_device_name(0),
          "source_hash": L.source_hash(), "deterministic": {}, "ensemble": {}}
signal = torch.randn(B, C, H, W, device=dev, generator=g)
prd, tar = signal + 0.75 * torch.randn(B, C, H, W, device=dev, generator=g), signal + 0.5 * torch.randn(B, C, H, W, device=dev, generator=g)
clim = 0.3 * torch.randn(C, H, W, device=dev, generator=g)
plain, with_clim = S.ForecastScorer(H, W, C, dev), S.ForecastScorer(H, W, C, dev, climatology=clim)
for base in (False, True):
    sc = with_clim if base else plain
    nb = N * 2 + (N // B if base else 0)
    for K in (1, 4, 8):
        thr = torch.linspace(-0.5, 0.5, K) if K > 1 else torch.zeros(1)
        r = sc.event_score(prd, tar, thr, anomaly=base)
        t = S.event_table_torch(prd, tar, thr, sc.w, sc.clim)
        same = float(((r.table - t[0]).abs() / t[0].abs().clamp_min(1.0)).max())
        assert torch.equal(r.n_invalid, t[1])
        ws, t3 = ops.event_workspace(B * C, H, W, K, dev), S.expand_thresholds(thr, B, C, dev)
        res = measure({"events": lambda: sc.event_score(prd, tar, thr, anomaly=base), "stream": lambda: sc.score(prd, tar),
                       "kernels": lambda: (ops.event_sums(prd, tar, t3, sc.w, ws, sc.clim), ops.event_finalize(ws, K, B, C, H, W)),
                       "torch": lambda: S.event_table_torch(prd, tar, thr, sc.w, sc.clim)}, {"events": nb, "stream": nb, "kernels": nb, "torch": nb})
        res["unique_bytes"], res["max_rel_difference_kernels_vs_torch"] = nb, same
        report["deterministic"][f"K{K}_{'base' if base else 'plain'}"] = ratios(res)
        print(f"K = {K} base = {base}: {res['events']['median_us']} us, stream {res['stream']['median_us']} us", file=sys.stderr, flush=True)
        del r, t
del prd, clim, with_clim
torch.cuda.empty_cache()
for m in a.members:
    ens = signal.unsqueeze(0) + torch.randn(m, B, C, H, W, device=dev, generator=g)
    other = torch.randn(m * B, C, H, W, device=dev, generator=g)          # the yardstick's second operand
    assert ops.ens_members_ok(ens), "the members must take the kernel path"
    nb, nbs = (m + 1) * N, 2 * m * N
    for K in (1, 4):
        for case, thr in (("spread", torch.linspace(-0.5, 0.5, K) if K > 1 else torch.zeros(1)), ("one_bin", torch.full((K,), 1.0e6))):
            r = plain.ensemble_event_score(ens, tar, m, thr)
            t = S.ensemble_event_sums_torch(ens, tar, thr, plain.w)
            equal = bool(torch.equal(r.hist, t[2]))
            del r, t
            ws, t3 = ops.ens_event_workspace(B * C, H, W, m, K, dev), S.expand_thresholds(thr, B, C, dev)
            res = measure({"events": lambda: plain.ensemble_event_score(ens, tar, m, thr),
                           "kernels": lambda: (ops.ens_event_sums(ens, tar, t3, plain.w, ws), ops.ens_event_finalize(ws, m, K, B, C, H, W)), "stream": lambda: plain.score(ens.view(m * B, C, H, W), other),
                           "crps": lambda: plain.ensemble_score(ens, tar, m), "torch": lambda: S.ensemble_event_sums_torch(ens, tar, thr, plain.w)},
                          {"events": nb, "kernels": nb, "stream": nbs, "crps": nb, "torch": nb})
            res["unique_bytes"], res["stream_bytes"], res["hist_equal_kernels_vs_torch"] = nb, nbs, equal
            res["crps_over_events"] = [x / y for x, y in zip(res["crps"]["median_us"], res["kernels"]["median_us"])]
            report["ensemble"][f"M{m}_K{K}_{case}"] = ratios(res)
            print(f"M = {m} K = {K} {case}: {res['events']['median_us']} us, stream {res['stream']['median_us']} us, crps {res['crps']['median_us']} us",
                  file=sys.stderr, flush=True)
    del ens, other
    torch.cuda.empty_cache()
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    json.dump(report, f, indent=1)
fmt = lambda v, p=0: "/".join(f"{x:.{p}f}" for x in v)      # noqa: E731
for part in ("deterministic", "ensemble"):
    for k, e in report[part].items():
        print(f"LABNOTES: {k}: kernels {fmt(e['kernels']['median_us'])} us, {fmt(e['kernels']['gb_per_s'])} GB/s, rate / stream rate "
              f"{fmt(e['kernels_rate_over_stream_rate'], 2)}; events {fmt(e['events']['median_us'])} us, {fmt(e['events']['gb_per_s'])} GB/s; stream {fmt(e['stream']['median_us'])} us; "
              f"rate / stream rate {fmt(e['events_rate_over_stream_rate'], 2)}; torch / events {fmt(e['torch_over_events'], 1)}x" +
              (f"; crps / kernels {fmt(e['crps_over_events'], 2)}x" if "crps_over_events" in e else ""))
