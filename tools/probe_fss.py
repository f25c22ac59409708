#!/usr/bin/env python3
"""Time the neighbourhood sums of the fractions skill score on the HIP kernels (csrc/fss.hip) against their yardsticks on the same device
tensors.  GPU box.

The method of DESIGN 4j (tools/probe_score.py, tools/probe_events.py): one process, HIP event pairs around every call, warm-up first, the
contenders ALTERNATING call by call, --launches each per repeat, the whole measurement --repeats times, medians.  Two samples of
73 x 720 x 1440, N(0, 1) fields around a common signal, thresholds near the median, K = 1 and 4, scales (0, 1, 2, 4, 8, 16, 32).

  kernels   swv2_fss_rows alone (ops.fss_rows: the mask launch and the box launch)
  events    swv2_event_sums + swv2_event_finalize on the same tensors and thresholds: the point-by-point scores, one streaming pass over the
            same bytes -- what the neighbourhoods cost on top of it
  fss       the whole ForecastScorer.neighbourhood_score call: the kernels AND the fp64 scores formed from the rows by small torch kernels
  torch     utils.events.fss_rows_torch on the same tensors (--torch-launches calls per repeat: it takes seconds and gigabytes)

Writes a JSON report (default profiles/fss_probe.json): median times, unique input bytes / time, box counts / time, torch / fss, and
whether rows and n_invalid of the kernels EQUAL the statement's."""
import argparse, json, os, statistics, sys
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
from swin_v2_weather_amd import _lib as L, ops
from swin_v2_weather_amd.utils import weighted_acc_rmse as S

ap = argparse.ArgumentParser()
ap.add_argument("--launches", type=int, default=6)
ap.add_argument("--torch-launches", type=int, default=1)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--batch", type=int, default=2)
ap.add_argument("--channels", type=int, default=73)
ap.add_argument("--height", type=int, default=720)
ap.add_argument("--width", type=int, default=1440)
ap.add_argument("--thresholds", type=int, nargs="+", default=[1, 4])
ap.add_argument("--scales", type=int, nargs="+", default=[0, 1, 2, 4, 8, 16, 32])
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fss_probe.json"))
a = ap.parse_args()
assert torch.cuda.is_available(), "the probe measures on an MI355X: no GPU, no number"
dev = torch.device("cuda:0")
B, C, H, W = a.batch, a.channels, a.height, a.width
N = B * C * H * W * 4
scales = tuple(a.scales)
g = torch.Generator(device=dev).manual_seed(0)


def measure(contenders, launches):
    """contenders: name -> callable; launches: name -> calls per repeat -> {name: median_us [repeats]}"""
    for i in range(a.warmup):
        for k, f in contenders.items():
            if i < launches[k]:
                f()
    torch.cuda.synchronize()
    out = {k: [] for k in contenders}
    for _ in range(a.repeats):
        ev = {k: [] for k in contenders}
        for i in range(max(launches.values())):
            for k, f in contenders.items():
                if i < launches[k]:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(); f(); e1.record()
                    ev[k].append((e0, e1))
        torch.cuda.synchronize()
        for k, pairs in ev.items():
            out[k].append(statistics.median(e0.elapsed_time(e1) * 1e3 for e0, e1 in pairs))
    return out


report = {"shape": [B, C, H, W], "scales": list(scales), "launches": a.launches, "torch_launches": a.torch_launches, "repeats": a.repeats,
          "device": torch.cuda.get_device_name(0), "source_hash": L.source_hash(), "cases": {}}
signal = torch.randn(B, C, H, W, device=dev, generator=g)
prd, tar = signal + 0.75 * torch.randn(B, C, H, W, device=dev, generator=g), signal + 0.5 * torch.randn(B, C, H, W, device=dev, generator=g)
del signal
sc = S.ForecastScorer(H, W, C, dev)
for K in a.thresholds:
    thr = torch.linspace(-0.5, 0.5, K) if K > 1 else torch.zeros(1)
    t3 = S.expand_thresholds(thr, B, C, dev)
    ws, wse = ops.fss_workspace(B * C, H, W, K, len(scales), dev), ops.event_workspace(B * C, H, W, K, dev)
    rows, ninv = ops.fss_rows(prd, tar, t3, scales, ws)
    want = S.fss_rows_torch(prd, tar, thr, scales)
    equal = bool(torch.equal(rows, want[0]) and torch.equal(ninv, want[1]))
    del rows, ninv, want
    torch.cuda.empty_cache()
    res = measure({"kernels": lambda: ops.fss_rows(prd, tar, t3, scales, ws),
                   "events": lambda: (ops.event_sums(prd, tar, t3, sc.w, wse), ops.event_finalize(wse, K, B, C, H, W)),
                   "fss": lambda: sc.neighbourhood_score(prd, tar, thr, scales),
                   "torch": lambda: S.fss_rows_torch(prd, tar, thr, scales)},
                  {"kernels": a.launches, "events": a.launches, "fss": a.launches, "torch": a.torch_launches})
    boxes = 2 * B * C * K * len(scales) * H * W                # box counts of one call: both fields, every threshold and scale
    report["cases"][f"K{K}"] = {"median_us": res, "unique_input_bytes": 2 * N, "workspace_bytes": ws.numel() * 4, "box_counts": boxes,
                                "band_rows": ops.fss_band_rows(B * C, H, K, scales[-1]),
                                "kernels_input_gb_per_s": [2 * N / t / 1e3 for t in res["kernels"]],
                                "kernels_gbox_per_s": [boxes / t / 1e3 for t in res["kernels"]],
                                "kernels_over_events": [x / y for x, y in zip(res["kernels"], res["events"])],
                                "torch_over_fss": [x / y for x, y in zip(res["torch"], res["fss"])],
                                "rows_equal_kernels_vs_torch": equal}
    print(f"K = {K}: kernels {res['kernels']} us, events {res['events']} us, fss {res['fss']} us, torch {res['torch']} us, equal {equal}", file=sys.stderr, flush=True)
    del ws, wse
    torch.cuda.empty_cache()
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    json.dump(report, f, indent=1)
fmt = lambda v, p=0: "/".join(f"{x:.{p}f}" for x in v)      # noqa: E731
for k, e in report["cases"].items():
    m = e["median_us"]
    print(f"LABNOTES: {k}: kernels {fmt(m['kernels'])} us, {fmt(e['kernels_input_gb_per_s'])} GB/s of input, {fmt(e['kernels_gbox_per_s'], 1)} G box counts/s, "
          f"{fmt(e['kernels_over_events'], 1)}x the event pass ({fmt(m['events'])} us); neighbourhood_score {fmt(m['fss'])} us; torch {fmt(m['torch'])} us = "
          f"{fmt(e['torch_over_fss'], 1)}x; rows equal: {e['rows_equal_kernels_vs_torch']}")
