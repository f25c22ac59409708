#!/usr/bin/env python3
"""Time the ensemble's neighbourhood sums (swv2_fss_ens_rows, csrc/fss.hip) against their yardsticks on the same device tensors.  GPU box.

The method of tools/probe_fss.py: one process, HIP event pairs around every call, warm-up first, the contenders ALTERNATING call
by call, --launches each per repeat, the whole measurement --repeats times, medians.  Two samples of --channels x 720 x 1440 (73 by default;
the members of 16 and 50 x 2 x 73 planes take 9.7 and 30 GB), N(0, 1) members around a common signal, thresholds near the median, K = 1 and
4, scales (0, 1, 2, 4, 8, 16, 32), M = 16 and 50.

  kernels   swv2_fss_ens_rows alone (ops.fss_ens_rows: the mask launch and the box launch; a kernel trace of this script splits the two)
  det       swv2_fss_rows on member 0: the yardstick of the box pass (2 bit rows against P + 1)
  events    swv2_event_ens_sums + swv2_event_ens_finalize on the same members: the same bytes read once, the yardstick of the mask pass
  score     the whole ForecastScorer.ensemble_neighbourhood_score call: the kernels AND the fp64 scores
  torch     utils.events.fss_ens_rows_torch on the first --torch-channels channels of the same tensors (--torch-launches calls per repeat),
            scaled to all channels by the plane count; `kernels_sub` is swv2_fss_ens_rows on that same subset, the like-for-like pair

Writes a JSON report (default profiles/efss_probe.json): median times, the ratios, and whether rows and n_invalid of the kernels EQUAL the
statement's on the subset."""
import argparse, json, os, statistics, sys
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
from swin_v2_weather_amd import _lib as L, ops
from swin_v2_weather_amd.utils import weighted_acc_rmse as S

ap = argparse.ArgumentParser()
ap.add_argument("--launches", type=int, default=4)
ap.add_argument("--torch-launches", type=int, default=1)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--batch", type=int, default=2)
ap.add_argument("--channels", type=int, default=73)
ap.add_argument("--torch-channels", type=int, default=4)
ap.add_argument("--height", type=int, default=720)
ap.add_argument("--width", type=int, default=1440)
ap.add_argument("--members", type=int, nargs="+", default=[16, 50])
ap.add_argument("--thresholds", type=int, nargs="+", default=[1, 4])
ap.add_argument("--scales", type=int, nargs="+", default=[0, 1, 2, 4, 8, 16, 32])
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "efss_probe.json"))
a = ap.parse_args()
assert torch.cuda.is_available(), "the probe measures on an MI355X: no GPU, no number"
dev = torch.device("cuda:0")
B, C, H, W, Ct = a.batch, a.channels, a.height, a.width, min(a.torch_channels, a.channels)
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


report = {"shape": [B, C, H, W], "torch_channels": Ct, "scales": list(scales), "launches": a.launches, "torch_launches": a.torch_launches,
          "repeats": a.repeats, "device": torch.cuda.get_device_name(0), "rocm": torch.version.hip, "source_hash": L.source_hash(), "cases": {}}
signal = torch.randn(B, C, H, W, device=dev, generator=g)
tar = signal + 0.5 * torch.randn(B, C, H, W, device=dev, generator=g)
sc, sct = S.ForecastScorer(H, W, C, dev), S.ForecastScorer(H, W, Ct, dev)
for M in a.members:
    ens = torch.empty(M, B, C, H, W, device=dev)
    for m in range(M):
        ens[m] = signal + 0.75 * torch.randn(B, C, H, W, device=dev, generator=g)
    es, ts = ens[:, :, :Ct], tar[:, :Ct]                      # channel blocks, read in place
    for K in a.thresholds:
        thr = torch.linspace(-0.5, 0.5, K) if K > 1 else torch.zeros(1)
        t3, t3s = S.expand_thresholds(thr, B, C, dev), S.expand_thresholds(thr, B, Ct, dev)
        ws, wss = ops.fss_ens_workspace(B * C, H, W, M, K, len(scales), dev), ops.fss_ens_workspace(B * Ct, H, W, M, K, len(scales), dev)
        wsd, wse = ops.fss_workspace(B * C, H, W, K, len(scales), dev), ops.ens_event_workspace(B * C, H, W, M, K, dev)
        rows, ninv = ops.fss_ens_rows(es, ts, t3s, scales, wss)
        want = S.fss_ens_rows_torch(es, ts, thr, scales)
        equal = bool(torch.equal(rows, want[0]) and torch.equal(ninv, want[1]))
        del rows, ninv, want
        torch.cuda.empty_cache()
        res = measure({"kernels": lambda: ops.fss_ens_rows(ens, tar, t3, scales, ws),
                       "det": lambda: ops.fss_rows(ens[0], tar, t3, scales, wsd),
                       "events": lambda: (ops.ens_event_sums(ens, tar, t3, sc.w, wse), ops.ens_event_finalize(wse, M, K, B, C, H, W)),
                       "score": lambda: sc.ensemble_neighbourhood_score(ens, tar, M, thr, scales),
                       "kernels_sub": lambda: ops.fss_ens_rows(es, ts, t3s, scales, wss),
                       "score_sub": lambda: sct.ensemble_neighbourhood_score(es, ts, M, thr, scales),
                       "torch": lambda: S.fss_ens_rows_torch(es, ts, thr, scales)},
                      {"kernels": a.launches, "det": a.launches, "events": a.launches, "score": a.launches, "kernels_sub": a.launches,
                       "score_sub": a.launches, "torch": a.torch_launches})
        report["cases"][f"M{M}_K{K}"] = {"median_us": res, "member_bytes": M * B * C * H * W * 4, "workspace_bytes": ws.numel() * 4,
                                        "bit_planes": int(M).bit_length(), "band_rows": ops.fss_ens_band_rows(B * C, H, M, K, scales[-1]),
                                        "kernels_over_det": [x / y for x, y in zip(res["kernels"], res["det"])],
                                        "kernels_over_events": [x / y for x, y in zip(res["kernels"], res["events"])],
                                        "torch_over_kernels_same_subset": [x / y for x, y in zip(res["torch"], res["kernels_sub"])],
                                        "torch_over_score_same_subset": [x / y for x, y in zip(res["torch"], res["score_sub"])],
                                        "rows_equal_kernels_vs_torch": equal}
        print(f"M = {M} K = {K}: " + ", ".join(f"{k} {[round(x) for x in v]}" for k, v in res.items()) + f" us, equal {equal}", file=sys.stderr, flush=True)
        del ws, wss, wsd, wse
        torch.cuda.empty_cache()
    del ens, es
    torch.cuda.empty_cache()
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    json.dump(report, f, indent=1)
fmt = lambda v, p=0: "/".join(f"{x:.{p}f}" for x in v)      # noqa: E731
for k, e in report["cases"].items():
    m = e["median_us"]
    print(f"LABNOTES: {k}: kernels {fmt(m['kernels'])} us = {fmt(e['kernels_over_det'], 1)}x swv2_fss_rows on one member ({fmt(m['det'])} us), "
          f"{fmt(e['kernels_over_events'], 1)}x the Brier pass ({fmt(m['events'])} us); the score call {fmt(m['score'])} us; on {Ct} channels: kernels "
          f"{fmt(m['kernels_sub'])} us, torch {fmt(m['torch'])} us = {fmt(e['torch_over_kernels_same_subset'], 1)}x; rows equal: "
          f"{e['rows_equal_kernels_vs_torch']}")
