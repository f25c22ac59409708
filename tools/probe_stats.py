#!/usr/bin/env python3
"""Does swv2_stats_accumulate hide behind the H2D copy of its slab?  GPU box.

One process, device events around every operation, warm-up first, the operations ALTERNATING launch by launch: the H2D copy of one
73 x 721 x 1440 fp32 slab from pinned memory, swv2_stats_accumulate with prev, the same without prev; --launches each per repeat, the
whole measurement --repeats times for the spread; swv2_stats_finalize timed beside them.  The condition of DESIGN 4i: the median of
the kernel with prev is below the median of the copy, so the pass over a dataset is bound by the copy and the disk.

Bytes come from the shapes.  The kernel's unique bytes per element: 4 (slab) + 4 (prev) + 8 + 8 (tsum read and written) = 24, 16 for
the first slab of a file (no prev).  Then tools/hbm_ceiling.py runs as a child process for the streaming figure of the same box, and
utils/dataset_stats.compute_stats streams a page-locked SyntheticYearSource end to end (slabs/s, wall clock around a synchronised
call).  Writes a JSON report (default profiles/stats_probe.json) and prints one line for LABNOTES.md."""
import argparse, json, os, re, statistics, subprocess, sys, time
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
from swin_v2_weather_amd import _lib as L, ops
from swin_v2_weather_amd.utils import dataset_stats as DS

ap = argparse.ArgumentParser()
ap.add_argument("--launches", type=int, default=30)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--channels", type=int, default=73)
ap.add_argument("--e2e-slabs", type=int, default=8, help="slabs of the end-to-end run (0: skip it)")
ap.add_argument("--no-ceiling", action="store_true", help="do not run tools/hbm_ceiling.py")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stats_probe.json"))
a = ap.parse_args()
assert torch.cuda.is_available(), "the probe measures on an MI355X: no GPU, no number"
dev = torch.device("cuda:0")
C, H, W = a.channels, 721, 1440
n = C * H * W

ceiling = None
if not a.no_ceiling:                                           # before this process holds its own buffers
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "hbm_ceiling.py")], capture_output=True, text=True, timeout=600, check=True).stdout
    ceiling = {m.group(1).strip(): float(m.group(2)) for m in re.finditer(r"^(.*?)\s+([0-9.]+) TB/s", out, flags=re.M)}

host = torch.empty((C, H, W), dtype=torch.float32, pin_memory=True)
torch.randn((C, H, W), generator=torch.Generator().manual_seed(0), out=host)
slab = [torch.empty((C, H, W), dtype=torch.float32, device=dev) for _ in range(2)]
slab[1].copy_(host).mul_(1.5)
pivot = torch.zeros(C, dtype=torch.float64, device=dev)
tsum = torch.empty((C, H, W), dtype=torch.float64, device=dev)
part = ops.stats_workspace(C, H, W, dev)
ops.stats_accumulate(slab[1], None, pivot, tsum, part, True)
ops_ = {
    "h2d_copy": lambda: slab[0].copy_(host, non_blocking=True),
    "stats_accumulate_prev": lambda: ops.stats_accumulate(slab[0], slab[1], pivot, tsum, part, False),
    "stats_accumulate_noprev": lambda: ops.stats_accumulate(slab[0], None, pivot, tsum, part, False),
    "stats_finalize": lambda: ops.stats_finalize(part, tsum, pivot, 1000),
}
unique_bytes = {"h2d_copy": 4 * n, "stats_accumulate_prev": 24 * n, "stats_accumulate_noprev": 20 * n, "stats_finalize": 12 * n}
for _ in range(a.warmup):
    for f in ops_.values():
        f()
torch.cuda.synchronize()
report = {"shape": [C, H, W], "slices": ops.stats_slices(C, H, W), "launches": a.launches, "device": torch.cuda.get_device_name(0),
          "source_hash": L.source_hash(), "unique_bytes": unique_bytes, "hbm_ceiling_tb_per_s": ceiling, "repeats": []}
for r in range(a.repeats):
    ev = {k: [] for k in ops_}
    for _ in range(a.launches):
        for k, f in ops_.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); f(); e1.record()
            ev[k].append((e0, e1))
    torch.cuda.synchronize()
    rep = {}
    for k, pairs in ev.items():
        us = [e0.elapsed_time(e1) * 1e3 for e0, e1 in pairs]
        rep[k] = {"median_us": statistics.median(us), "mean_us": statistics.fmean(us), "min_us": min(us), "max_us": max(us),
                  "tb_per_s_median": unique_bytes[k] / statistics.median(us) / 1e6}
    report["repeats"].append(rep)
summary = {k: {"median_us": [rep[k]["median_us"] for rep in report["repeats"]], "tb_per_s": [rep[k]["tb_per_s_median"] for rep in report["repeats"]]}
           for k in ops_}
report["summary"] = summary
report["kernel_below_copy"] = all(k < c for k, c in zip(summary["stats_accumulate_prev"]["median_us"], summary["h2d_copy"]["median_us"]))
del host, slab, tsum, part
torch.cuda.empty_cache()

if a.e2e_slabs > 0:
    src = DS.SyntheticYearSource(n_years=1, n_samples=a.e2e_slabs, shape=(C, H, W), pinned=True)
    pv = DS.source_pivot(src)
    runs = []
    for _ in range(a.repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        st = DS.accumulate_source(src, dev, pv)                  # ends with a synchronise of its copy stream
        torch.cuda.synchronize()
        runs.append(a.e2e_slabs / (time.perf_counter() - t0))
        del st
    report["end_to_end"] = {"source": "SyntheticYearSource(pinned=True)", "slabs": a.e2e_slabs, "slabs_per_s": runs,
                            "gb_per_s": [r * 4 * n / 1e9 for r in runs]}

os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    json.dump(report, f, indent=1)
fmt = lambda k: "/".join(f"{v:.0f}" for v in summary[k]["median_us"]) + " us (" + "/".join(f"{v:.2f}" for v in summary[k]["tb_per_s"]) + " TB/s)"
print(f"LABNOTES: stats probe {C}x{H}x{W}, {a.launches} launches x {a.repeats} repeats, medians: H2D copy {fmt('h2d_copy')}; "
      f"accumulate with prev {fmt('stats_accumulate_prev')}; without {fmt('stats_accumulate_noprev')}; finalize {fmt('stats_finalize')}; "
      f"kernel below copy: {report['kernel_below_copy']}; hbm_ceiling {ceiling}; end to end "
      + ("/".join(f"{v:.1f}" for v in report["end_to_end"]["slabs_per_s"]) + " slabs/s" if a.e2e_slabs > 0 else "skipped"))
