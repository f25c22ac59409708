#!/usr/bin/env python3
"""Time the spherical-harmonics synthesis (swv2_sht_synth, csrc/sht.hip) and what is built on it.  GPU box.

One process, device events around every item, warm-up first, the items ALTERNATING call by call, --calls each per repeat, the whole
measurement --repeats times for the spread.  At B * C = 146 planes of 720 x 1440 (two samples of the 73-variable model), lmax = 720,
mmax = 721, the fp32 table of utils/sht.py for every path.  Writes a JSON report (default profiles/isht_probe.json) and prints one
line for LABNOTES.md.

Items: swv2_sht_synth (null response, a response per plane) beside swv2_sht_adjoint on the same coefficients -- the same triangular
product, so the adjoint is the yardstick; spectral_filter against spectral_filter_torch on the same tensors and table; one row of
spherical_noise (73 planes) against spherical_noise_torch from the same normals.  TFLOP/s count 2 nlat 2 planes sum_m (lmax - m) flops
over the median time.  `ratio` is the kernel path's median over its yardstick's in the same repeat; no ratio was fixed in advance."""
import argparse, json, os, statistics, sys
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
from swin_v2_weather_amd import _lib as L, ops
from swin_v2_weather_amd.utils import sht

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=10)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--batch", type=int, default=2)
ap.add_argument("--channels", type=int, default=73)
ap.add_argument("--nlat", type=int, default=720)
ap.add_argument("--nlon", type=int, default=1440)
ap.add_argument("--length-scale-km", type=float, default=500.0)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "isht_probe.json"))
a = ap.parse_args()
assert torch.cuda.is_available(), "the probe measures on an MI355X: no GPU, no number"
dev = torch.device("cuda:0")
B, C, H, W = a.batch, a.channels, a.nlat, a.nlon
planes = B * C
g = torch.Generator(device=dev).manual_seed(0)
x = torch.randn(B, C, H, W, device=dev, generator=g)
table, rw = sht.device_table(H, W, dev), sht.inverse_weights(H, dev)
mmax, lmax, nlat = table.shape
gp = torch.rand(planes, lmax, device=dev, generator=g) + 0.5
_, coef = ops.sht_power(table, sht.spectral_operand(x), keep_coeffs=True)
resp = torch.exp(-torch.arange(lmax, device=dev, dtype=torch.float32) * (torch.arange(lmax, device=dev, dtype=torch.float32) + 1.0) * 1e-4)
sigma = sht.gaussian_noise_spectrum(H, W, a.length_scale_km)
sig = torch.from_numpy(sigma).to(device=dev, dtype=torch.float32)
z = torch.randn(mmax, 2 * C, lmax, device=dev, generator=g)


def no_grad(fn):
    with torch.no_grad():
        return fn()


items = {
    "sht_adjoint": lambda: ops.sht_adjoint(table, coef, gp),
    "sht_synth": lambda: ops.sht_synth(table, rw, coef, nlon=W),
    "sht_synth_per_plane": lambda: ops.sht_synth(table, rw, coef, gp, nlon=W),
    "spectral_filter": lambda: no_grad(lambda: sht.spectral_filter(x, resp)),
    "spectral_filter_torch": lambda: no_grad(lambda: sht.spectral_filter_torch(x, resp, table, rw)),
    "spherical_noise_row": lambda: no_grad(lambda: sht.spherical_noise(z, sigma, W)),
    "spherical_noise_row_torch": lambda: no_grad(lambda: sht.spherical_noise_torch(z, sig, table, rw, W)),
}
flops = 2.0 * nlat * 2 * planes * sum(lmax - m for m in range(min(mmax, lmax)))
counted = {"sht_adjoint": flops, "sht_synth": flops, "sht_synth_per_plane": flops, "spectral_filter": 2 * flops, "spectral_filter_torch": 2 * flops,
           "spherical_noise_row": flops * C / planes, "spherical_noise_row_torch": flops * C / planes}
pairs_of = {"sht_synth": "sht_adjoint", "sht_synth_per_plane": "sht_adjoint", "spectral_filter": "spectral_filter_torch",
            "spherical_noise_row": "spherical_noise_row_torch"}
for _ in range(a.warmup):
    for f in items.values():
        f()
torch.cuda.synchronize()
report = {"shape": [B, C, H, W], "lmax": lmax, "mmax": mmax, "calls": a.calls, "device": torch.cuda.get_device_name(0), "source_hash": L.source_hash(),
          "triangle_flops": flops, "table_bytes": table.numel() * 4, "coefficient_bytes": coef.numel() * 4, "noise_row_planes": C,
          "length_scale_km": a.length_scale_km, "repeats": []}
for r in range(a.repeats):
    ev = {k: [] for k in items}
    for _ in range(a.calls):
        for k, f in items.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); f(); e1.record()
            ev[k].append((e0, e1))
        torch.cuda.synchronize()
    rep = {}
    for k, pairs in ev.items():
        ms = [e0.elapsed_time(e1) for e0, e1 in pairs]
        rep[k] = {"median_ms": statistics.median(ms), "mean_ms": statistics.fmean(ms), "min_ms": min(ms), "max_ms": max(ms),
                  "tflops_median": counted[k] / statistics.median(ms) / 1e9}
    for k, nb in pairs_of.items():
        rep[k]["ratio_to_" + nb] = rep[k]["median_ms"] / rep[nb]["median_ms"]
    report["repeats"].append(rep)
summary = {k: {"median_ms": [rep[k]["median_ms"] for rep in report["repeats"]], "tflops": [rep[k]["tflops_median"] for rep in report["repeats"]]}
           for k in items}
for k, nb in pairs_of.items():
    summary[k]["ratio_to_" + nb] = [rep[k]["ratio_to_" + nb] for rep in report["repeats"]]
adj = summary["sht_adjoint"]["median_ms"]
summary["sht_synth"]["within_adjoint_spread"] = min(adj) <= statistics.median(summary["sht_synth"]["median_ms"]) <= max(adj)
report["summary"] = summary
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    json.dump(report, f, indent=1)
fmt = lambda k: "/".join(f"{v:.2f}" for v in summary[k]["median_ms"]) + " ms (" + "/".join(f"{v:.1f}" for v in summary[k]["tflops"]) + " TF)"
rat = lambda k: "/".join(f"{v:.3f}" for v in summary[k]["ratio_to_" + pairs_of[k]])
print(f"LABNOTES: isht probe B*C={planes} {H}x{W}, {a.calls} calls x {a.repeats} repeats, medians: " + "; ".join(f"{k} {fmt(k)}" for k in items) +
      f"; synth / adjoint {rat('sht_synth')} (per plane {rat('sht_synth_per_plane')}), filter / statement {rat('spectral_filter')}, "
      f"noise row / statement {rat('spherical_noise_row')}")
