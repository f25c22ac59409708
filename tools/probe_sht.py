#!/usr/bin/env python3
"""Time the spherical-harmonic degree power (csrc/sht.hip) against its plain-torch statement on the same tensors.  GPU box.

One process, device events around every item, warm-up first, the items ALTERNATING call by call, --calls each per repeat, the whole
measurement --repeats times for the spread.  At B * C = 146 planes of 720 x 1440 (two samples of the 73-variable model), lmax = 720,
mmax = 721, the fp32 table of utils/sht.py for both paths.  Writes a JSON report (default profiles/sht_probe.json) and prints one
line for LABNOTES.md.

Items: the rfft alone and with the repack into the kernels' operand (spectral_operand); swv2_sht_power without and with the coefficient write;
swv2_sht_adjoint; degree_power forward (no gradient) and forward + backward; degree_power_torch the same two ways.  TFLOP/s count
2 nlat 2 planes sum_m (lmax - m) flops, the products on the l >= m triangle, over the median time.  `ratio` is the kernel path's median
over the statement's in the same repeat: the operation count predicts about 0.5, at or above 1.0 the kernels are not finished."""
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sht_probe.json"))
a = ap.parse_args()
assert torch.cuda.is_available(), "the probe measures on an MI355X: no GPU, no number"
dev = torch.device("cuda:0")
B, C, H, W = a.batch, a.channels, a.nlat, a.nlon
planes = B * C
g = torch.Generator(device=dev).manual_seed(0)
x = torch.randn(B, C, H, W, device=dev, generator=g)
table = sht.device_table(H, W, dev)
mmax, lmax, nlat = table.shape
gp = torch.rand(planes, lmax, device=dev, generator=g) + 0.5
X = sht.spectral_operand(x)
_, coef = ops.sht_power(table, X, keep_coeffs=True)
xg = x.clone().requires_grad_(True)
gout = gp.reshape(B, C, lmax)


def fwd_bwd(fn):
    xg.grad = None
    (fn(xg) * gout).sum().backward()


def no_grad(fn):
    with torch.no_grad():
        return fn(x)


items = {
    "rfft": lambda: sht.longitude_transform(x),
    "rfft_repack": lambda: sht.spectral_operand(x),
    "sht_power": lambda: ops.sht_power(table, X),
    "sht_power_coeffs": lambda: ops.sht_power(table, X, keep_coeffs=True),
    "sht_adjoint": lambda: ops.sht_adjoint(table, coef, gp),
    "degree_power_fwd": lambda: no_grad(sht.degree_power),
    "degree_power_fwd_bwd": lambda: fwd_bwd(sht.degree_power),
    "torch_fwd": lambda: no_grad(lambda t: sht.degree_power_torch(t, table)),
    "torch_fwd_bwd": lambda: fwd_bwd(lambda t: sht.degree_power_torch(t, table)),
}
flops = 2.0 * nlat * 2 * planes * sum(lmax - m for m in range(min(mmax, lmax)))
counted = {"sht_power": flops, "sht_power_coeffs": flops, "sht_adjoint": flops, "degree_power_fwd": flops, "degree_power_fwd_bwd": 2 * flops,
           "torch_fwd": flops, "torch_fwd_bwd": 2 * flops}
for _ in range(a.warmup):
    for f in items.values():
        f()
torch.cuda.synchronize()
report = {"shape": [B, C, H, W], "lmax": lmax, "mmax": mmax, "calls": a.calls, "device": torch.cuda.get_device_name(0), "source_hash": L.source_hash(),
          "triangle_flops": flops, "table_bytes": table.numel() * 4, "operand_bytes": X.numel() * 4,
          "workspace_bytes": int(L.load().swv2_sht_ws_bytes(planes, lmax, mmax)), "repeats": []}
pairs_of = {"degree_power_fwd": "torch_fwd", "degree_power_fwd_bwd": "torch_fwd_bwd"}
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
        rep[k] = {"median_ms": statistics.median(ms), "mean_ms": statistics.fmean(ms), "min_ms": min(ms), "max_ms": max(ms)}
        if k in counted:
            rep[k]["tflops_median"] = counted[k] / statistics.median(ms) / 1e9
    for k, nb in pairs_of.items():
        rep[k]["ratio_to_" + nb] = rep[k]["median_ms"] / rep[nb]["median_ms"]
    report["repeats"].append(rep)
summary = {k: {"median_ms": [rep[k]["median_ms"] for rep in report["repeats"]]} for k in items}
for k in counted:
    summary[k]["tflops"] = [rep[k]["tflops_median"] for rep in report["repeats"]]
for k, nb in pairs_of.items():
    summary[k]["ratio_to_" + nb] = [rep[k]["ratio_to_" + nb] for rep in report["repeats"]]
report["summary"] = summary
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    json.dump(report, f, indent=1)
fmt = lambda k: "/".join(f"{v:.2f}" for v in summary[k]["median_ms"]) + " ms" + \
    (" (" + "/".join(f"{v:.1f}" for v in summary[k]["tflops"]) + " TF)" if k in counted else "")
rat = lambda k: "/".join(f"{v:.3f}" for v in summary[k]["ratio_to_" + pairs_of[k]])
print(f"LABNOTES: sht probe B*C={planes} {H}x{W}, {a.calls} calls x {a.repeats} repeats, medians: " + "; ".join(f"{k} {fmt(k)}" for k in items) +
      f"; kernels / statement forward {rat('degree_power_fwd')}, forward + backward {rat('degree_power_fwd_bwd')}")
