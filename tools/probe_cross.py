#!/usr/bin/env python3
"""Time the cross spectra (swv2_sht_cross_power / swv2_sht_cross_adjoint, csrc/sht.hip) beside the plain spectra on the same planes, and
the adjusted spectral MSE beside its torch statement and beside GeometricH1Loss.  GPU box.

One process, device events around every item, warm-up first, the items ALTERNATING call by call, --calls each per repeat, the whole
measurement --repeats times for the spread (as tools/probe_sht.py).  Two samples of the 73-variable model at 720 x 1440: 146 pairs
(forecast, target) = 292 planes, lmax = 720, mmax = 721, the fp32 table of utils/sht.py for every path.  Writes a JSON report (default
profiles/cross_probe.json) and prints one line for LABNOTES.md.

Kernel legs: swv2_sht_cross_power on the 146 pairs beside swv2_sht_power on the same 292 planes (the same MFMA work, the same table
traffic: the pair epilogue adds four fmas per pair and lane), both without and with the coefficient write; swv2_sht_cross_adjoint beside
swv2_sht_adjoint on the same coefficients (the functor reads each coefficient twice, once as itself and once as its partner's partner).
Loss legs, forward + backward to the forecast: GeometricAMSELoss on the kernels, the same formula on cross_power_torch, and
GeometricH1Loss, which transforms one plane per channel (prd - tar, and tar for the relative form) where AMSE transforms the pair.
`ratio` is an item's median over its yardstick's in the same repeat."""
import argparse, json, os, statistics, sys
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
from swin_v2_weather_amd import _lib as L, ops
from swin_v2_weather_amd.utils import sht
from swin_v2_weather_amd.utils.losses import GeometricAMSELoss, GeometricH1Loss, amse_from_spectra

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=10)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--batch", type=int, default=2)
ap.add_argument("--channels", type=int, default=73)
ap.add_argument("--nlat", type=int, default=720)
ap.add_argument("--nlon", type=int, default=1440)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cross_probe.json"))
a = ap.parse_args()
assert torch.cuda.is_available(), "the probe measures on an MI355X: no GPU, no number"
dev = torch.device("cuda:0")
B, C, H, W = a.batch, a.channels, a.nlat, a.nlon
pairs = B * C
g = torch.Generator(device=dev).manual_seed(0)
tar = torch.randn(B, C, H, W, device=dev, generator=g)
prd = (tar + 0.5 * torch.randn(B, C, H, W, device=dev, generator=g)).requires_grad_(True)
table = sht.device_table(H, W, dev)
mmax, lmax, nlat = table.shape
X = sht.spectral_operand(torch.stack((prd.detach(), tar), dim=2))          # planes prd_0, tar_0, prd_1, ...
_, coef = ops.sht_power(table, X, keep_coeffs=True)
gp = torch.rand(2 * pairs, lmax, device=dev, generator=g) + 0.5
gs = torch.rand(3, pairs, lmax, device=dev, generator=g) + 0.5
amse, h1 = GeometricAMSELoss((H, W)).to(dev), GeometricH1Loss((H, W)).to(dev)


def fwd_bwd(fn):
    prd.grad = None
    fn(prd, tar).sum().backward()


items = {
    "sht_power": lambda: ops.sht_power(table, X),
    "sht_cross_power": lambda: ops.sht_cross_power(table, X),
    "sht_power_coeffs": lambda: ops.sht_power(table, X, keep_coeffs=True),
    "sht_cross_power_coeffs": lambda: ops.sht_cross_power(table, X, keep_coeffs=True),
    "sht_adjoint": lambda: ops.sht_adjoint(table, coef, gp),
    "sht_cross_adjoint": lambda: ops.sht_cross_adjoint(table, coef, gs),
    "amse_fwd_bwd": lambda: fwd_bwd(amse),
    "amse_torch_fwd_bwd": lambda: fwd_bwd(lambda p, t: amse_from_spectra(*sht.cross_power_torch(p, t, table))),
    "h1_fwd_bwd": lambda: fwd_bwd(h1),
}
pairs_of = {"sht_cross_power": "sht_power", "sht_cross_power_coeffs": "sht_power_coeffs", "sht_cross_adjoint": "sht_adjoint",
            "amse_fwd_bwd": "amse_torch_fwd_bwd", "h1_fwd_bwd": "amse_fwd_bwd"}
flops = 2.0 * nlat * 4 * pairs * sum(lmax - m for m in range(min(mmax, lmax)))
counted = {k: flops for k in ("sht_power", "sht_cross_power", "sht_power_coeffs", "sht_cross_power_coeffs", "sht_adjoint", "sht_cross_adjoint")}
for _ in range(a.warmup):
    for f in items.values():
        f()
torch.cuda.synchronize()
report = {"shape": [B, C, H, W], "pairs": pairs, "lmax": lmax, "mmax": mmax, "calls": a.calls, "device": torch.cuda.get_device_name(0),
          "source_hash": L.source_hash(), "triangle_flops": flops, "table_bytes": table.numel() * 4, "operand_bytes": X.numel() * 4,
          "workspace_bytes": int(L.load().swv2_sht_cross_ws_bytes(pairs, lmax, mmax)), "repeats": []}
for r in range(a.repeats):
    ev = {k: [] for k in items}
    for _ in range(a.calls):
        for k, f in items.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); f(); e1.record()
            ev[k].append((e0, e1))
        torch.cuda.synchronize()
    rep = {}
    for k, evs in ev.items():
        ms = [e0.elapsed_time(e1) for e0, e1 in evs]
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
print(f"LABNOTES: cross probe {pairs} pairs {H}x{W}, {a.calls} calls x {a.repeats} repeats, medians: " + "; ".join(f"{k} {fmt(k)}" for k in items) +
      "; ratios " + ", ".join(f"{k} / {nb} {rat(k)}" for k, nb in pairs_of.items()))
