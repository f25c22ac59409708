#!/usr/bin/env python3
"""Timing probe of mlp_fwd at the benchmark block shape (C 128, hidden 512, B = 2) -- GPU box."""
import os, sys, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
from swin_v2_weather_amd import ops
dev = torch.device("cuda:0")
T, Cc, hid = 64800, 128, 512
M = 2 * T
w1, w2 = ops.prep_weight(torch.randn(hid, Cc, device=dev) * 0.1), ops.prep_weight(torch.randn(Cc, hid, device=dev) * 0.1)
z = lambda n: torch.zeros(n, device=dev)
xs = [torch.randn(M, Cc, device=dev) for _ in range(6)]          # rotate inputs: no help from the infinity cache
g, b1, b2, bt = torch.ones(Cc, device=dev), z(hid), z(Cc), z(Cc)
def run(i):
    return ops.mlp_fwd(xs[i % len(xs)], w1, b1, w2, b2, g, bt, None, T)
for i in range(6):
    run(i)
torch.cuda.synchronize()
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
e0.record()
for i in range(30):
    run(i)
e1.record(); torch.cuda.synchronize()
print(f"mlp_fwd: {e0.elapsed_time(e1) / 30 * 1e3:.1f} us per launch (incl. output allocation)")
