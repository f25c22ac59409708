#!/usr/bin/env python3
"""Feeding training from int16-packed fields against fp32 fields: writes profiles/packed_probe.json (needs an MI355X).

Shape: local batch 2, slabs of 73 x 721 x 1440, a SyntheticYearSource against its packed copy (utils/packed.py).  The fp32 leg of every
pair is the yardstick: it is the unchanged fp32 path, measured in the same process, alternating with the packed leg.  Each leg gets
`--repeats` repeats of `--steps` timed steps after two untimed ones; the medians are reported, every repeat is kept.

  (d) the packer on the device: range pass + pack pass over the year, slabs/s  (its int16 output is the packed source of the other legs)
  (c) swv2_era5_select_normalize against swv2_era5_select_normalize_i16 on the same slabs, device events
  (a) the pipeline alone (iterate, touch nothing): samples/s and H2D GB/s, staged and zero-copy
  (b) the pipeline feeding the training step of the benchmark configuration (bench.py's host leg, restated)
Per-stage times of every pipeline leg: the producer's fill of one pinned slot (host clock), the copy stream's H2D + assembly of one batch
(device events), the whole step (host clock around a synchronise).
"""
import argparse
import json
import os
import statistics
import sys
import time
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPE = (73, 721, 1440)
SLAB_ELEMS = SHAPE[0] * SHAPE[1] * SHAPE[2]


class P(dict):
    __getattr__ = dict.__getitem__


class PinnedSource:
    """page-locked fp32 year arrays: the zero-copy source of the fp32 legs"""
    pinned = True

    def __init__(self, years, tensors):
        self.years, self._t = list(years), tensors
        self.n_samples_year, self.shape = [int(t.shape[0]) for t in tensors], tuple(tensors[0].shape[1:])

    def slab(self, year_idx, t):
        return self._t[year_idx][t]


def med(v):
    return statistics.median(v)


def run_pipeline(pipe, steps, step_fn=None):
    """one epoch of 2 untimed + `steps` timed batches -> (seconds per step, producer fill ms, copy-stream ms per batch)"""
    fills, pairs = [], []
    fill, submit = pipe._fill, pipe._submit

    def timed_fill(slot, locs):
        t = time.perf_counter()
        fill(slot, locs)
        fills.append(1e3 * (time.perf_counter() - t))

    def timed_submit(slot_pin, slot_dev, locs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(pipe.copy_stream)
        ev = submit(slot_pin, slot_dev, locs)
        e1.record(pipe.copy_stream)
        pairs.append((e0, e1))
        return ev
    pipe._fill, pipe._submit = timed_fill, timed_submit
    try:
        t1 = None
        for bi, (inp, tar, _) in enumerate(pipe):
            if bi == 2:                                      # two untimed steps fill the ring
                torch.cuda.synchronize()
                t1 = time.perf_counter()
            if step_fn is not None:
                step_fn(inp, tar)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t1) / steps
    finally:
        pipe._fill, pipe._submit = fill, submit
    copy_ms = [a.elapsed_time(b) for a, b in pairs[3:]]
    return dt, (med(fills[3:]) if len(fills) > 3 else None), med(copy_ms)


def pipeline_legs(sources, dev, B, steps, repeats, H, W, step_fn=None):
    """sources: {leg name: source}; the legs alternate, repeat by repeat"""
    from swin_v2_weather_amd.utils.host_pipeline import Era5HostPipeline
    prm = P(local_batch_size=B, dt=1, n_future=0, img_size=(H, W), in_channels=list(range(73)), out_channels=list(range(73)),
            add_zenith=False, seed=333, data_num_shards=1, data_shard_id=0, num_data_workers=16)
    pipes = {k: Era5HostPipeline(prm, s, dev, train=True, steps_per_epoch=steps + 2) for k, s in sources.items()}
    raw = {k: [] for k in pipes}
    for _ in range(repeats):
        for k, pipe in pipes.items():
            raw[k].append(run_pipeline(pipe, steps, step_fn))
    out = {}
    for k, rows in raw.items():
        bytes_per_sample = 2 * SLAB_ELEMS * (2 if pipes[k].packed else 4)
        sps = [B / r[0] for r in rows]
        out[k] = {"samples_per_s": med(sps), "samples_per_s_repeats": sps, "ms_per_step": 1e3 * med([r[0] for r in rows]),
                  "h2d_gb_per_s": med(sps) * bytes_per_sample / 1e9, "h2d_bytes_per_sample": bytes_per_sample,
                  "producer_fill_ms_per_batch": None if rows[0][1] is None else med([r[1] for r in rows]),
                  "copy_stream_ms_per_batch": med([r[2] for r in rows])}
    for pipe in pipes.values():
        pipe.pool.shutdown(wait=True)
    return out


def kernel_times(f32_src, packed_src, dev, B, H, W, n=20):
    from swin_v2_weather_amd import ops
    from swin_v2_weather_amd.utils.packed import param_tables
    raw16 = torch.stack([packed_src.slab(0, b) for b in range(B)]).unsqueeze(1).to(dev)
    raw32 = torch.stack([f32_src.slab(0, b) for b in range(B)]).unsqueeze(1).to(dev)
    off, sc = (torch.from_numpy(a).to(dev) for a in param_tables(packed_src))
    rows = torch.zeros(B, 1, dtype=torch.int32, device=dev)
    chan = torch.arange(73, dtype=torch.int32, device=dev)
    mean, std = torch.zeros(73, device=dev), torch.ones(73, device=dev)
    out = torch.empty(B, 73, H, W, device=dev)
    calls = {"era5_select_normalize": lambda: ops.era5_select_normalize(raw32, out, chan, mean, std),
             "era5_select_normalize_i16": lambda: ops.era5_select_normalize_i16(raw16, out, chan, mean, std, off, sc, rows)}
    ms = {k: [] for k in calls}
    for k, fn in calls.items():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    for _ in range(n):                                       # alternating, one event pair per launch
        for k, fn in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    elems = B * 73 * H * W
    res = {}
    for k, v in ms.items():
        bpe = 6 if k.endswith("i16") else 8
        res[k] = {"ms_median": med(v), "ms_min": min(v), "ms_max": max(v), "launches": n, "bytes_per_element": bpe,
                  "tb_per_s": elems * bpe / (med(v) * 1e-3) / 1e12}
    res["i16_over_fp32"] = res["era5_select_normalize_i16"]["ms_median"] / res["era5_select_normalize"]["ms_median"]
    return res


def pack_on_device(f32_src, dev, repeats):
    """-> (PackedMemorySource, measurement): the packer's two passes over year 0 on the device"""
    from swin_v2_weather_amd.utils import pack_dataset as D
    from swin_v2_weather_amd.utils import packed as PK
    n = f32_src.n_samples_year[0]
    out = np.empty((n,) + SHAPE, np.int16)
    secs = []
    for _ in range(repeats + 1):                             # the first is the untimed one
        torch.cuda.synchronize()
        t = time.perf_counter()
        lo, hi, mi = D._range_cuda(f32_src, 0, dev, 3, None)
        off, sc = PK.pack_params(lo, hi)
        D._pack_cuda(f32_src, 0, off, sc, out, dev, 3, None)
        torch.cuda.synchronize()
        secs.append(time.perf_counter() - t)
    secs = secs[1:]
    src = PK.PackedMemorySource(f32_src.years, [torch.from_numpy(out)], [(off, sc)], [mi], pinned=False)
    return src, {"slabs": n, "seconds_repeats": secs, "slabs_per_s": n / med(secs), "passes": 2,
                 "host_read_gb_per_s": 2 * n * SLAB_ELEMS * 4 / med(secs) / 1e9}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "packed_probe.json"))
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--samples", type=int, default=6, help="slabs of the synthetic year")
    ap.add_argument("--local-batch", type=int, default=2)
    ap.add_argument("--no-train", action="store_true", help="skip (b)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("probe_packed.py needs an MI355X (nothing here is measured on a CPU)")
    from swin_v2_weather_amd import _lib
    from swin_v2_weather_amd.utils import packed as PK
    from swin_v2_weather_amd.utils.host_pipeline import SyntheticYearSource
    _lib.load()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    B, H, W = a.local_batch, 720, 1440
    res = {"shape": {"local_batch": B, "slab": list(SHAPE), "img_size": [H, W]}, "steps": a.steps, "repeats": a.repeats,
           "source_hash": _lib.source_hash(), "device": torch.cuda.get_device_name(0)}

    f32 = SyntheticYearSource(n_years=1, n_samples=a.samples, seed=333, pinned=False)
    i16, res["packer_on_device"] = pack_on_device(f32, dev, a.repeats)
    # the device packer wrote what the numpy statement writes (one slab checked here; tests/test_packed_gpu.py holds the whole rule)
    assert np.array_equal(i16.slab(0, 1).numpy(), PK.pack_array(f32.slab(0, 1).numpy(), *i16.params(0)))
    res["pack"] = {"scale_max": float(np.max(i16.params(0)[1])), "field_std": 1.0, "missing": int(np.sum(i16.missing(0)))}
    res["kernels"] = kernel_times(f32, i16, dev, B, H, W)

    step_fn = None
    if not a.no_train:                                       # bench.py's model, loss, optimizer and step
        from swin_v2_weather_amd.networks.helpers import get_model
        from swin_v2_weather_amd.utils.losses import LossHandler
        from swin_v2_weather_amd.utils.optim import HipAdam
        torch.manual_seed(333)
        mp = SimpleNamespace(nettype="swin", img_size=[H, W], patch_size=4, depth=12, num_heads=8, n_in_channels=73, n_out_channels=73,
                             embed_dim=128, window_ratio=80, drop_path_rate=0.1, full_pos_embed=True, rel_pos=False, mlp_ratio=4,
                             activation_ckpt=False, residual=False, n_future=0, add_orography=False, add_landmask=False)
        net = get_model(mp).to(dev)
        net.train()
        loss_obj = LossHandler(SimpleNamespace(n_future=0, img_shape_x=H, img_shape_y=W, loss="l2", channel_weights="none",
                                               n_out_channels=73, model_grid_type="equiangular")).to(dev)
        opt = HipAdam(net.parameters(), lr=1e-3, betas=(0.9, 0.95))

        def step_fn(inp, tar):
            net.zero_grad()
            with loss_obj.fused_with(net, tar):
                gen = net(inp)
            loss_obj(gen, tar, inp).backward()
            opt.step()
        g = torch.Generator(device=dev).manual_seed(333)
        pool = [(torch.randn(B, 73, H, W, device=dev, generator=g), torch.randn(B, 73, H, W, device=dev, generator=g)) for _ in range(2)]
        for i in range(11):                                  # settle + warm-up on resident batches, as bench.py does
            step_fn(*pool[i % 2])
        torch.cuda.synchronize()
        t = time.perf_counter()
        for i in range(a.steps):
            step_fn(*pool[i % 2])
        torch.cuda.synchronize()
        res["resident_samples_per_s"] = B * a.steps / (time.perf_counter() - t)
        del pool

    def legs(sources, tag):
        res["pipeline_alone_" + tag] = pipeline_legs(sources, dev, B, a.steps, a.repeats, H, W)
        if step_fn is not None:
            res["pipeline_training_" + tag] = pipeline_legs(sources, dev, B, a.steps, a.repeats, H, W, step_fn)
    legs({"fp32": f32, "i16": i16}, "staged")
    # the page-locked copies (the zero-copy path): made from the same arrays
    f32_pin = PinnedSource(f32.years, [f32._t[0].pin_memory()])
    i16_pin = PK.PackedMemorySource(i16.years, [i16._t[0].pin_memory()], [i16.params(0)], [i16.missing(0)], pinned=True)
    del f32, i16
    legs({"fp32": f32_pin, "i16": i16_pin}, "pinned")

    checks = {}
    for k in [k for k in res if k.startswith("pipeline_")]:
        checks[k + ": packed not slower than fp32"] = res[k]["i16"]["samples_per_s"] >= res[k]["fp32"]["samples_per_s"]
        res[k]["i16_over_fp32"] = res[k]["i16"]["samples_per_s"] / res[k]["fp32"]["samples_per_s"]
    checks["kernels: i16 within 1.05 x fp32"] = res["kernels"]["i16_over_fp32"] <= 1.05
    res["checks"] = checks
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: res[k] for k in ("kernels", "packer_on_device", "checks")}))
    for k in [k for k in res if k.startswith("pipeline_")]:
        print(k, {n: round(v["samples_per_s"], 1) for n, v in res[k].items() if isinstance(v, dict)})
    return 0 if all(checks.values()) else 1


if __name__ == "__main__":
    raise SystemExit(main())
