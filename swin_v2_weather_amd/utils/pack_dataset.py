"""Pack a folder of fp32 year files into int16 year files (utils/packed.py), or unpack one.

    python -m swin_v2_weather_amd.utils.pack_dataset --data DIR --out DIR [--years 1979 ...] [--device cuda:0|cpu] [--overwrite] [--stds FILE]
    python -m swin_v2_weather_amd.utils.pack_dataset unpack --data DIR --out DIR [--overwrite]

Each year file takes two passes: the range of every channel (minimum and maximum of the finite values, the number of the others), then
the codes.  On a CUDA device the slabs go through the staging of dataset_stats (pinned ring, copy stream, two device slabs) into
swv2_pack_range and swv2_era5_pack_i16, the int16 slab comes back into a pinned buffer and is written into a memory-mapped .npy; on `cpu`
the numpy statement of utils/packed.py runs.  Both write byte-identical files.  The .npy is written under a temporary name and renamed
after the sidecar: an interrupted run leaves no folder that opens as packed.  `unpack` is the reverse, on the cpu.
"""
from __future__ import annotations

import argparse
import os
import time

import numpy as np
import torch

from . import packed as P
from .dataset_stats import select_years, staged_slabs
from .host_pipeline import YearArraySource


def _range_cuda(source, y, device, ring, workers):
    from .. import ops
    C, H, W = source.shape
    rng = torch.empty(C, 2, dtype=torch.float32, device=device)
    missing = torch.empty(C, dtype=torch.int64, device=device)
    ws = ops.pack_range_workspace(C, H, W, device)
    items = [(y, t) for t in range(source.n_samples_year[y])]
    for i, slab, _, cs in staged_slabs(source, items, device, ring=ring, workers=workers):
        ops.pack_range(slab, rng, missing, ws, first=i == 0, stream=cs.cuda_stream)
    r = rng.cpu().numpy()
    return r[:, 0].copy(), r[:, 1].copy(), missing.cpu().numpy()


def _pack_cuda(source, y, offset, scale, out, device, ring, workers):
    from .. import ops
    off, sc = torch.from_numpy(offset).to(device), torch.from_numpy(scale).to(device)
    q = [torch.empty(tuple(source.shape), dtype=torch.int16, device=device) for _ in range(2)]
    host = [torch.empty(tuple(source.shape), dtype=torch.int16, pin_memory=True) for _ in range(2)]
    done = [None, None]                                          # the D2H-done event and the slab index of each pinned buffer

    def flush(k):
        if done[k] is not None:
            ev, t = done[k]
            ev.synchronize()
            out[t] = host[k].numpy()
            done[k] = None
    items = [(y, t) for t in range(source.n_samples_year[y])]
    for i, slab, _, cs in staged_slabs(source, items, device, ring=ring, workers=workers):
        k = i % 2
        flush(k)                                                 # slab i - 2 leaves the pinned buffer before slab i enters it
        with torch.cuda.stream(cs):
            ops.era5_pack_i16(slab, q[k], off, sc, stream=cs.cuda_stream)
            host[k].copy_(q[k], non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(cs)
        done[k] = (ev, i)
    flush(0), flush(1)


def pack_year(source, y, out_path, device="cpu", ring=3, workers=None):
    """year file y of the fp32 `source` -> out_path (.npy int16) + its sidecar; returns (offset, scale, missing)"""
    device = torch.device(device)
    if device.type == "cuda":
        lo, hi, missing = _range_cuda(source, y, device, ring, workers)
    else:
        lo, hi, missing = P.source_range(source, y)
    offset, scale = P.pack_params(lo, hi)
    tmp = out_path + ".tmp"
    out = np.lib.format.open_memmap(tmp, mode="w+", dtype=np.int16, shape=(source.n_samples_year[y],) + tuple(source.shape))
    if device.type == "cuda":
        _pack_cuda(source, y, offset, scale, out, device, ring, workers)
    else:
        buf = np.empty(source.shape, np.float32)
        for t in range(source.n_samples_year[y]):
            source.read(y, t, buf)
            out[t] = P.pack_array(buf, offset, scale)
    out.flush()
    del out
    P.write_sidecar(out_path, offset, scale, missing)
    os.replace(tmp, out_path)                                    # last: only now does the folder open as packed
    return offset, scale, missing


def pack_folder(data, out_dir, years=None, device="cpu", overwrite=False, stds=None, ring=3, workers=None, log=print):
    source = YearArraySource(str(data))
    if not source.paths[0].endswith(".npy"):
        raise ValueError(f"{data}: only *.npy year files are packed (HDF5 stays fp32)")
    if np.load(source.paths[0], mmap_mode="r").dtype != np.float32:
        raise ValueError(f"{data}: fp32 year files expected (an int16 folder is packed already)")
    os.makedirs(out_dir, exist_ok=True)
    gstd = None if stds is None else np.load(stds).reshape(-1).astype(np.float64)
    for y in select_years(source, years):
        dst = os.path.join(str(out_dir), os.path.basename(source.paths[y]))
        if os.path.exists(dst) and not overwrite:
            raise FileExistsError(f"{dst} exists (give --overwrite)")
        t0 = time.perf_counter()
        offset, scale, missing = pack_year(source, y, dst, device=device, ring=ring, workers=workers)
        dt = time.perf_counter() - t0
        log(f"{os.path.basename(dst)}: {source.n_samples_year[y]} slabs on {device} in {dt:.2f} s ({2 * source.n_samples_year[y] / dt:.1f} slab passes/s)")
        for c in range(source.shape[0]):
            rel = "" if gstd is None or c >= gstd.size else f"  scale/std {float(scale[c]) / gstd[c]:.3e}"
            log(f"  channel {c:3d}: scale {float(scale[c]):.6e}{rel}  missing {int(missing[c])}")
    return out_dir


def unpack_folder(data, out_dir, overwrite=False, log=print):
    source = P.PackedYearSource(str(data))
    os.makedirs(out_dir, exist_ok=True)
    for y, path in enumerate(source.paths):
        dst = os.path.join(str(out_dir), os.path.basename(path))
        if os.path.exists(dst) and not overwrite:
            raise FileExistsError(f"{dst} exists (give --overwrite)")
        out = np.lib.format.open_memmap(dst + ".tmp", mode="w+", dtype=np.float32, shape=(source.n_samples_year[y],) + tuple(source.shape))
        for t in range(source.n_samples_year[y]):
            source.read_f32(y, t, out[t])
        out.flush()
        del out
        os.replace(dst + ".tmp", dst)
        log(f"{os.path.basename(dst)}: {source.n_samples_year[y]} slabs unpacked")
    return out_dir


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="python -m swin_v2_weather_amd.utils.pack_dataset", description=__doc__.split("\n\n")[0])
    ap.add_argument("--data", required=True, help="folder of fp32 year files (*.npy, [N, C, H, W])")
    ap.add_argument("--out", required=True, help="folder the packed year files and their sidecars are written to")
    ap.add_argument("--years", type=int, nargs="+", help="only these year files (four-digit file stems)")
    ap.add_argument("--device", default="cuda:0" if torch.cuda.is_available() else "cpu")
    ap.add_argument("--overwrite", action="store_true")
    ap.add_argument("--stds", help="global_stds.npy: print scale / global_std per channel")
    ap.add_argument("--ring", type=int, default=3, help="pinned staging slabs")
    ap.add_argument("--workers", type=int, default=None, help="producer threads")
    return ap


def build_unpack_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="python -m swin_v2_weather_amd.utils.pack_dataset unpack")
    ap.add_argument("--data", required=True, help="packed folder")
    ap.add_argument("--out", required=True, help="folder the fp32 year files are written to")
    ap.add_argument("--overwrite", action="store_true")
    return ap


def main(argv=None):
    import sys
    argv = list(sys.argv[1:] if argv is None else argv)
    if argv and argv[0] == "unpack":
        a = build_unpack_parser().parse_args(argv[1:])
        unpack_folder(a.data, a.out, overwrite=a.overwrite)
        return 0
    a = build_parser().parse_args(argv)
    pack_folder(a.data, a.out, years=a.years, device=a.device, overwrite=a.overwrite, stds=a.stds, ring=a.ring, workers=a.workers)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
