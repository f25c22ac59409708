"""int16-packed year files: each (year file, channel) stored as 16-bit codes with one fp32 offset and one fp32 scale, as GRIB does.

A packed folder holds, for each year file `<stem>.npy` (`<stem>` ends in the four-digit year):
    <stem>.npy        int16 [N, C, H, W], C order
    <stem>.pack.npz   offset [C] fp32, scale [C] fp32, missing [C] int64 (values that were not finite), version
Parameters are per (year file, channel): a new year is packed without touching the old ones.  The `*.npy` / `*.h5` globs do not find
the sidecar.  Only `.npy` is packed; HDF5 stays fp32.

The rule, in fp32 operations numpy reproduces bit for bit (no fused multiply-add anywhere; csrc/packed.hip is held to these functions):
    lo, hi   the smallest and largest finite value of the (file, channel), fp32
    offset   fp32((lo64 + hi64) / 2) + 0.0f                    (the added zero turns -0 into +0)
    scale    fp32((hi64 - lo64) / 65534); 1 when hi == lo or nothing is finite (offset lo, or 0); FLT_MIN when the quotient is positive
             but below the normal range
    pack     q  = clamp(rint((x - offset) / scale), -32767, 32767)      one subtraction, one division, round half to even
             q  = -32768 for a non-finite x
    unpack   xh = (float(q) * scale) + offset                           two roundings;  xh = NaN for q = -32768
tests/packed_reference.py restates the rule independently and derives the error bound.
"""
from __future__ import annotations

import glob
import os

import numpy as np
import torch

VERSION = 1
MISSING = -32768
QMAX = 32767
SIDECAR = ".pack.npz"
F32 = np.float32


# ---- the rule ------------------------------------------------------------------------------------------------------
def pack_params(lo, hi):
    """(offset, scale), fp32, from the fp32 minimum and maximum of the finite values; lo > hi (+inf, -inf: the fold of nothing) or a
    non-finite bound means the channel has no finite value"""
    lo, hi = np.asarray(lo, F32), np.asarray(hi, F32)
    none = ~((lo <= hi) & np.isfinite(lo) & np.isfinite(hi))
    lo64, hi64 = np.where(none, 0.0, lo.astype(np.float64)), np.where(none, 0.0, hi.astype(np.float64))
    offset = ((lo64 + hi64) / 2.0).astype(F32) + F32(0.0)
    quot = (hi64 - lo64) / 65534.0
    with np.errstate(under="ignore"):
        scale = quot.astype(F32)
    tiny = np.finfo(F32).tiny
    scale = np.where((quot > 0) & (scale < tiny), tiny, scale)
    scale = np.where(quot > 0, scale, F32(1.0)).astype(F32)
    return offset.astype(F32), scale


def finite_range(x):
    """per-channel (lo [C], hi [C], missing [C] int64) of x [..., C, H, W] fp32: minimum / maximum of the finite values (+inf / -inf
    where there is none) and the number of the others"""
    x = np.asarray(x)
    assert x.dtype == F32 and x.ndim >= 3
    x = x.reshape((-1,) + x.shape[-3:])
    fin = np.isfinite(x)
    lo = np.where(fin, x, F32(np.inf)).min(axis=(0, 2, 3))
    hi = np.where(fin, x, F32(-np.inf)).max(axis=(0, 2, 3))
    return lo.astype(F32), hi.astype(F32), (~fin).sum(axis=(0, 2, 3)).astype(np.int64)


def _per_channel(p):
    return np.asarray(p, F32).reshape((-1, 1, 1))


def pack_array(x, offset, scale):
    """x [..., C, H, W] fp32 -> int16 codes with offset [C], scale [C]"""
    x = np.asarray(x)
    if x.dtype != F32:
        raise ValueError(f"pack_array: fp32 expected, got {x.dtype}")
    off, sc = _per_channel(offset), _per_channel(scale)
    with np.errstate(invalid="ignore", over="ignore"):
        r = np.rint((x - off) / sc)                    # fp32 throughout: one subtraction, one division, half to even
        r = np.clip(r, F32(-QMAX), F32(QMAX))
    return np.where(np.isfinite(x), r, F32(MISSING)).astype(np.int16)


def unpack_array(q, offset, scale):
    """int16 codes [..., C, H, W] -> fp32 with offset [C], scale [C]"""
    q = np.asarray(q)
    if q.dtype != np.int16:
        raise ValueError(f"unpack_array: int16 expected, got {q.dtype}")
    off, sc = _per_channel(offset), _per_channel(scale)
    v = (q.astype(F32) * sc) + off                     # two fp32 roundings
    return np.where(q == MISSING, F32(np.nan), v).astype(F32)


# ---- the sidecar ---------------------------------------------------------------------------------------------------
def sidecar_path(npy_path) -> str:
    return os.path.splitext(str(npy_path))[0] + SIDECAR


def write_sidecar(npy_path, offset, scale, missing) -> str:
    p = sidecar_path(npy_path)
    with open(p, "wb") as f:
        np.savez(f, offset=np.asarray(offset, F32), scale=np.asarray(scale, F32), missing=np.asarray(missing, np.int64),
                 version=np.int64(VERSION))
    return p


def read_sidecar(npy_path, channels=None):
    """-> (offset [C] fp32, scale [C] fp32, missing [C] int64); raises on a missing or mis-shaped sidecar and on an unknown version"""
    p = sidecar_path(npy_path)
    if not os.path.isfile(p):
        raise FileNotFoundError(f"packed year file {npy_path}: its sidecar {os.path.basename(p)} is missing")
    with np.load(p) as z:
        if not {"offset", "scale", "missing", "version"} <= set(z.files):
            raise ValueError(f"{p}: not a pack sidecar (holds {sorted(z.files)})")
        if int(z["version"]) != VERSION:
            raise ValueError(f"{p}: format version {int(z['version'])}, this package reads version {VERSION}")
        off, sc, mi = z["offset"], z["scale"], z["missing"]
    if off.dtype != F32 or sc.dtype != F32 or mi.dtype != np.int64 or off.ndim != 1 or sc.shape != off.shape or mi.shape != off.shape \
            or (channels is not None and off.shape != (channels,)):
        raise ValueError(f"{p}: offset {off.dtype}{off.shape}, scale {sc.dtype}{sc.shape}, missing {mi.dtype}{mi.shape}: expected float32, "
                         f"float32, int64 of shape ({channels if channels is not None else 'C'},)")
    if not (np.all(np.isfinite(off)) and np.all(np.isfinite(sc)) and np.all(sc > 0)):
        raise ValueError(f"{p}: offset / scale must be finite and scale positive")
    return off, sc, mi


# ---- sources -------------------------------------------------------------------------------------------------------
class PackedYearSource:
    """Packed year files under `location`: the attributes of YearArraySource, `read` delivering int16 slabs, and the parameters."""

    pinned = False
    packed = True

    def __init__(self, location):
        paths = sorted(glob.glob(os.path.join(location, "*.npy")))
        if not paths:
            raise FileNotFoundError(f"no *.npy year files under {location}")
        self.paths = paths
        self.years = [int(os.path.splitext(os.path.basename(p))[0][-4:]) for p in paths]
        self._arrays = [np.load(p, mmap_mode="r") for p in paths]
        for p, a in zip(paths, self._arrays):
            if a.dtype != np.int16 or a.ndim != 4:
                raise ValueError(f"{p}: int16 [N, C, H, W] expected in a packed folder, got {a.dtype} {a.shape}")
        self.shape = tuple(self._arrays[0].shape[1:])
        self.n_samples_year = [a.shape[0] for a in self._arrays]
        self._params = [read_sidecar(p, self.shape[0]) for p in paths]

    def params(self, year_idx):
        off, sc, _ = self._params[year_idx]
        return off, sc

    def missing(self, year_idx):
        return self._params[year_idx][2]

    def read(self, year_idx, t, out):
        """copy the int16 time slab t of year file year_idx ([C, H, W], uncropped) into the (pinned) numpy view `out`"""
        np.copyto(out, self._arrays[year_idx][t])

    def read_f32(self, year_idx, t, out):
        off, sc = self.params(year_idx)
        np.copyto(out, unpack_array(self._arrays[year_idx][t], off, sc))


class PackedMemorySource:
    """what pack_source returns: an in-memory packed copy of an fp32 source (page-locked when pinned: `slab(y, t)` is copied from in place)"""

    packed = True

    def __init__(self, years, tensors, params, missing, pinned):
        self.years, self._t, self._params, self._missing, self.pinned = list(years), tensors, params, missing, bool(pinned)
        self.n_samples_year = [int(t.shape[0]) for t in tensors]
        self.shape = tuple(tensors[0].shape[1:])

    def params(self, year_idx):
        return self._params[year_idx]

    def missing(self, year_idx):
        return self._missing[year_idx]

    def slab(self, year_idx, t):
        return self._t[year_idx][t]

    def read(self, year_idx, t, out):
        np.copyto(out, self._t[year_idx][t].numpy())

    def read_f32(self, year_idx, t, out):
        off, sc = self.params(year_idx)
        np.copyto(out, unpack_array(self._t[year_idx][t].numpy(), off, sc))


def source_range(source, year_idx):
    """(lo [C], hi [C], missing [C]) over every slab of one year file of an fp32 source"""
    C = source.shape[0]
    lo, hi, mi = np.full(C, np.inf, F32), np.full(C, -np.inf, F32), np.zeros(C, np.int64)
    buf = np.empty(source.shape, F32)
    for t in range(source.n_samples_year[year_idx]):
        source.read(year_idx, t, buf)
        l, h, m = finite_range(buf)
        lo, hi, mi = np.minimum(lo, l), np.maximum(hi, h), mi + m
    return lo, hi, mi


def pack_source(source, pinned=False) -> PackedMemorySource:
    """an in-memory packed copy of any fp32 source (numpy on the host: two passes per year, range then pack)"""
    tensors, params, missing = [], [], []
    buf = np.empty(source.shape, F32)
    for y in range(len(source.years)):
        lo, hi, mi = source_range(source, y)
        off, sc = pack_params(lo, hi)
        t = torch.empty((source.n_samples_year[y],) + tuple(source.shape), dtype=torch.int16, pin_memory=bool(pinned))
        for k in range(source.n_samples_year[y]):
            source.read(y, k, buf)
            np.copyto(t[k].numpy(), pack_array(buf, off, sc))
        tensors.append(t)
        params.append((off, sc))
        missing.append(mi)
    return PackedMemorySource(source.years, tensors, params, missing, pinned)


def param_tables(source):
    """(offset, scale) [years, C] fp32: the tables swv2_era5_select_normalize_i16 indexes with the year-file index"""
    rows = [source.params(y) for y in range(len(source.years))]
    return np.stack([r[0] for r in rows]).astype(F32), np.stack([r[1] for r in rows]).astype(F32)


def open_year_source(location):
    """PackedYearSource when the first `*.npy` under `location` holds int16, else YearArraySource(location)"""
    from .host_pipeline import YearArraySource
    paths = sorted(glob.glob(os.path.join(str(location), "*.npy")))
    if paths and np.load(paths[0], mmap_mode="r").dtype == np.int16:
        return PackedYearSource(str(location))
    return YearArraySource(str(location))
