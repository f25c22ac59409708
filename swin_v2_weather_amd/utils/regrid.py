"""First-order conservative regridding between global lat-lon grids, and the scorer's way onto the 1.5 degree grid of the published
tables (WeatherBench 2 scorecards: 121 x 240 with both poles; the older 5.625 degree tables: 32 x 64 without).

The statement (fp64 numpy, no GPU).  A grid is its strictly descending latitude centres and `nlon` longitude centres 360 i / nlon.
Cells: in latitude the bounds are the midpoints between neighbouring centres and the outer bounds are ALWAYS +90 and -90 (a grid with
pole rows has half cells there; the model's 720-row crop of the 721-row grid ends in a cell that reaches the south pole), so every grid
covers the sphere and no target cell is empty.  In longitude the bounds are 360 (i +- 1/2) / nlon, periodic.  The operator is separable:

    A[J, j]  = overlap of target cell J and source cell j in sin(lat) / the row's total
    Bm[I, i] = overlap in longitude modulo 360 / the row's total
    y = A x Bm^T

which is what WeatherBench 2 calls conservative regridding; that package is not a dependency and no number here was compared with it:
the operator is pinned by this definition and its invariants (rows sum to 1, constants map to constants, the area integral
sum area * x is conserved), as the spherical-harmonics transform is.  `area_weights` are that convention's latitude weights: the
sin(lat) extent of a cell, normalised to mean 1.

`Regridder` owns the band tables on a device: on CUDA fp32 tensors that need no gradient, with contiguous planes and W % 4 == 0, it
runs swv2_regrid (csrc/regrid.hip); everything else runs the dense statement `regrid_torch`.  Global grids only, first order only,
coarsening only in any useful sense (fine targets work but are piecewise constant).
"""
from __future__ import annotations

import numpy as np
import torch

BAND_CAP = 32                 # the K cap of swv2_regrid
_OFFSET_DEGREES = (5.625, 2.8125, 1.40625)        # WeatherBench 2's grids without pole rows


class LatLonGrid:
    """strictly descending latitude centres in degrees, nlon longitude centres at 360 i / nlon"""

    def __init__(self, lat_deg, nlon: int):
        lat = np.array(lat_deg, dtype=np.float64).reshape(-1)
        if lat.size < 1 or int(nlon) < 1 or np.any(np.diff(lat) >= 0) or lat[0] > 90.0 or lat[-1] < -90.0:
            raise ValueError("LatLonGrid: latitude centres must descend strictly within [90, -90] and nlon must be positive")
        self.lat, self.nlon = lat, int(nlon)

    nlat = property(lambda self: self.lat.size)
    shape = property(lambda self: (self.lat.size, self.nlon))
    poles = property(lambda self: bool(self.lat[0] == 90.0 and self.lat[-1] == -90.0))

    def rows(self, a: int, b: int) -> "LatLonGrid":
        """the grid of the rows a .. b - 1 (its outer cells then reach the poles)"""
        return LatLonGrid(self.lat[a:b], self.nlon)

    def lat_bounds(self) -> np.ndarray:
        """[nlat + 1] degrees, descending: +90, the midpoints, -90"""
        return np.concatenate(([90.0], 0.5 * (self.lat[:-1] + self.lat[1:]), [-90.0]))

    def sin_bounds(self) -> np.ndarray:
        s = np.sin(np.deg2rad(self.lat_bounds()))
        s[0], s[-1] = 1.0, -1.0
        return s

    def __eq__(self, other):
        return isinstance(other, LatLonGrid) and self.nlon == other.nlon and self.lat.shape == other.lat.shape and bool(np.all(self.lat == other.lat))

    __hash__ = None

    def __repr__(self):
        return f"LatLonGrid({self.nlat} x {self.nlon}, lat {self.lat[0]:g} .. {self.lat[-1]:g})"


def equiangular_grid(nlat: int, nlon: int, poles: bool = True) -> LatLonGrid:
    """centres 90 - 180 j / (nlat - 1) with pole rows, 90 - 180 (j + 1/2) / nlat without"""
    j = np.arange(int(nlat), dtype=np.float64)
    if poles and nlat < 2:
        raise ValueError("equiangular_grid: a grid with both poles has at least two rows")
    return LatLonGrid(90.0 - 180.0 * j / (nlat - 1) if poles else 90.0 - 180.0 * (j + 0.5) / nlat, nlon)


def model_grid(H: int, W: int) -> LatLonGrid:
    """the grid the model sees: the first H rows of the (H + 1)-row equiangular grid with both poles (720 of ERA5's 721 at 0.25 degrees)"""
    return equiangular_grid(H + 1, W).rows(0, H)


def grid_for_degrees(deg: float) -> LatLonGrid:
    """1.5 -> 121 x 240 with poles, 5.625 -> 32 x 64 without.  180 / deg must be an integer n; the poles are rows iff n is even and deg is
    none of WeatherBench 2's offset grids (5.625, 2.8125, 1.40625): then n + 1 rows, else n.  2 n columns."""
    deg = float(deg)
    if not (deg > 0 and np.isfinite(deg)):
        raise ValueError(f"grid_for_degrees: {deg} degrees")
    n = 180.0 / deg
    if abs(n - round(n)) > 1e-9 or round(n) < 1:
        raise ValueError(f"grid_for_degrees: 180 / {deg} is not an integer")
    n = int(round(n))
    poles = n % 2 == 0 and deg not in _OFFSET_DEGREES
    return equiangular_grid(n + 1 if poles else n, 2 * n, poles)


def _overlap(top_a, bot_a, top_b, bot_b):
    """[na, nb] overlap lengths of the intervals [bot, top]"""
    return np.minimum(top_a[:, None], top_b[None, :]) - np.maximum(bot_a[:, None], bot_b[None, :])


def conservative_weights(src: LatLonGrid, dst: LatLonGrid):
    """-> (A [Hd, H], Bm [Wd, W]) in fp64.  Which cells overlap is decided in degrees (two bounds closer than 1e-9 degrees are one
    bound: no sliver weights from rounding); how much, in sin(lat) and in degrees of longitude."""
    tol = 1e-9
    bs, bd, ss, sd = src.lat_bounds(), dst.lat_bounds(), src.sin_bounds(), dst.sin_bounds()
    touch = _overlap(bd[:-1], bd[1:], bs[:-1], bs[1:]) > tol
    A = np.where(touch, np.maximum(_overlap(sd[:-1], sd[1:], ss[:-1], ss[1:]), 0.0), 0.0)
    A /= A.sum(axis=1, keepdims=True)
    W, Wd = src.nlon, dst.nlon
    lo_s, hi_s = 360.0 * (np.arange(W) - 0.5) / W, 360.0 * (np.arange(W) + 0.5) / W
    lo_d, hi_d = 360.0 * (np.arange(Wd) - 0.5) / Wd, 360.0 * (np.arange(Wd) + 0.5) / Wd
    Bm = np.zeros((Wd, W))
    for shift in (-360.0, 0.0, 360.0):
        ov = _overlap(hi_d, lo_d, hi_s + shift, lo_s + shift)
        Bm += np.where(ov > tol, ov, 0.0)
    Bm /= Bm.sum(axis=1, keepdims=True)
    return A, Bm


def band_tables(M, cap: int = BAND_CAP, periodic: bool = True):
    """dense [n, W] -> (start int32 [n], count int32 [n], w float32 [n, K]), K the largest count: row r has its non-zeros at
    (start[r] + k) mod W, k < count[r]; the entries k >= count are 0 and are never to be multiplied in.  A row whose non-zeros are one
    linear run keeps it; otherwise the run is the cyclic one that leaves out the longest gap (the band of longitude 0 at 1440 -> 240 is
    the 7 columns from 1437), which periodic=False refuses.  Every entry inside a run must be non-zero, as in every overlap matrix: a
    zero there would be multiplied in and carry a NaN to a cell that does not depend on it.  ValueError: an empty row, a zero inside a
    run, a wrapped run with periodic=False, more than `cap` entries in a row."""
    M = np.asarray(M, dtype=np.float64)
    n, W = M.shape
    start, count = np.zeros(n, np.int32), np.zeros(n, np.int32)
    for r in range(n):
        nz = np.flatnonzero(M[r])
        if nz.size == 0:
            raise ValueError(f"band_tables: row {r} is empty")
        s, c = int(nz[0]), int(nz[-1] - nz[0] + 1)
        if c != nz.size and nz.size > 1:                                    # not one linear run: leave out the longest cyclic gap
            gaps = np.diff(np.concatenate((nz, [nz[0] + W])))
            g = int(np.argmax(gaps))
            if int(W - gaps[g] + 1) < c:
                if not periodic:
                    raise ValueError(f"band_tables: row {r} is not one run of columns")
                s, c = int(nz[(g + 1) % nz.size]), int(W - gaps[g] + 1)
        if c != nz.size:
            raise ValueError(f"band_tables: row {r} has zeros inside its run of {c} columns")
        if c > cap:
            raise ValueError(f"band_tables: row {r} needs {c} entries, the cap is {cap}")
        start[r], count[r] = s, c
    K = int(count.max())
    w = np.zeros((n, K), np.float32)
    for r in range(n):
        w[r, :count[r]] = M[r, (start[r] + np.arange(count[r])) % W]
    return start, count, w


def area_weights(grid: LatLonGrid) -> np.ndarray:
    """[nlat] fp32: the sin(lat) extent of each cell, normalised to mean 1 (WeatherBench 2's latitude weights), from fp64, rounded once"""
    a = -np.diff(grid.sin_bounds())
    return (a * (a.size / a.sum())).astype(np.float32)


def regrid_torch(x: torch.Tensor, A, Bm) -> torch.Tensor:
    """the statement in plain torch: [..., H, W] -> [..., Hd, Wd] = A x Bm^T, two matmuls in x's dtype on x's device; differentiable.
    Dense products spread a NaN over every target cell of its rows and columns (0 * NaN): Regridder masks instead."""
    A = torch.as_tensor(A).to(device=x.device, dtype=x.dtype)
    Bm = torch.as_tensor(Bm).to(device=x.device, dtype=x.dtype)
    return torch.matmul(torch.matmul(A, x), Bm.transpose(0, 1))


class Regridder:
    """src -> dst on one device.  Owns the band tables (int32 / fp32 device tensors), the dense fp64 matrices A, Bm and `area_weights`
    [Hd] fp32 of the target.  regridder(x, out=None): [..., H, W] -> [..., Hd, Wd].

    CUDA fp32 tensors on this device that need no gradient, with contiguous planes and W % 4 == 0, run swv2_regrid: [B, C, H, W] blocks
    (channel blocks of wider tensors included) in place, 5-D [M, B, C, H, W] as M B samples when the strides allow, else member by
    member.  Everything else -- CPU tensors, other dtypes, inputs that require grad, bands above the cap of 32 -- runs regrid_torch on
    cached dense matrices, with the kernel's NaN locality: non-finite source cells are taken out of the products and every target cell
    whose bands contain one is set to NaN (the kernel gives NaN or +-Inf there; no other cell differs).  src == dst returns the input."""

    def __init__(self, src: LatLonGrid, dst: LatLonGrid, device="cpu"):
        self.src, self.dst = src, dst
        self.device = torch.empty(0, device=device).device
        self.identity = src == dst
        self.A, self.Bm = conservative_weights(src, dst)
        self.area_weights = torch.from_numpy(area_weights(dst)).to(self.device)
        self._dense, self.tables = {}, None
        try:
            lat, lon = band_tables(self.A, BAND_CAP, periodic=False), band_tables(self.Bm, BAND_CAP)
        except ValueError:
            lat = lon = None                              # bands above the cap: the dense statement
        if lat is not None:
            # what the kernel trusts: 0 <= lat_start, lat_start + lat_count <= H; 0 <= lon_start < W, lon_count <= W
            assert lat[0].min() >= 0 and int((lat[0] + lat[1]).max()) <= src.nlat and lon[0].min() >= 0 and lon[0].max() < src.nlon \
                and lon[1].max() <= src.nlon
            self.band_counts = (lat[1].copy(), lon[1].copy())
            self.tables = tuple(torch.from_numpy(np.ascontiguousarray(t)).to(self.device) for t in lat + lon)

    def _matrices(self, dtype, device):
        key = (dtype, device)
        if key not in self._dense:
            self._dense[key] = (torch.from_numpy(self.A).to(device=device, dtype=dtype), torch.from_numpy(self.Bm).to(device=device, dtype=dtype))
        return self._dense[key]

    def _statement(self, x):
        dt = x.dtype if x.is_floating_point() else torch.float32
        A, Bm = self._matrices(dt, x.device)
        x = x.to(dt)
        bad = ~torch.isfinite(x)
        if not bool(bad.any()):
            return regrid_torch(x, A, Bm)
        y = regrid_torch(torch.where(bad, torch.zeros((), dtype=dt, device=x.device), x), A, Bm)
        hit = regrid_torch(bad.to(dt), (A != 0).to(dt), (Bm != 0).to(dt)) > 0
        return torch.where(hit, torch.full((), float("nan"), dtype=dt, device=x.device), y)

    def _on_kernel(self, x) -> bool:
        return (self.tables is not None and x.is_cuda and x.device == self.device and x.dtype == torch.float32 and x.shape[-1] % 4 == 0
                and x.numel() > 0 and not (x.requires_grad and torch.is_grad_enabled()))

    def __call__(self, x: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
        H, W = self.src.shape
        Hd, Wd = self.dst.shape
        if x.dim() < 2 or tuple(x.shape[-2:]) != (H, W):
            raise ValueError(f"Regridder: input {tuple(x.shape)}, expected [..., {H}, {W}]")
        shape = tuple(x.shape[:-2]) + (Hd, Wd)
        if out is not None and tuple(out.shape) != shape:
            raise ValueError(f"Regridder: out {tuple(out.shape)}, expected {shape}")
        if self.identity:
            return x if out is None else out.copy_(x)
        if not self._on_kernel(x):
            y = self._statement(x)
            return y if out is None else out.copy_(y)
        from .. import ops
        x4 = x[(None,) * (4 - x.dim())] if x.dim() < 4 else x            # (indexing with None: always a view)
        if x4.dim() > 5:
            x4 = x4.reshape((-1,) + tuple(x4.shape[-4:]))
        direct = out is not None and out.is_cuda and out.device == x.device and out.dtype == torch.float32 and \
            (out.dim() <= 5 or out.is_contiguous())
        y = out if direct else torch.empty(shape, dtype=torch.float32, device=x.device)
        y4 = y[(None,) * (4 - y.dim())] if y.dim() < 4 else y
        if y4.dim() > 5:
            y4 = y4.view((-1,) + tuple(y4.shape[-4:]))
        pairs = self._samples(x4, y4, ops)
        if pairs is None:                                  # planes that do not lie as the kernel reads or writes them
            r = self._statement(x)
            return r if out is None else out.copy_(r)
        for xs, ys in pairs:
            ops.regrid(xs, ys, *self.tables)
        return y if (out is None or direct) else out.copy_(y)

    @staticmethod
    def _samples(x4, y4, ops):
        """the [B, C, ., .] block pairs to launch on, or None"""
        if x4.dim() == 4:
            return [(x4, y4)] if ops.regrid_planes_ok(x4, True) and ops.regrid_planes_ok(y4, False) else None
        M, B = x4.shape[:2]
        if (M == 1 or x4.stride(0) == B * x4.stride(1)) and (M == 1 or y4.stride(0) == B * y4.stride(1)):
            xf, yf = x4.flatten(0, 1), y4.flatten(0, 1)              # views: the strides allow it
            if ops.regrid_planes_ok(xf, True) and ops.regrid_planes_ok(yf, False):
                return [(xf, yf)]
        pairs = [(x4[m], y4[m]) for m in range(M)]
        return pairs if all(ops.regrid_planes_ok(a, True) and ops.regrid_planes_ok(b, False) for a, b in pairs) else None
