"""fp64 numpy statement of first-order conservative regridding between global lat-lon grids, as `swv2_regrid` (csrc/regrid.hip) and
`utils/regrid.py` define it, and the error bounds the tests hold the fp32 code to.  Shared by tests/test_regrid_gpu.py and
tests/test_regrid_host.py.  Independent of utils/regrid.py: the matrices are built here from the definition, cell by cell, the longitude
overlaps in exact integer arithmetic.

Grids.  A grid is its descending latitude centres (degrees) and nlon; `centres(nlat, poles)` gives 90 - 180 j / (nlat - 1) or
90 - 180 (j + 1/2) / nlat.  Latitude bounds: +90, the midpoints of neighbouring centres, -90.  Longitude cell i: 360 (i +- 1/2) / nlon.
    A[J, j]  = (sin of the overlap's top - sin of its bottom) / the row's total         overlaps below 1e-9 degrees are none
    Bm[I, i] = overlap modulo 360 / the row's total; in units of 360 / (2 W Wd) degrees source cell i is [(2 i - 1) Wd, (2 i + 1) Wd)
               and target cell I is [(2 I - 1) W, (2 I + 1) W): integers, so the overlap is exact
    y = A x Bm^T        area[J] = sin extent of cell J, normalised to mean 1

Bounds, u = 2^-24.  The kernel reads the fp32 tables (start, count, weights) and computes, with cl = lat_count[J], cn = lon_count[I],
    r[J][i] = fma chain over k < cl from zero,   y[J][I] = fma chain over k < cn from zero.
A term a32[J, j] b32[I, i] x[j, i] (exact product of three fp32 numbers) is rounded once per fma it passes through: at most cl in the
first chain (it enters at some k and every later fma of the chain rounds the sum that holds it; the fma that brings it in rounds too)
and at most cn in the second.  So, with a32, b32 the fp32 table weights taken as exact,
    |got - sum a32 b32 x| <= ((1 + u)^(cl + cn) - 1) sum |a32| |b32| |x| <= (cl + cn + 2) u sum |a32| |b32| |x|
((1 + u)^n - 1 <= n u / (1 - n u) and n <= 64: the second-order part is below 4e-6 n u, far inside the 2 u of slack).  That is
`kernel_bound`.  The statement with fp64 weights differs from the one with the rounded weights by at most
    ((1 + u)^2 - 1) sum |a| |b| |x|        (|a32 - a| <= u |a|, |b32 - b| <= u |b|)
which is `weight_bound`, stated separately: `judge` compares with the fp64-weight statement and allows the sum of the two.
The torch paths (two matmuls in an order this file does not know) are held to the same form with the chain lengths H and W:
any order of a sum of n terms rounds a term at most n times.
"""
import numpy as np

from tests.plane_reference import U, worst  # noqa: F401  (re-exported)


def centres(nlat: int, poles: bool = True) -> np.ndarray:
    j = np.arange(nlat, dtype=np.float64)
    return 90.0 - 180.0 * j / (nlat - 1) if poles else 90.0 - 180.0 * (j + 0.5) / nlat


def lat_bounds(lat) -> np.ndarray:
    lat = np.asarray(lat, dtype=np.float64)
    return np.concatenate(([90.0], 0.5 * (lat[:-1] + lat[1:]), [-90.0]))


def _sin_deg(d: float) -> float:
    return 1.0 if d >= 90.0 else (-1.0 if d <= -90.0 else float(np.sin(np.deg2rad(d))))


def lat_matrix(src_lat, dst_lat) -> np.ndarray:
    bs, bd = lat_bounds(src_lat), lat_bounds(dst_lat)
    A = np.zeros((len(dst_lat), len(src_lat)))
    for J in range(len(dst_lat)):
        for j in range(len(src_lat)):
            top, bot = min(bd[J], bs[j]), max(bd[J + 1], bs[j + 1])
            if top - bot > 1e-9:
                A[J, j] = _sin_deg(top) - _sin_deg(bot)
        A[J] /= A[J].sum()
    return A


def lon_matrix(W: int, Wd: int) -> np.ndarray:
    Bm = np.zeros((Wd, W))
    for I in range(Wd):
        lo_d, hi_d = (2 * I - 1) * W, (2 * I + 1) * W
        # the unwrapped source cells that can touch [lo_d, hi_d): cell i is [(2 i - 1) Wd, (2 i + 1) Wd); column i mod W
        for i in range(lo_d // (2 * Wd) - 1, hi_d // (2 * Wd) + 2):
            ov = min(hi_d, (2 * i + 1) * Wd) - max(lo_d, (2 * i - 1) * Wd)
            if ov > 0:
                Bm[I, i % W] += ov
        assert Bm[I].sum() == 2 * W                           # the target cell is covered exactly once
        Bm[I] /= Bm[I].sum()
    return Bm


def area(lat) -> np.ndarray:
    """[nlat] fp64: sin extent of each cell, mean 1"""
    b = lat_bounds(lat)
    a = np.array([_sin_deg(b[j]) - _sin_deg(b[j + 1]) for j in range(len(lat))])
    return a * (a.size / a.sum())


def regrid(x, A, Bm):
    """[..., H, W] -> [..., Hd, Wd] in fp64"""
    return np.matmul(np.matmul(A, np.asarray(x, dtype=np.float64)), Bm.T)


def counts(M) -> np.ndarray:
    """[n] the length of each row's band: the shortest cyclic run of columns that holds its non-zeros"""
    n, W = M.shape
    out = np.zeros(n, np.int64)
    for r in range(n):
        nz = np.flatnonzero(M[r])
        gaps = np.diff(np.concatenate((nz, [nz[0] + W])))
        out[r] = W - gaps.max() + 1
    return out


def dense_from_tables(start, count, w, W: int) -> np.ndarray:
    """the fp32 tables back as a dense fp64 matrix [n, W]"""
    M = np.zeros((len(start), W))
    for r in range(len(start)):
        for k in range(int(count[r])):
            M[r, (int(start[r]) + k) % W] += float(w[r, k])
    return M


def kernel_bound(x, A32, B32, cl, cn):
    """[..., Hd, Wd]: (cl[J] + cn[I] + 2) u sum |a32| |b32| |x|"""
    mag = regrid(np.abs(np.asarray(x, dtype=np.float64)), np.abs(A32), np.abs(B32))
    return (np.asarray(cl, dtype=np.float64)[:, None] + np.asarray(cn, dtype=np.float64)[None, :] + 2.0) * U * mag


def weight_bound(x, A, Bm):
    return ((1.0 + U) ** 2 - 1.0) * regrid(np.abs(np.asarray(x, dtype=np.float64)), np.abs(A), np.abs(Bm))


def judge(got, x, A, Bm, cl, cn, tag="", finite_only=None):
    """element-by-element verdict on got [..., Hd, Wd] (numpy fp32) against the fp64-weight statement of the fp32 input x; cl [Hd], cn [Wd]
    the chain lengths.  finite_only: a boolean mask of the outputs to judge (default all).  Prints and returns the worst error / bound."""
    A32, B32 = A.astype(np.float32).astype(np.float64), Bm.astype(np.float32).astype(np.float64)
    ref = regrid(x, A, Bm)
    bound = kernel_bound(x, A32, B32, cl, cn) + weight_bound(x, A, Bm)
    err = np.abs(got.astype(np.float64) - ref)
    if finite_only is not None:
        err, bound = err[finite_only], bound[finite_only]
    r = worst(err, bound)
    print(f"{tag}: worst error / bound {r:.3f}")
    return r
