"""The statement of the dataset statistics (utils/dataset_stats.py, csrc/stats.hip) in numpy, two-pass and in np.longdouble (fp64 where
the platform has nothing wider), the mirror of the kernels' plan, and the error bounds the tests hold the code to.  Shared by
tests/test_dataset_stats_host.py and tests/test_dataset_stats_gpu.py.

Statement.  Year files y of N_y slabs x[y, t, c, i, j] (fp32, taken as exact), T = sum N_y, N = T H W, N_d = sum (N_y - 1) H W:
    global_means[c] = sum x / N                       global_stds[c] = sqrt(sum (x - global_means[c])^2 / N)
    time_means[c, i, j] = sum_{y, t} x / T            d[y, t] = x[y, t + 1] - x[y, t] (t < N_y - 1, inside a file only)
    time_diff_stds[c] = sqrt(sum (d - mean d)^2 / N_d)

State.  The code keeps one-pass shifted sums in fp64, with a pivot p[c] (an fp32 value) and x' = x - p[c]:
    folded[c] = (sum x', sum x'^2, sum d, sum d^2, number of non-finite x, 0)        tsum[c, i, j] = sum_{y, t} x'
The reference forms x' and d in fp64 (each a difference of two fp32 values: exact unless their exponents lie more than 29 apart) and
squares and sums them in np.longdouble.

Bounds, u = 2^-53 (one fp64 rounding), g(k) = k u / (1 - k u).
  State:  |S - S_ref| <= g(n + c) A,  A = the sum of the magnitudes of the terms (sum |x'|, sum x'^2, sum |d|, sum d^2; sum_t |x'| for tsum).
    c = 2 per-term roundings at the most: x' (or d) 1 -- 0 whenever the difference is exact -- entering a square twice; the product
    itself is not rounded in the kernel (fma) and once in numpy, which forms x' x' before it sums: 2 covers both for the sums of the
    values, and the numpy path gets c = 3.
    n = chain_length(H, W, slices, T): the longest chain of fp64 additions a term passes through under the kernels' plan
        4 ceil(v / 256)    the thread's running sum: v 16-byte vectors in the largest slice, 256 threads, 4 elements per vector
        6                  wave64 butterfly
        2                  the four waves through LDS, (w0 + w1) + (w2 + w3)
        T                  part[c][slice] += the slab's slice sum, once per slab
        ceil(slices / 64)  swv2_stats_finalize: lane l adds the slices l, l + 64, ... in ascending order
        6                  wave64 butterfly
    tsum: T additions per element, one per slab: n = T.
    The numpy path (device cpu) sums a plane in an order this file does not know, then adds the slabs: n = H W + T, any order.
    Merged states add the per-file sums once more: + the number of states.
  Written fp32 values: at most 1 fp32 ulp from the statement rounded to fp32.  The fp64 arithmetic behind them is good to ~1e-15
    relative, 8 orders below an fp32 ulp, so the two roundings to fp32 differ only when the exact value sits on a rounding boundary: the
    values agree to 0 ulp in practice and the one ulp allows for that boundary.
"""
import functools
import math

import numpy as np

from tests import plane_reference as P
from tests.plane_reference import BLOCKS, plan_slices, slice_bounds, worst  # noqa: F401  (re-exported)

U = 2.0 ** -53         # the sums are fp64
C_TERM = 2
LD = np.longdouble

# (C, H, W) -> T: the smallest shapes that reach each branch of the plan
SHAPES = {(1, 1, 4): 3,            # a single vector: 2047 empty slices
          (3, 5, 8): 5,            # 682 slices per channel over 10 vectors, cutting rows
          (2, 33, 132): 4,         # 4356 elements over 1024 slices: most of them empty or a single vector
          (73, 16, 32): 3,         # the production channel count: 28 slices over 128 vectors, a count the 16 rows do not divide
          (1024, 49, 104): 2,      # 2 slices of 2548 elements: one pass of the 2 x unrolled main loop (2048 elements) + a tail for
                                   # threads 0 .. 124
          (2, 721, 1440): 2}       # the real plane, odd row count, index width; 1024 slices of ~1013 elements: tail loop only


def gamma(k: float) -> float:
    return P.gamma(k, U)


def chain_length(H: int, W: int, slices: int, T: int) -> int:
    v = max((hi - lo) // 4 for lo, hi in slice_bounds(H * W, slices))
    return 4 * math.ceil(v / 256) + 6 + 2 + T + math.ceil(slices / 64) + 6


def chain_any_order(H: int, W: int, T: int) -> int:
    return H * W + T


def make_years(C: int, H: int, W: int, counts, seed: int = 0, jump: float = 0.0):
    """one fp32 array [N_y, C, H, W] per entry of `counts`: a smooth field that drifts in time plus noise; channel c % 3 == 0 is
    geopotential-like (offset 2e5, std ~3e3: the one an fp32 accumulator fails on), c % 3 == 1 sits near 280 +- 15, c % 3 == 2 is
    N(0, 1).  jump: a constant added to every slab of file k, k times (a file boundary the differences must not cross)."""
    rng = np.random.default_rng(seed * 7919 + C * 31 + H * 17 + W)
    y, x = np.linspace(0, np.pi, H)[:, None], np.linspace(0, 2 * np.pi, W)[None, :]
    kind = np.arange(C) % 3
    off = np.choose(kind, [2.0e5, 280.0, 0.0])[:, None, None]
    scl = np.choose(kind, [3.0e3, 15.0, 1.0])[:, None, None]
    out, t0 = [], 0
    for k, n in enumerate(counts):
        a = np.empty((n, C, H, W), np.float32)
        for t in range(n):
            smooth = np.sin(y + 0.3 * np.arange(C)[:, None, None] + 0.2 * (t0 + t)) * np.cos(2 * x)
            a[t] = (off + scl * (0.8 * smooth + 0.6 * rng.standard_normal((C, H, W))) + jump * k).astype(np.float32)
        t0 += n
        a.setflags(write=False)
        out.append(a)
    return out


@functools.lru_cache(maxsize=None)
def case(C: int, H: int, W: int, T: int):
    """the one-file input of a shape of SHAPES, its pivot (the rule of utils/dataset_stats.py::pivot_of, restated) and its references;
    computed once per shape and never modified"""
    years = make_years(C, H, W, (T,))
    pivot = years[0][0].astype(np.float64).mean(axis=(1, 2)).astype(np.float32).astype(np.float64)
    return years, pivot, statement(years), state(years, pivot)


def statement(years):
    """the four statistics of the statement, two-pass, in LD: dict of global_means [C], global_stds [C], time_diff_stds [C],
    time_means [C, H, W]"""
    C = years[0].shape[1]
    T = sum(a.shape[0] for a in years)
    gm, gs, td, tm = np.empty(C, LD), np.empty(C, LD), np.empty(C, LD), np.empty((C,) + years[0].shape[2:], LD)
    for c in range(C):                                                  # a channel at a time: LD temporaries stay small
        X = np.concatenate([a[:, c] for a in years]).astype(LD)
        gm[c] = X.sum() / X.size
        gs[c] = np.sqrt(((X - gm[c]) ** 2).sum() / X.size)
        tm[c] = X.sum(axis=0) / T
        D = np.concatenate([a[1:, c].astype(LD) - a[:-1, c].astype(LD) for a in years])
        if D.size:
            td[c] = np.sqrt(((D - D.sum() / D.size) ** 2).sum() / D.size)
        else:
            td[c] = np.nan
    return dict(global_means=gm, global_stds=gs, time_diff_stds=td, time_means=tm)


def state(years, pivot):
    """the shifted sums the code keeps and the sums of the magnitudes of their terms, in LD:
    (folded [C, 4], A [C, 4], tsum [C, H, W], A_tsum [C, H, W])"""
    C = years[0].shape[1]
    S, A = np.zeros((C, 4), LD), np.zeros((C, 4), LD)
    ts, At = np.empty((C,) + years[0].shape[2:], LD), np.empty((C,) + years[0].shape[2:], LD)
    for c in range(C):
        xs = (np.concatenate([a[:, c] for a in years]).astype(np.float64) - pivot[c]).astype(LD)
        D = np.concatenate([a[1:, c].astype(np.float64) - a[:-1, c].astype(np.float64) for a in years]).astype(LD)
        S[c] = xs.sum(), (xs * xs).sum(), D.sum(), (D * D).sum()
        A[c] = np.abs(xs).sum(), (xs * xs).sum(), np.abs(D).sum(), (D * D).sum()
        ts[c], At[c] = xs.sum(axis=0), np.abs(xs).sum(axis=0)
    return S, A, ts, At


def judge_state(folded, tsum, ref_state, n: int, T: int, c_term: int = C_TERM, tag=""):
    """got folded [C, 6] and tsum [C, H, W] (fp64) against the reference state with chain length n; prints and returns the worst
    error / bound ratios (sums, tsum).  The non-finite count and the spare must be exactly 0."""
    S, A, ts, At = ref_state
    assert folded.dtype == np.float64 and tsum.dtype == np.float64
    rs = worst(np.abs(folded[:, :4].astype(LD) - S), gamma(n + c_term) * A)
    rt = worst(np.abs(tsum.astype(LD) - ts), gamma(T + 1) * At)
    print(f"{tag} n = {n}: worst error / bound  folded {rs:.3f}  tsum {rt:.3f}")
    assert np.all(folded[:, 4:] == 0.0)
    return rs, rt


def ulps(got, ref) -> float:
    """largest distance of the fp32 array `got` from `ref` (LD) rounded to fp32, in fp32 ulps of that rounded value"""
    got = np.asarray(got)
    assert got.dtype == np.float32
    r32 = np.asarray(ref).astype(np.float32).reshape(got.shape)
    assert np.all(np.isfinite(got)) and np.all(np.isfinite(r32))
    d = np.abs(got.astype(np.float64) - r32.astype(np.float64)) / np.spacing(np.abs(r32)).astype(np.float64)
    return float(d.max())


def judge_written(got: dict, ref: dict, tag=""):
    """the four written arrays ([1, C, 1, 1] x3, [1, C, H, W]) against the statement: prints and returns the worst ulp distances"""
    r = {k: ulps(got[k], ref[k]) for k in ("global_means", "global_stds", "time_diff_stds", "time_means")}
    print(f"{tag} fp32 ulps from the statement: " + "  ".join(f"{k} {v:.0f}" for k, v in r.items()))
    return r
