"""fp64 numpy statement of the forecast scores as `swv2_score_sums` / `swv2_score_finalize` (csrc/score.hip) and
`utils/weighted_acc_rmse.ForecastScorer` define them, and the error bounds the tests hold the fp32 code to.  Shared by
tests/test_score_gpu.py and tests/test_score_host.py.

Everything is built from exactly what the kernels read: the fp32 prediction, truth, climatology and row weights, taken as exact.
    S_dd = sum w (p - t)^2    S_pt = sum w p' t'    S_pp = sum w p'^2    S_tt = sum w t'^2      p' = p - clim, t' = t - clim (or p, t)
    rmse = sqrt(S_dd / (H W))    acc = S_pt / sqrt(S_pp S_tt)    rmse_mean[c] = mean_b rmse[b, c] * scale[c]    acc_mean[c] = mean_b acc[b, c]

Bounds, u = 2^-24 (one fp32 rounding), g(k) = k u / (1 - k u) (the usual bound of k accumulated roundings).

Sums:  |S_k - S_k^ref| <= g(n + c) A_k,   A_k = sum |w| |a| |b| in fp64 (a, b the two fp64 factors of the term).
    |w|, not w: in fp32 cos(3.1416 / 180 * 90) < 0, both pole rows carry the weight -3.62e-6 (seen for H = 9 and H = 720), so the terms
    are not all of one sign and |S| can be smaller than the sum of their magnitudes.
    c = 4 per-term roundings, counted in score.hip's score_vec as written:
        S_dd  d = p - t: 1, entering twice = 2;  q d: 1;  the fma: 1                         = 4
        S_pt  p' = p - clim: 1;  t' = t - clim: 1;  q p': 1;  the fma: 1                      = 4   (2 without clim)
        S_pp  p': 1, entering twice = 2;  q p': 1;  the fma: 1                                = 4   (2 without clim)
        S_tt  as S_pp
    A subtraction of two exact fp32 values is off by u of the exact difference, so the relative statement holds against |p'|, |t'|, |d|
    themselves, however much cancels in them.
    n = chain_length(H, W, slices): the longest chain of fp32 additions a term passes through under the kernel's plan
        4 ceil(v / 256)    the thread's running sum: v 16-byte vectors in the largest slice, 256 threads, 4 fma per vector
        6                  wave64 butterfly
        2                  the four waves through LDS, (w0 + w1) + (w2 + w3)
        ceil(slices / 64)  swv2_score_finalize: lane l adds the slices l, l + 64, ... in ascending order
        6                  wave64 butterfly
    The plain-torch path (CPU tensors, odd widths) sums in an order this file does not know: n = H W, any order of a sum of H W terms.
    Its terms are formed as (w a) b or w (d^2) from the same rounded p', t', d: at most 4 roundings too.

RMSE:  with x = dS_dd / S_dd < 1:  |rmse - rmse^ref| <= rmse^ref ((1 - sqrt(1 - x)) + 2 u).  1 - sqrt(1 - x) = x / 2 + O(x^2) is the half
    relative bound on S_dd, taken on its larger (lower) side; the division by H W (exact in fp32 below 2^24, asserted) 1 rounding, halved
    by the root; the root 1: 1.5 u, held to 2 u.
ACC:   first order  dS_pt / sqrt(S_pp S_tt) + |ACC| (dS_pp / 2 S_pp + dS_tt / 2 S_tt) + 3 u |ACC|, stated without dropping the higher orders:
    with f = 1 / sqrt((1 - x_pp)(1 - x_tt)), x = dS / S:   (dS_pt f + |S_pt| (f - 1)) / sqrt(S_pp S_tt) + 3 u (|S_pt| + dS_pt) f / sqrt(S_pp S_tt).
    Final operations: the product S_pp S_tt 1 rounding, halved by the root; the root 1; the division 1: 2.5 u, held to 3 u.
    By Cauchy-Schwarz A_pt <= sqrt(A_pp A_tt), so the bound is finite for every plane with x_pp, x_tt < 1 (non-degenerate).
Batch means:  (B + 1) u sum_b |v_b| / B (x |scale|), judged from the kernel's OWN stored per-plane values so that no error is counted
    twice: B - 1 additions in ascending b, the division by B, the product with the scale.
"""
import math

import numpy as np

from tests.plane_reference import BLOCKS, U, gamma, plan_slices, slice_bounds, worst  # noqa: F401  (re-exported)

C_TERM = 4


def chain_length(H: int, W: int, slices: int) -> int:
    v = max((hi - lo) // 4 for lo, hi in slice_bounds(H * W, slices))
    return 4 * math.ceil(v / 256) + 6 + 2 + math.ceil(slices / 64) + 6


def latitude_weights(num_lat: int) -> np.ndarray:
    """the reference's weights in fp64 numpy -- NOT what the code under test uses (that is fp32, compared bit for bit against the torch
    formula in test_score_host.py); for tests that only need weights of the right shape and sign pattern"""
    j = np.arange(num_lat, dtype=np.float64)
    c = np.cos(3.1416 / 180.0 * (90.0 - j * 180.0 / max(num_lat - 1, 1)))
    return (num_lat * c / c.sum()).astype(np.float32)


def sums(prd, tar, w, clim=None):
    """fp32 arrays [B, C, H, W] x2, [H], [C, H, W] | None -> (S [B, C, 4], A [B, C, 4]) in fp64: the sums and the sums of magnitudes"""
    p, t, q = prd.astype(np.float64), tar.astype(np.float64), w.astype(np.float64).reshape(1, 1, -1, 1)
    d = p - t
    pa, ta = (p, t) if clim is None else (p - clim.astype(np.float64)[None], t - clim.astype(np.float64)[None])
    pairs = ((d, d), (pa, ta), (pa, pa), (ta, ta))
    S = np.stack([(q * a * b).sum(axis=(2, 3)) for a, b in pairs], axis=-1)
    A = np.stack([(np.abs(q) * np.abs(a) * np.abs(b)).sum(axis=(2, 3)) for a, b in pairs], axis=-1)
    return S, A


def sum_bounds(A, n: int):
    return gamma(n + C_TERM) * A


def rmse(S, dS, H: int, W: int):
    """-> (rmse [B, C], bound [B, C]) from the reference sums and their bounds"""
    assert H * W < 2 ** 24
    x = dS[..., 0] / S[..., 0]
    assert np.all((x >= 0) & (x < 1)), "degenerate plane: S_dd is not above its own error bound"
    r = np.sqrt(S[..., 0] / (H * W))
    return r, r * ((1.0 - np.sqrt(1.0 - x)) + 2 * U)


def acc(S, dS):
    """-> (acc [B, C], bound [B, C]); a plane with S_pp = 0 or S_tt = 0 gives (nan, nan)"""
    with np.errstate(invalid="ignore", divide="ignore"):
        den = np.sqrt(S[..., 2] * S[..., 3])
        a = S[..., 1] / den
        xp, xt = dS[..., 2] / S[..., 2], dS[..., 3] / S[..., 3]
        ok = np.isfinite(a)
        assert np.all((xp[ok] < 1) & (xt[ok] < 1)), "degenerate plane: S_pp / S_tt not above their own error bounds"
        f = 1.0 / np.sqrt((1.0 - xp) * (1.0 - xt))
        b = (dS[..., 1] * f + np.abs(S[..., 1]) * (f - 1.0)) / den + 3 * U * (np.abs(S[..., 1]) + dS[..., 1]) * f / den
    return a, b


def batch_mean(v, scale=None):
    """v [B, C]: the code's OWN fp32 per-plane values -> (mean [C], bound [C]) in fp64"""
    v = v.astype(np.float64)
    B = v.shape[0]
    s = 1.0 if scale is None else scale.astype(np.float64)
    return v.mean(axis=0) * s, gamma(B + 1) * np.abs(v).sum(axis=0) / B * np.abs(s)


def judge(got_sums, got_rmse, got_acc, prd, tar, w, clim, n: int, tag=""):
    """element-by-element verdict on a finalize result (numpy fp32 arrays) against the fp64 statement; prints the worst ratios and
    returns them (sums, rmse, acc); NaN is required exactly where the reference has it"""
    B, C, H, W = prd.shape
    S, A = sums(prd, tar, w, clim)
    dS = sum_bounds(A, n)
    rs = worst(np.abs(got_sums.astype(np.float64) - S), dS)
    r_ref, r_b = rmse(S, dS, H, W)
    rr = worst(np.abs(got_rmse.astype(np.float64) - r_ref), r_b)
    a_ref, a_b = acc(S, dS)
    nan = np.isnan(a_ref)
    assert np.array_equal(np.isnan(got_acc), nan), "NaN ACC in other planes than the reference's"
    ra = worst(np.abs(got_acc.astype(np.float64) - a_ref)[~nan], a_b[~nan])
    print(f"{tag} n = {n}: worst error / bound  sums {rs:.3f}  rmse {rr:.3f}  acc {ra:.3f}")
    return rs, rr, ra
