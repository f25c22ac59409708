"""fp64 numpy statement of the ensemble scores as `swv2_ens_sums` / `swv2_ens_finalize` (csrc/ensemble.hip) and
`utils/weighted_acc_rmse.ensemble_scores_torch` define them, and the error bounds the tests hold the fp32 code to.  Shared by
tests/test_ensemble_gpu.py and tests/test_ensemble_host.py.  Nothing here is tuned to what the code under test returns.

Everything is built from exactly what the kernels read: the fp32 members x_m [M, B, C, H, W], truth y [B, C, H, W] and row weights w [H],
taken as exact.  Per grid point
    xbar = (1 / M) sum_m x_m     s2 = (1 / (M - 1)) sum_m (x_m - xbar)^2   (two passes)     e = xbar - y
    e1 = sum_m |x_m - y|         e2 = sum_{m<n} |x_m - x_n|   (the plain pairwise sum)     rank = #{m : x_m < y}   (fp32 compare, strict)
per plane, N = H W
    S_mse = sum w e^2    S_var = sum w s2    S_1 = sum w e1    S_2 = sum w e2    hist[r] = #{points of rank r}
    ens_rmse = sqrt(S_mse / N)   spread = sqrt(S_var / N)   crps = (S_1 / M - S_2 / M^2) / N   fair_crps = (S_1 / M - S_2 / (M (M - 1))) / N

Bounds, u = 2^-24, g(k) = k u / (1 - k u).  They follow the operations as csrc/ensemble.hip documents them (ensemble_scores_torch forms the
same per-point quantities from the same differences); |w|, not w: the pole rows of the fp32 latitude weights are negative (tests/score_reference.py).
n is the number of fp32 additions a term passes through on its way into the plane's sum (chain_length for the kernel's plan; H W M, any
order, for the torch path).

  S_1    e1 is a sum of M non-negative terms |x_m - y|, each one rounding, M - 1 additions: g(M) e1.  The fma with w and the chain: n + 1.
         |S_1 - ref| <= g(n + M + 1) A_1,  A_1 = sum |w| e1.
  S_2    the code sums the gaps of the sorted members, i (M - i) (x_(i+1) - x_(i)), i = 1 .. M - 1: sorting is exact (min / max), the
         coefficients are exact integers, each gap one rounding, M - 1 fused (or multiply-then-add: at most one more rounding, absorbed in
         the + 2) accumulations of non-negative terms.   |S_2 - ref| <= g(n + M + 2) A_2,  A_2 = sum |w| e2.
  abar   with a_m = x_m - x_0: abar^ = fl(fl(sum_m fl(a_m)) fl(1 / M)): one rounding per a_m, M - 2 additions, the reciprocal, the product:
         |abar^ - abar| <= dab = g(M + 1) sum_m |a_m| / M.
  S_var  v_m = a_m - abar (= x_m - xbar): |v_m^ - v_m| <= dv_m = (u |a_m| + dab) (1 + u) + u |v_m|.   sum_m v_m^2 through M accumulations:
         |vv^ - vv| <= Evv = E + g(M + 1) (vv + E),  E = sum_m (2 |v_m| dv_m + dv_m^2).  Then w vv through the chain (n + 1) and ONE division by
         M - 1 per plane:   |S_var - ref| <= (g(n + 2) sum |w| vv + (1 + g(n + 2)) sum |w| Evv) / (M - 1).
  S_mse  e^ = fl(fl(x_0 - y) + abar^):  |e^ - e| <= de = (u |x_0 - y| + dab) (1 + u) + u |e|.   w e^ one rounding, the fma and the chain n + 1:
         |S_mse - ref| <= g(n + 2) sum |w| e^2 + (1 + g(n + 2)) sum |w| (2 |e| de + de^2).
  Every bound is relative to a sum of non-negative quantities made of DIFFERENCES of the inputs: adding 1e4 to every field changes none of
  them by more than the roundings of the differences.  A code that formed e2 from sum_i (2 i - M - 1) x_(i), or the variance from
  sum x^2 - M xbar^2, would miss them at once there.
  ens_rmse, spread   sqrt((S +- dS) / N) around the reference, plus 2 u for the division (N < 2^24 exact) and the root.
  crps, fair_crps    a difference of two sums: absolute, (dS_1 / M + dS_2 / M^2) / N + 4 u ((|S_1| + dS_1) / M + (|S_2| + dS_2) / M^2) / N
         (each sum passes through its division, the subtraction -- relative to the difference, which is below the sum -- and the division
         by N: 3 roundings, held to 4 u); M (M - 1) for the fair form.
  NaN    a NaN in any member or in the truth of a plane makes all four scores of that plane NaN (the spread too, which the truth does not
         enter otherwise) and that channel's batch means; no other plane is touched; the plane's hist still adds up to N.
  Batch means   tests/score_reference.py::batch_mean, judged from the code's own stored per-plane values.
"""
import math

import numpy as np

from tests.plane_reference import U, gamma, plan_slices, slice_bounds, worst  # noqa: F401  (re-exported)
from tests.score_reference import batch_mean  # noqa: F401  (re-exported)

CAPACITIES = (8, 16, 32, 64)
CHUNK = 128
POINTS = {8: 4, 16: 4, 32: 1, 64: 1}          # grid points per thread and iteration at each member capacity (csrc/ensemble.hip)


def capacity(M: int) -> int:
    assert 2 <= M <= 64
    return next(c for c in CAPACITIES if M <= c)


def chain_length(H: int, W: int, slices: int, M: int) -> int:
    """the longest chain of fp32 additions a term passes through under the plan of csrc/ensemble.hip"""
    pts = POINTS[capacity(M)]
    g = max((hi - lo) // pts for lo, hi in slice_bounds(H * W, slices))
    return pts * math.ceil(g / 256) + 6 + 2 + math.ceil(slices / 64) + 6


def pairwise_e2(x):
    """x [M, ...] fp64 -> sum_{m<n} |x_m - x_n|, the plain pairwise sum"""
    out = np.zeros(x.shape[1:], np.float64)
    for m in range(x.shape[0] - 1):
        out += np.abs(x[m + 1:] - x[m]).sum(axis=0)
    return out


def gap_e2(x):
    """the same number from the gaps of the sorted members (the identity the kernel relies on; checked in tests/test_ensemble_host.py)"""
    M = x.shape[0]
    s = np.sort(x, axis=0)
    i = np.arange(1, M, dtype=np.float64).reshape((-1,) + (1,) * (x.ndim - 1))
    return (i * (M - i) * np.diff(s, axis=0)).sum(axis=0)


def point_terms(ens, tar):
    """fp32 arrays [M, B, C, H, W], [B, C, H, W] -> dict of fp64 [B, C, H, W] arrays: e, vv = sum_m (x_m - xbar)^2, e1, e2, the integer rank,
    and what the bounds need: |x_0 - y|, sum_m |a_m| / M, Evv-ingredients"""
    M = ens.shape[0]
    x, y = ens.astype(np.float64), tar.astype(np.float64)
    with np.errstate(invalid="ignore"):
        xbar = x.mean(axis=0)
        v = x - xbar
        a = x - x[0]
        t = dict(e=xbar - y, vv=(v * v).sum(axis=0), e1=np.abs(x - y).sum(axis=0), e2=pairwise_e2(x), rank=(ens < tar[None]).sum(axis=0),
                 d0=np.abs(x[0] - y))
        dab = gamma(M + 1) * np.abs(a).sum(axis=0) / M
        dv = (U * np.abs(a) + dab) * (1 + U) + U * np.abs(v)
        E = (2 * np.abs(v) * dv + dv * dv).sum(axis=0)
        t["Evv"] = E + gamma(M + 1) * (t["vv"] + E)
        de = (U * t["d0"] + dab) * (1 + U) + U * np.abs(t["e"])
        t["Emse"] = 2 * np.abs(t["e"]) * de + de * de
    return t


def sums(ens, tar, w, n: int):
    """-> (S [B, C, 4] = (S_mse, S_var, S_1, S_2), dS [B, C, 4]: the bounds above for a chain of n additions, hist [B, C, M + 1] int64)"""
    M, B, C, H, W = ens.shape
    if C > CHUNK:                                  # channel blocks: the fp64 temporaries are M-sized
        parts = [sums(ens[:, :, c:c + CHUNK], tar[:, c:c + CHUNK], w, n) for c in range(0, C, CHUNK)]
        return tuple(np.concatenate([p[k] for p in parts], axis=1) for k in range(3))
    t = point_terms(ens, tar)
    q = w.astype(np.float64).reshape(1, 1, -1, 1)
    aq = np.abs(q)

    def ws(f, weight=q):
        return (weight * f).sum(axis=(2, 3))
    S = np.stack([ws(t["e"] ** 2), ws(t["vv"]) / (M - 1), ws(t["e1"]), ws(t["e2"])], axis=-1)
    dS = np.stack([gamma(n + 2) * ws(t["e"] ** 2, aq) + (1 + gamma(n + 2)) * ws(t["Emse"], aq),
                   (gamma(n + 2) * ws(t["vv"], aq) + (1 + gamma(n + 2)) * ws(t["Evv"], aq)) / (M - 1),
                   gamma(n + M + 1) * ws(t["e1"], aq), gamma(n + M + 2) * ws(t["e2"], aq)], axis=-1)
    rank = t["rank"].reshape(B, C, H * W)
    hist = np.stack([(rank == r).sum(axis=-1) for r in range(M + 1)], axis=-1)
    return S, dS, hist


def root_score(S, dS, N: int):
    """sqrt(S / N) and its bound from S +- dS"""
    assert N < 2 ** 24
    with np.errstate(invalid="ignore"):
        r = np.sqrt(S / N)
        hi, lo = np.sqrt((S + dS) / N), np.sqrt(np.maximum(S - dS, 0.0) / N)
        return r, np.maximum(hi - r, r - lo) + 2 * U * hi


def crps_score(S, dS, M: int, N: int, fair: bool):
    den = float(M * (M - 1)) if fair else float(M * M)
    c = (S[..., 2] / M - S[..., 3] / den) / N
    b = (dS[..., 2] / M + dS[..., 3] / den) / N + 4 * U * ((np.abs(S[..., 2]) + dS[..., 2]) / M + (np.abs(S[..., 3]) + dS[..., 3]) / den) / N
    return c, b


def scores(S, dS, M: int, N: int):
    """-> {name: (reference [B, C], bound [B, C])} of the four finalised scores"""
    return {"ens_rmse": root_score(S[..., 0], dS[..., 0], N), "spread": root_score(S[..., 1], dS[..., 1], N),
            "crps": crps_score(S, dS, M, N, False), "fair_crps": crps_score(S, dS, M, N, True)}


NAMES = ("ens_rmse", "spread", "crps", "fair_crps")


def judge(got, ens, tar, w, n: int, scale=None, tag="", ref=None):
    """element-by-element verdict on one result.  got: dict of numpy arrays sums [B, C, 4], hist [B, C, M + 1], the four scores [B, C] and
    means [4, C].  Prints the worst error / bound ratios, asserts every bound, hist exactly (in planes without a NaN; every plane's hist
    must add up to N) and NaN exactly where the reference has it.  ref: a (S, dS, hist) computed before for the same inputs and n."""
    M, B, C, H, W = ens.shape
    N = H * W
    S, dS, hist = sums(ens, tar, w, n) if ref is None else ref
    nan = np.isnan(S).any(axis=-1)
    assert got["hist"].shape == hist.shape and np.all(got["hist"].sum(axis=-1) == N), "a rank histogram does not add up to N"
    assert np.array_equal(got["hist"][~nan], hist[~nan]), "rank histogram differs from the strict-compare statement"
    ratios = {}
    assert not np.isnan(got["sums"][~nan]).any(), "NaN sums in a plane without NaN inputs"
    ratios["sums"] = [worst(np.abs(got["sums"][..., k].astype(np.float64) - S[..., k])[~nan], dS[..., k][~nan]) for k in range(4)]
    sc = scores(S, dS, M, N)
    for name in NAMES:
        r, b = sc[name]
        assert np.array_equal(np.isnan(got[name]), nan), f"{name}: NaN in other planes than the reference's"
        ratios[name] = worst(np.abs(got[name].astype(np.float64) - r)[~nan], b[~nan])
    nanc = nan.any(axis=0)
    ratios["means"] = []
    for k, name in enumerate(NAMES):
        m_ref, m_b = batch_mean(got[name], scale if k < 3 else None)
        assert np.array_equal(np.isnan(got["means"][k]), nanc), f"{name} mean: NaN in other channels than the reference's"
        ratios["means"].append(worst(np.abs(got["means"][k].astype(np.float64) - m_ref)[~nanc], m_b[~nanc]))
    print(f"{tag} n = {n}: worst error / bound  sums " + " ".join(f"{v:.3f}" for v in ratios["sums"]) + "  scores " +
          " ".join(f"{ratios[k]:.3f}" for k in NAMES) + "  means " + " ".join(f"{v:.3f}" for v in ratios["means"]))
    worst_all = max(ratios["sums"] + [ratios[k] for k in NAMES] + ratios["means"])
    assert worst_all <= 1.0, f"{tag}: outside the derived bounds: {ratios}"
    return ratios
