"""fp64 / int64 numpy statement of the forecast-event sums as `swv2_event_*` / `swv2_event_ens_*` (csrc/events.hip) and
`utils/events.event_table_torch` / `ensemble_event_sums_torch` define them, and the bounds the tests hold the fp32 code to.  Shared by
tests/test_events_gpu.py and tests/test_events_host.py.  Written from the definitions, on boolean masks; nothing here is tuned to what the
code under test returns, and nothing is compared with a verification package (none is at hand): the identities of test_events_host.py
pin the scores.

    theta = thr[b][c][k], or np.float32(base) + np.float32(thr): ONE fp32 addition, which numpy reproduces bit for bit
    event: x > theta (x < theta with below), strict, on the fp32 values;  valid: no NaN in prediction (any member), truth, base
    deterministic  a, b, c, d = sum w [P and O], [P and not O], [not P and O], [not P and not O] over the valid points
    ensemble       n = #{m: x_m event}, o = [truth event]:  S_e = sum w (n - M o)^2   S_f = sum w n (M - n)   S_o = sum w o   W_v = sum w
                   hist[0][j] = #{valid, n = j}   hist[1][j] = #{valid, n = j, o = 1}

Bounds, u = 2^-24 (2^-53 for an fp64 statement).  A term is 0 or w[row] (no product), so a cell carries the roundings of its additions
only: with `chain` additions on the way into the plane's sum,
    |cell - ref| <= chain u sum|w| over that cell            ((1 + u)^(chain - 1) - 1 <= chain u while chain (chain - 1) u <= 1: asserted)
S_e and S_f multiply w by an exact integer (< 2^12), one more rounding:  (chain + 1) u sum |w| term.   S_o and W_v are cells.
With unit weights and H W <= 2^24 every partial sum is an integer below 2^24: cells, S_o, W_v, and S_e, S_f while they stay below 2^24, are
EXACT.  The counts are integers and exact always.  |w|, not w: the pole rows of the fp32 latitude weights are negative.
chain_length: the kernels' plan (csrc/plane_stream.h): 4 ceil(v / 256) additions in the thread's running sum, v = 16-byte vectors of the
largest slice, both kernels; then 6 + 2 + ceil(slices / 64) + 6.  A torch statement sums H W terms in an order of its own: chain = H W.
"""
import math

import numpy as np

from tests.plane_reference import U, plan_slices, slice_bounds, worst  # noqa: F401  (re-exported)

CHUNK = 64                    # channels per block of the fp64 / boolean temporaries
MAX_K = 8                     # thresholds per kernel call
MBATCH = 8                    # members per batch of loads in ens_event_sums_kernel


def chain_length(H: int, W: int, slices: int) -> int:
    v = max((hi - lo) // 4 for lo, hi in slice_bounds(H * W, slices))
    return 4 * math.ceil(v / 256) + 6 + 2 + math.ceil(slices / 64) + 6


def thresholds_3d(thr, B, C):
    """[K] | [C, K] | [B, C, K] -> fp32 [1 or B, C, K]"""
    t = np.asarray(thr, dtype=np.float32)
    if t.ndim == 1:
        t = np.broadcast_to(t[None, None], (1, C, t.shape[0]))
    elif t.ndim == 2:
        t = t[None]
    assert t.ndim == 3 and t.shape[1] == C and t.shape[0] in (1, B)
    return t


def theta(thr, base):
    """fp32 [1 or B, C, K, H or 1, W or 1]"""
    th = thr[..., None, None]
    if base is not None:
        th = np.float32(base)[None, :, None] + np.float32(th)
        assert th.dtype == np.float32
    return th


def _event(x, th, below):
    with np.errstate(invalid="ignore"):
        return x < th if below else x > th


def _rows(mask, wt):
    """sum over (h, w) of wt[h] * mask: the row counts are exact integers, the weighted sum is fp64"""
    return (mask.sum(axis=-1, dtype=np.int64) * wt).sum(axis=-1)


def table(prd, tar, thr, w, base=None, below=False):
    """fp32 (or fp64 holding fp32 values) [B, C, H, W] x2 -> (T [B, C, K, 4] fp64, A [B, C, K, 4] = sum |w| per cell, n_invalid [B, C] int64)"""
    B, C, H, W = prd.shape
    thr = thresholds_3d(thr, B, C)
    if C > CHUNK:
        parts = [table(prd[:, c:c + CHUNK], tar[:, c:c + CHUNK], thr[:, c:c + CHUNK], w, None if base is None else base[c:c + CHUNK], below)
                 for c in range(0, C, CHUNK)]
        return tuple(np.concatenate([p[k] for p in parts], axis=1) for k in range(3))
    x, y = prd.astype(np.float32)[:, :, None], tar.astype(np.float32)[:, :, None]
    valid = ~(np.isnan(prd) | np.isnan(tar))
    if base is not None:
        valid &= ~np.isnan(base)[None]
    th = theta(thr, base)
    P, O = _event(x, th, below), _event(y, th, below)
    v = valid[:, :, None]
    w64 = w.astype(np.float64)
    cells = [P & O & v, P & ~O & v, ~P & O & v, ~P & ~O & v]
    T = np.stack([_rows(m, w64) for m in cells], axis=-1)
    A = np.stack([_rows(m, np.abs(w64)) for m in cells], axis=-1)
    return T, A, (~valid).sum(axis=(-1, -2), dtype=np.int64)


def ens_sums(ens, tar, thr, w, base=None, below=False):
    """[M, B, C, H, W], [B, C, H, W] -> dict: S [B, C, K, 3] = (S_e, S_f, S_o) fp64, A [B, C, K, 3]: the same with |w|, wv, awv [B, C],
    hist [B, C, K, 2, M + 1] int64, n_invalid [B, C] int64"""
    M, B, C, H, W = ens.shape
    thr = thresholds_3d(thr, B, C)
    K = thr.shape[2]
    if C > CHUNK:
        parts = [ens_sums(ens[:, :, c:c + CHUNK], tar[:, c:c + CHUNK], thr[:, c:c + CHUNK], w, None if base is None else base[c:c + CHUNK], below)
                 for c in range(0, C, CHUNK)]
        return {k: np.concatenate([p[k] for p in parts], axis=1) for k in parts[0]}
    valid = ~(np.isnan(tar) | np.isnan(ens).any(axis=0))
    if base is not None:
        valid &= ~np.isnan(base)[None]
    th = theta(thr, base)
    n = np.zeros((B, C, K, H, W), np.int64)
    for m in range(M):
        n += _event(ens[m].astype(np.float32)[:, :, None], th, below)
    o = np.broadcast_to(_event(tar.astype(np.float32)[:, :, None], th, below), n.shape).astype(np.int64)
    v = np.broadcast_to(valid[:, :, None], n.shape)
    w64 = w.astype(np.float64)

    def rows(term, wt):
        return ((term * v).sum(axis=-1) * wt).sum(axis=-1)
    terms = ((n - M * o) ** 2, n * (M - n), o)
    S = np.stack([rows(t, w64) for t in terms], axis=-1)
    A = np.stack([rows(t, np.abs(w64)) for t in terms], axis=-1)
    wv, awv = _rows(valid, w64), _rows(valid, np.abs(w64))
    pk = np.arange(B * C * K).reshape(B, C, K, 1, 1)
    hist = np.zeros((B, C, K, 2, M + 1), np.int64)
    flat = (pk * (M + 1) + n)[v]
    hist[:, :, :, 0] = np.bincount(flat, minlength=B * C * K * (M + 1)).reshape(B, C, K, M + 1)
    hist[:, :, :, 1] = np.bincount(flat, weights=o[v], minlength=B * C * K * (M + 1)).astype(np.int64).reshape(B, C, K, M + 1)
    return dict(S=S, A=A, wv=wv, awv=awv, hist=hist, n_invalid=(~valid).sum(axis=(-1, -2), dtype=np.int64))


def _unit(w, H, W):
    return bool(np.all(w == 1.0)) and H * W <= 2 ** 24


def _chain_ok(n, u):
    assert n * (n - 1) * u <= 1.0, "the first-order bound chain * u does not hold for a chain this long"


def judge_table(got_table, got_ninv, prd, tar, thr, w, n: int, base=None, below=False, u=U, tag="", ref=None):
    """element-by-element verdict on a contingency table.  Asserts n_invalid exactly, no NaN anywhere in the table (a NaN input removes its
    point and nothing else), every cell within chain u sum|w|, and -- unit weights, H W <= 2^24 -- every cell EQUAL to its integer."""
    B, C, H, W = prd.shape
    T, A, ninv = table(prd, tar, thr, w, base, below) if ref is None else ref
    _chain_ok(n, u)
    assert got_table.shape == T.shape and got_ninv.shape == ninv.shape
    assert np.array_equal(got_ninv.astype(np.int64), ninv), f"{tag}: n_invalid differs"
    assert not np.isnan(got_table).any(), f"{tag}: a NaN reached a table"
    g = got_table.astype(np.float64)
    if _unit(w, H, W):
        assert np.array_equal(g, T), f"{tag}: unit-weight cells are not the exact integers"
        assert np.array_equal(g.sum(axis=-1), np.broadcast_to((H * W - ninv)[..., None], g.shape[:-1])), f"{tag}: a + b + c + d != valid points"
    r = worst(np.abs(g - T), n * u * A)
    print(f"{tag} chain = {n}: worst table error / bound {r:.3f}")
    assert r <= 1.0, f"{tag}: a table cell outside chain u sum|w|: {r}"
    return T, A, ninv


def judge_ens(got, ens, tar, thr, w, n: int, base=None, below=False, u=U, tag="", ref=None):
    """got: dict sums [B, C, K, 3], wv [B, C], hist [B, C, K, 2, M + 1], n_invalid [B, C].  Asserts the counts and n_invalid exactly, the
    histogram's own identities, the float sums within their bounds, exact integers for unit weights."""
    M, B, C, H, W = ens.shape
    R = ens_sums(ens, tar, thr, w, base, below) if ref is None else ref
    _chain_ok(n + 1, u)
    assert np.array_equal(got["n_invalid"].astype(np.int64), R["n_invalid"]), f"{tag}: n_invalid differs"
    h = got["hist"].astype(np.int64)
    assert h.shape == R["hist"].shape and np.array_equal(h, R["hist"]), f"{tag}: counts differ from the statement"
    assert np.array_equal(h[..., 0, :].sum(axis=-1), np.broadcast_to((H * W - R["n_invalid"])[..., None], h.shape[:3]))
    assert not np.isnan(got["sums"]).any() and not np.isnan(got["wv"]).any(), f"{tag}: a NaN reached a sum"
    s, wv = got["sums"].astype(np.float64), got["wv"].astype(np.float64)
    if _unit(w, H, W):
        small = R["S"] < 2 ** 24
        assert np.array_equal(s[small], R["S"][small]) and np.array_equal(wv, R["wv"]), f"{tag}: unit-weight sums are not the exact integers"
    k = np.array([n + 1, n + 1, n], np.float64)
    r = [worst(np.abs(s[..., j] - R["S"][..., j]), k[j] * u * R["A"][..., j]) for j in range(3)] + [worst(np.abs(wv - R["wv"]), n * u * R["awv"])]
    print(f"{tag} chain = {n}: worst error / bound  S_e {r[0]:.3f}  S_f {r[1]:.3f}  S_o {r[2]:.3f}  W_v {r[3]:.3f}")
    assert max(r) <= 1.0, f"{tag}: a sum outside its bound: {r}"
    return R


def judge(got, *args, **kw):
    """one door for both: got = (table, n_invalid) -> judge_table, got = dict -> judge_ens"""
    return judge_ens(got, *args, **kw) if isinstance(got, dict) else judge_table(got[0], got[1], *args, **kw)


# ---- scores, fp64, written from the definitions (for the identities of test_events_host.py) --------------------------------------------
def scores(T):
    a, b, c, d = (T[..., k].astype(np.float64) for k in range(4))
    n = a + b + c + d
    with np.errstate(invalid="ignore", divide="ignore"):
        H, F = a / (a + c), b / (b + d)
        ar = (a + b) * (a + c) / n
        num = np.log(F) - np.log(H) - np.log(1 - F) + np.log(1 - H)
        den = np.log(F) + np.log(H) + np.log(1 - F) + np.log(1 - H)
        return dict(base_rate=(a + c) / n, freq_bias=(a + b) / (a + c), pod=H, far=b / (a + b), csi=a / (a + b + c),
                    ets=(a - ar) / (a + b + c - ar), sedi=num / den)


def brier_from_hist(hist):
    """hist [..., 2, M + 1] -> the unweighted Brier score from the counts: sum_j [no_j (1 - j / M)^2 + (nf_j - no_j) (j / M)^2] / N"""
    nf, no = hist[..., 0, :].astype(np.float64), hist[..., 1, :].astype(np.float64)
    M = nf.shape[-1] - 1
    p = np.arange(M + 1) / M
    return (no * (1 - p) ** 2 + (nf - no) * p ** 2).sum(axis=-1) / nf.sum(axis=-1)
