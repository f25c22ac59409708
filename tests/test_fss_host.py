"""No GPU: the plain-torch statement of the neighbourhood sums (utils/events.py::fss_rows_torch) against the independent numpy statement of
tests/fss_reference.py -- integers, so equality -- the identities that pin the fractions skill score, the refusals, queries and plan of
the C entry points, and the layers above on the CPU: ForecastScorer.neighbourhood_score, score_rollout(..., neighbourhoods=), the table
and the parser."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch

from swin_v2_weather_amd import _lib as L
from swin_v2_weather_amd import inference
from swin_v2_weather_amd.utils import events as E
from swin_v2_weather_amd.utils.weighted_acc_rmse import EventSpec, ForecastScorer, event_table_torch
from tests import fss_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (H, W), scales: the shapes of tests/test_fss_gpu.py (the smallest at which the kernels can go wrong) and an odd width
SHAPES = [((5, 8), (0, 1, 2, 3)), ((12, 36), (0, 1, 5, 17)), ((9, 240), (0, 1, 5, 17)), ((33, 96), (0, 16, 32)), ((70, 1440), (0, 2, 32)),
          ((12, 36), (0, 1, 2, 3, 4, 6, 9, 17)), ((7, 10), (0, 1, 4))]


@functools.lru_cache(maxsize=None)
def fields(B, C, H, W, seed=0, quantum=0.0):
    """as tests/test_events_gpu.py::_fields: the analysis is N(0, 1) around a smooth base field [C, H, W], the forecast the analysis + 0.75
    N(0, 1); fp32, optionally on a lattice of `quantum`; made once per shape and never modified"""
    rng = np.random.default_rng(1000 * seed + 7 * B + 3 * C + H + W)
    y, x = np.linspace(0, np.pi, H)[:, None], np.linspace(0, 2 * np.pi, W)[None, :]
    base = ((1.0 + np.arange(C)[:, None, None] % 3) * 0.5 * np.sin(y + 0.3 * np.arange(C)[:, None, None]) * np.cos(2 * x)).astype(np.float32)
    tar = base[None] + rng.standard_normal((B, C, H, W), dtype=np.float32)
    prd = tar + 0.75 * rng.standard_normal((B, C, H, W), dtype=np.float32)
    if quantum:
        prd, tar, base = (np.round(a / quantum) * quantum for a in (prd, tar, base))
    prd, tar, base = prd.astype(np.float32), tar.astype(np.float32), base.astype(np.float32)
    for a in (prd, tar, base):
        a.setflags(write=False)
    return prd, tar, base


def thresholds(K):
    return (np.linspace(-0.6, 0.8, K) if K > 1 else np.zeros(1)).astype(np.float32)


def _t(*arrays):
    return [None if a is None else torch.tensor(np.asarray(a)) for a in arrays]


def _one_point(H, W, h, w):
    x = np.zeros((1, 1, H, W), np.float32)
    x[0, 0, h, w] = 1.0
    return x


@pytest.mark.parametrize("shape,scales", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("use_base,below", [(False, False), (True, True)], ids=["plain-above", "base-below"])
def test_statement_equals_the_reference(shape, scales, use_base, below):
    (H, W), (B, C) = shape, ((2, 2) if shape[1] < 1000 else (1, 2))
    prd, tar, base = fields(B, C, H, W)
    base = base if use_base else None
    thr = thresholds(2)[None, None] + 0.05 * np.arange(C, dtype=np.float32)[None, :, None] - 0.03 * np.arange(B, dtype=np.float32)[:, None, None]
    want, ninv = R.rows(prd, tar, thr, scales, base, below)
    assert R.populated(want, H, W, scales), "the case is degenerate in the reference itself"
    got, gi = E.fss_rows_torch(*_t(prd, tar, thr), scales, _t(base)[0], below)
    assert got.dtype == torch.int64 and tuple(got.shape) == (B, C, 2, len(scales), H, 3) and gi.dtype == torch.int32
    assert np.array_equal(got.numpy(), want) and np.array_equal(gi.numpy(), ninv)
    assert np.array_equal(E.box_sizes(H, scales).numpy(), R.box_sizes(H, scales))
    g64 = E.fss_rows_torch(torch.tensor(prd).double(), torch.tensor(tar).double(), torch.tensor(thr), scales, _t(base)[0], below)[0]
    assert torch.equal(g64, got)                              # any dtype: compared in fp32


def test_scale_0_is_the_contingency_table_and_gives_the_base_rate():
    B, C, H, W = 2, 3, 9, 16
    prd, tar, base = fields(B, C, H, W)
    thr, ones = thresholds(3), torch.ones(H)
    rows, _ = E.fss_rows_torch(*_t(prd, tar, thr), (0, 2), _t(base)[0])
    tab = event_table_torch(*_t(prd, tar, thr), ones, _t(base)[0])[0].to(torch.int64)          # unit weights: exact integers
    a, b, c, d = tab.unbind(-1)
    assert torch.equal(rows[:, :, :, 0].sum(dim=-2), torch.stack((b + c, a + b, a + c), dim=-1))
    w = ForecastScorer(H, W, C, "cpu").w
    s = E.fss_scores(rows, w, (0, 2), W)
    tw = event_table_torch(*_t(prd, tar, thr), w, _t(base)[0])[0].double()
    assert torch.allclose(s["base_rate"], (tw[..., 0] + tw[..., 2]) / tw.sum(-1), rtol=1e-6, atol=0) and torch.equal(s["fss_uniform"], 0.5 + 0.5 * s["base_rate"])
    assert torch.allclose(s["fbs"][..., 0], tw[..., 1] + tw[..., 2], rtol=1e-6, atol=0)
    with pytest.raises(ValueError):
        E.fss_scores(rows, w, (1, 2), W)                      # the base rate is read at scale 0


def test_identical_fields_score_1_and_disjoint_events_0():
    B, C, H, W = 1, 2, 9, 16
    prd, tar, _ = fields(B, C, H, W)
    sc = (0, 1, 3)
    rows, _ = E.fss_rows_torch(*_t(tar, tar, thresholds(2)), sc)
    assert torch.equal(rows[..., 0], torch.zeros_like(rows[..., 0])) and torch.equal(rows[..., 1], rows[..., 2])
    assert torch.equal(E.fss_scores(rows, torch.ones(H), sc, W)["fss"], torch.ones(B, C, 2, 3, dtype=torch.float64))
    x = np.zeros((1, 1, H, W), np.float32)
    x[..., ::2] = 1.0                                         # even columns against odd columns: disjoint at r = 0
    rows, _ = E.fss_rows_torch(*_t(x, 1.0 - x, np.array([0.5], np.float32)), sc)
    f = E.fss_scores(rows, torch.ones(H), sc, W)["fss"][0, 0, 0]
    # r = 1: a row of the box holds 1 event of one field and 2 of the other, so FSS = 1 - (1 / 9) / (1 / 9 + 4 / 9), also where a pole clips the box
    assert float(f[0]) == 0.0 and float(f[1]) == pytest.approx(0.8, abs=1e-14)
    none = E.fss_scores(E.fss_rows_torch(*_t(x, x, np.array([2.0], np.float32)), sc)[0], torch.ones(H), sc, W)
    assert bool(torch.isnan(none["fss"]).all()) and float(none["base_rate"]) == 0.0           # no event at all: 0 / 0 in that entry


@pytest.mark.parametrize("w0", [20, 37], ids=["interior", "across-the-date-line"])
def test_a_displaced_point_scores_1_minus_d_over_the_box_width(w0):
    """one event point on an interior row, the forecast's d columns to the east: the boxes overlap in 2 r + 1 - d columns, so with unit
    weights FSS = 1 - d / (2 r + 1), and 0 once they are disjoint -- also where the displacement crosses the date line"""
    H, W, h0, sc = 21, 40, 10, (0, 1, 2, 4)                   # H > 2 r + 1 around row 10 for every r
    thr = np.array([0.5], np.float32)
    for d in (0, 1, 2, 3, 5, 9, 10):
        rows, _ = E.fss_rows_torch(*_t(_one_point(H, W, h0, (w0 + d) % W), _one_point(H, W, h0, w0), thr), sc)
        fss = E.fss_scores(rows, torch.ones(H), sc, W)["fss"][0, 0, 0]
        for i, r in enumerate(sc):
            assert float(fss[i]) == pytest.approx(max(0.0, 1.0 - d / (2 * r + 1)), abs=1e-14), (d, r)


def test_rolling_leaves_the_rows_unchanged_and_flipping_reverses_them():
    B, C, H, W = 2, 2, 12, 36
    prd, tar, base = fields(B, C, H, W)
    sc, thr = (0, 1, 5, 17), thresholds(2)
    rows, _ = E.fss_rows_torch(*_t(prd, tar, thr), sc, _t(base)[0])
    for k in (1, 7, 35, -13):
        rk, _ = E.fss_rows_torch(*_t(np.roll(prd, k, -1), np.roll(tar, k, -1), thr), sc, _t(np.roll(base, k, -1))[0])
        assert torch.equal(rk, rows), k
    rf, _ = E.fss_rows_torch(*_t(prd[:, :, ::-1].copy(), tar[:, :, ::-1].copy(), thr), sc, _t(base[:, ::-1].copy())[0])
    assert torch.equal(rf, rows.flip(-2))


def test_an_invalid_point_is_counted_once_and_is_an_event_nowhere():
    B, C, H, W = 2, 2, 9, 16
    prd, tar, base = fields(B, C, H, W)
    sc, thr = (0, 2), np.array([-1.0e30], np.float32)         # everything is an event ...
    p2, t2, b2 = prd.copy(), tar.copy(), base.copy()
    p2[0, 0, 0, 0] = np.nan                                   # the first row and column
    p2[0, 0, 4, 5] = t2[0, 0, 4, 5] = np.nan                  # both at once: one point
    t2[1, 1, H - 1, W - 1] = np.nan                           # the last row and column
    t2[1, 0, 3, 3] = np.inf                                   # +-inf are values
    p2[1, 0, 3, 4] = -np.inf
    rows, ninv = E.fss_rows_torch(*_t(p2, t2, thr), sc)
    assert ninv.tolist() == [[2, 0], [0, 1]]
    per_plane = rows[:, :, 0, 0].sum(dim=-2)                  # ... except the invalid points, in BOTH fields
    assert per_plane[..., 1].tolist() == [[H * W - 2, H * W], [H * W - 1, H * W - 1]] and torch.equal(per_plane[..., 2], per_plane[..., 1] + torch.tensor([[0, 0], [1, 0]]))          # (-inf is below any threshold: the forecast alone loses that point)
    assert np.array_equal(rows.numpy(), R.rows(p2, t2, thr, sc)[0])
    b2[1, 2, 2] = np.nan                                      # the base field: that point leaves channel 1 of every sample
    rows, ninv = E.fss_rows_torch(*_t(prd, tar, thresholds(1)), sc, _t(b2)[0])
    assert ninv.tolist() == [[0, 1], [0, 1]] and np.array_equal(rows.numpy(), R.rows(prd, tar, thresholds(1), sc, b2)[0])


def test_ties_on_theta_are_no_event():
    B, C, H, W = 2, 2, 6, 16
    prd, tar, base = fields(B, C, H, W, quantum=0.25)
    thr = np.array([-0.25, 0.0, 0.5], np.float32)
    assert (tar[:, :, None] == (base[None, :, None] + thr[None, None, :, None, None])).mean() > 0.03
    for below in (False, True):
        got = E.fss_rows_torch(*_t(prd, tar, thr), (0, 1, 2), _t(base)[0], below)[0]
        assert np.array_equal(got.numpy(), R.rows(prd, tar, thr, (0, 1, 2), base, below)[0])


def test_pooled_scores_are_the_scores_of_the_summed_rows_and_useful_scale():
    B, C, H, W = 3, 2, 9, 16
    prd, tar, base = fields(B, C, H, W)
    sc_ = ForecastScorer(H, W, C, "cpu", climatology=base)
    thr, scales = thresholds(2), (0, 1, 3)
    r = sc_.neighbourhood_score(*_t(prd, tar, thr), scales, anomaly=True)
    want = R.scores(R.rows(prd, tar, thr, scales, base)[0].sum(0), sc_.w.numpy(), scales, W)
    assert np.allclose(r.pooled["fss"].numpy(), want["fss"], rtol=0, atol=1e-12)
    assert np.allclose(r.pooled["base_rate"].numpy() * B, want["base_rate"], rtol=1e-12, atol=0)          # B fields were pooled
    assert not np.allclose(r.pooled["fss"].numpy(), r.scores["fss"].mean(0).numpy(), rtol=0, atol=1e-9)   # never the mean of the scores
    curve = torch.tensor([[0.1, 0.4, 0.7, 0.9], [0.1, 0.2, 0.3, 0.4], [0.8, 0.7, 0.9, 1.0], [float("nan"), 0.9, 0.9, 0.9]], dtype=torch.float64)
    assert E.useful_scale(curve, torch.tensor([0.6, 0.6, 0.6, 0.6], dtype=torch.float64), (0, 2, 8, 32)).tolist() == [8, -1, 0, 2]


def test_scales_are_checked():
    x = torch.zeros(1, 1, 4, 8)
    for bad in ((), (1, 1), (2, 1), (-1, 0), (0, 33), (0, 4), (0.5,)):
        with pytest.raises(ValueError):
            E.fss_rows_torch(x, x, torch.zeros(1), bad)
    assert E.check_scales((0, 3), 8) == (0, 3) and E.FSS_MAX_S == 8


# ---- the C entry points without a GPU: queries, plan, refusals, the header ------------------------------------------------------
def test_queries_and_plan():
    from swin_v2_weather_amd import ops
    assert L.ABI_VERSION == 113 and "fss.hip" in L.SOURCES
    lib = L.load()
    for (B, C, H, W) in ((1, 1, 5, 8), (2, 3, 12, 36), (2, 73, 720, 1440), (1, 2100, 2, 4), (1, 2, 9, 240)):
        slices = lib.swv2_score_slices(B * C, H, W)
        for K in (1, 4, 8):
            assert lib.swv2_fss_ws_bytes(B * C, H, W, K, 3) == 4 * B * C * (2 * K * H * ((W + 31) // 32) + slices)
    for bad in ((0, 4, 4, 1, 1), (4, 0, 4, 1, 1), (4, 4, 0, 1, 1), (4, 4, 4, 0, 1), (4, 4, 4, 9, 1), (4, 4, 4, 1, 0), (4, 4, 4, 1, 9)):
        assert lib.swv2_fss_ws_bytes(*bad) == 0, bad
    for bad in ((0, 4, 1, 1), (4, 0, 1, 1), (4, 4, 0, 1), (4, 4, 9, 1), (4, 4, 1, -1), (4, 4, 1, 33)):
        assert lib.swv2_fss_band_rows(*bad) == 0, bad
    band = ops.fss_band_rows
    assert band(146, 720, 4, 32) == 66                        # 11 bands, each at least as tall as the 65-row box
    assert band(146, 720, 4, 2) == 33 and band(146, 720, 4, 0) == 33             # small boxes: at least 32 rows
    assert band(12, 70, 1, 32) == 70 and band(2, 70, 1, 32) == 18                # one band per plane; fewer than 8 workgroups: 4 bands per plane
    assert band(1, 70, 1, 32) == 9 and band(1, 16, 1, 0) == 8                    # ... never bands of fewer than 8 rows
    assert band(2000, 100, 8, 32) == 80 and band(1, 5, 1, 3) == 5                # never more than 80 rows (the LDS image)
    for planes, H, K, r in ((1, 1, 1, 0), (3, 33, 2, 32), (12, 70, 8, 32), (2, 70, 1, 32), (146, 720, 8, 16), (5, 1000, 1, 32)):
        b = band(planes, H, K, r)
        assert 1 <= b <= min(H, 80) and (b >= min(H, 8)), (planes, H, K, r, b)


def refusals(lib):
    """every refusal of swv2_fss_rows: -1, its name and the reason in the message, before any HIP call (the pointers are never touched)"""
    P = 4096
    K, S, B, C, H, W = 3, 3, 2, 3, 8, 16
    span = C * H * W
    ok = lib.swv2_fss_ws_bytes(B * C, H, W, K, S)

    def sc(*r):
        return (ctypes.c_int * len(r))(*r)

    def call(prd=P, ps=span, tar=P, ts=span, base=None, thr=P, tbs=0, scales=sc(0, 1, 4), K=K, S=S, below=0, B=B, C=C, H=H, W=W, ws=P, wb=ok, rows=P,
             ninv=P):
        return lib.swv2_fss_rows(prd, ps, tar, ts, base, thr, tbs, scales, K, S, below, B, C, H, W, ws, wb, rows, ninv, None)
    cases = [(lambda: call(prd=None), b"null"), (lambda: call(tar=None), b"null"), (lambda: call(thr=None), b"null"), (lambda: call(scales=None), b"null"),
             (lambda: call(ws=None), b"null"), (lambda: call(rows=None), b"null"), (lambda: call(ninv=None), b"null"),
             (lambda: call(K=0), b"thresholds K"), (lambda: call(K=9), b"thresholds K"), (lambda: call(S=0), b"scales S"), (lambda: call(S=9), b"scales S"),
             (lambda: call(scales=sc(0, 1, 1)), b"ascending"), (lambda: call(scales=sc(2, 1, 4)), b"ascending"), (lambda: call(scales=sc(-1, 1, 4)), b"outside 0 .. 32"),
             (lambda: call(scales=sc(0, 1, 33)), b"outside 0 .. 32"), (lambda: call(scales=sc(0, 1, 8)), b"wider than W"), (lambda: call(W=18), b"W % 4"),
             (lambda: call(prd=P + 4), b"aligned"), (lambda: call(tar=P + 8), b"aligned"), (lambda: call(base=P + 4), b"aligned"),
             (lambda: call(ws=P + 4), b"aligned"), (lambda: call(thr=P + 2), b"aligned"), (lambda: call(rows=P + 4), b"aligned"),
             (lambda: call(ninv=P + 2), b"aligned"), (lambda: call(ps=span + 1), b"stride"), (lambda: call(ts=H * W), b"stride"),
             (lambda: call(tbs=C * K - 1), b"stride"), (lambda: call(B=0), b"shape"), (lambda: call(H=0), b"shape"),
             (lambda: call(B=1 << 12, C=1 << 8), b"shape"), (lambda: call(H=1 << 15, W=1 << 15), b"shape"), (lambda: call(wb=ok - 1), b"workspace"),
             (lambda: call(wb=lib.swv2_fss_ws_bytes(B * C, H, W, K - 1, S)), b"workspace")]
    for fn, word in cases:
        assert fn() == -1
        msg = lib.swv2_last_error()
        assert msg.startswith(b"swv2_fss_rows:") and word in msg, msg
    return len(cases)


def test_every_refusal_names_the_entry_point_without_a_gpu():
    assert refusals(L.load()) == 33
    with pytest.raises(L.Swv2Error):
        L.check(-1, "swv2_fss_rows")


def test_header_and_ctypes_agree_on_the_fss_entry_points():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "swv2.h")).read(), flags=re.S)
    kinds = {"int": ctypes.c_int, "long": ctypes.c_long, "size_t": ctypes.c_size_t}
    seen = []
    for ret, name, args in re.findall(r"\b(int|size_t)\s+(swv2_fss_[a-z_]+)\s*\(([^)]*)\)\s*;", txt):
        want = [(ctypes.POINTER(ctypes.c_int) if a.startswith("const int*") else ctypes.c_void_p) if "*" in a else kinds[a.split()[0]]
                for a in (x.strip() for x in args.split(","))]
        res, argtypes = L.SYMBOLS[name]
        assert res is kinds[ret] and argtypes == want, name
        seen.append(name)
    assert sorted(seen) == ["swv2_fss_band_rows", "swv2_fss_rows", "swv2_fss_ws_bytes"]
    assert all(hasattr(L.load(), n) for n in seen) and "SWV2_VERSION 113" in open(os.path.join(ROOT, "include", "swv2.h")).read()


def test_python_wrappers_refuse_what_the_kernels_cannot_read():
    from swin_v2_weather_amd import ops
    x = torch.zeros(1, 2, 4, 8)
    with pytest.raises(L.Swv2Error):
        ops.fss_rows(x, x, torch.zeros(1, 2, 1), (0, 1), torch.zeros(64, dtype=torch.int32))            # CPU tensors
    with pytest.raises(L.Swv2Error):
        ops.fss_workspace(2, 4, 8, 9, 1, "cpu")
    with pytest.raises(L.Swv2Error):
        ops.fss_workspace(2, 4, 8, 1, 9, "cpu")


# ---- the scorer, the rollout and the command line on the CPU statement ------------------------------------------------------------
def test_neighbourhood_score_on_the_cpu_statement():
    B, C, H, W = 2, 3, 6, 12
    prd, tar, clim = fields(B, 5, H, W)
    tp, tt = _t(prd, tar)
    sc = ForecastScorer(H, W, C, "cpu", climatology=clim[1:4])
    thr = torch.linspace(-1.0, 1.0, 11)                       # K = 11
    r = sc.neighbourhood_score(tp, tt, thr, (0, 1, 3), anomaly=True, coff_prd=1, coff_tar=1)
    rows, ni = E.fss_rows_torch(tp[:, 1:4], tt[:, 1:4], thr, (0, 1, 3), torch.tensor(clim[1:4]))
    assert torch.equal(r.rows, rows) and torch.equal(r.n_invalid, ni) and len(sc._ws) == 0
    assert tuple(r.scores["fss"].shape) == (B, C, 11, 3) and tuple(r.pooled["fss"].shape) == (C, 11, 3) and tuple(r.pooled["useful_scale"].shape) == (C, 11)
    assert torch.equal(r.pooled["fss"], E.fss_scores(rows.sum(0), sc.w, (0, 1, 3), W, B)["fss"]) and r.scores["fss"].dtype == torch.float64
    # scale 0 left out by the caller: computed all the same (the base rate), and dropped from what is reported
    q = sc.neighbourhood_score(tp, tt, thr, (1, 3), anomaly=True, coff_prd=1, coff_tar=1)
    assert torch.equal(q.rows, rows[:, :, :, 1:]) and torch.equal(q.scores["fss"], r.scores["fss"][..., 1:]) and tuple(q.pooled["fbs"].shape) == (C, 11, 2)
    assert torch.equal(q.scores["base_rate"], r.scores["base_rate"]) and torch.equal(q.pooled["fss_uniform"], r.pooled["fss_uniform"])
    assert torch.equal(q.pooled["useful_scale"], E.useful_scale(q.pooled["fss"], q.pooled["fss_uniform"], (1, 3)))
    b = sc.neighbourhood_score(tp, tt, thr[:2], (0, 2), base=clim[1:4].copy(), below=True, coff_prd=1, coff_tar=1)
    assert torch.equal(b.rows, E.fss_rows_torch(tp[:, 1:4], tt[:, 1:4], thr[:2], (0, 2), torch.tensor(clim[1:4]), True)[0])
    for bad, kw in (((2, 1), {}), ((0, 33), {}), ((0, 6), {}), ((), {}), ((0, 1), dict(anomaly=True, base=clim[1:4].copy()))):
        with pytest.raises(ValueError):
            sc.neighbourhood_score(tp, tt, thr, bad, coff_prd=1, coff_tar=1, **kw)
    with pytest.raises(ValueError, match="climatology"):
        ForecastScorer(H, W, C, "cpu").neighbourhood_score(tp, tt, thr, (0, 1), anomaly=True, coff_prd=1, coff_tar=1)
    with pytest.raises(ValueError, match="blocks"):
        sc.neighbourhood_score(tp, tt, thr, (0, 1), coff_prd=3)


class _Net:
    """a stand-in for the model in the rollout loops: damps the fields and shifts them one column"""
    out_chans = 3

    def forward_rollout(self, x, out, coff, extra):
        y = 0.9 * torch.roll(x[:, :3], 1, dims=-1)
        out[:, coff:coff + 3] = y
        return None, y if extra is None else torch.cat([y, extra], 1)


def test_rollout_with_neighbourhoods_equals_the_scorer_called_by_hand():
    B, C, H, W, steps = 2, 3, 6, 12, 3
    rng = np.random.default_rng(5)
    clim = fields(B, C, H, W)[2]
    truth = torch.tensor(rng.standard_normal((B, steps, C, H, W)).astype(np.float32))
    x0 = torch.tensor(rng.standard_normal((B, C, H, W)).astype(np.float32))
    sc = ForecastScorer(H, W, C, "cpu", climatology=clim)
    spec = EventSpec("anomaly", (0.0, 0.5), False)
    ev = inference.score_rollout(_Net(), x0, truth, steps, scorer=sc, keep_forecast=True, events=spec)
    got = inference.score_rollout(_Net(), x0, truth, steps, scorer=sc, keep_forecast=True, events=spec, neighbourhoods=(1, 4))
    assert ev.neighbourhoods is None and all(torch.equal(a, b) for a, b in zip(ev[:5], got[:5])) and torch.equal(ev.events.table, got.events.table)
    nb = got.neighbourhoods
    assert nb.scales == (1, 4) and tuple(nb.rows.shape) == (steps, B, C, 2, 2, H, 3) and tuple(nb.scores["fss"].shape) == (steps, C, 2, 2)
    for s in range(steps):
        r = sc.neighbourhood_score(got.forecast[:, s], truth[:, s], torch.tensor(spec.levels), (1, 4), anomaly=True)
        assert torch.equal(nb.rows[s], r.rows) and torch.equal(nb.n_invalid[s], r.n_invalid)
        assert all(torch.equal(nb.scores[k][s], r.pooled[k]) for k in ("fss", "fbs", "fss_uniform", "base_rate", "useful_scale"))
    txt = inference.lead_time_table(got, [("u", 0), ("v", 1)]).splitlines()
    assert txt[0].split()[-12:] == ["ets0_u", "ets0_v", "ets1_u", "ets1_v", "fss0_r1_u", "fss0_r1_v", "fss0_r4_u", "fss0_r4_v", "fss1_r1_u", "fss1_r1_v",
                                    "fss1_r4_u", "fss1_r4_v"]
    assert float(txt[2].split()[-1]) == pytest.approx(float(nb.scores["fss"][1, 1, 1, 1]), abs=1e-5)
    assert float(txt[3].split()[-8]) == pytest.approx(float(nb.scores["fss"][2, 0, 0, 0]), abs=1e-5)
    old = inference.lead_time_table(ev, [("u", 0), ("v", 1)]).splitlines()                               # without neighbourhoods: the columns of before
    assert all(line.startswith(o) for line, o in zip(txt, old)) and "fss" not in old[0]
    with pytest.raises(ValueError, match="EventSpec"):
        inference.score_rollout(_Net(), x0, truth, steps, scorer=sc, neighbourhoods=(1, 4))
    with pytest.raises(ValueError, match="ensemble"):
        inference.ensemble_rollout(_Net(), x0, truth, steps, 3, 0.3, 5, scorer=sc, events=spec, neighbourhoods=(1, 4))


def test_parser_takes_event_scales_only_where_they_fit():
    ap = inference.build_parser()
    a = ap.parse_args(["--registry", "R", "--truth", "t.npy", "--event-anomaly", "1.0", "2.0", "--event-scales", "1", "4", "16"])
    assert a.event_scales == [1, 4, 16]
    assert ap.parse_args(["--registry", "R", "--truth", "t.npy", "--event-quantile", "0.9"]).event_scales is None
    for bad in (["--truth", "t.npy", "--event-scales", "1"],                                             # no events
                ["--truth", "t.npy", "--event-anomaly", "1.0", "--event-scales"],
                ["--truth", "t.npy", "--event-anomaly", "1.0", "--event-scales", "4", "1"],
                ["--truth", "t.npy", "--event-anomaly", "1.0", "--event-scales", "0", "33"],
                ["--truth", "t.npy", "--event-anomaly", "1.0", "--event-scales", "1.5"],
                ["--truth", "t.npy", "--event-quantile", "0.9", "--event-scales", "1", "--ensemble", "3", "--perturbation", "0.1"]):
        with pytest.raises(SystemExit) as e:
            ap.parse_args(["--registry", "R"] + bad)
        assert e.value.code == 2, bad
