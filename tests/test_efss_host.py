"""No GPU: the plain-torch statement of the ensemble's neighbourhood sums (utils/events.py::fss_ens_rows_torch) against the independent numpy
statement of tests/efss_reference.py -- integers, so equality -- the identities that pin the probabilistic fractions skill score, the
refusals, queries and plan of the three swv2_fss_ens_* entry points, and the layers above on the CPU:
ForecastScorer.ensemble_neighbourhood_score, ensemble_rollout(..., ensemble_neighbourhoods=), the table and the parser."""
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
from swin_v2_weather_amd.utils.weighted_acc_rmse import EventSpec, ForecastScorer
from tests import efss_reference as ER
from tests import fss_reference as R
from tests.test_fss_host import _Net, fields, thresholds

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (B, C, H, W), K, scales, M: between them M crosses every bit-plane count of the kernel (P = bit_length(M) = 2 .. 7)
CASES = [((2, 3, 5, 8), 2, (0, 1, 2, 3), 2),           # the box clips at both poles; 2 r + 1 = W - 1; P = 2
         ((2, 2, 12, 36), 3, (0, 1, 5, 17), 7),        # W % 32 != 0 wrap; P = 3, all planes set at c = 7
         ((1, 2, 9, 240), 2, (0, 1, 5, 17), 8),        # P = 4, the top plane alone at c = 8
         ((2, 2, 12, 36), 3, (0, 1, 5, 17), 33),       # P = 6
         ((1, 2, 33, 96), 1, (0, 16, 32), 64)]         # P = 7; 65-bit windows; rows beyond both poles
CASE_IDS = [f"{'x'.join(map(str, s))}-K{k}-M{m}" for s, k, _, m in CASES]


@functools.lru_cache(maxsize=None)
def reference(B, C, H, W, K, scales, M, use_base=False, below=False, per_sample=False, two_pass=False):
    """the members and truth of a case, its thresholds and the reference's rows and n_invalid: computed once, shared, never modified.  The
    reference itself must not be degenerate: every point count 0 .. M occurs for every threshold, and all three sums are populated."""
    _, tar, base = fields(B, C, H, W)
    ens = ER.members(M, B, C, H, W)
    thr = thresholds(K)
    if per_sample:
        thr = thr[None, None] + 0.05 * np.arange(C, dtype=np.float32)[None, :, None] - 0.03 * np.arange(B, dtype=np.float32)[:, None, None]
    base = base if use_base else None
    c = ER.counts(ens, tar, thr, base, below)
    assert (c.min(axis=(0, 1, 3, 4)) == 0).all() and (c.max(axis=(0, 1, 3, 4)) == M).all(), "the point counts do not span 0 .. M"
    want, ninv = ER.rows(ens, tar, thr, scales, base, below, two_pass)
    assert R.populated(want, H, W, scales), "the case is degenerate in the reference itself"
    want.setflags(write=False)
    return ens, tar, base, thr, want, ninv


def _t(*arrays):
    return [None if a is None else torch.tensor(np.asarray(a)) for a in arrays]


@pytest.mark.parametrize("shape,K,scales,M", CASES, ids=CASE_IDS)
def test_statement_equals_the_reference(shape, K, scales, M):
    ens, tar, _, thr, want, ninv = reference(*shape, K, scales, M)
    got, gi = E.fss_ens_rows_torch(*_t(ens, tar, thr), scales)
    assert got.dtype == torch.int64 and tuple(got.shape) == shape[:2] + (K, len(scales), shape[2], 3) and gi.dtype == torch.int32
    assert np.array_equal(got.numpy(), want) and np.array_equal(gi.numpy(), ninv)


@pytest.mark.parametrize("use_base,below", [(False, True), (True, False), (True, True)], ids=["plain-below", "base-above", "base-below"])
def test_statement_with_base_direction_and_per_sample_thresholds(use_base, below):
    shape, K, scales, M = (3, 2, 12, 36), 2, (0, 1, 5, 17), 5
    ens, tar, base, thr, want, ninv = reference(*shape, K, scales, M, use_base, below, True)
    got, gi = E.fss_ens_rows_torch(*_t(ens, tar, thr), scales, _t(base)[0], below)
    assert np.array_equal(got.numpy(), want) and np.array_equal(gi.numpy(), ninv)
    g64 = E.fss_ens_rows_torch(torch.tensor(ens).double(), torch.tensor(tar).double(), torch.tensor(thr), scales, _t(base)[0], below)[0]
    assert torch.equal(g64, got)                              # any dtype: compared in fp32


def test_the_reference_two_pass_box_sum_is_the_sum_of_the_members_box_counts():
    shape, K, scales, M = (2, 2, 12, 36), 3, (0, 1, 5, 17), 7
    ens, tar, _, thr, want, _ = reference(*shape, K, scales, M)
    assert np.array_equal(ER.rows(ens, tar, thr, scales, two_pass=True)[0], want)
    assert np.array_equal(ER.rows(ens, tar, thr, (0, 3), fields(*shape)[2], True, two_pass=True)[0], ER.rows(ens, tar, thr, (0, 3), fields(*shape)[2], True)[0])


def test_invalid_points_ties_and_a_threshold_nobody_exceeds():
    B, C, H, W, M, scales = 2, 2, 12, 36, 5, (0, 1, 5, 17)
    _, tar, base = (a.copy() for a in fields(B, C, H, W, quantum=0.25))
    ens = (np.round(ER.members(M, B, C, H, W) / 0.25) * 0.25).astype(np.float32)
    thr = np.array([-0.25, 0.5, 1.0e6], np.float32)
    assert (ens[:, :, :, None] == (base[None, None, :, None] + thr[None, None, None, :, None, None])).mean() > 0.02      # ties on theta
    ens[3, 0, 0, 0, 0] = np.nan                               # ONE member only: the point is invalid in all
    tar[0, 0, H - 1, W - 1] = np.nan
    ens[1, 0, 1, 5, W - 1] = tar[0, 1, 5, W - 1] = np.nan     # both at once: one point
    tar[1, 0, 0, W - 1] = np.inf                              # +-inf are values
    ens[2, 1, 0, H - 1, 0] = -np.inf
    base[1, 6, 0] = np.nan
    for below in (False, True):
        want, ninv = ER.rows(ens, tar, thr, scales, base, below)
        assert ninv.tolist() == [[2, 2], [0, 1]]
        got, gi = E.fss_ens_rows_torch(*_t(ens, tar, thr), scales, _t(base)[0], below)
        assert np.array_equal(got.numpy(), want) and np.array_equal(gi.numpy(), ninv)
        if not below:                                         # nothing exceeds 1e6 but the +inf of the truth of plane (1, 0)
            assert not want[0, :, 2].any() and not want[1, 1, 2].any() and int(want[1, 0, 2, 0, :, 2].sum()) == 1
    c = ER.counts(ens, tar, thr[:1], base)
    assert c[0, 0, 0, 0, 0] == 0 and ER.counts(np.nan_to_num(ens, nan=9.0), tar, thr[:1], base)[0, 0, 0, 0, 0] >= 1


def test_copies_of_one_forecast_give_the_deterministic_rows():
    B, C, H, W = 2, 2, 12, 36
    prd, tar, base = fields(B, C, H, W)
    thr, scales = thresholds(3), (0, 1, 5, 17)
    det = E.fss_rows_torch(*_t(prd, tar, thr), scales, _t(base)[0])[0]
    w = ForecastScorer(H, W, C, "cpu").w
    fss = E.fss_scores(det, w, scales, W)
    for M in (2, 4, 5, 64):
        ens = torch.tensor(prd).unsqueeze(0).expand(M, B, C, H, W)
        rows = E.fss_ens_rows_torch(ens, torch.tensor(tar), torch.tensor(thr), scales, _t(base)[0])[0]
        assert torch.equal(rows, det * torch.tensor([M * M, M * M, 1]))
        s = E.fss_ens_scores(rows, w, scales, W, M)
        assert torch.allclose(s["pfss"], fss["fss"], rtol=0, atol=1e-14) and torch.equal(s["base_rate"], fss["base_rate"])
        if M in (2, 4, 64):                                   # M^2 a power of two: the division is exact
            assert torch.equal(s["pfss"], fss["fss"]) and torch.equal(s["fbs"], fss["fbs"])


def test_member_order_does_not_matter_and_scale_0_is_the_brier_sum():
    shape, K, scales, M = (2, 2, 12, 36), 3, (0, 1, 5, 17), 7
    ens, tar, _, thr, want, _ = reference(*shape, K, scales, M)
    perm = np.random.default_rng(1).permutation(M)
    assert np.array_equal(E.fss_ens_rows_torch(*_t(ens[perm], tar, thr), scales)[0].numpy(), want)
    sums = E.ensemble_event_sums_torch(torch.tensor(ens).double(), torch.tensor(tar).double(), torch.tensor(thr), torch.ones(shape[2], dtype=torch.float64))[0]
    assert torch.equal(torch.tensor(want[:, :, :, 0, :, 0].sum(-1)), sums[..., 0].to(torch.int64))       # S_e with unit weights
    assert np.array_equal(want[:, :, :, 0, :, 2].sum(-1), sums[..., 2].numpy())                            # S_o


def test_scores_are_those_of_the_reference_and_pooled_over_summed_rows():
    shape, K, scales, M = (2, 2, 12, 36), 3, (0, 1, 5, 17), 7
    ens, tar, _, thr, want, _ = reference(*shape, K, scales, M)
    B, C, H, W = shape
    sc = ForecastScorer(H, W, C, "cpu")
    r = sc.ensemble_neighbourhood_score(torch.tensor(ens), torch.tensor(tar), M, thr, scales)
    per, pooled = ER.scores(want, sc.w.numpy(), scales, W, M), ER.scores(want.sum(0), sc.w.numpy(), scales, W, M, B)
    for k in ("pfss", "fbs", "fss_uniform", "base_rate"):
        assert np.allclose(r.scores[k].numpy(), per[k], rtol=0, atol=1e-12) and np.allclose(r.pooled[k].numpy(), pooled[k], rtol=0, atol=1e-12), k
    assert not np.allclose(r.pooled["pfss"].numpy(), r.scores["pfss"].mean(0).numpy(), rtol=0, atol=1e-9)      # never the mean of the scores
    assert torch.equal(r.pooled["useful_scale"], E.useful_scale(r.pooled["pfss"], r.pooled["fss_uniform"], scales))
    assert 0.0 < float(r.pooled["pfss"].min()) and float(r.pooled["pfss"].max()) < 1.0 and r.member_rows is None
    with pytest.raises(ValueError):
        E.fss_ens_scores(torch.tensor(want), sc.w, (1, 2, 3, 4), W, M)
    with pytest.raises(ValueError):
        E.fss_ens_scores(torch.tensor(want), sc.w, scales, W, 1)
    with pytest.raises(ValueError):
        E.fss_ens_rows_torch(torch.tensor(ens)[:1], torch.tensor(tar), thr, scales)


def test_scorer_on_the_cpu_statement_chunks_blocks_and_member_rows():
    B, C, H, W, M = 2, 3, 6, 12, 4
    _, tar, clim = fields(B, 5, H, W)
    ens = ER.members(M, B, 5, H, W)
    te, tt = torch.tensor(ens).reshape(M * B, 5, H, W), torch.tensor(tar)       # member-major rows, as the rollout's ring
    sc = ForecastScorer(H, W, C, "cpu", climatology=clim[1:4])
    thr = torch.linspace(-1.0, 1.0, 11)
    r = sc.ensemble_neighbourhood_score(te, tt, M, thr, (0, 1, 3), anomaly=True, coff_ens=1, coff_tar=1, members=True)
    e5 = torch.tensor(ens)[:, :, 1:4]
    rows, ni = E.fss_ens_rows_torch(e5, tt[:, 1:4], thr, (0, 1, 3), torch.tensor(clim[1:4]))
    assert torch.equal(r.rows, rows) and torch.equal(r.n_invalid, ni) and len(sc._ws) == 0
    assert tuple(r.scores["pfss"].shape) == (B, C, 11, 3) and tuple(r.pooled["pfss"].shape) == (C, 11, 3) and r.pooled["pfss"].dtype == torch.float64
    assert torch.equal(r.pooled["pfss"], E.fss_ens_scores(rows.sum(0), sc.w, (0, 1, 3), W, M, B)["pfss"])
    det = [E.fss_rows_torch(e5[m], tt[:, 1:4], thr, (0, 1, 3), torch.tensor(clim[1:4]))[0] for m in range(M)]
    dis = [E.fss_rows_torch(e5[m], e5[0], thr, (0, 1, 3), torch.tensor(clim[1:4]))[0] for m in range(1, M)]
    assert torch.equal(r.member_rows, sum(det)) and torch.equal(r.dispersion_rows, sum(dis))
    assert torch.equal(r.member_scores["fss"], E.fss_scores(sum(det).sum(0), sc.w, (0, 1, 3), W, B * M)["fss"])
    assert torch.equal(r.dispersion_scores["fss"], E.fss_scores(sum(dis).sum(0), sc.w, (0, 1, 3), W, B * (M - 1))["fss"])
    assert tuple(r.member_scores["useful_scale"].shape) == (C, 11) and tuple(r.dispersion_scores["fss"].shape) == (C, 11, 3)
    q = sc.ensemble_neighbourhood_score(te, tt, M, thr, (1, 3), anomaly=True, coff_ens=1, coff_tar=1, members=True)          # scale 0 left out
    assert torch.equal(q.rows, rows[:, :, :, 1:]) and torch.equal(q.scores["pfss"], r.scores["pfss"][..., 1:]) and torch.equal(q.member_rows, r.member_rows[:, :, :, 1:])
    assert torch.equal(q.pooled["fss_uniform"], r.pooled["fss_uniform"]) and torch.equal(q.dispersion_scores["fss"], r.dispersion_scores["fss"][..., 1:])
    for bad in ((2, 1), (0, 33), (0, 6), ()):
        with pytest.raises(ValueError):
            sc.ensemble_neighbourhood_score(te, tt, M, thr, bad, coff_ens=1, coff_tar=1)
    with pytest.raises(ValueError, match="members"):
        sc.ensemble_neighbourhood_score(te, tt, 3, thr, (0, 1), coff_ens=1, coff_tar=1)


# ---- the C entry points without a GPU: queries, plan, refusals, the header ------------------------------------------------------
def bit_planes(M):
    return int(M).bit_length()


def lds_need(fields_, tcols, band, rmax, S=8):
    return band * S * 3 * 8 + fields_ * (band + 2 * rmax) * ((tcols + 63) // 32 + 4) * 4


def planned_tile(M, rmax):
    """the column tile of the plan as include/swv2.h states it: halved from 1024 to 256 while a band of max(2 r_max + 1, 32) rows needs
    more than 80 KiB"""
    tall, tile = min(80, max(2 * rmax + 1, 32)), 1024
    while tile > 256 and lds_need(bit_planes(M) + 1, tile, tall, rmax) > 80 * 1024:
        tile //= 2
    return tile


def test_queries_and_plan():
    from swin_v2_weather_amd import ops
    assert L.ABI_VERSION == 113 and "fss.hip" in L.SOURCES
    lib = L.load()
    for (B, C, H, W) in ((1, 1, 5, 8), (2, 3, 12, 36), (2, 73, 720, 1440), (1, 2100, 2, 4), (1, 2, 9, 240)):
        slices = lib.swv2_score_slices(B * C, H, W)
        for M in (2, 3, 4, 7, 8, 33, 64):
            for K in (1, 4, 8):
                assert lib.swv2_fss_ens_ws_bytes(B * C, H, W, M, K, 3) == 4 * B * C * ((bit_planes(M) + 1) * K * H * ((W + 31) // 32) + slices)
    for bad in ((0, 4, 4, 2, 1, 1), (4, 0, 4, 2, 1, 1), (4, 4, 0, 2, 1, 1), (4, 4, 4, 1, 1, 1), (4, 4, 4, 65, 1, 1), (4, 4, 4, 2, 0, 1), (4, 4, 4, 2, 9, 1),
                (4, 4, 4, 2, 1, 0), (4, 4, 4, 2, 1, 9)):
        assert lib.swv2_fss_ens_ws_bytes(*bad) == 0, bad
    for bad in ((0, 4, 2, 1, 1), (4, 0, 2, 1, 1), (4, 4, 1, 1, 1), (4, 4, 65, 1, 1), (4, 4, 2, 0, 1), (4, 4, 2, 9, 1), (4, 4, 2, 1, -1), (4, 4, 2, 1, 33)):
        assert lib.swv2_fss_ens_band_rows(*bad) == 0, bad
    band = ops.fss_ens_band_rows
    for M in (2, 3, 4, 7, 8, 31, 32, 63, 64):
        for rmax in (0, 16, 32):
            tile = planned_tile(M, rmax)
            for W in (8, 240, 1440, 16384):
                tiles = -(-W // tile)
                tcols = -(-W // tiles)
                for planes, H, K in ((146, 720, 4), (12, 70, 1), (2, 70, 1), (1, 5, 1), (2000, 100, 8), (1, 16, 1), (3, 33, 2)):
                    b = band(planes, H, M, K, rmax)
                    assert 1 <= b <= min(H, 80) and b >= min(H, 8), (M, rmax, planes, H, K, b)
                    assert lds_need(bit_planes(M) + 1, tcols, b, rmax) <= 80 * 1024, (M, rmax, W, planes, H, K, b)
                    nb = -(-H // b)
                    assert nb * b >= H and (nb - 1) * b < H                                   # the bands cover H, none is empty
                    assert planes * K * nb >= 8 or b <= 8 or nb == -(-H // 8), (planes, H, K, b)          # small calls: 8 workgroups where H allows
            # a large call keeps bands as tall as the largest box (the tile is given up first)
            assert band(146, 720, M, 4, rmax) >= max(2 * rmax + 1, 32), (M, rmax)
    assert band(146, 720, 64, 4, 32) == 66 and band(12, 70, 16, 1, 32) == 70 and band(2, 70, 16, 1, 32) == 18 and band(1, 16, 64, 1, 0) == 8
    assert planned_tile(2, 32) == 1024 and planned_tile(7, 32) == 512 and planned_tile(64, 32) == 256 and planned_tile(64, 0) == 1024


def refusals(lib):
    """every refusal of swv2_fss_ens_rows: -1, its name and the reason in the message, before any HIP call (the pointers are never touched)"""
    P = 4096
    M, K, S, B, C, H, W = 5, 3, 3, 2, 3, 8, 16
    span = C * H * W
    ok = lib.swv2_fss_ens_ws_bytes(B * C, H, W, M, K, S)

    def sc(*r):
        return (ctypes.c_int * len(r))(*r)

    def call(ens=P, ms=B * span, es=span, tar=P, ts=span, base=None, thr=P, tbs=0, scales=sc(0, 1, 4), M=M, K=K, S=S, below=0, B=B, C=C, H=H, W=W,
             ws=P, wb=ok, rows=P, ninv=P):
        return lib.swv2_fss_ens_rows(ens, ms, es, tar, ts, base, thr, tbs, scales, M, K, S, below, B, C, H, W, ws, wb, rows, ninv, None)
    cases = [(lambda: call(ens=None), b"null"), (lambda: call(tar=None), b"null"), (lambda: call(thr=None), b"null"), (lambda: call(scales=None), b"null"),
             (lambda: call(ws=None), b"null"), (lambda: call(rows=None), b"null"), (lambda: call(ninv=None), b"null"),
             (lambda: call(M=1), b"members M"), (lambda: call(M=65), b"members M"), (lambda: call(ms=B * span + 2), b"member stride"),
             (lambda: call(K=0), b"thresholds K"), (lambda: call(K=9), b"thresholds K"), (lambda: call(S=0), b"scales S"), (lambda: call(S=9), b"scales S"),
             (lambda: call(scales=sc(0, 1, 1)), b"ascending"), (lambda: call(scales=sc(2, 1, 4)), b"ascending"), (lambda: call(scales=sc(-1, 1, 4)), b"outside 0 .. 32"),
             (lambda: call(scales=sc(0, 1, 33)), b"outside 0 .. 32"), (lambda: call(scales=sc(0, 1, 8)), b"wider than W"), (lambda: call(W=18), b"W % 4"),
             (lambda: call(ens=P + 4), b"aligned"), (lambda: call(tar=P + 8), b"aligned"), (lambda: call(base=P + 4), b"aligned"),
             (lambda: call(ws=P + 4), b"aligned"), (lambda: call(thr=P + 2), b"aligned"), (lambda: call(rows=P + 4), b"aligned"),
             (lambda: call(ninv=P + 2), b"aligned"), (lambda: call(es=span + 1), b"stride"), (lambda: call(ts=H * W), b"stride"),
             (lambda: call(tbs=C * K - 1), b"stride"), (lambda: call(B=0), b"shape"), (lambda: call(H=0), b"shape"),
             (lambda: call(B=1 << 12, C=1 << 8), b"shape"), (lambda: call(H=1 << 15, W=1 << 15), b"shape"), (lambda: call(wb=ok - 1), b"workspace"),
             (lambda: call(wb=lib.swv2_fss_ens_ws_bytes(B * C, H, W, 3, K, S)), b"workspace"),           # a workspace made for fewer bit planes
             (lambda: call(wb=lib.swv2_fss_ws_bytes(B * C, H, W, K, S)), b"workspace")]                  # ... or for the deterministic entry point
    for fn, word in cases:
        assert fn() == -1
        msg = lib.swv2_last_error()
        assert msg.startswith(b"swv2_fss_ens_rows:") and word in msg, msg
    return len(cases)


def test_every_refusal_names_the_entry_point_without_a_gpu():
    assert refusals(L.load()) == 37


def test_header_and_ctypes_agree_on_the_ensemble_entry_points():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "swv2.h")).read(), flags=re.S)
    kinds = {"int": ctypes.c_int, "long": ctypes.c_long, "size_t": ctypes.c_size_t}
    seen = []
    for ret, name, args in re.findall(r"\b(int|size_t)\s+SWV2_ENS\s+(swv2_fss_ens_[a-z_]+)\s*\(([^)]*)\)\s*;", txt):
        want = [(ctypes.POINTER(ctypes.c_int) if a.startswith("const int*") else ctypes.c_void_p) if "*" in a else kinds[a.split()[0]]
                for a in (x.strip() for x in args.split(","))]
        res, argtypes = L.SYMBOLS[name]
        assert res is kinds[ret] and argtypes == want, name
        seen.append(name)
    assert sorted(seen) == ["swv2_fss_ens_band_rows", "swv2_fss_ens_rows", "swv2_fss_ens_ws_bytes"] and all(hasattr(L.load(), n) for n in seen)


def test_python_wrappers_refuse_what_the_kernels_cannot_read():
    from swin_v2_weather_amd import ops
    x = torch.zeros(1, 2, 4, 8)
    with pytest.raises(L.Swv2Error):
        ops.fss_ens_rows(x.expand(3, 1, 2, 4, 8), x, torch.zeros(1, 2, 1), (0, 1), torch.zeros(64, dtype=torch.int32))            # CPU tensors
    for bad in ((2, 4, 8, 1, 1, 1), (2, 4, 8, 65, 1, 1), (2, 4, 8, 2, 9, 1), (2, 4, 8, 2, 1, 9)):
        with pytest.raises(L.Swv2Error):
            ops.fss_ens_workspace(*bad, "cpu")
    assert ops.fss_ens_workspace(2, 4, 8, 5, 2, 3, "cpu").numel() * 4 == L.load().swv2_fss_ens_ws_bytes(2, 4, 8, 5, 2, 3)


# ---- the rollout and the command line on the CPU statement ----------------------------------------------------------------------
def test_rollout_with_ensemble_neighbourhoods_equals_the_scorer_called_by_hand():
    B, C, H, W, steps, M = 2, 3, 6, 12, 3, 4
    rng = np.random.default_rng(5)
    clim = fields(B, C, H, W)[2]
    truth = torch.tensor(rng.standard_normal((B, steps, C, H, W)).astype(np.float32))
    x0 = torch.tensor(rng.standard_normal((B, C, H, W)).astype(np.float32))
    sc = ForecastScorer(H, W, C, "cpu", climatology=clim)
    spec = EventSpec("anomaly", (0.0, 0.5), False)
    kw = dict(scorer=sc, events=spec, keep_forecast=True, score_control=True)
    ev = inference.ensemble_rollout(_Net(), x0, truth, steps, M, 0.3, 5, **kw)
    got = inference.ensemble_rollout(_Net(), x0, truth, steps, M, 0.3, 5, ensemble_neighbourhoods=(1, 4), member_neighbourhoods=True, **kw)
    plain = inference.ensemble_rollout(_Net(), x0, truth, steps, M, 0.3, 5, ensemble_neighbourhoods=(1, 4), **kw)
    assert ev.neighbourhoods is None and all(torch.equal(a, b) for a, b in zip(ev[:10], got[:10]))
    assert all(torch.equal(getattr(ev.events, k), getattr(got.events, k)) for k in ("sums", "wv", "hist", "n_invalid"))
    assert all(torch.equal(a, b) for a, b in zip(ev.control[:4], got.control[:4])) and torch.equal(ev.control.events.table, got.control.events.table)
    nb = got.neighbourhoods
    assert nb.scales == (1, 4) and tuple(nb.rows.shape) == (steps, B, C, 2, 2, H, 3) and tuple(nb.scores["pfss"].shape) == (steps, C, 2, 2)
    assert plain.neighbourhoods.member_rows is None and torch.equal(plain.neighbourhoods.rows, nb.rows)
    for s in range(steps):
        r = sc.ensemble_neighbourhood_score(got.forecast[:, s], truth[:, s], M, torch.tensor(spec.levels), (1, 4), anomaly=True, members=True)
        assert torch.equal(nb.rows[s], r.rows) and torch.equal(nb.n_invalid[s], r.n_invalid)
        assert torch.equal(nb.member_rows[s], r.member_rows) and torch.equal(nb.dispersion_rows[s], r.dispersion_rows)
        assert all(torch.equal(nb.scores[k][s], r.pooled[k]) for k in ("pfss", "fbs", "fss_uniform", "base_rate", "useful_scale"))
        assert torch.equal(nb.member_scores["fss"][s], r.member_scores["fss"]) and torch.equal(nb.dispersion_scores["fss"][s], r.dispersion_scores["fss"])
        want = ER.rows(got.forecast[:, s].reshape(M, B, C, H, W).numpy(), truth[:, s].numpy(), np.asarray(spec.levels, np.float32), (0, 1, 4), clim)[0]
        assert np.array_equal(nb.rows[s].numpy(), want[:, :, :, 1:])
    names = [("u", 0), ("v", 1)]
    txt = inference.lead_time_table(got.control, names, ensemble=got).splitlines()
    old = inference.lead_time_table(ev.control, names, ensemble=ev).splitlines()
    assert all(line.startswith(o) for line, o in zip(txt, old)) and "pfss" not in old[0]
    tail = [f"{k}{j}_r{r}_{n}" for k in ("pfss", "efss", "dfss") for j in (0, 1) for r in (1, 4) for n in ("u", "v")]
    assert txt[0].split()[-24:] == tail
    assert float(txt[2].split()[-24 + 7]) == pytest.approx(float(nb.scores["pfss"][1, 1, 1, 1]), abs=1e-5)
    assert float(txt[3].split()[-1]) == pytest.approx(float(nb.dispersion_scores["fss"][2, 1, 1, 1]), abs=1e-5)
    assert inference.lead_time_table(plain.control, names, ensemble=plain).splitlines()[0].split()[-8:] == tail[:8]
    with pytest.raises(ValueError, match="ensemble_neighbourhoods"):
        inference.ensemble_rollout(_Net(), x0, truth, steps, M, 0.3, 5, scorer=sc, events=spec, neighbourhoods=(1, 4))
    with pytest.raises(ValueError, match="EventSpec"):
        inference.ensemble_rollout(_Net(), x0, truth, steps, M, 0.3, 5, scorer=sc, ensemble_neighbourhoods=(1, 4))
    with pytest.raises(ValueError, match="member_neighbourhoods"):
        inference.ensemble_rollout(_Net(), x0, truth, steps, M, 0.3, 5, scorer=sc, events=spec, member_neighbourhoods=True)


def test_parser_takes_ensemble_scales_only_where_they_fit():
    ap = inference.build_parser()
    ens = ["--registry", "R", "--truth", "t.npy", "--ensemble", "3", "--perturbation", "0.1"]
    a = ap.parse_args(ens + ["--event-anomaly", "1.0", "2.0", "--ensemble-scales", "1", "4", "16", "--ensemble-member-scores"])
    assert a.ensemble_scales == [1, 4, 16] and a.ensemble_member_scores and a.event_scales is None
    a = ap.parse_args(ens + ["--event-quantile", "0.9", "--ensemble-scales", "0", "2"])
    assert a.ensemble_scales == [0, 2] and not a.ensemble_member_scores
    assert ap.parse_args(ens + ["--event-quantile", "0.9"]).ensemble_scales is None
    for bad in (ens + ["--ensemble-scales", "1"],                                                            # no events
                ["--registry", "R", "--truth", "t.npy", "--event-anomaly", "1.0", "--ensemble-scales", "1"],  # no ensemble
                ens + ["--event-anomaly", "1.0", "--ensemble-scales"],
                ens + ["--event-anomaly", "1.0", "--ensemble-scales", "4", "1"],
                ens + ["--event-anomaly", "1.0", "--ensemble-scales", "0", "33"],
                ens + ["--event-anomaly", "1.0", "--ensemble-scales", "1.5"],
                ens + ["--event-anomaly", "1.0", "--ensemble-member-scores"],
                ens + ["--event-quantile", "0.9", "--event-scales", "1"],                                     # stays an error
                ens + ["--event-quantile", "0.9", "--event-scales", "1", "--ensemble-scales", "1"]):
        with pytest.raises(SystemExit) as e:
            ap.parse_args(bad)
        assert e.value.code == 2, bad
