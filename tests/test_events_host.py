"""No GPU: the plain-torch statements of the forecast-event scores (utils/events.py) against the independent numpy statement of
tests/event_reference.py, the identities that pin the scores (no verification package is at hand to compare with), the host halves of
the six swv2_event_* entry points, the parser errors, and score_rollout / ensemble_rollout with events= on the CPU statements."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from swin_v2_weather_amd import _lib as L
from swin_v2_weather_amd import inference
from swin_v2_weather_amd.utils import events as E
from swin_v2_weather_amd.utils.weighted_acc_rmse import (EventSpec, ForecastScorer, brier_scores, contingency_scores, ensemble_event_sums_torch,
                                                         event_table_torch, latitude_weights, quantile_thresholds, reliability_scores)
from tests import event_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fields(M, B, C, H, W, seed=0, quantum=0.0):
    """truth [B, C, H, W]: N(0, 1) around a smooth base field [C, H, W]; members [M, B, C, H, W]: the truth + 0.75 N(0, 1), forecasts with
    skill, so that every cell of a table is populated; fp32"""
    rng = np.random.default_rng(100 * seed + 31 * M + 7 * B + 3 * C + H + W)
    y, x = np.linspace(0, np.pi, H)[:, None], np.linspace(0, 2 * np.pi, W)[None, :]
    base = ((1.0 + np.arange(C)[:, None, None] % 3) * 0.5 * np.sin(y + 0.3 * np.arange(C)[:, None, None]) * np.cos(2 * x)).astype(np.float32)
    tar = base[None] + rng.standard_normal((B, C, H, W), dtype=np.float32)
    ens = tar[None] + 0.75 * rng.standard_normal((M, B, C, H, W), dtype=np.float32)
    if quantum:
        ens, tar, base = (np.round(a / quantum) * quantum for a in (ens, tar, base))
    return ens.astype(np.float32), tar.astype(np.float32), base.astype(np.float32)


def _w(H, unit=False):
    return np.ones(H, np.float32) if unit or H < 2 else latitude_weights(H).numpy()


def _t(*arrays, dtype=None):
    return [None if a is None else torch.tensor(a if dtype is None else a.astype(dtype)) for a in arrays]


THR3 = np.array([-0.4, 0.2, 0.7], np.float32)


def _thr(kind, B, C):
    if kind == "K":
        return THR3
    t = THR3[None] + 0.125 * np.arange(C, dtype=np.float32)[:, None]
    return t if kind == "CK" else t[None] - 0.0625 * np.arange(B, dtype=np.float32)[:, None, None]


# ---- the statements against the reference ----------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("W,below,use_base,tk", [(8, False, False, "K"), (7, False, True, "CK"), (12, True, True, "BCK"), (5, True, False, "CK")])
def test_table_statement_against_the_reference(dtype, W, below, use_base, tk):
    M, B, C, H = 1, 2, 3, 12
    ens, tar, base = _fields(M, B, C, H, W)
    prd, base = ens[0], (base if use_base else None)
    thr, w = _thr(tk, B, C), _w(H)
    T, A, ninv = R.table(prd, tar, thr, w, base, below)
    assert (A > 0).all(), "the reference's own cells: all four non-empty for every threshold"
    tp, tt, tb, tw = _t(prd, tar, None, w, dtype=dtype)
    tb = None if base is None else torch.tensor(base)
    tab, ni = event_table_torch(tp, tt, torch.tensor(thr), tw, tb, below)
    assert tab.dtype == (torch.float32 if dtype is np.float32 else torch.float64) and ni.dtype == torch.int32
    R.judge((tab.numpy(), ni.numpy()), prd, tar, thr, w, H * W, base, below, u=R.U if dtype is np.float32 else 2.0 ** -53, tag=f"statement {tk}",
            ref=(T, A, ninv))
    tu, _ = event_table_torch(tp, tt, torch.tensor(thr), torch.ones(H, dtype=tp.dtype), tb, below)      # unit weights: exact integers
    R.judge((tu.numpy(), ni.numpy()), prd, tar, thr, _w(H, True), H * W, base, below, tag="statement, unit weights")


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("M,W,below,use_base,tk", [(2, 8, False, False, "K"), (7, 7, False, True, "CK"), (16, 12, True, True, "BCK"), (5, 5, True, False, "K")])
def test_ensemble_statement_against_the_reference(dtype, M, W, below, use_base, tk):
    B, C, H = 2, 3, 6
    ens, tar, base = _fields(M, B, C, H, W)
    base = base if use_base else None
    thr, w = _thr(tk, B, C), _w(H)
    ref = R.ens_sums(ens, tar, thr, w, base, below)
    assert (ref["hist"][..., 1, :].sum(-1) > 0).all() and (ref["hist"][..., 0, :].sum(-1) > ref["hist"][..., 1, :].sum(-1)).all()
    te, tt, tw = _t(ens, tar, w, dtype=dtype)
    tb = None if base is None else torch.tensor(base)
    s, wv, h, ni = ensemble_event_sums_torch(te, tt, torch.tensor(thr), tw, tb, below)
    assert h.dtype == torch.int32 and tuple(h.shape) == (B, C, 3, 2, M + 1) and tuple(s.shape) == (B, C, 3, 3)
    R.judge(dict(sums=s.numpy(), wv=wv.numpy(), hist=h.numpy(), n_invalid=ni.numpy()), ens, tar, thr, w, H * W, base, below,
            u=R.U if dtype is np.float32 else 2.0 ** -53, tag=f"ensemble statement M = {M}", ref=ref)


def test_ties_on_theta_are_no_event_either_way():
    """fields, base and thresholds on a lattice of 0.25: many values sit exactly on theta"""
    M, B, C, H, W = 4, 2, 2, 6, 8
    ens, tar, base = _fields(M, B, C, H, W, quantum=0.25)
    thr, w = np.array([-0.25, 0.0, 0.5], np.float32), _w(H, True)
    th = R.theta(R.thresholds_3d(thr, B, C), base)
    assert (tar[:, :, None] == th).mean() > 0.03 and (ens[0][:, :, None] == th).mean() > 0.03
    for below in (False, True):
        tab, ni = event_table_torch(*_t(ens[0], tar), torch.tensor(thr), torch.tensor(w), torch.tensor(base), below)
        R.judge((tab.numpy(), ni.numpy()), ens[0], tar, thr, w, H * W, base, below, tag="ties")
        s, wv, h, ni = ensemble_event_sums_torch(*_t(ens, tar), torch.tensor(thr), torch.tensor(w), torch.tensor(base), below)
        R.judge(dict(sums=s.numpy(), wv=wv.numpy(), hist=h.numpy(), n_invalid=ni.numpy()), ens, tar, thr, w, H * W, base, below, tag="ties")
    up = event_table_torch(*_t(ens[0], tar), torch.tensor(thr), torch.tensor(w), torch.tensor(base), False)[0]
    dn = event_table_torch(*_t(ens[0], tar), torch.tensor(thr), torch.tensor(w), torch.tensor(base), True)[0]
    assert float((up[..., 0] + dn[..., 0]).max()) < H * W           # a tie is an event in neither direction


def test_inf_is_valid_and_nan_removes_exactly_its_point():
    M, B, C, H, W = 3, 2, 3, 5, 8
    ens, tar, base = _fields(M, B, C, H, W)
    ens, tar, base = ens.copy(), tar.copy(), base.copy()
    ens[0, 0, 0, 1, 2], tar[0, 0, 2, 3], ens[1, 0, 0, 0, 0], tar[1, 0, 4, 7] = np.inf, -np.inf, -np.inf, np.inf
    ens[0, 1, 1, 2, 3] = np.nan              # prediction (member 0)
    tar[1, 2, 0, 0] = np.nan                 # truth
    ens[2, 0, 2, 4, 4] = np.nan              # a member that is not the prediction
    base[1, 1, 1] = np.nan                   # base: every sample's channel 1
    thr, w = THR3, _w(H)
    T, A, ninv = R.table(ens[0], tar, thr, w, base)
    assert ninv.tolist() == [[0, 1, 0], [0, 2, 1]]
    tab, ni = event_table_torch(*_t(ens[0], tar), torch.tensor(thr), torch.tensor(w), torch.tensor(base))
    R.judge((tab.numpy(), ni.numpy()), ens[0], tar, thr, w, H * W, base, tag="nan / inf", ref=(T, A, ninv))
    clean = event_table_torch(*_t(np.nan_to_num(ens[0], nan=0.0), tar), torch.tensor(thr), torch.tensor(w), torch.tensor(base))[0]
    assert torch.equal(clean[0, 0], tab[0, 0]) and torch.equal(clean[0, 2], tab[0, 2])      # planes without the NaN: the same bits
    ref = R.ens_sums(ens, tar, thr, w, base)
    assert ref["n_invalid"].tolist() == [[0, 1, 1], [0, 2, 1]]
    s, wv, h, ni = ensemble_event_sums_torch(*_t(ens, tar), torch.tensor(thr), torch.tensor(w), torch.tensor(base))
    R.judge(dict(sums=s.numpy(), wv=wv.numpy(), hist=h.numpy(), n_invalid=ni.numpy()), ens, tar, thr, w, H * W, base, tag="nan / inf", ref=ref)


# ---- identities, fp64 --------------------------------------------------------------------------------------------------------
def test_identities_of_the_tables_and_scores():
    M, B, C, H, W = 9, 2, 3, 8, 12
    ens, tar, base = _fields(M, B, C, H, W)
    w, thr = _w(H), THR3
    te, tt, tw, tb = *_t(ens, tar, w, dtype=np.float64), torch.tensor(base)
    tab, _ = event_table_torch(te[0], tt, torch.tensor(thr), tw, tb)
    s, wv, h, _ = ensemble_event_sums_torch(te, tt, torch.tensor(thr), tw, tb)
    assert torch.allclose(tab.sum(-1), wv.unsqueeze(-1).expand(-1, -1, 3), rtol=1e-13, atol=0)                  # a + b + c + d = W_v
    swapped, _ = event_table_torch(tt, te[0], torch.tensor(thr), tw, tb)
    assert torch.equal(swapped, tab[..., [0, 2, 1, 3]])                                                        # the transpose
    sc = contingency_scores(tab)
    want = R.scores(tab.numpy())
    for k in E.CONTINGENCY_NAMES:
        assert np.allclose(sc[k].numpy(), want[k], rtol=1e-13, atol=0, equal_nan=True), k
    assert set(sc) == set(E.CONTINGENCY_NAMES) and all(v.dtype == torch.float64 for v in sc.values())
    # unit weights: Brier from S_e = Brier from the counts; REL - RES + UNC = BS
    one = torch.ones(H, dtype=torch.float64)
    s1, wv1, h1, _ = ensemble_event_sums_torch(te, tt, torch.tensor(thr), one, tb)
    bs = brier_scores(s1, wv1, M)
    assert np.allclose(bs["brier"].numpy(), R.brier_from_hist(h1.numpy()), rtol=1e-13, atol=0)
    rel = reliability_scores(h1[..., 0, :], h1[..., 1, :])
    assert float((rel["reliability"] - rel["resolution"] + rel["uncertainty"] - bs["brier"]).abs().max()) <= 1e-12
    assert float((bs["brier_skill"] - (1 - bs["brier"] / rel["uncertainty"])).abs().max()) <= 1e-12
    assert bool((bs["fair_brier"] < bs["brier"]).all()) and bool(((rel["roc_area"] > 0.5) & (rel["roc_area"] < 1)).all())
    assert torch.equal(h1, h)                                                                                  # counts carry no weights
    # pooled scores are the scores of the summed tables
    pooled = contingency_scores(tab.sum(0))
    assert not torch.allclose(pooled["ets"], sc["ets"].mean(0), rtol=1e-6, atol=0)
    a, b, c, d = tab.sum(0).unbind(-1)
    assert torch.allclose(pooled["csi"], a / (a + b + c), rtol=1e-15, atol=0)


def test_two_identical_members_reproduce_the_deterministic_table():
    _, B, C, H, W = 1, 2, 3, 6, 8
    ens, tar, base = _fields(1, B, C, H, W)
    two = np.concatenate([ens, ens], axis=0)
    tab, _ = event_table_torch(*_t(ens[0], tar), torch.tensor(THR3), torch.ones(H))
    s, wv, h, _ = ensemble_event_sums_torch(*_t(two, tar), torch.tensor(THR3), torch.ones(H))
    h = h.to(torch.float32)
    assert bool((h[..., 1] == 0).all())                                        # n is 0 or 2
    got = torch.stack([h[..., 1, 2], h[..., 0, 2] - h[..., 1, 2], h[..., 1, 0], h[..., 0, 0] - h[..., 1, 0]], dim=-1)
    assert torch.equal(got, tab)
    assert torch.equal(s[..., 0], 4 * (tab[..., 1] + tab[..., 2])) and bool((s[..., 1] == 0).all())            # S_e = M^2 (b + c), S_f = 0


def test_roc_area_of_a_perfect_and_of_a_constant_probability_ensemble():
    M = 5
    nf = torch.tensor([[70, 0, 0, 0, 0, 30], [0, 0, 100, 0, 0, 0]])
    no = torch.tensor([[0, 0, 0, 0, 0, 30], [0, 0, 40, 0, 0, 0]])
    r = reliability_scores(nf, no)
    assert r["roc_area"].tolist() == [1.0, 0.5]
    assert r["reliability"][0].item() == 0.0 and r["resolution"][0].item() == pytest.approx(0.21) and r["resolution"][1].item() == 0.0
    assert r["reliability"][1].item() == pytest.approx((2 / M - 0.4) ** 2, abs=1e-15)


def test_closed_form_tables_on_a_hand_made_field():
    """4 x 8: prediction 0 .. 31 row by row, truth the same shifted by 4 (one row); event: value > 15.5"""
    prd = np.arange(32, dtype=np.float32).reshape(1, 1, 4, 8)
    tar = prd + 4.0
    thr = np.array([15.5], np.float32)
    tab, ni = event_table_torch(*_t(prd, tar), torch.tensor(thr), torch.ones(4))
    assert tab.reshape(-1).tolist() == [16.0, 0.0, 4.0, 12.0] and ni.item() == 0          # P: 16 .. 31; O: 12 .. 31 (prd index)
    w = torch.tensor([1.0, 2.0, 3.0, 4.0])
    tab, _ = event_table_torch(*_t(prd, tar), torch.tensor(thr), w)
    assert tab.reshape(-1).tolist() == [8 * 3.0 + 8 * 4.0, 0.0, 4 * 2.0, 8 * 1.0 + 4 * 2.0]
    tab, _ = event_table_torch(*_t(prd, tar), torch.tensor(thr), torch.ones(4), below=True)
    assert tab.reshape(-1).tolist() == [12.0, 4.0, 0.0, 16.0]
    sc = contingency_scores(torch.tensor([16.0, 0.0, 4.0, 12.0]))
    assert sc["pod"].item() == 0.8 and sc["far"].item() == 0.0 and sc["csi"].item() == 0.8 and sc["freq_bias"].item() == 0.8
    assert sc["base_rate"].item() == 0.625 and sc["ets"].item() == pytest.approx((16 - 10) / (20 - 10))
    # base field = the row index: theta = row + 0.5 -> P where prd > row + 0.5
    base = np.broadcast_to(np.arange(4, dtype=np.float32)[:, None], (1, 4, 8)).copy()
    tab, _ = event_table_torch(*_t(prd, prd), torch.tensor([0.5], dtype=torch.float32), torch.ones(4), torch.tensor(base))
    assert tab.reshape(-1).tolist() == [31.0, 0.0, 0.0, 1.0]
    # ensemble of 3: members prd - 8, prd, prd + 8 against truth prd, event > 15.5: n = 0 below 8, 1 for 8 .. 15, 2 for 16 .. 23, 3 above
    ens = np.stack([prd - 8, prd, prd + 8])
    s, wv, h, _ = ensemble_event_sums_torch(*_t(ens, prd), torch.tensor(thr), torch.ones(4))
    assert h[0, 0, 0, 0].tolist() == [8, 8, 8, 8] and h[0, 0, 0, 1].tolist() == [0, 0, 8, 8] and wv.item() == 32.0
    assert s.reshape(-1).tolist() == [8 * 1.0 + 8 * 1.0, 8 * 2.0 + 8 * 2.0, 16.0]


def test_a_threshold_above_every_value_leaves_d_alone():
    M, B, C, H, W = 3, 1, 2, 5, 8
    ens, tar, _ = _fields(M, B, C, H, W)
    tab, _ = event_table_torch(*_t(ens[0], tar), torch.tensor([1.0e6]), torch.ones(H))
    assert tab.reshape(-1, 4).tolist() == [[0.0, 0.0, 0.0, float(H * W)]] * C
    sc = contingency_scores(tab)
    nan = {k: bool(torch.isnan(v).all()) for k, v in sc.items()}
    assert nan == dict(base_rate=False, freq_bias=True, pod=True, far=True, csi=True, ets=True, sedi=True) and bool((sc["base_rate"] == 0).all())
    s, wv, h, _ = ensemble_event_sums_torch(*_t(ens, tar), torch.tensor([1.0e6]), torch.ones(H))
    assert bool((s == 0).all()) and bool((h[..., 0, 0] == H * W).all()) and int(h.sum()) == B * C * H * W
    bs = brier_scores(s, wv, M)
    assert bool((bs["brier"] == 0).all()) and bool(torch.isnan(bs["brier_skill"]).all())
    finite = event_table_torch(*_t(ens[0], tar), torch.tensor([0.0, 1.0e6]), torch.ones(H))[0]
    assert not torch.isnan(contingency_scores(finite)["ets"][..., 0]).any()             # the NaN stays in its (channel, threshold)


def test_quantile_thresholds_are_the_planes_own_quantiles():
    _, tar, _ = _fields(1, 2, 3, 6, 8)
    t = quantile_thresholds(torch.tensor(tar), [0.5, 0.9])
    assert tuple(t.shape) == (2, 3, 2) and t.dtype == torch.float32
    assert torch.equal(t[1, 2], torch.quantile(torch.tensor(tar[1, 2]).reshape(-1), torch.tensor([0.5, 0.9])))


# ---- the host halves of the entry points -----------------------------------------------------------------------------------
NAMES = ["swv2_event_ens_finalize", "swv2_event_ens_sums", "swv2_event_ens_ws_bytes", "swv2_event_finalize", "swv2_event_sums", "swv2_event_ws_bytes"]


def test_workspace_queries_and_chain_lengths():
    assert L.ABI_VERSION == 113 and "events.hip" in L.SOURCES
    lib = L.load()
    for (B, C, H, W) in ((1, 1, 1, 4), (2, 3, 5, 8), (2, 73, 720, 1440), (1, 2100, 2, 4), (3, 5, 16, 32)):
        slices = lib.swv2_score_slices(B * C, H, W)
        assert slices == R.plan_slices(B * C)
        for K in range(1, 9):
            assert lib.swv2_event_ws_bytes(B * C, H, W, K) == B * C * slices * (16 * K + 4)
            for M in (2, 7, 50, 64):
                assert lib.swv2_event_ens_ws_bytes(B * C, H, W, M, K) == B * C * slices * (16 * K + 4 + 8 * K * (M + 1))
    for bad in ((0, 4, 4, 1), (4, 0, 4, 1), (4, 4, 0, 1), (4, 4, 4, 0), (4, 4, 4, 9), (-1, 4, 4, 1)):
        assert lib.swv2_event_ws_bytes(*bad) == 0, bad
    for bad in ((0, 4, 4, 2, 1), (4, 4, 4, 1, 1), (4, 4, 4, 65, 1), (4, 4, 4, 2, 0), (4, 4, 4, 2, 9)):
        assert lib.swv2_event_ens_ws_bytes(*bad) == 0, bad
    assert R.chain_length(1, 4, 2048) == 4 + 14 + 32 and R.chain_length(2, 4, 1) == 4 + 14 + 1
    assert R.chain_length(4, 1028, 1) == 4 * 5 + 15 and R.chain_length(8, 1028, 1) == 4 * 9 + 15
    assert R.chain_length(720, 1440, 14) == 4 * 73 + 15           # the production pair of samples: 146 planes, 14 slices of 74 056 or 74 060 elements


def test_every_refusal_returns_invalid_with_the_entry_points_name_and_without_a_gpu():
    """Arguments are checked before anything is launched, so the pointers only have to be non-null here: a refused call touches nothing."""
    lib = L.load()
    P = 4096
    M, K, B, C, H, W = 5, 3, 2, 3, 8, 16
    span = C * H * W
    ok, oke = lib.swv2_event_ws_bytes(B * C, H, W, K), lib.swv2_event_ens_ws_bytes(B * C, H, W, M, K)

    def sums(prd=P, ps=span, tar=P, ts=span, base=None, thr=P, tbs=0, w=P, K=K, below=0, B=B, C=C, H=H, W=W, ws=P, wb=ok):
        return lib.swv2_event_sums(prd, ps, tar, ts, base, thr, tbs, w, K, below, B, C, H, W, ws, wb, None)

    def fin(ws=P, wb=ok, K=K, B=B, C=C, H=H, W=W, table=P, ninv=P):
        return lib.swv2_event_finalize(ws, wb, K, B, C, H, W, table, ninv, None)

    def esums(ens=P, ms=B * span, bs=span, tar=P, ts=span, base=None, thr=P, tbs=0, w=P, M=M, K=K, below=0, B=B, C=C, H=H, W=W, ws=P, wb=oke):
        return lib.swv2_event_ens_sums(ens, ms, bs, tar, ts, base, thr, tbs, w, M, K, below, B, C, H, W, ws, wb, None)

    def efin(ws=P, wb=oke, M=M, K=K, B=B, C=C, H=H, W=W, s=P, wv=P, h=P, ninv=P):
        return lib.swv2_event_ens_finalize(ws, wb, M, K, B, C, H, W, s, wv, h, ninv, None)
    cases = {
        b"swv2_event_sums": [(lambda: sums(prd=None), b"null"), (lambda: sums(tar=None), b"null"), (lambda: sums(thr=None), b"null"),
                             (lambda: sums(w=None), b"null"), (lambda: sums(ws=None), b"null"), (lambda: sums(K=0), b"thresholds K"),
                             (lambda: sums(K=9), b"thresholds K"), (lambda: sums(W=18), b"W % 4"), (lambda: sums(prd=P + 4), b"aligned"),
                             (lambda: sums(tar=P + 8), b"aligned"), (lambda: sums(base=P + 4), b"aligned"), (lambda: sums(ws=P + 4), b"aligned"),
                             (lambda: sums(thr=P + 2), b"aligned"), (lambda: sums(ps=span + 1), b"stride"), (lambda: sums(ts=H * W), b"stride"),
                             (lambda: sums(tbs=C * K - 1), b"stride"), (lambda: sums(W=0), b"shape"), (lambda: sums(B=0), b"shape"),
                             (lambda: sums(B=1 << 12, C=1 << 8), b"shape"), (lambda: sums(H=1 << 15, W=1 << 15), b"shape"),
                             (lambda: sums(wb=ok - 1), b"workspace"), (lambda: sums(wb=lib.swv2_event_ws_bytes(B * C, H, W, K - 1)), b"workspace")],
        b"swv2_event_finalize": [(lambda: fin(ws=None), b"null"), (lambda: fin(table=None), b"null"), (lambda: fin(ninv=None), b"null"),
                                 (lambda: fin(K=0), b"thresholds K"), (lambda: fin(K=9), b"thresholds K"), (lambda: fin(table=P + 4), b"aligned"),
                                 (lambda: fin(ws=P + 8), b"aligned"), (lambda: fin(ninv=P + 2), b"aligned"), (lambda: fin(C=0), b"shape"),
                                 (lambda: fin(wb=ok - 4), b"workspace")],
        b"swv2_event_ens_sums": [(lambda: esums(ens=None), b"null"), (lambda: esums(tar=None), b"null"), (lambda: esums(thr=None), b"null"),
                                 (lambda: esums(w=None), b"null"), (lambda: esums(ws=None), b"null"), (lambda: esums(K=0), b"thresholds K"),
                                 (lambda: esums(K=9), b"thresholds K"), (lambda: esums(M=1), b"members"), (lambda: esums(M=65), b"members"),
                                 (lambda: esums(W=18), b"W % 4"), (lambda: esums(ens=P + 4), b"aligned"), (lambda: esums(tar=P + 8), b"aligned"),
                                 (lambda: esums(base=P + 4), b"aligned"), (lambda: esums(ws=P + 4), b"aligned"), (lambda: esums(thr=P + 1), b"aligned"),
                                 (lambda: esums(ms=B * span + 2), b"stride"), (lambda: esums(bs=span + 1), b"stride"), (lambda: esums(ts=H * W), b"stride"),
                                 (lambda: esums(tbs=1), b"stride"), (lambda: esums(B=0), b"shape"), (lambda: esums(H=1 << 15, W=1 << 15), b"shape"),
                                 (lambda: esums(wb=oke - 1), b"workspace"),
                                 (lambda: esums(wb=lib.swv2_event_ens_ws_bytes(B * C, H, W, M - 1, K)), b"workspace")],
        b"swv2_event_ens_finalize": [(lambda: efin(ws=None), b"null"), (lambda: efin(s=None), b"null"), (lambda: efin(wv=None), b"null"),
                                     (lambda: efin(h=None), b"null"), (lambda: efin(ninv=None), b"null"), (lambda: efin(K=9), b"thresholds K"),
                                     (lambda: efin(M=1), b"members"), (lambda: efin(M=65), b"members"), (lambda: efin(ws=P + 8), b"aligned"),
                                     (lambda: efin(h=P + 2), b"aligned"), (lambda: efin(C=0), b"shape"), (lambda: efin(wb=oke - 4), b"workspace")]}
    for name, calls in cases.items():
        for call, word in calls:
            assert call() == -1
            msg = lib.swv2_last_error()
            assert msg.startswith(name + b":") and word in msg, msg
    with pytest.raises(L.Swv2Error):
        L.check(sums(W=18), "swv2_event_sums")
    assert sums(B=1, ps=0, ts=0, tbs=1, wb=0) == -1 and b"workspace" in lib.swv2_last_error()      # B == 1: the batch strides are not looked at


def test_header_and_ctypes_agree_on_the_event_entry_points():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "swv2.h")).read(), flags=re.S)
    kinds = {"int": ctypes.c_int, "long": ctypes.c_long, "size_t": ctypes.c_size_t}
    seen = []
    for ret, name, args in re.findall(r"\b(int|size_t)\s+(swv2_event_[a-z_]+)\s*\(([^)]*)\)\s*;", txt):
        want = [ctypes.c_void_p if "*" in a else kinds[a.split()[0]] for a in (x.strip() for x in args.split(","))]
        res, argtypes = L.SYMBOLS[name]
        assert res is kinds[ret] and argtypes == want, name
        seen.append(name)
    assert sorted(seen) == NAMES
    lib = L.load()
    assert all(hasattr(lib, n) for n in seen)


def test_python_wrappers_refuse_what_the_kernels_cannot_read():
    from swin_v2_weather_amd import ops
    x = torch.zeros(1, 2, 4, 8)
    with pytest.raises(L.Swv2Error):
        ops.event_sums(x, x, torch.zeros(1, 2, 1), torch.ones(4), torch.zeros(64))
    with pytest.raises(L.Swv2Error):
        ops.event_workspace(2, 4, 8, 9, "cpu")
    with pytest.raises(L.Swv2Error):
        ops.ens_event_workspace(2, 4, 8, 65, 1, "cpu")
    with pytest.raises(ValueError):
        E.expand_thresholds(torch.zeros(3, 2), 1, 2)               # [C, K] with the wrong C


# ---- the scorer, the rollouts and the command line on the CPU statements -------------------------------------------------------
def test_scorer_methods_on_the_cpu_statements():
    M, B, C, H, W = 4, 2, 3, 6, 10                                 # W % 4 != 0 and CPU tensors: the statements
    ens, tar, clim = _fields(M, B, 5, H, W)
    te, tt = torch.tensor(ens).reshape(M * B, 5, H, W), torch.tensor(tar)
    sc = ForecastScorer(H, W, C, "cpu", climatology=clim[1:4])
    thr = torch.linspace(-1.0, 1.0, 11)                            # K = 11
    r = sc.event_score(te[:B], tt, thr, anomaly=True, coff_prd=1, coff_tar=1)
    tab, ni = event_table_torch(te[:B, 1:4], tt[:, 1:4], thr, sc.w, torch.tensor(clim[1:4]))
    assert torch.equal(r.table, tab) and torch.equal(r.n_invalid, ni) and tuple(r.scores["ets"].shape) == (B, C, 11) and tuple(r.pooled["ets"].shape) == (C, 11)
    assert torch.equal(r.pooled["pod"], contingency_scores(tab.double().sum(0))["pod"])
    e = sc.ensemble_event_score(te, tt, M, thr[:3], base=clim[1:4], below=True, coff_ens=1, coff_tar=1)
    s, wv, h, ni = ensemble_event_sums_torch(te.unflatten(0, (M, B))[:, :, 1:4], tt[:, 1:4], thr[:3], sc.w, torch.tensor(clim[1:4]), True)
    assert torch.equal(e.sums, s) and torch.equal(e.hist, h) and torch.equal(e.wv, wv) and tuple(e.reliability["roc_area"].shape) == (C, 3)
    assert torch.equal(e.pooled["brier"], brier_scores(s.double().sum(0), wv.double().sum(0), M)["brier"]) and len(sc._ws) == 0
    with pytest.raises(ValueError):
        ForecastScorer(H, W, C, "cpu").event_score(te[:B], tt, thr, anomaly=True)          # no climatology
    with pytest.raises(ValueError):
        sc.event_score(te[:B], tt, thr, anomaly=True, base=clim[1:4])


class _Net:
    """a stand-in for the model in the rollout loops: damps the fields and shifts them one column"""
    out_chans = 3

    def forward_rollout(self, x, out, coff, extra):
        y = 0.9 * torch.roll(x[:, :3], 1, dims=-1)
        out[:, coff:coff + 3] = y
        return None, y if extra is None else torch.cat([y, extra], 1)


def test_rollouts_with_events_equal_the_scorer_called_by_hand():
    M, B, C, H, W, steps = 4, 2, 3, 6, 8, 3
    ens, tar, clim = _fields(steps, B, C, H, W, seed=3)
    x0, truth = torch.tensor(ens[0]), torch.tensor(ens).permute(1, 0, 2, 3, 4).contiguous()
    sc = ForecastScorer(H, W, C, "cpu", climatology=clim)
    spec = EventSpec("anomaly", (0.0, 0.5), False)
    plain = inference.score_rollout(_Net(), x0, truth, steps, scorer=sc, keep_forecast=True)
    got = inference.score_rollout(_Net(), x0, truth, steps, scorer=sc, keep_forecast=True, events=spec)
    assert plain.events is None and len(got) == 6 and got.tqe is None and all(torch.equal(a, b) for a, b in zip(plain[:5], got[:5]))
    ev = got.events
    assert tuple(ev.table.shape) == (steps, B, C, 2, 4) and tuple(ev.scores["ets"].shape) == (steps, C, 2) and ev.spec is spec
    for s in range(steps):
        r = sc.event_score(got.forecast[:, s], truth[:, s], torch.tensor(spec.levels), anomaly=True)
        assert torch.equal(ev.table[s], r.table) and torch.equal(ev.n_invalid[s], r.n_invalid)
        assert all(torch.equal(ev.scores[k][s], r.pooled[k]) for k in E.CONTINGENCY_NAMES)
    q = EventSpec("quantile", (0.25,), True)
    gq = inference.score_rollout(_Net(), x0, truth, steps, scorer=ForecastScorer(H, W, C, "cpu"), keep_forecast=True, events=q)
    thr = quantile_thresholds(truth[:, 1], q.levels)
    assert torch.equal(gq.events.thresholds[1], thr)
    assert torch.equal(gq.events.table[1], event_table_torch(gq.forecast[:, 1], truth[:, 1], thr, sc.w, None, True)[0])
    assert float(gq.events.scores["base_rate"][1].mean()) == pytest.approx(0.25, abs=0.03)
    with pytest.raises(ValueError):
        inference.score_rollout(_Net(), x0, truth, steps, scorer=ForecastScorer(H, W, C, "cpu"), events=spec)      # anomaly without a climatology
    pe = inference.ensemble_rollout(_Net(), x0, truth, steps, M, 0.3, 5, scorer=sc, keep_forecast=True, score_control=True)
    ge = inference.ensemble_rollout(_Net(), x0, truth, steps, M, 0.3, 5, scorer=sc, keep_forecast=True, score_control=True, events=spec)
    assert pe.events is None and len(ge) == 11 and all(torch.equal(a, b) for a, b in zip(pe[:10], ge[:10]))
    assert all(torch.equal(a, b) for a, b in zip(pe.control[:4], ge.control[:4])) and pe.control.events is None
    for s in range(steps):
        r = sc.ensemble_event_score(ge.forecast[:, s], truth[:, s], M, torch.tensor(spec.levels), anomaly=True)
        assert torch.equal(ge.events.sums[s], r.sums) and torch.equal(ge.events.hist[s], r.hist) and torch.equal(ge.events.wv[s], r.wv)
        assert all(torch.equal(ge.events.scores[k][s], r.pooled[k]) for k in E.BRIER_NAMES)
        assert all(torch.equal(ge.events.scores[k][s], r.reliability[k]) for k in E.RELIABILITY_NAMES)
        c = sc.event_score(ge.forecast[:B, s], truth[:, s], torch.tensor(spec.levels), anomaly=True)
        assert torch.equal(ge.control.events.table[s], c.table)
    txt = inference.lead_time_table(ge.control, [("u", 0), ("v", 1)], ensemble=ge).splitlines()
    assert txt[0].split()[-8:] == ["ets0_u", "ets0_v", "ets1_u", "ets1_v", "bs0_u", "bs0_v", "bs1_u", "bs1_v"]
    assert float(txt[2].split()[-1]) == pytest.approx(float(ge.events.scores["brier"][1, 1, 1]), abs=1e-5)
    old = inference.lead_time_table(pe.control, [("u", 0)], ensemble=pe).splitlines()                  # without events: the columns of before
    assert old[0].split() == ["lead_h", "rmse_u", "acc_u", "crps_u", "spread_u", "ens_rmse_u"]
    assert all(line.startswith(o) for line, o in zip(inference.lead_time_table(ge.control, [("u", 0)], ensemble=ge).splitlines(), old))


def test_parser_refuses_event_flags_that_do_not_fit():
    ap = inference.build_parser()
    a = ap.parse_args(["--registry", "R", "--truth", "t.npy", "--event-anomaly", "1.0", "2.0", "--event-below"])
    assert (a.event_anomaly, a.event_quantile, a.event_below) == ([1.0, 2.0], None, True)
    b = ap.parse_args(["--registry", "R", "--truth", "t.npy", "--event-quantile", "0.99", "--score-grid", "5.625"])
    assert (b.event_anomaly, b.event_quantile, b.event_below, b.score_grid) == (None, [0.99], False, 5.625)
    c = ap.parse_args(["--registry", "R", "--truth", "t.npy"])
    assert (c.event_anomaly, c.event_quantile, c.event_below) == (None, None, False)                   # without the flags nothing changes
    for bad in (["--event-anomaly", "1.0"], ["--event-quantile", "0.9"],                                # no --truth
                ["--truth", "t.npy", "--event-anomaly", "1.0", "--event-quantile", "0.9"],
                ["--truth", "t.npy", "--event-below"], ["--truth", "t.npy", "--event-quantile", "1.5"],
                ["--truth", "t.npy", "--event-anomaly"]):
        with pytest.raises(SystemExit) as e:
            ap.parse_args(["--registry", "R"] + bad)
        assert e.value.code == 2, bad
