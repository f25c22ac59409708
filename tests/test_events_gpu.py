"""GPU (-m gpu): swv2_event_sums / _finalize and swv2_event_ens_sums / _finalize through the C ABI into sentinel-guarded buffers, judged
element by element by tests/event_reference.py (every bound is derived there; counts and unit-weight tables must be exact), then the
Python layer on top of them: ForecastScorer.event_score / ensemble_event_score, RegriddedScorer, the rollouts with events= and the
command line."""
import functools
import json

import numpy as np
import pytest
import torch

from tests import event_reference as R
from tests.plane_harness import Guarded, _weights, dev, lib  # noqa: F401  (dev, lib: fixtures)

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _fields(M, B, C, H, W, offset=0.0, quantum=0.0, seed=0):
    """truth [B, C, H, W]: N(0, 1) around a smooth base field [C, H, W] (+ offset); members [M, B, C, H, W]: the truth + 0.75 N(0, 1), so
    every cell of a table is populated; fp32, optionally rounded to multiples of `quantum`; made once per shape and never modified.
    A plane of four points is set by hand: one point per cell at threshold 0."""
    rng = np.random.default_rng(1000 * seed + 31 * M + 7 * B + 3 * C + H + W)
    y, x = np.linspace(0, np.pi, H)[:, None], np.linspace(0, 2 * np.pi, W)[None, :]
    base = (offset + (1.0 + np.arange(C)[:, None, None] % 3) * 0.5 * np.sin(y + 0.3 * np.arange(C)[:, None, None]) * np.cos(2 * x)).astype(np.float32)
    tar = base[None] + rng.standard_normal((B, C, H, W), dtype=np.float32)
    ens = tar[None] + 0.75 * rng.standard_normal((M, B, C, H, W), dtype=np.float32)
    if H * W == 4:
        tar[...] = offset + np.array([1, -1, 1, -1], np.float32)
        ens[...] = offset + np.array([1, 1, -1, -1], np.float32)
        ens[1:, ..., 1] = offset - 1.0                          # (further members: the second point is forecast by member 0 alone)
    if quantum:
        ens, tar, base = (np.round(a / quantum) * quantum for a in (ens, tar, base))
    ens, tar, base = ens.astype(np.float32), tar.astype(np.float32), base.astype(np.float32)
    for a in (ens, tar, base):
        a.setflags(write=False)
    return ens, tar, base


def _thr(K, offset=0.0):
    return (offset + (np.linspace(-0.6, 0.8, K) if K > 1 else np.zeros(1))).astype(np.float32)


def _populated(A, H, W):
    """the reference's own verdict that a case is not degenerate: every cell kind is populated -- in every plane where a plane has the
    points for it, somewhere in the batch otherwise"""
    return bool((A > 0).all()) if H * W >= 160 or H * W == 4 else bool((A.sum(axis=(0, 1)) > 0).all())


def _d(dev, *arrays):
    return [None if a is None else torch.tensor(a).to(dev) for a in arrays]


def _thr_dev(dev, thr, B, C):
    t = torch.tensor(np.ascontiguousarray(R.thresholds_3d(thr, B, C))).to(dev)
    return t, (C * t.shape[2] if t.shape[0] == B and B > 1 else 0)


def _launch(lib, dev, prd, tar, thr, w, base=None, below=False, ws_fill=None):
    """prd, tar [B, C, H, W] device tensors or channel-block views, thr numpy -> (Guarded with ws / table / ninv, slices)"""
    from swin_v2_weather_amd import _lib as L
    B, C, H, W = prd.shape
    t, tbs = _thr_dev(dev, thr, B, C)
    K = t.shape[2]
    slices = lib.swv2_score_slices(B * C, H, W)
    wsb = lib.swv2_event_ws_bytes(B * C, H, W, K)
    assert wsb == B * C * slices * (16 * K + 4)
    g = Guarded(dev, ws=wsb // 4, table=B * C * K * 4, ninv=(B * C, torch.int32))
    if ws_fill is not None:
        g.ints("ws").fill_(ws_fill)
    st = torch.cuda.current_stream().cuda_stream
    span = C * H * W
    L.check(lib.swv2_event_sums(prd.data_ptr(), prd.stride(0) if B > 1 else span, tar.data_ptr(), tar.stride(0) if B > 1 else span,
                                None if base is None else base.data_ptr(), t.data_ptr(), tbs, w.data_ptr(), K, int(below), B, C, H, W,
                                g["ws"].data_ptr(), wsb, st), "swv2_event_sums")
    L.check(lib.swv2_event_finalize(g["ws"].data_ptr(), wsb, K, B, C, H, W, g["table"].data_ptr(), g["ninv"].data_ptr(), st), "swv2_event_finalize")
    torch.cuda.synchronize()
    return g, slices


def _launch_ens(lib, dev, ens, tar, thr, w, base=None, below=False, ws_fill=None):
    from swin_v2_weather_amd import _lib as L
    M, B, C, H, W = ens.shape
    t, tbs = _thr_dev(dev, thr, B, C)
    K = t.shape[2]
    slices = lib.swv2_score_slices(B * C, H, W)
    wsb = lib.swv2_event_ens_ws_bytes(B * C, H, W, M, K)
    assert wsb == B * C * slices * (16 * K + 4 + 8 * K * (M + 1))
    g = Guarded(dev, ws=wsb // 4, sums=B * C * K * 3, wv=B * C, hist=(B * C * K * 2 * (M + 1), torch.int32), ninv=(B * C, torch.int32))
    if ws_fill is not None:
        g.ints("ws").fill_(ws_fill)
    st = torch.cuda.current_stream().cuda_stream
    span = C * H * W
    L.check(lib.swv2_event_ens_sums(ens.data_ptr(), ens.stride(0), ens.stride(1) if B > 1 else span, tar.data_ptr(), tar.stride(0) if B > 1 else span,
                                    None if base is None else base.data_ptr(), t.data_ptr(), tbs, w.data_ptr(), M, K, int(below), B, C, H, W,
                                    g["ws"].data_ptr(), wsb, st), "swv2_event_ens_sums")
    L.check(lib.swv2_event_ens_finalize(g["ws"].data_ptr(), wsb, M, K, B, C, H, W, g["sums"].data_ptr(), g["wv"].data_ptr(), g["hist"].data_ptr(),
                                        g["ninv"].data_ptr(), st), "swv2_event_ens_finalize")
    torch.cuda.synchronize()
    return g, slices


def _intact(g):
    assert g.guards_intact(), "a kernel wrote outside its outputs"
    for k in g.sizes:
        assert g.written(k), f"{k}: slots the plan names were left unwritten"


def _verdict(g, slices, prd, tar, thr, w, base=None, below=False, tag="", populated=True):
    B, C, H, W = prd.shape
    _intact(g)
    K = R.thresholds_3d(thr, B, C).shape[2]
    ref = R.table(prd, tar, thr, w, base, below)
    if populated:
        assert _populated(ref[1], H, W), f"{tag}: the case is degenerate in the reference itself"
    got = (g["table"].cpu().numpy().reshape(B, C, K, 4), g["ninv"].cpu().numpy().reshape(B, C))
    R.judge(got, prd, tar, thr, w, R.chain_length(H, W, slices), base, below, tag=tag, ref=ref)
    return got


def _verdict_ens(g, slices, ens, tar, thr, w, base=None, below=False, tag=""):
    M, B, C, H, W = ens.shape
    _intact(g)
    K = R.thresholds_3d(thr, B, C).shape[2]
    got = dict(sums=g["sums"].cpu().numpy().reshape(B, C, K, 3), wv=g["wv"].cpu().numpy().reshape(B, C),
               hist=g["hist"].cpu().numpy().reshape(B, C, K, 2, M + 1), n_invalid=g["ninv"].cpu().numpy().reshape(B, C))
    R.judge(got, ens, tar, thr, w, R.chain_length(H, W, slices), base, below, tag=tag)
    return got


# (B, C, H, W), K: the smallest shapes that reach each branch of the plan (tests/plane_reference.py: slices = 2048 // planes)
DET = [((1, 1, 1, 4), 1),            # a single vector: 2047 empty slices
       ((2, 3, 5, 8), 1), ((2, 3, 5, 8), 3), ((2, 3, 5, 8), 8),          # 341 slices that cut rows
       ((1, 2, 33, 132), 2),         # 4356 elements over 1024 slices: mostly empty or single-vector slices
       ((1, 2100, 2, 4), 2),         # B * C above the slice threshold: one slice per plane
       ((1, 2048, 4, 1028), 1), ((1, 2048, 4, 1028), 3), ((1, 2048, 4, 1028), 8),      # 4112 elements: one unrolled round of plane_stream_slice + a tail vector
       ((1, 2048, 8, 1028), 3)]      # 8224 elements: two rounds + a tail vector


@pytest.mark.parametrize("shape,K", DET, ids=lambda s: "x".join(map(str, s)) if isinstance(s, tuple) else f"K{s}")
@pytest.mark.parametrize("unit", [True, False], ids=["unit", "lat"])
def test_table_kernels_element_by_element(dev, lib, shape, K, unit):
    B, C, H, W = shape
    ens, tar, _ = _fields(1, B, C, H, W)
    w = np.ones(H, np.float32) if unit else _weights(H)
    assert R.plan_slices(B * C) == (2048 // (B * C) if B * C < 2048 else 1)
    g, slices = _launch(lib, dev, *_d(dev, ens[0], tar), _thr(K), torch.tensor(w).to(dev))
    _verdict(g, slices, ens[0], tar, _thr(K), w, tag=f"{shape} K = {K} {'unit' if unit else 'lat'}")


@pytest.mark.parametrize("below", [False, True], ids=["above", "below"])
@pytest.mark.parametrize("use_base", [False, True], ids=["plain", "base"])
@pytest.mark.parametrize("K", range(1, 9))
def test_every_instantiation_of_both_kernels(dev, lib, K, use_base, below):
    """K, the base field and the direction select the kernel: all 32 of each family, on B > 1 with a base field (the workgroup index
    (c * slices + sl) * B + b) and per-sample thresholds"""
    M, B, C, H, W = 5, 3, 5, 16, 32
    ens, tar, base = _fields(M, B, C, H, W)
    base = base if use_base else None
    w = _weights(H)
    thr = _thr(K)[None, None] + 0.05 * np.arange(C, dtype=np.float32)[None, :, None] - 0.03 * np.arange(B, dtype=np.float32)[:, None, None]
    de, dt, db, dw = _d(dev, ens, tar, base, w)
    g, slices = _launch(lib, dev, de[0], dt, thr, dw, db, below)
    assert slices == 136
    _verdict(g, slices, ens[0], tar, thr, w, base, below, tag=f"K = {K}")
    ge, _ = _launch_ens(lib, dev, de, dt, thr, dw, db, below)
    _verdict_ens(ge, slices, ens, tar, thr, w, base, below, tag=f"ensemble K = {K}")


# (M, B, C, H, W), K.  Members are loaded in batches of 8: M = 8 and 9, 16 and 17 are the last of a batch and the first of the next.
ENS = [((2, 1, 1, 1, 4), 1), ((2, 2, 3, 5, 8), 3), ((7, 1, 2, 33, 132), 2), ((8, 2, 3, 5, 8), 2), ((9, 2, 3, 5, 8), 2), ((16, 2, 3, 5, 8), 8),
       ((17, 2, 3, 5, 8), 1), ((50, 2, 2, 5, 8), 4), ((64, 1, 2, 16, 32), 8), ((2, 1, 2100, 2, 4), 2),
       ((3, 1, 2048, 4, 260), 2)]    # one slice of 1040 elements per plane: threads 0 .. 3 go through the kernel's one loop twice


@pytest.mark.parametrize("shape,K", ENS, ids=lambda s: "x".join(map(str, s)) if isinstance(s, tuple) else f"K{s}")
@pytest.mark.parametrize("unit", [True, False], ids=["unit", "lat"])
def test_ensemble_kernels_element_by_element(dev, lib, shape, K, unit):
    M, B, C, H, W = shape
    ens, tar, _ = _fields(M, B, C, H, W)
    w = np.ones(H, np.float32) if unit else _weights(H)
    g, slices = _launch_ens(lib, dev, *_d(dev, ens, tar), _thr(K), torch.tensor(w).to(dev))
    got = _verdict_ens(g, slices, ens, tar, _thr(K), w, tag=f"{shape} K = {K}")
    assert (got["hist"][..., 1, :].sum() > 0) and (got["hist"][..., 0, 1:].sum() > 0)         # (not everything sits in the derived bin)


def test_ties_on_theta(dev, lib):
    """fields, base and thresholds on a lattice of 0.25: a value equal to theta is no event, above or below"""
    M, B, C, H, W = 6, 2, 3, 6, 16
    ens, tar, base = _fields(M, B, C, H, W, quantum=0.25)
    thr, w = np.array([-0.25, 0.0, 0.5], np.float32), np.ones(H, np.float32)
    th = R.theta(R.thresholds_3d(thr, B, C), base)
    assert (tar[:, :, None] == th).mean() > 0.03 and (ens[:, :, :, None] == th[None]).mean() > 0.03
    de, dt, db, dw = _d(dev, ens, tar, base, w)
    for below in (False, True):
        g, slices = _launch(lib, dev, de[0], dt, thr, dw, db, below)
        _verdict(g, slices, ens[0], tar, thr, w, base, below, tag=f"ties below = {below}")
        ge, _ = _launch_ens(lib, dev, de, dt, thr, dw, db, below)
        _verdict_ens(ge, slices, ens, tar, thr, w, base, below, tag=f"ties, ensemble, below = {below}")


def test_fields_of_mean_1e4_give_the_statements_tables_exactly(dev, lib):
    """comparisons are exact whatever the magnitude: unit-weight tables and all counts EQUAL the statement's"""
    from swin_v2_weather_amd.utils.events import ensemble_event_sums_torch, event_table_torch
    M, B, C, H, W = 7, 2, 2, 9, 16
    ens, tar, base = _fields(M, B, C, H, W, offset=1.0e4)
    assert abs(float(tar.mean()) - 1.0e4) < 1.0
    w = np.ones(H, np.float32)
    de, dt, db, dw = _d(dev, ens, tar, base, w)
    for thr, b, dbase in ((_thr(4, 1.0e4), None, None), (_thr(4), base, db)):
        g, slices = _launch(lib, dev, de[0], dt, thr, dw, dbase)
        got = _verdict(g, slices, ens[0], tar, thr, w, b, tag="offset 1e4")
        tab, ni = event_table_torch(de[0], dt, torch.tensor(thr), dw, dbase)
        assert np.array_equal(tab.cpu().numpy(), got[0]) and np.array_equal(ni.cpu().numpy(), got[1])
        ge, _ = _launch_ens(lib, dev, de, dt, thr, dw, dbase)
        gote = _verdict_ens(ge, slices, ens, tar, thr, w, b, tag="offset 1e4, ensemble")
        s, wv, h, ni = ensemble_event_sums_torch(de, dt, torch.tensor(thr), dw, dbase)
        assert np.array_equal(h.cpu().numpy(), gote["hist"]) and np.array_equal(s.cpu().numpy(), gote["sums"]) and np.array_equal(wv.cpu().numpy(), gote["wv"])


def test_nan_removes_its_point_and_reaches_no_other_plane(dev, lib):
    M, B, C, H, W = 4, 3, 4, 16, 32
    ens, tar, base = _fields(M, B, C, H, W)
    thr, w = _thr(3), _weights(H)
    clean = _d(dev, ens, tar, base, w)
    g0, slices = _launch(lib, dev, clean[0][0], clean[1], thr, clean[3], clean[2])
    e0, _ = _launch_ens(lib, dev, clean[0], clean[1], thr, clean[3], clean[2])
    ens2, tar2 = ens.copy(), tar.copy()
    ens2[0, 1, 2, 7, 9] = np.nan             # the prediction (member 0), plane (1, 2)
    ens2[3, 1, 2, 7, 10] = np.nan            # another member, the same plane
    tar2[0, 3, 0, 0] = np.nan                # the truth, plane (0, 3)
    tar2[0, 3, 15, 31] = np.inf              # +-inf are valid values
    de, dt = _d(dev, ens2, tar2)
    g, _ = _launch(lib, dev, de[0], dt, thr, clean[3], clean[2])
    got = _verdict(g, slices, ens2[0], tar2, thr, w, base, tag="nan")
    assert got[1].tolist() == [[0, 0, 0, 1], [0, 0, 1, 0], [0, 0, 0, 0]]
    ge, _ = _launch_ens(lib, dev, de, dt, thr, clean[3], clean[2])
    gote = _verdict_ens(ge, slices, ens2, tar2, thr, w, base, tag="nan, ensemble")
    assert gote["n_invalid"].tolist() == [[0, 0, 0, 1], [0, 0, 2, 0], [0, 0, 0, 0]]
    keep = np.ones((B, C), bool)
    keep[1, 2] = keep[0, 3] = False
    t0, t1 = g0["table"].view(B, C, -1).cpu().numpy(), g["table"].view(B, C, -1).cpu().numpy()
    assert np.array_equal(t0[keep].view(np.int32), t1[keep].view(np.int32)) and not np.array_equal(t0[1, 2], t1[1, 2])      # other planes: the same bits
    for k in ("sums", "hist"):
        a, b = e0[k].view(B, C, -1).cpu().numpy(), ge[k].view(B, C, -1).cpu().numpy()
        assert np.array_equal(a[keep].view(np.int32), b[keep].view(np.int32)), k
    base2 = base.copy()
    base2[1, 4, 4] = np.nan                  # the base field: that point leaves channel 1 of every sample
    gb, _ = _launch(lib, dev, clean[0][0], clean[1], thr, clean[3], torch.tensor(base2).to(dev))
    assert _verdict(gb, slices, ens[0], tar, thr, w, base2, tag="nan in the base")[1].tolist() == [[0, 1, 0, 0]] * 3


def test_a_threshold_no_value_exceeds(dev, lib):
    """every point in the bin (n = 0, o = 0), which the kernel does not count but derives: d = N, the rest exactly zero"""
    M, B, C, H, W = 16, 2, 2, 9, 16
    ens, tar, _ = _fields(M, B, C, H, W)
    thr, w = np.array([1.0e6, 0.0], np.float32), np.ones(H, np.float32)
    de, dt, dw = _d(dev, ens, tar, w)
    g, slices = _launch(lib, dev, de[0], dt, thr, dw)
    tab, _ = _verdict(g, slices, ens[0], tar, thr, w, tag="nothing exceeds", populated=False)
    assert np.array_equal(tab[..., 0, :], np.broadcast_to(np.array([0, 0, 0, H * W], np.float32), (B, C, 4)))
    ge, _ = _launch_ens(lib, dev, de, dt, thr, dw)
    got = _verdict_ens(ge, slices, ens, tar, thr, w, tag="nothing exceeds, ensemble")
    assert np.all(got["hist"][..., 0, 0, 0] == H * W) and got["hist"][..., 0, :, :].sum() == B * C * H * W and np.all(got["sums"][..., 0, :] == 0)
    gb, _ = _launch_ens(lib, dev, de, dt, -thr, dw, below=True)             # the same events from below, on the negated fields' thresholds
    assert _verdict_ens(gb, slices, ens, tar, -thr, w, below=True, tag="nothing falls below")["hist"][..., 0, 0, 0].min() == H * W


@pytest.mark.parametrize("M", [5, 50])
def test_reruns_and_a_dirty_workspace_give_the_same_bits(dev, lib, M):
    B, C, H, W = 2, 3, 17, 40
    ens, tar, base = _fields(M, B, C, H, W)
    thr, w = _thr(3), _weights(H)
    de, dt, db, dw = _d(dev, ens, tar, base, w)
    g1, _ = _launch(lib, dev, de[0], dt, thr, dw, db)
    g2, _ = _launch(lib, dev, de[0], dt, thr, dw, db)
    g3, _ = _launch(lib, dev, de[0], dt, thr, dw, db, ws_fill=-1)          # a workspace full of 0xFF bytes: nothing is accumulated into
    assert torch.equal(g1.raw, g2.raw) and torch.equal(g1.raw, g3.raw)
    e1, _ = _launch_ens(lib, dev, de, dt, thr, dw, db)
    e2, _ = _launch_ens(lib, dev, de, dt, thr, dw, db)
    e3, _ = _launch_ens(lib, dev, de, dt, thr, dw, db, ws_fill=-1)
    assert torch.equal(e1.raw, e2.raw) and torch.equal(e1.raw, e3.raw)     # workspace, sums and counts, bit for bit


def test_channel_blocks_of_wider_tensors_in_place(dev, lib):
    """members as the rows of [M B, 15, H, W], channels 5:10, against channels 7:12 of an 18-channel truth: nothing is copied"""
    M, B, C, H, W = 5, 2, 5, 9, 12
    ens_w = _fields(M, B, 15, H, W)[0]
    tar_w, base_w = _fields(1, B, 18, H, W, seed=1)[1:]
    w, thr = _weights(H), _thr(2)
    rows, dt = torch.tensor(ens_w).to(dev).view(M * B, 15, H, W), torch.tensor(tar_w).to(dev)
    ve, vt = rows.unflatten(0, (M, B))[:, :, 5:10], dt[:, 7:12]
    assert ve.stride() == (B * 15 * H * W, 15 * H * W, H * W, W, 1) and vt.stride(0) == 18 * H * W
    base = np.ascontiguousarray(base_w[7:12])
    db, dw = _d(dev, base, w)
    g, slices = _launch(lib, dev, ve[0], vt, thr, dw, db)
    assert slices == 204
    _verdict(g, slices, ens_w[0, :, 5:10], tar_w[:, 7:12], thr, w, base, tag="block 5:10 / 7:12")
    ge, _ = _launch_ens(lib, dev, ve, vt, thr, dw, db)
    _verdict_ens(ge, slices, ens_w[:, :, 5:10], tar_w[:, 7:12], thr, w, base, tag="block 5:10 / 7:12, ensemble")


# ---- the Python layer ------------------------------------------------------------------------------------------------------
def test_forecast_scorer_event_scores_against_the_statements(dev, lib):
    from swin_v2_weather_amd import ops
    from swin_v2_weather_amd.utils.weighted_acc_rmse import (ForecastScorer, brier_scores, contingency_scores, ensemble_event_sums_torch,
                                                             event_table_torch, reliability_scores)
    M, B, C, H, W = 5, 2, 5, 9, 12
    ens_w = _fields(M, B, 15, H, W)[0]
    tar_w, clim_w = _fields(1, B, 18, H, W, seed=1)[1:]
    clim = np.ascontiguousarray(clim_w[7:12])
    rows, dt = torch.tensor(ens_w).to(dev).view(M * B, 15, H, W), torch.tensor(tar_w).to(dev)
    sc = ForecastScorer(H, W, C, dev, climatology=clim)
    w = sc.w.cpu().numpy()
    n = R.chain_length(H, W, ops.score_slices(B * C, H, W))
    thr = np.linspace(-1.0, 1.0, 11).astype(np.float32)                        # K = 11: chunks of 8 and 3
    r = sc.event_score(rows[:B], dt, thr, anomaly=True, coff_prd=5, coff_tar=7)
    assert set(sc._ws) == {("event", B, 8), ("event", B, 3)} and tuple(r.table.shape) == (B, C, 11, 4) and r.n_invalid.dtype == torch.int32
    R.judge((r.table.cpu().numpy(), r.n_invalid.cpu().numpy()), ens_w[0, :, 5:10], tar_w[:, 7:12], thr, w, n, clim, tag="event_score, K = 11")
    st = event_table_torch(rows[:B, 5:10], dt[:, 7:12], torch.tensor(thr), sc.w, sc.clim)[0]
    assert torch.allclose(r.table, st, rtol=1e-5, atol=1e-5)
    assert torch.equal(r.pooled["ets"], contingency_scores(r.table.double().sum(0))["ets"]) and r.scores["ets"].dtype == torch.float64
    e = sc.ensemble_event_score(rows, dt, M, thr, anomaly=True, below=True, coff_ens=5, coff_tar=7)
    assert {k for k in sc._ws if k[0] == "ens_event"} == {("ens_event", M, B, 8), ("ens_event", M, B, 3)} and tuple(e.hist.shape) == (B, C, 11, 2, M + 1)
    R.judge(dict(sums=e.sums.cpu().numpy(), wv=e.wv.cpu().numpy(), hist=e.hist.cpu().numpy(), n_invalid=e.n_invalid.cpu().numpy()),
            ens_w[:, :, 5:10], tar_w[:, 7:12], thr, w, n, clim, True, tag="ensemble_event_score, K = 11")
    s, wv, h, _ = ensemble_event_sums_torch(rows.unflatten(0, (M, B))[:, :, 5:10], dt[:, 7:12], torch.tensor(thr), sc.w, sc.clim, True)
    assert torch.equal(e.hist, h) and torch.allclose(e.sums, s, rtol=1e-5, atol=1e-5)
    assert torch.equal(e.pooled["brier"], brier_scores(e.sums.double().sum(0), e.wv.double().sum(0), M)["brier"])
    hp = h.long().sum(0)
    assert torch.equal(e.reliability["roc_area"], reliability_scores(hp[..., 0, :], hp[..., 1, :])["roc_area"])
    assert bool(((e.reliability["roc_area"] >= 0.0) & (e.reliability["roc_area"] <= 1.0)).all())
    # an odd width: the statements on the device, no workspace
    so = ForecastScorer(H, 10, C, dev)
    ro = so.event_score(rows[:B, :, :, :10], dt[..., :10], thr[:2], coff_prd=5, coff_tar=7)
    assert len(so._ws) == 0
    R.judge((ro.table.cpu().numpy(), ro.n_invalid.cpu().numpy()), ens_w[0, :, 5:10, :, :10], tar_w[:, 7:12, :, :10], thr[:2], w, H * 10, tag="odd width")


def test_regridded_scorer_takes_the_events_on_the_coarse_grid(dev, lib):
    from swin_v2_weather_amd.utils import regrid as G
    from swin_v2_weather_amd.utils.weighted_acc_rmse import EventSpec, ForecastScorer, RegriddedScorer
    M, B, C, H, W = 3, 2, 2, 48, 72
    ens, tar, clim = _fields(M, B, C, H, W)
    de, dt, dc = _d(dev, ens, tar, clim)
    rg = G.Regridder(G.model_grid(H, W), G.grid_for_degrees(15.0), dev)
    rs = RegriddedScorer(rg, C, climatology=dc)
    thr = np.array([-0.2, 0.3], np.float32)
    r = rs.event_score(de[0], dt, thr, anomaly=True)
    inner = ForecastScorer(13, 24, C, dev, climatology=rg(dc), weights=rg.area_weights)
    want = inner.event_score(rg(de[0]), rg(dt), thr, anomaly=True)
    assert torch.equal(r.table, want.table) and tuple(r.table.shape) == (B, C, 2, 4) and float(r.table.sum()) > 0
    e = rs.ensemble_event_score(de.reshape(M * B, C, H, W), dt, M, thr, anomaly=True)
    we = inner.ensemble_event_score(rg(de), rg(dt), M, thr, anomaly=True)
    assert torch.equal(e.hist, we.hist) and torch.equal(e.sums, we.sums) and int(e.hist[..., 0, :].sum()) == B * C * 2 * 13 * 24
    q = rs.event_thresholds(EventSpec("quantile", (0.9,)), dt)
    assert tuple(q.shape) == (B, C, 1) and torch.equal(q, inner.event_thresholds(EventSpec("quantile", (0.9,)), rg(dt)))


def test_rollouts_with_events_leave_every_other_score_bit_identical(dev, lib, tmp_path):
    from tests.test_score_gpu import _registry_model
    from swin_v2_weather_amd import inference
    from swin_v2_weather_amd.utils.weighted_acc_rmse import EventSpec, ForecastScorer
    model = _registry_model(dev, tmp_path)
    M, B, Cout, H, W, steps = 3, 2, 5, 48, 72, 2
    g = torch.Generator(device=dev).manual_seed(3)
    x0 = torch.randn(B, 9, H, W, device=dev, generator=g)
    cz = torch.rand(B, steps - 1, H, W, device=dev, generator=g) * 2 - 1
    truth = torch.randn(B, steps, Cout, H, W, device=dev, generator=g)
    scorer = ForecastScorer(H, W, Cout, dev, climatology=0.3 * torch.randn(Cout, H, W, device=dev, generator=g))
    spec = EventSpec("quantile", (0.5, 0.9), False)
    plain = inference.score_rollout(model, x0, truth, steps, cz, n_invar=3, scorer=scorer, keep_forecast=True)
    got = inference.score_rollout(model, x0, truth, steps, cz, n_invar=3, scorer=scorer, keep_forecast=True, events=spec)
    assert plain.events is None and all(torch.equal(a, b) for a, b in zip(plain[:5], got[:5]))             # rmse, acc, the samples, the forecast
    for s in range(steps):
        thr = scorer.event_thresholds(spec, truth[:, s])
        r = scorer.event_score(got.forecast[:, s], truth[:, s], thr)
        assert torch.equal(got.events.table[s], r.table) and torch.equal(got.events.scores["ets"][s], r.pooled["ets"])
    assert float(got.events.scores["base_rate"][:, :, 1].mean()) == pytest.approx(0.1, abs=0.01)
    a = EventSpec("anomaly", (0.5,), True)
    pe = inference.ensemble_rollout(model, x0, truth, steps, M, 0.05, 1, cz, 3, scorer, keep_forecast=True, score_control=True)
    ge = inference.ensemble_rollout(model, x0, truth, steps, M, 0.05, 1, cz, 3, scorer, keep_forecast=True, score_control=True, events=a)
    assert all(torch.equal(x, y) for x, y in zip(pe[:10], ge[:10])) and torch.equal(pe.control.rmse, ge.control.rmse)
    for s in range(steps):
        r = scorer.ensemble_event_score(ge.forecast[:, s], truth[:, s], M, torch.tensor(a.levels), anomaly=True, below=True)
        assert torch.equal(ge.events.hist[s], r.hist) and torch.equal(ge.events.scores["brier"][s], r.pooled["brier"])
    assert tuple(ge.control.events.table.shape) == (steps, B, Cout, 1, 4)


def test_cli_writes_the_events_key(dev, lib, tmp_path, capsys):
    from tests.test_score_gpu import _registry_model
    from swin_v2_weather_amd import inference
    _registry_model(dev, tmp_path)
    reg = tmp_path / "swin_test_registry"
    rng = np.random.default_rng(11)
    B, Cout, H, W, steps, M = 2, 5, 48, 72, 2, 3
    tm = rng.standard_normal((1, 73, 49, 80)).astype(np.float32)
    x0, truth = rng.standard_normal((B, 9, H, W)).astype(np.float32), rng.standard_normal((B, steps, Cout, H, W)).astype(np.float32)
    np.save(reg / "time_means.npy", tm); np.save(tmp_path / "x0.npy", x0); np.save(tmp_path / "truth.npy", truth)
    base = ["--registry", str(reg), "--steps", str(steps), "--init", str(tmp_path / "x0.npy"), "--truth", str(tmp_path / "truth.npy")]
    inference.main(base + ["--scores-out", str(tmp_path / "plain.json")])
    plain_out = capsys.readouterr().out.splitlines()
    inference.main(base + ["--scores-out", str(tmp_path / "ev.json"), "--event-anomaly", "0.0", "1.0"])
    ev_out = capsys.readouterr().out.splitlines()
    plain, ev = json.load(open(tmp_path / "plain.json")), json.load(open(tmp_path / "ev.json"))
    assert list(plain) == ["lead_hours", "rmse", "acc", "tracked"] and ev["rmse"] == plain["rmse"] and ev["acc"] == plain["acc"]
    e = ev["events"]
    assert e["kind"] == "anomaly" and e["levels"] == [0.0, 1.0] and e["below"] is False
    assert np.asarray(e["table"]).shape == (steps, Cout, 2, 4) and all(np.asarray(e[k]).shape == (steps, Cout, 2) for k in
                                                                      ("base_rate", "freq_bias", "pod", "far", "csi", "ets", "sedi"))
    assert ev_out[1].split()[-4:] == ["ets0_u10m", "ets0_v10m", "ets1_u10m", "ets1_v10m"] and ev_out[1].startswith(plain_out[1])
    assert float(ev_out[2].split()[-4]) == pytest.approx(e["ets"][0][0][0], abs=1e-5)
    inference.main(base + ["--scores-out", str(tmp_path / "ens.json"), "--event-quantile", "0.9", "--event-below", "--ensemble", str(M),
                           "--perturbation", "0.1", "--score-grid", "15"])
    out = capsys.readouterr().out.splitlines()
    en = json.load(open(tmp_path / "ens.json"))["events"]
    assert en["kind"] == "quantile" and en["below"] is True and np.asarray(en["table"]).shape == (steps, Cout, 1, 4)
    assert all(np.asarray(en[k]).shape == (steps, Cout, 1) for k in ("brier", "fair_brier", "brier_skill", "reliability", "resolution", "roc_area"))
    assert out[2].split()[-4:] == ["ets0_u10m", "ets0_v10m", "bs0_u10m", "bs0_v10m"]
