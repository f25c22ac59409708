"""GPU (-m gpu): swv2_regrid through the C ABI with guard bands, judged element by element against the fp64 statement of
tests/regrid_reference.py (the bound is derived there), then the Python layer: Regridder on CUDA, RegriddedScorer, score_rollout with a
regridded scorer and the --score-grid flag.

The scorer tests judge in two steps, both strict.  The coarse fields RegriddedScorer hands its inner ForecastScorer are judged against the
statement like every kernel output; the scores are then bit for bit the ForecastScorer's on kernel-regridded copies, and (score, mae,
ensemble_score) inside the bounds of tests/score_reference.py, l1_reference.py and ensemble_reference.py for those coarse fields and the
cell-area weights.  (A score of statement-regridded copies differs from
a score of kernel-regridded ones by the regridding error carried through the score, which the score suites' bounds do not hold.)"""
import functools
import json

import numpy as np
import pytest
import torch

from tests import regrid_reference as R
from tests import ensemble_reference as ER
from tests import l1_reference as L1
from tests import score_reference as SR
from tests.plane_harness import SENTINEL, Guarded, dev, lib  # noqa: F401  (dev, lib: fixtures)

pytestmark = pytest.mark.gpu

# name: (B, C, source (nlat, poles, crop | None, nlon), target (nlat, poles, nlon))
CASES = {"a": (1, 3, (25, True, 24, 48), (5, True, 8)),            # the workload in small: 7-wide bands, half cells at the poles, the cropped last row, the wrap at I = 0
         "b": (2, 2, (25, True, None, 48), (4, False, 8)),         # a pole grid onto an offset grid; batch of 2
         "c": (1, 2, (24, False, None, 48), (7, False, 20)),       # a non-integer ratio, varying counts, Wd % 4 != 0
         "d": (1, 2, (14, True, None, 1440), (3, True, 240)),      # the production row width: the LDS row, the loads in flight and the wrap
         "e": (2, 1100, (12, False, None, 16), (3, False, 4)),     # many planes: the grid-index arithmetic
         "f": (1, 1, (64, False, None, 124), (2, False, 4)),       # latitude bands of exactly 32 entries (the cap), longitude 31
         # the work split: swv2_regrid runs R = 4, 2 or 1 target rows per workgroup, the largest that leaves B C ceil(Hd / R) >= 1024 workgroups
         "g": (1, 600, (25, True, 24, 48), (5, True, 8)),          # R = 4: 2 runs per plane, the last of one row (production: 31 runs, a last run of one)
         "h": (1, 400, (25, True, 24, 48), (5, True, 8)),          # R = 2 (400 * 3 >= 1024 > 400 * 2): 3 runs, the last of one row
         "i": (1, 344, (26, True, None, 1440), (9, True, 240)),    # R = 4 at the production row width: 4 rows of 1440 in LDS, 3 runs, the last of one row
         "j": (1, 2, (44, False, None, 48), (2, False, 8)),        # latitude bands of 22 entries: two full chunks of 8 loads and one of 6 (5.625 degrees has 22 - 23)
         "k": (1, 1, (4, False, None, 16384), (2, False, 1024))}   # the widest accepted row: 64 KB of dynamic LDS
RUN_ROWS = {"g": 4, "h": 2, "i": 4, "e": 4, "a": 1, "k": 1}        # what the rule above gives: asserted, so a changed rule cannot move a case off its path
OVER_CAP = (1, 1, (66, False, None, 64), (2, False, 2))            # 33 entries both ways: refused by the entry point


@functools.lru_cache(maxsize=None)
def _setup(src_spec, dst_spec):
    """-> dict: product grids and tables (numpy), reference matrices and chain lengths; made once, never modified"""
    from swin_v2_weather_amd.utils import regrid as G
    nlat, poles, crop, W = src_spec
    src = G.equiangular_grid(nlat, W, poles)
    src_lat = R.centres(nlat, poles)
    if crop is not None:
        src, src_lat = src.rows(0, crop), src_lat[:crop]
    dst = G.equiangular_grid(dst_spec[0], dst_spec[2], dst_spec[1])
    A, Bm = G.conservative_weights(src, dst)
    Ar, Br = R.lat_matrix(src_lat, R.centres(dst_spec[0], dst_spec[1])), R.lon_matrix(W, dst_spec[2])
    lat, lon = G.band_tables(A, cap=64, periodic=False), G.band_tables(Bm, cap=64)
    # what the kernel trusts of the tables, and that they are the reference's operator after fp32 rounding of ITS weights up to 1e-14
    assert lat[0].min() >= 0 and (lat[0] + lat[1]).max() <= src.nlat and lon[0].min() >= 0 and lon[0].max() < W and lon[1].max() <= W
    assert lat[1].min() >= 1 and lon[1].min() >= 1
    assert np.abs(R.dense_from_tables(*lat, src.nlat) - Ar).max() <= 2.0 ** -24 and np.abs(R.dense_from_tables(*lon, W) - Br).max() <= 2.0 ** -24
    assert np.array_equal(R.counts(Ar), lat[1]) and np.array_equal(R.counts(Br), lon[1])
    return dict(src=src, dst=dst, lat=lat, lon=lon, Ar=Ar, Br=Br, H=src.nlat, W=W, Hd=dst.nlat, Wd=dst.nlon)


@functools.lru_cache(maxsize=None)
def _field(B, C, H, W, seed=0):
    x = np.random.default_rng(100 * seed + B + 3 * C + 7 * H + W).standard_normal((B, C, H, W)).astype(np.float32)
    x.setflags(write=False)
    return x


def _tables(dev, s):
    return [torch.from_numpy(np.ascontiguousarray(t)).to(dev) for t in s["lat"] + s["lon"]]


def _call(lib, xt, yt, s, tabs, **over):
    """swv2_regrid on the views xt [B, C, H, W] and yt [B, C, Hd, Wd] -> status; over: arguments replaced by name"""
    x, y = xt, yt
    B, C, H, W = x.shape
    Hd, Wd = y.shape[2:]
    a = dict(x=x.data_ptr(), xbs=x.stride(0) if B > 1 else C * H * W, y=y.data_ptr(), ybs=y.stride(0) if B > 1 else C * Hd * Wd, B=B, C=C, H=H, W=W,
             Hd=Hd, Wd=Wd, ls=tabs[0].data_ptr(), lc=tabs[1].data_ptr(), lw=tabs[2].data_ptr(), KH=tabs[2].shape[1], ns=tabs[3].data_ptr(),
             nc=tabs[4].data_ptr(), nw=tabs[5].data_ptr(), KW=tabs[5].shape[1])
    a.update(over)
    rc = lib.swv2_regrid(*a.values(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc


def _run_case(lib, dev, B, C, s, x):
    g = Guarded(dev, x=x.size, y=B * C * s["Hd"] * s["Wd"])
    g["x"].copy_(torch.tensor(x).reshape(-1))
    xv, yv = g["x"].view(B, C, s["H"], s["W"]), g["y"].view(B, C, s["Hd"], s["Wd"])
    assert _call(lib, xv, yv, s, _tables(dev, s)) == 0, lib.swv2_last_error()
    return g, yv


@pytest.mark.parametrize("case", list(CASES))
def test_kernel_element_by_element_against_fp64(dev, lib, case):
    B, C, src_spec, dst_spec = CASES[case]
    s = _setup(src_spec, dst_spec)
    if case == "f":
        assert s["lat"][1].tolist() == [32, 32] and s["lon"][1].max() == 31
    if case == "a":
        assert s["lon"][1].tolist() == [7] * 8 and s["lon"][0][0] == 45 and s["lat"][1].min() == 3 and s["lat"][1].max() == 7
    if case == "j":
        assert s["lat"][1].tolist() == [22, 22]
    if case in RUN_ROWS:
        R_ = 4
        while R_ > 1 and (R_ * s["W"] * 4 > 65536 or B * C * -(-s["Hd"] // R_) < 1024):
            R_ //= 2
        assert R_ == RUN_ROWS[case]
    x = _field(B, C, s["H"], s["W"])
    g, yv = _run_case(lib, dev, B, C, s, x)
    assert g.guards_intact(), "the kernel wrote outside its output"
    assert g.written("y"), "output slots were left unwritten"
    assert R.judge(yv.cpu().numpy(), x, s["Ar"], s["Br"], s["lat"][1], s["lon"][1], f"case {case} {x.shape} -> {s['Hd']} x {s['Wd']}") <= 1.0


def test_bands_above_the_cap_are_refused_and_the_regridder_runs_the_statement(dev, lib):
    from swin_v2_weather_amd.utils import regrid as G
    B, C, src_spec, dst_spec = OVER_CAP
    s = _setup(src_spec, dst_spec)
    assert s["lat"][1].max() == 33 and s["lon"][1].max() == 33
    x = _field(B, C, s["H"], s["W"])
    g = Guarded(dev, x=x.size, y=4)
    g["x"].copy_(torch.tensor(x).reshape(-1))
    rc = _call(lib, g["x"].view(1, 1, 66, 64), g["y"].view(1, 1, 2, 2), s, _tables(dev, s))
    assert rc != 0 and lib.swv2_last_error().decode().startswith("regrid:") and not g.written("y") and bool((g.ints("y") == SENTINEL).all())
    rg = G.Regridder(s["src"], s["dst"], dev)
    assert rg.tables is None
    y = rg(torch.from_numpy(x.copy()).to(dev))
    assert y.is_cuda and R.judge(y.cpu().numpy(), x, s["Ar"], s["Br"], np.full(2, 66), np.full(2, 64), "statement above the cap") <= 1.0


def test_channel_block_of_wider_tensors_with_different_strides(dev, lib):
    """channels 1:4 of a 6-channel input into channels 2:5 of a 7-channel output, in place"""
    B, C, src_spec, dst_spec = CASES["a"]
    s = _setup(src_spec, dst_spec)
    B = 2
    xw = _field(B, 6, 24, 48, seed=2)
    g = Guarded(dev, x=xw.size, y=B * 7 * 5 * 8)
    g["x"].copy_(torch.tensor(xw).reshape(-1))
    xv, yw = g["x"].view(B, 6, 24, 48)[:, 1:4], g["y"].view(B, 7, 5, 8)
    yv = yw[:, 2:5]
    assert xv.stride(0) == 6 * 24 * 48 and yv.stride(0) == 7 * 40 and xv.data_ptr() % 16 == 0
    assert _call(lib, xv, yv, s, _tables(dev, s)) == 0, lib.swv2_last_error()
    assert g.guards_intact()
    raw = g.ints("y").view(B, 7, 5, 8)
    assert bool((raw[:, :2] == SENTINEL).all()) and bool((raw[:, 5:] == SENTINEL).all()) and bool((raw[:, 2:5] != SENTINEL).all())
    assert R.judge(yv.cpu().numpy(), xw[:, 1:4], s["Ar"], s["Br"], s["lat"][1], s["lon"][1], "block 1:4 -> 2:5") <= 1.0


def test_nan_and_inf_reach_exactly_the_bands_that_hold_them_and_reruns_agree_bit_for_bit(dev, lib):
    B, C, src_spec, dst_spec = CASES["a"]
    s = _setup(src_spec, dst_spec)
    x = _field(B, C, 24, 48, seed=3).copy()
    bad = {0: (0, 45, np.nan), 1: (23, 2, np.inf), 2: (11, 20, -np.inf)}          # plane: (row, column, value); column 45 lies in the wrapped band of I = 0
    for c, (j, i, v) in bad.items():
        x[0, c, j, i] = v
    g, yv = _run_case(lib, dev, B, C, s, x)
    assert g.guards_intact() and g.written("y")
    y = yv.cpu().numpy()
    Al, Bl = R.dense_from_tables(*s["lat"], 24) != 0, R.dense_from_tables(*s["lon"], 48) != 0
    for c, (j, i, v) in bad.items():
        hit = np.outer(Al[:, j], Bl[:, i])                                       # the count comes from the tables
        assert hit.sum() >= 1 and np.array_equal(~np.isfinite(y[0, c]), hit), f"plane {c}: {(~np.isfinite(y[0, c])).sum()} cells, {hit.sum()} bands hold the cell"
        if np.isinf(v):
            assert np.all(y[0, c][hit] == v)                                     # one infinite term in a chain of finite ones
        x0 = x[0, c].copy()
        x0[j, i] = 0.0
        assert R.judge(y[0, c], x0, s["Ar"], s["Br"], s["lat"][1], s["lon"][1], f"plane {c} beside the bad cell", finite_only=~hit) <= 1.0
    g2, _ = _run_case(lib, dev, B, C, s, x)
    assert torch.equal(g.raw, g2.raw)                                            # NaN compared as bits


def test_every_host_check_returns_its_status_without_a_launch(dev, lib):
    B, C, src_spec, dst_spec = CASES["b"]
    s = _setup(src_spec, dst_spec)
    x = _field(B, C, s["H"], s["W"])
    g = Guarded(dev, x=x.size + 8, y=B * C * s["Hd"] * s["Wd"] + 8)
    g["x"][:x.size].copy_(torch.tensor(x).reshape(-1))
    xv, yv = g["x"][:x.size].view(B, C, s["H"], s["W"]), g["y"][:B * C * 32].view(B, C, s["Hd"], s["Wd"])
    tabs = _tables(dev, s)
    span_x, span_y = C * s["H"] * s["W"], C * s["Hd"] * s["Wd"]
    null, shape = "null pointer", "B, C, H, W, Hd, Wd > 0"
    bad = [(dict(x=None), null), (dict(y=None), null), (dict(ls=None), null), (dict(lc=None), null), (dict(lw=None), null), (dict(ns=None), null),
           (dict(nc=None), null), (dict(nw=None), null),
           (dict(B=0), shape), (dict(C=0), shape), (dict(H=0), shape), (dict(W=0), shape), (dict(Hd=0), shape), (dict(Wd=0), shape), (dict(B=-1), shape),
           (dict(W=50), "W % 4"), (dict(x=xv.data_ptr() + 4), "16-byte"), (dict(xbs=span_x + 2), "multiple of 4"), (dict(ybs=span_y + 2), "multiple of 4"),
           (dict(xbs=span_x - 4), "smaller than"), (dict(ybs=span_y - 4), "smaller than"),
           (dict(KH=0), "band width"), (dict(KH=33), "band width"), (dict(KW=0), "band width"), (dict(KW=33), "band width"),
           (dict(B=1 << 10, C=1 << 10, xbs=span_x << 10, ybs=span_y << 10), "B * C >= 2^20"), (dict(H=1 << 15, W=1 << 15), "H * W >= 2^30"),
           (dict(Hd=1 << 15, Wd=1 << 15), "Hd * Wd >= 2^30"),
           (dict(W=16388), "16384"), (dict(B=1 << 9, C=1 << 10, Hd=1 << 14, xbs=1 << 40, ybs=1 << 40), "grid index")]
    for over, word in bad:
        rc = _call(lib, xv, yv, s, tabs, **over)
        msg = lib.swv2_last_error().decode()
        assert rc != 0 and msg.startswith("regrid:") and word in msg, (over, rc, msg)
    assert bool((g.ints("y") == SENTINEL).all()) and g.guards_intact(), "a refused call launched"
    # B == 1 never uses the batch strides' size
    assert _call(lib, xv[:1], yv[:1], s, tabs, xbs=0, ybs=0) == 0 and bool((g.ints("y")[:span_y] != SENTINEL).all())
    assert bool((g.ints("y")[span_y:] == SENTINEL).all()) and g.guards_intact()


# ---- the Python layer ------------------------------------------------------------------------------------------------------
def test_regridder_on_cuda_agrees_with_the_statement_and_writes_into_a_channel_block(dev, lib):
    from swin_v2_weather_amd.utils import regrid as G
    s = _setup(*CASES["a"][2:])
    rg = G.Regridder(s["src"], s["dst"], dev)
    assert rg.device == dev and all(t.device == dev for t in rg.tables) and rg.area_weights.device == dev
    assert torch.equal(rg.area_weights.cpu(), torch.from_numpy(G.area_weights(s["dst"])))
    x = _field(2, 6, 24, 48, seed=4)
    dx = torch.from_numpy(x.copy()).to(dev)
    cl, cn = s["lat"][1], s["lon"][1]
    y = rg(dx)
    assert y.is_cuda and y.dtype == torch.float32 and tuple(y.shape) == (2, 6, 5, 8)
    assert R.judge(y.cpu().numpy(), x, s["Ar"], s["Br"], cl, cn, "Regridder cuda") <= 1.0
    wide = torch.full((2, 9, 5, 8), 7.0, device=dev)
    got = rg(dx[:, 1:4], out=wide[:, 2:5])
    assert got.data_ptr() == wide[:, 2:5].data_ptr() and torch.equal(wide[:, 2:5], y[:, 1:4]) and bool((wide[:, :2] == 7).all()) and bool((wide[:, 5:] == 7).all())
    # the kernel's bits whatever the rank: [H, W], [C, H, W], [M, B, C, H, W] as one launch and member by member
    assert torch.equal(rg(dx[0, 0]), y[0, 0]) and torch.equal(rg(dx[1]), y[1])
    ens = torch.stack([dx, dx + 1.0, dx * 2.0])
    e = rg(ens)
    assert tuple(e.shape) == (3, 2, 6, 5, 8) and torch.equal(e[0], y) and torch.equal(e[1], rg(dx + 1.0))
    assert torch.equal(rg(ens[:, :, 1:4]), e[:, :, 1:4])                         # a channel block of members: M B samples, strides allow
    assert torch.equal(rg(ens.transpose(0, 1)), e.transpose(0, 1))               # member stride below the batch stride: member by member
    # what the kernel does not take runs the statement: fp64, a gradient, planes that are not contiguous
    assert R.worst(np.abs(rg(dx.double()).cpu().numpy() - R.regrid(x, s["Ar"], s["Br"])), 1e-13) <= 1.0
    xg = dx.clone().requires_grad_(True)
    yg = rg(xg)
    assert yg.requires_grad and R.judge(yg.detach().cpu().numpy(), x, s["Ar"], s["Br"], np.full(5, 24), np.full(8, 48), "statement, grad") <= 1.0
    with torch.no_grad():
        assert torch.equal(rg(xg), y)                                            # no gradient asked for: the kernel
    nc = torch.from_numpy(np.ascontiguousarray(x.transpose(0, 1, 3, 2))).to(dev).transpose(2, 3)
    assert R.judge(rg(nc).cpu().numpy(), x, s["Ar"], s["Br"], np.full(5, 24), np.full(8, 48), "statement, non-contiguous") <= 1.0


def _score_inputs(dev):
    s = _setup(*CASES["a"][2:])
    C = 3
    prd, tar = _field(2, 7, 24, 48, seed=5), _field(2, 5, 24, 48, seed=6)
    clim = (0.3 * _field(1, C, 24, 48, seed=7)[0]).astype(np.float32)
    stds = np.array([1.5, 2.0, 0.25], np.float32)
    return s, C, prd, tar, clim, stds


def test_regridded_scorer_agrees_with_the_forecast_scorer_on_regridded_copies(dev, lib):
    from swin_v2_weather_amd import ops
    from swin_v2_weather_amd.utils import regrid as G
    from swin_v2_weather_amd.utils.weighted_acc_rmse import ForecastScorer, RegriddedScorer
    s, C, prd, tar, clim, stds = _score_inputs(dev)
    rg = G.Regridder(s["src"], s["dst"], dev)
    rs = RegriddedScorer(rg, C, climatology=clim, stds=stds)
    assert (rs.C, rs.H, rs.W) == (C, 24, 48) and rs.grid == s["dst"] and rs.clim.device == dev
    dp, dt = torch.from_numpy(prd.copy()).to(dev), torch.from_numpy(tar.copy()).to(dev)
    cl, cn = s["lat"][1], s["lon"][1]
    got = rs.score(dp, dt, coff_prd=2, coff_tar=1)
    # 1. the coarse fields the inner scorer read, against the statement
    cp, ct = rs._buf[("prd", (2, C), torch.float32, dev)].cpu().numpy(), rs._buf[("tar", (2, C), torch.float32, dev)].cpu().numpy()
    cc = rs.inner.clim.cpu().numpy()
    assert R.judge(cp, prd[:, 2:5], s["Ar"], s["Br"], cl, cn, "coarse prediction") <= 1.0
    assert R.judge(ct, tar[:, 1:4], s["Ar"], s["Br"], cl, cn, "coarse truth") <= 1.0
    assert R.judge(cc, clim, s["Ar"], s["Br"], cl, cn, "coarse climatology") <= 1.0
    # 2. the scores of those fields inside the score suite's own bounds, with the cell-area weights
    w = G.area_weights(s["dst"])
    n = SR.chain_length(5, 8, ops.score_slices(2 * C, 5, 8))
    rs_, rr, ra = SR.judge(got.sums.cpu().numpy(), got.rmse.cpu().numpy(), got.acc.cpu().numpy(), cp, ct, w, cc, n, "RegriddedScorer.score")
    assert rs_ <= 1.0 and rr <= 1.0 and ra <= 1.0
    m_ref, m_b = SR.batch_mean(got.rmse.cpu().numpy(), stds)
    assert np.all(np.abs(got.rmse_mean.cpu().numpy() - m_ref) <= m_b)
    # 3. bit for bit the ForecastScorer on kernel-regridded copies: score, mae, quantile_error, ensemble_score
    fs = ForecastScorer(5, 8, C, dev, climatology=rg(torch.from_numpy(clim.copy()).to(dev)), stds=stds, weights=rg.area_weights)
    p, t = rg(dp[:, 2:5]), rg(dt[:, 1:4])
    for a, b in zip(got, fs.score(p, t)):
        assert torch.equal(a, b)
    gm, wm = rs.mae(dp, dt, 2, 1), fs.mae(p, t)
    assert torch.equal(gm.sums, wm.sums) and torch.equal(gm.mae_mean, wm.mae_mean)
    # (the cell-area weights reach the l1 and ensemble kernels: their sums against fp64 with those weights, inside those suites' bounds)
    assert L1.judge_sums(gm.sums.cpu().numpy(), cp, ct, w, L1.chain_length(5, 8, ops.score_slices(2 * C, 5, 8)), "RegriddedScorer.mae") <= 1.0
    assert torch.equal(rs.quantile_error(dp, dt, 2, 1), fs.quantile_error(p, t))
    ens = torch.from_numpy(_field(8, 7, 24, 48, seed=8).copy()).to(dev)           # 4 members x 2 samples, member-major
    ge, we = rs.ensemble_score(ens, dt, 4, coff_ens=2, coff_tar=1), fs.ensemble_score(rg(ens[:, 2:5]), t, 4)
    for a, b in zip(ge, we):
        assert torch.equal(a, b)
    ce = rs._buf[("ens", (4, 2, C), torch.float32, dev)].cpu().numpy()
    assert R.judge(ce, ens.cpu().numpy().reshape(4, 2, 7, 24, 48)[:, :, 2:5], s["Ar"], s["Br"], cl, cn, "coarse members") <= 1.0
    got_e = {k: getattr(ge, k).cpu().numpy() for k in ("sums", "hist") + ER.NAMES}
    got_e["means"] = np.stack([getattr(ge, k + "_mean").cpu().numpy() for k in ER.NAMES])
    ER.judge(got_e, ce, ct, w, ER.chain_length(5, 8, ops.score_slices(2 * C, 5, 8), 4), stds, "RegriddedScorer.ensemble_score")
    assert len(rs._buf) == 3 and rs.score(dp, dt, 2, 1).rmse.data_ptr() != got.rmse.data_ptr() and len(rs._buf) == 3          # buffers are reused
    with pytest.raises(ValueError):
        rs.power_spectrum(dp)


def test_score_rollout_with_a_regridded_scorer_keeps_the_forecast_and_scores_the_stored_one(dev, lib, tmp_path):
    from tests.test_score_gpu import _registry_model
    from swin_v2_weather_amd import inference
    from swin_v2_weather_amd.utils import regrid as G
    from swin_v2_weather_amd.utils.weighted_acc_rmse import RegriddedScorer
    model = _registry_model(dev, tmp_path)
    B, Cout, H, W, steps = 2, 5, 48, 72, 3
    g = torch.Generator(device=dev).manual_seed(3)
    x0 = torch.randn(B, 9, H, W, device=dev, generator=g)
    cz = torch.rand(B, steps - 1, H, W, device=dev, generator=g) * 2 - 1
    truth = torch.randn(B, steps, Cout, H, W, device=dev, generator=g)
    clim = 0.3 * torch.randn(Cout, H, W, device=dev, generator=g)
    grid = G.grid_for_degrees(15.0)
    assert grid.shape == (13, 24) and grid.poles
    scorer = RegriddedScorer(G.Regridder(G.model_grid(H, W), grid, dev), Cout, climatology=clim, stds=torch.tensor([1.0, 2.0, 3.0, 4.0, 5.0]))
    assert scorer.regridder.tables is not None
    y = inference.rollout(model, x0, steps, cz, n_invar=3)
    kept = inference.score_rollout(model, x0, truth, steps, cz, n_invar=3, scorer=scorer, keep_forecast=True, extremes=True)
    assert torch.equal(kept.forecast, y)                                         # the predictions are rollout's, bit for bit
    assert kept.rmse.shape == (steps, Cout) and kept.acc.shape == (steps, Cout) and kept.tqe.shape == (steps, B, Cout)
    for s in range(steps):
        r = scorer.score(y[:, s], truth[:, s])
        assert torch.equal(kept.rmse[s], r.rmse_mean) and torch.equal(kept.acc[s], r.acc_mean)
        assert torch.equal(kept.rmse_samples[s], r.rmse) and torch.equal(kept.acc_samples[s], r.acc)
        assert torch.equal(kept.tqe[s], scorer.quantile_error(y[:, s], truth[:, s]))
    ring = inference.score_rollout(model, x0, truth, steps, cz, n_invar=3, scorer=scorer)
    assert ring.forecast is None and all(torch.equal(a, b) for a, b in zip(ring[:4], kept[:4]))
    with pytest.raises(ValueError, match="spectrum"):
        inference.score_rollout(model, x0, truth, steps, cz, n_invar=3, scorer=scorer, spectrum=True)
    ens = inference.ensemble_rollout(model, x0, truth, 2, 3, 0.05, seed=1, coszen=cz[:, :1], n_invar=3, scorer=scorer, score_control=True)
    assert ens.crps.shape == (2, Cout) and bool(torch.isfinite(ens.crps).all()) and ens.control.rmse.shape == (2, Cout)
    assert bool((ens.crps > 0).all()) and bool(torch.isfinite(ens.control.acc).all())


def test_cli_score_grid_writes_the_grid_key_and_changes_nothing_without_the_flag(dev, lib, tmp_path, capsys):
    from tests.test_score_gpu import _registry_model
    from swin_v2_weather_amd import inference
    from swin_v2_weather_amd.utils import regrid as G
    from swin_v2_weather_amd.utils.data_loader_era5 import cos_zenith
    from swin_v2_weather_amd.utils.weighted_acc_rmse import ForecastScorer, RegriddedScorer
    model = _registry_model(dev, tmp_path)
    reg = tmp_path / "swin_test_registry"
    rng = np.random.default_rng(11)
    B, Cout, H, W, steps = 2, 5, 48, 72, 2
    tm = rng.standard_normal((1, 73, 49, 80)).astype(np.float32)
    x0, truth = rng.standard_normal((B, 9, H, W)).astype(np.float32), rng.standard_normal((B, steps, Cout, H, W)).astype(np.float32)
    np.save(reg / "time_means.npy", tm); np.save(tmp_path / "x0.npy", x0); np.save(tmp_path / "truth.npy", truth)
    base = ["--registry", str(reg), "--steps", str(steps), "--init", str(tmp_path / "x0.npy"), "--truth", str(tmp_path / "truth.npy")]
    inference.main(base + ["--scores-out", str(tmp_path / "plain.json")])
    plain_out = capsys.readouterr().out.splitlines()
    inference.main(base + ["--scores-out", str(tmp_path / "coarse.json"), "--score-grid", "15"])
    coarse_out = capsys.readouterr().out.splitlines()
    plain, coarse = json.load(open(tmp_path / "plain.json")), json.load(open(tmp_path / "coarse.json"))
    cz = torch.stack([cos_zenith(2018, 6.0 * (s + 1), H, W) for s in range(steps - 1)], 0).unsqueeze(0).expand(B, -1, -1, -1).to(dev)
    cl, stds = tm[0, :Cout, :H, :W] / 2.0, np.full(Cout, 2.0, np.float32)
    dx, dt = torch.tensor(x0).to(dev), torch.tensor(truth).to(dev)
    # without the flag: the keys and numbers of before
    want = inference.score_rollout(model, dx, dt, steps, cz, 3, ForecastScorer(H, W, Cout, dev, climatology=cl, stds=stds))
    assert list(plain) == ["lead_hours", "rmse", "acc", "tracked"] and plain["rmse"] == want.rmse.cpu().tolist() and plain["acc"] == want.acc.cpu().tolist()
    assert len(plain_out) == 2 + steps and "grid" not in " ".join(plain_out)
    # with it: one more line that names the grid, the "grid" key, the regridded scorer's numbers
    grid = G.grid_for_degrees(15.0)
    want = inference.score_rollout(model, dx, dt, steps, cz, 3, RegriddedScorer(G.Regridder(G.model_grid(H, W), grid, dev), Cout, climatology=cl, stds=stds))
    assert coarse["grid"] == {"degrees": 15.0, "nlat": 13, "nlon": 24, "poles": True, "weights": "cell-area"}
    assert coarse["rmse"] == want.rmse.cpu().tolist() and coarse["acc"] == want.acc.cpu().tolist() and coarse["rmse"] != plain["rmse"]
    assert len(coarse_out) == 3 + steps and coarse_out[0] == plain_out[0] and "15 degree grid (13 x 24" in coarse_out[1] and coarse_out[2] == plain_out[1]
