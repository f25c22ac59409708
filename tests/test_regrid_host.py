"""CPU: the statement of conservative regridding (utils/regrid.py) against the independent construction of tests/regrid_reference.py and
its invariants; band tables; the CPU paths of Regridder and RegriddedScorer; ForecastScorer's weights argument; the --score-grid flag."""
import functools

import numpy as np
import pytest
import torch

from tests import regrid_reference as R
from swin_v2_weather_amd.utils import regrid as G

# (source grid, target grid) by (nlat, poles, crop rows or None, nlon)
PAIRS = {"721->121": ((721, True, None, 1440), (121, True, None, 240)),
         "720crop->121": ((721, True, 720, 1440), (121, True, None, 240)),
         "720crop->32": ((721, True, 720, 1440), (32, False, None, 64)),
         "24crop->5": ((25, True, 24, 48), (5, True, None, 8)),
         "25->4": ((25, True, None, 48), (4, False, None, 8)),
         "24->7": ((24, False, None, 48), (7, False, None, 20))}


def _grid(spec):
    nlat, poles, crop, nlon = spec
    g = G.equiangular_grid(nlat, nlon, poles)
    return g if crop is None else g.rows(0, crop)


def _ref_lat(spec):
    nlat, poles, crop, _ = spec
    c = R.centres(nlat, poles)
    return c if crop is None else c[:crop]


@functools.lru_cache(maxsize=None)
def _pair(name):
    """(src, dst, A, Bm) of utils/regrid.py and (A, Bm) of the reference; made once, never modified"""
    s, d = PAIRS[name]
    src, dst = _grid(s), _grid(d)
    A, Bm = G.conservative_weights(src, dst)
    Ar, Br = R.lat_matrix(_ref_lat(s), _ref_lat(d)), R.lon_matrix(s[3], d[3])
    for a in (A, Bm, Ar, Br):
        a.setflags(write=False)
    return src, dst, A, Bm, Ar, Br


@pytest.mark.parametrize("name", list(PAIRS))
def test_weights_match_the_definition_rows_sum_to_one_and_the_area_integral_is_conserved(name):
    src, dst, A, Bm, Ar, Br = _pair(name)
    assert A.dtype == np.float64 and A.shape == (dst.nlat, src.nlat) and Bm.shape == (dst.nlon, src.nlon)
    assert np.all(A >= 0) and np.all(Bm >= 0)
    assert np.abs(A.sum(axis=1) - 1).max() <= 1e-14 and np.abs(Bm.sum(axis=1) - 1).max() <= 1e-14
    assert np.array_equal(A != 0, Ar != 0) and np.array_equal(Bm != 0, Br != 0)           # the same cells overlap
    assert np.abs(A - Ar).max() <= 1e-14 and np.abs(Bm - Br).max() <= 1e-14
    # constants map to constants
    y = R.regrid(np.full(src.shape, 3.25), A, Bm)
    assert np.abs(y - 3.25).max() <= 1e-13
    # sum area_dst y = sum area_src x, with the reference's fp64 areas (means over the grid: both are the sphere's mean)
    x = np.random.default_rng(5).standard_normal((2,) + src.shape)
    a_src, a_dst = R.area(src.lat), R.area(dst.lat)
    lhs = (a_dst[:, None] * R.regrid(x, A, Bm)).sum(axis=(-1, -2)) / (dst.nlat * dst.nlon)
    rhs = (a_src[:, None] * x).sum(axis=(-1, -2)) / (src.nlat * src.nlon)
    scale = (a_src[:, None] * np.abs(x)).sum(axis=(-1, -2)) / (src.nlat * src.nlon)
    print(name, "area integral: relative difference", np.abs(lhs - rhs) / scale)
    assert np.all(np.abs(lhs - rhs) <= 1e-12 * scale)


def test_closed_forms_at_the_production_pair():
    src, dst, A, Bm, _, _ = _pair("720crop->121")
    st, cnt, w = G.band_tables(Bm)
    assert st.dtype == np.int32 and cnt.dtype == np.int32 and w.dtype == np.float32 and w.shape == (240, 7)
    assert np.all(cnt == 7) and st[0] == 1437 and np.array_equal(st[1:], 6 * np.arange(1, 240) - 3)
    assert np.array_equal(w, np.tile((np.array([1, 2, 2, 2, 2, 2, 1]) / 12.0).astype(np.float32), (240, 1)))
    assert np.flatnonzero(Bm[0]).tolist() == [0, 1, 2, 3, 1437, 1438, 1439]
    # target row 60 (the equator, bounds +-0.75 degrees) over the source rows 357 .. 363 (centres 0.75 .. -0.75): sin differences
    ls, lc, lw = G.band_tables(A, periodic=False)
    assert ls[60] == 357 and lc[60] == 7
    edges = np.array([0.75, 0.625, 0.375, 0.125, -0.125, -0.375, -0.625, -0.75])
    want = -np.diff(np.sin(np.deg2rad(edges))) / (2 * np.sin(np.deg2rad(0.75)))
    assert np.abs(A[60, 357:364] - want).max() <= 1e-15 and np.array_equal(lw[60], want.astype(np.float32))
    # band counts: 3 - 7 from the 720-row crop, 4 - 7 from the full 721 rows, <= 24 at 5.625 degrees
    assert lc.min() == 3 and lc.max() == 7
    full = G.band_tables(_pair("721->121")[2], periodic=False)[1]
    assert full.min() == 4 and full.max() == 7
    _, _, A5, B5, _, _ = _pair("720crop->32")
    c5 = np.concatenate((G.band_tables(A5, periodic=False)[1], G.band_tables(B5)[1]))
    assert c5.min() == 22 and c5.max() == 24
    assert np.array_equal(R.counts(Bm), cnt) and np.array_equal(R.counts(A), lc)


@pytest.mark.parametrize("name", ["720crop->121", "24crop->5", "24->7"])
def test_band_tables_reproduce_the_dense_matrix_after_fp32_rounding(name):
    _, _, A, Bm, _, _ = _pair(name)
    for M, periodic in ((A, False), (Bm, True)):
        st, cnt, w = G.band_tables(M, periodic=periodic)
        assert w.shape == (M.shape[0], cnt.max()) and cnt.min() >= 1
        for r in range(M.shape[0]):
            assert np.all(w[r, cnt[r]:] == 0)
        assert np.array_equal(R.dense_from_tables(st, cnt, w, M.shape[1]), M.astype(np.float32).astype(np.float64))
        if not periodic:
            assert st.min() >= 0 and (st + cnt).max() <= M.shape[1]


def test_band_tables_raise_above_the_cap():
    A33, B33 = G.conservative_weights(G.equiangular_grid(66, 64, False), G.equiangular_grid(2, 2, False))
    assert R.counts(A33).max() == 33 and R.counts(B33).max() == 33
    for M in (A33, B33):
        with pytest.raises(ValueError, match="cap"):
            G.band_tables(M)
        assert G.band_tables(M, cap=33)[1].max() == 33
    A32, B31 = G.conservative_weights(G.equiangular_grid(64, 124, False), G.equiangular_grid(2, 4, False))
    assert G.band_tables(A32, periodic=False)[1].tolist() == [32, 32] and G.band_tables(B31)[1].max() == 31
    with pytest.raises(ValueError, match="one run"):
        G.band_tables(np.array([[0.5, 0.0, 0.0, 0.0, 0.0, 0.5]]), periodic=False)
    assert [t.tolist() for t in G.band_tables(np.array([[0.5, 0.0, 0.0, 0.0, 0.0, 0.5]]))] == [[5], [2], [[0.5, 0.5]]]
    for holes in ([[0.5, 0.0, 0.0, 0.5, 0.0, 0.0]], [[0.25, 0.0, 0.25, 0.0, 0.0, 0.5]], [[0.0] * 6]):                # a zero inside the run; no run at all
        with pytest.raises(ValueError, match="zeros inside|empty"):
            G.band_tables(np.array(holes))


def test_area_weights_and_grids():
    for grid, lat in ((G.grid_for_degrees(1.5), R.centres(121)), (G.grid_for_degrees(5.625), R.centres(32, False)),
                      (G.model_grid(720, 1440), R.centres(721)[:720])):
        a = G.area_weights(grid)
        assert a.dtype == np.float32 and a.shape == (grid.nlat,) and np.array_equal(grid.lat, lat)
        assert np.array_equal(a, R.area(lat).astype(np.float32)) and abs(float(a.astype(np.float64).mean()) - 1) <= 1e-7
        if grid.lat[0] == -grid.lat[-1]:
            assert np.array_equal(a, a[::-1])                                   # symmetric grids: symmetric weights, bit for bit
    g15, g56 = G.grid_for_degrees(1.5), G.grid_for_degrees(5.625)
    assert g15.shape == (121, 240) and g15.poles and g56.shape == (32, 64) and not g56.poles and g56.lat[0] == 90 - 5.625 / 2
    assert G.grid_for_degrees(0.25) == G.equiangular_grid(721, 1440) and G.grid_for_degrees(0.25).rows(0, 720) == G.model_grid(720, 1440)
    assert G.grid_for_degrees(2.8125).shape == (64, 128) and G.grid_for_degrees(1.40625).shape == (128, 256)
    assert G.grid_for_degrees(1.0).shape == (181, 360) and G.grid_for_degrees(12.0).shape == (15, 30) and not G.grid_for_degrees(12.0).poles
    for bad in (7.0, 0.0, -1.5, float("nan"), 360.0):
        with pytest.raises(ValueError):
            G.grid_for_degrees(bad)
    with pytest.raises(ValueError):
        G.LatLonGrid([10.0, 20.0], 8)


def _x(shape, seed=0):
    return np.random.default_rng(seed).standard_normal(shape).astype(np.float32)


def test_regridder_on_cpu_tensors_matches_the_statement():
    src, dst, A, Bm, Ar, Br = _pair("24crop->5")
    rg = G.Regridder(src, dst)
    assert rg.device == torch.device("cpu") and rg.tables is not None and torch.equal(rg.area_weights, torch.from_numpy(G.area_weights(dst)))
    x = _x((2, 3, 24, 48))
    for dt, chain in ((torch.float32, (24, 48)), (torch.float64, None)):
        y = rg(torch.from_numpy(x).to(dt))
        assert y.dtype == dt and tuple(y.shape) == (2, 3, 5, 8)
        if chain is None:
            assert np.abs(y.numpy() - R.regrid(x, Ar, Br)).max() <= 1e-13
        else:
            assert R.judge(y.numpy(), x, Ar, Br, np.full(5, chain[0]), np.full(8, chain[1]), "Regridder cpu fp32") <= 1.0
    # other ranks, out=, autograd
    assert torch.equal(rg(torch.from_numpy(x[0, 0])), rg(torch.from_numpy(x))[0, 0])
    wide = torch.zeros(2, 7, 5, 8)
    got = rg(torch.from_numpy(x), out=wide[:, 2:5])
    assert got.data_ptr() == wide[:, 2:5].data_ptr() and torch.equal(wide[:, 2:5], rg(torch.from_numpy(x))) and float(wide[:, :2].abs().sum()) == 0
    xg = torch.from_numpy(x).double().requires_grad_(True)
    rg(xg).sum().backward()
    assert np.abs(xg.grad.numpy() - (Ar.sum(axis=0)[:, None] * Br.sum(axis=0)[None, :])).max() <= 1e-13
    with pytest.raises(ValueError):
        rg(torch.zeros(2, 3, 25, 48))
    with pytest.raises(ValueError):
        rg(torch.from_numpy(x), out=torch.zeros(2, 3, 5, 9))
    # src == dst: the input itself
    same = G.Regridder(src, G.equiangular_grid(25, 48).rows(0, 24))
    t = torch.from_numpy(x)
    assert same.identity and same(t) is t
    # bands above the cap: no tables, the statement all the same
    big = G.Regridder(G.equiangular_grid(66, 64, False), G.equiangular_grid(2, 2, False))
    assert big.tables is None
    xb = _x((1, 1, 66, 64), 3)
    Ab, Bb = R.lat_matrix(R.centres(66, False), R.centres(2, False)), R.lon_matrix(64, 2)
    assert R.judge(big(torch.from_numpy(xb)).numpy(), xb, Ab, Bb, np.full(2, 66), np.full(2, 64), "above the cap") <= 1.0


def test_nan_locality_of_the_torch_path():
    """the dense products would spread a NaN over whole target rows and columns (0 * NaN); Regridder's torch path masks instead: exactly
    the target cells whose bands contain a non-finite source cell become NaN, every other output is what it is without that cell"""
    src, dst, A, Bm, Ar, Br = _pair("24crop->5")
    rg = G.Regridder(src, dst)
    x = _x((1, 2, 24, 48), 7)
    x[0, 0, 10, 5], x[0, 1, 23, 47] = np.nan, np.inf
    y = rg(torch.from_numpy(x)).numpy()
    plain = G.regrid_torch(torch.from_numpy(x), A.copy(), Bm.copy()).numpy()
    for c, (j, i) in enumerate(((10, 5), (23, 47))):
        hit = np.outer(Ar[:, j] != 0, Br[:, i] != 0)
        assert hit.sum() >= 1 and np.array_equal(np.isnan(y[0, c]), hit)
        assert np.isnan(plain[0, c]).sum() > hit.sum()                          # what the mask is there for
        x0 = x[0, c].copy()
        x0[j, i] = 0.0
        ok = ~hit
        assert R.judge(y[0, c], x0, Ar, Br, np.full(5, 24), np.full(8, 48), f"plane {c} beside the bad cell", finite_only=ok) <= 1.0


def _golden_fields():
    j = np.arange(2 * 3 * 6 * 8, dtype=np.float64).reshape(2, 3, 6, 8)
    p, t = np.sin(0.37 * j + 0.1).astype(np.float32), np.cos(0.23 * j - 0.4).astype(np.float32)
    c = (0.25 * np.sin(0.11 * np.arange(3 * 6 * 8)).reshape(3, 6, 8)).astype(np.float32)
    return torch.from_numpy(p), torch.from_numpy(t), torch.from_numpy(c)


def test_forecast_scorer_default_weights_keep_their_bits_and_weights_replace_them():
    """the numbers below are the scorer's before it had a weights argument (CPU path, this fixed input)"""
    from swin_v2_weather_amd.utils.weighted_acc_rmse import ForecastScorer, latitude_weights
    p, t, c = _golden_fields()
    stds = np.array([1.5, 2.0, 0.25], np.float32)
    sc = ForecastScorer(6, 8, 3, "cpu", climatology=c, stds=stds)
    r, m = sc.score(p, t), sc.mae(p, t)
    hexes = lambda v: [float(e).hex() for e in v.reshape(-1)]          # noqa: E731
    assert hexes(r.rmse) == ['0x1.2638e00000000p+0', '0x1.2806f20000000p+0', '0x1.3a40ba0000000p+0', '0x1.317ad40000000p+0',
                             '0x1.1ee5c00000000p+0', '0x1.1b22fe0000000p+0']
    assert hexes(r.acc) == ['-0x1.f4de020000000p-4', '-0x1.12e46c0000000p-3', '-0x1.c010740000000p-3', '-0x1.02e4680000000p-1',
                            '-0x1.30ae040000000p-2', '-0x1.1ea5b40000000p-3']
    assert hexes(r.rmse_mean) == ['0x1.c1c6c80000000p+0', '0x1.2376580000000p+1', '0x1.2ab1dc0000000p-2']
    assert hexes(m.mae) == ['0x1.f3ce000000000p-1', '0x1.ff07fe0000000p-1', '0x1.1851a60000000p+0', '0x1.0bc0e20000000p+0',
                            '0x1.e571680000000p-1', '0x1.d76ab00000000p-1']
    assert sc.w is latitude_weights(6)
    same = ForecastScorer(6, 8, 3, "cpu", climatology=c, stds=stds, weights=latitude_weights(6)).score(p, t)
    assert torch.equal(same.sums, r.sums) and torch.equal(same.rmse, r.rmse) and torch.equal(same.acc, r.acc)
    w = np.array([0.5, 1.0, 1.5, 1.5, 1.0, 0.5], np.float32)
    other = ForecastScorer(6, 8, 3, "cpu", climatology=c, weights=w)
    d = (p.double() - t.double()) ** 2
    want = np.sqrt((torch.from_numpy(w).double().reshape(1, 1, 6, 1) * d).sum(dim=(-1, -2)).numpy() / 48.0)
    assert np.abs(other.score(p, t).rmse.numpy() - want).max() <= 1e-6 and not torch.equal(other.score(p, t).rmse, r.rmse)
    with pytest.raises(ValueError):
        ForecastScorer(6, 8, 3, "cpu", weights=w[:5])


def test_regridded_scorer_on_cpu_equals_the_forecast_scorer_on_statement_regridded_fields():
    from swin_v2_weather_amd.utils.weighted_acc_rmse import ForecastScorer, RegriddedScorer
    src, dst, A, Bm, Ar, Br = _pair("24crop->5")
    rg = G.Regridder(src, dst)
    C = 3
    prd, tar, clim = _x((2, 7, 24, 48), 1), _x((2, 5, 24, 48), 2), 0.3 * _x((C, 24, 48), 3)
    stds = np.array([1.5, 2.0, 0.25], np.float32)
    rs = RegriddedScorer(rg, C, climatology=clim, stds=stds)
    assert (rs.C, rs.H, rs.W) == (C, 24, 48) and rs.grid == dst and tuple(rs.clim.shape) == (C, 24, 48)
    coarse = lambda a: G.regrid_torch(torch.from_numpy(np.ascontiguousarray(a)), A.copy(), Bm.copy())          # noqa: E731
    fs = ForecastScorer(5, 8, C, "cpu", climatology=coarse(clim), stds=stds, weights=G.area_weights(dst))
    p, t = coarse(prd[:, 2:5]), coarse(tar[:, 1:4])
    got, want = rs.score(torch.from_numpy(prd), torch.from_numpy(tar), coff_prd=2, coff_tar=1), fs.score(p, t)
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    gm, wm = rs.mae(torch.from_numpy(prd), torch.from_numpy(tar), 2, 1), fs.mae(p, t)
    assert torch.equal(gm.mae, wm.mae) and torch.equal(gm.mae_mean, wm.mae_mean)
    assert torch.equal(rs.quantile_error(torch.from_numpy(prd), torch.from_numpy(tar), 2, 1), fs.quantile_error(p, t))
    # the coarse fields themselves against the fp64 statement, through the sums: RMSE of the regridded difference with the cell areas
    d = R.regrid(prd[:, 2:5].astype(np.float64) - tar[:, 1:4], Ar, Br)
    want_rmse = np.sqrt((R.area(dst.lat)[:, None] * d * d).sum(axis=(-1, -2)) / 40.0)
    assert np.abs(got.rmse.numpy() - want_rmse).max() <= 1e-5 * want_rmse.max()
    ens = _x((4, 2, 7, 24, 48), 4)
    ge = rs.ensemble_score(torch.from_numpy(ens), torch.from_numpy(tar), 4, coff_ens=2, coff_tar=1)
    we = fs.ensemble_score(coarse(ens[:, :, 2:5]), t, 4)
    for a, b in zip(ge, we):
        assert torch.equal(a, b)
    flat = rs.ensemble_score(torch.from_numpy(ens).flatten(0, 1), torch.from_numpy(tar), 4, coff_ens=2, coff_tar=1)
    assert torch.equal(flat.crps, ge.crps)
    with pytest.raises(ValueError, match="native|own grid"):
        rs.power_spectrum(torch.from_numpy(prd))
    with pytest.raises(ValueError):
        rs.score(torch.from_numpy(prd), torch.from_numpy(tar), coff_prd=5)
    # no climatology: no ACC, as the ForecastScorer
    assert RegriddedScorer(rg, C).score(torch.from_numpy(prd), torch.from_numpy(tar), 2, 1).acc is None and RegriddedScorer(rg, C).clim is None


def test_score_rollout_refuses_a_spectrum_on_a_regridded_scorer_before_any_model_call():
    from swin_v2_weather_amd import inference
    from swin_v2_weather_amd.utils.weighted_acc_rmse import RegriddedScorer
    src, dst = _pair("24crop->5")[:2]

    class Net:
        out_chans = 3

        def forward_rollout(self, *a):
            raise AssertionError("the model was called")
    with pytest.raises(ValueError, match="spectrum"):
        inference.score_rollout(Net(), torch.zeros(1, 3, 24, 48), torch.zeros(1, 2, 3, 24, 48), 2, scorer=RegriddedScorer(G.Regridder(src, dst), 3),
                                spectrum=True)


def test_cli_score_grid_parses_and_is_rejected_with_spectrum(capsys):
    from swin_v2_weather_amd import inference
    ap = inference.build_parser()
    base = ["--registry", "R", "--truth", "t.npy"]
    assert ap.parse_args(base).score_grid is None
    assert ap.parse_args(base + ["--score-grid", "1.5"]).score_grid == 1.5
    a = ap.parse_args(base + ["--score-grid", "5.625", "--extremes"])
    assert a.score_grid == 5.625 and a.extremes
    assert ap.parse_args(base + ["--score-grid", "1.5", "--ensemble", "4", "--perturbation", "0.1"]).ensemble == 4
    for bad in (["--score-grid", "1.5", "--spectrum"], ["--score-grid", "7"], ["--score-grid", "-1.5"]):
        with pytest.raises(SystemExit) as e:
            ap.parse_args(base + bad)
        assert e.value.code == 2
    with pytest.raises(SystemExit) as e:                                       # nothing to score without the verifying analysis
        ap.parse_args(["--registry", "R", "--score-grid", "1.5"])
    assert e.value.code == 2
    assert "--score-grid" in capsys.readouterr().err


def test_library_declares_the_regrid_entry_point():
    from swin_v2_weather_amd import _lib as L
    assert "regrid.hip" in L.SOURCES and "swv2_regrid" in L.SYMBOLS
    L.build_library()
    lib = L.load()
    assert lib.swv2_version() == L.ABI_VERSION and lib.swv2_regrid.argtypes == L.SYMBOLS["swv2_regrid"][1] and len(lib.swv2_regrid.argtypes) == 19
