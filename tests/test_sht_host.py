"""No GPU: the tables of utils/sht.py against closed forms, scipy and orthonormality in fp64; the plain-torch statement against the
independent fp64 statement of tests/sht_reference.py; GeometricH1Loss against a literal numpy restatement; the C ABI's host side."""
import math

import numpy as np
import pytest
import torch

from tests import sht_reference as R
from swin_v2_weather_amd.utils import sht

GRIDS = [(2, 4), (8, 32), (24, 16), (16, 32), (33, 64), (65, 128), (19, 15), (96, 192), (9, 16)]
GRID_IDS = [f"{a}x{b}" for a, b in GRIDS]


@pytest.mark.parametrize("nlat", [2, 3, 8, 9, 16, 19, 33, 64])
def test_weights_sum_symmetry_and_polynomial_exactness(nlat):
    w = sht.clenshaw_curtis_weights(nlat)
    x = np.cos(np.pi * np.arange(nlat) / (nlat - 1))
    assert abs(w.sum() - 2.0) < 1e-13 and np.allclose(w, w[::-1], rtol=0, atol=1e-15)
    for k in range(nlat):                                    # exact for every polynomial of degree <= nlat - 1
        assert abs(np.sum(w * x ** k) - (2.0 / (k + 1) if k % 2 == 0 else 0.0)) < 1e-13, k
    assert np.allclose(w, R.weights(nlat), rtol=0, atol=1e-13)


def test_weights_of_the_two_row_grid():
    assert np.array_equal(sht.clenshaw_curtis_weights(2), np.array([1.0, 1.0]))


def test_table_against_closed_forms():
    """Y_00 .. Y_22 pin normalisation and Condon-Shortley phase without the recursion"""
    nlat, nlon = 17, 32
    T = sht.legendre_table(nlat, nlon) / sht.clenshaw_curtis_weights(nlat)
    th = np.pi * np.arange(nlat) / (nlat - 1)
    x, s = np.cos(th), np.sin(th)
    pi = math.pi
    closed = {(0, 0): np.full(nlat, 0.5 / math.sqrt(pi)),
              (1, 0): 0.5 * math.sqrt(3 / pi) * x,
              (1, 1): -0.5 * math.sqrt(3 / (2 * pi)) * s,
              (2, 0): 0.25 * math.sqrt(5 / pi) * (3 * x * x - 1),
              (2, 1): -0.5 * math.sqrt(15 / (2 * pi)) * s * x,
              (2, 2): 0.25 * math.sqrt(15 / (2 * pi)) * s * s}
    for (l, m), v in closed.items():
        assert np.allclose(T[m, l], v, rtol=0, atol=1e-14), (l, m)


def test_table_against_scipy():
    from scipy.special import gammaln, lpmv
    nlat, nlon = 21, 40
    T = sht.legendre_table(nlat, nlon) / sht.clenshaw_curtis_weights(nlat)
    x = np.cos(np.pi * np.arange(nlat) / (nlat - 1))
    for l in range(13):
        for m in range(l + 1):
            norm = math.sqrt((2 * l + 1) / (4 * math.pi) * math.exp(gammaln(l - m + 1) - gammaln(l + m + 1)))
            assert np.allclose(T[m, l], norm * lpmv(m, l, x), rtol=1e-12, atol=1e-13), (l, m)          # lpmv carries the phase


@pytest.mark.parametrize("grid", GRIDS, ids=GRID_IDS)
def test_entries_below_the_diagonal_and_past_lmax_are_zero(grid):
    T = sht.legendre_table(*grid)
    assert T.shape == (grid[1] // 2 + 1, grid[0], grid[0])
    assert np.all(T[~R.tri(T.shape[0], T.shape[1])] == 0.0)
    assert np.all(T[grid[0]:] == 0.0)


def _synthesis(nlat, nlon, L0, rng):
    """a real field with random coefficients for l <= L0, and those coefficients [lmax, mmax] (complex; zero elsewhere)"""
    T = sht.legendre_table(nlat, nlon) / sht.clenshaw_curtis_weights(nlat)
    mmax = T.shape[0]
    c = np.zeros((nlat, mmax), complex)
    lon = 2 * np.pi * np.arange(nlon) / nlon
    f = np.zeros((nlat, nlon))
    for l in range(L0 + 1):
        for m in range(min(l, mmax - 1, (nlon - 1) // 2) + 1):
            c[l, m] = rng.standard_normal() + (1j * rng.standard_normal() if m else 0.0)
            f += (1.0 if m == 0 else 2.0) * np.real(c[l, m] * np.exp(1j * m * lon))[None, :] * T[m, l][:, None]
    return f, c


@pytest.mark.parametrize("grid", [(17, 32), (9, 16), (24, 16), (19, 15), (33, 64)], ids=lambda g: f"{g[0]}x{g[1]}")
def test_recovery_and_parseval(grid):
    """orthonormality: coefficients for l <= L0 with 2 L0 <= nlat - 1 come back to 1e-12, every other coefficient the rule is exact for
    vanishes, and sum_l P[l] is the quadrature of f^2"""
    nlat, nlon = grid
    L0 = (nlat - 1) // 2
    f, c = _synthesis(nlat, nlon, L0, np.random.default_rng(nlat))
    table = torch.from_numpy(sht.legendre_table(nlat, nlon))
    got = sht.real_sht_torch(torch.from_numpy(f), table).numpy()
    exact = np.arange(nlat) + L0 <= nlat - 1                 # degrees the quadrature resolves against a field of degree L0
    assert np.abs(got - c)[exact].max() < 1e-12
    P = sht.degree_power_torch(torch.from_numpy(f), table).numpy()
    w = sht.clenshaw_curtis_weights(nlat)
    assert abs(P[exact].sum() - np.sum(w[:, None] * f * f) * 2 * np.pi / nlon) < 1e-11 * max(1.0, P.sum())
    assert abs(P[: L0 + 1].sum() - (np.abs(c[:, 0]) ** 2).sum() - 2 * (np.abs(c[:, 1:]) ** 2).sum()) < 1e-11 * P.sum()


def _field(grid, planes=3):
    rng = np.random.default_rng(grid[0] * 100 + grid[1])
    return rng.standard_normal((planes,) + grid).cumsum(-1) + rng.standard_normal((planes, 1, 1))


@pytest.mark.parametrize("grid", GRIDS, ids=GRID_IDS)
def test_statement_against_the_independent_reference(grid):
    x = _field(grid)
    T = R.legendre(*grid)
    table = sht.legendre_table(*grid)
    assert np.abs(table - T).max() < 1e-13
    c_ref, mag = R.coeffs(T, R.operand(x, T.shape[0]))
    c = torch.view_as_real(sht.real_sht_torch(torch.from_numpy(x), torch.from_numpy(table))).numpy()          # [planes, lmax, mmax, 2]
    got = c.transpose(2, 0, 3, 1).reshape(c_ref.shape)
    assert np.all(np.abs(got - c_ref) <= 1e-12 * mag + 1e-14 * mag.max())
    P_ref = R.power(c_ref)
    P = sht.degree_power_torch(torch.from_numpy(x), torch.from_numpy(table)).numpy()
    assert np.all(np.abs(P - P_ref) <= 1e-11 * P_ref + 1e-14 * P_ref.max())


def test_degree_power_on_the_cpu_is_the_statement_and_caches_its_table():
    x = torch.from_numpy(_field((9, 16))).float()
    a = sht.degree_power(x)
    assert a.shape == (3, 9) and a.dtype == torch.float32
    assert sht.device_table(9, 16, "cpu") is sht.device_table(9, 16, "cpu")
    assert torch.equal(a, sht.degree_power_torch(x, sht.device_table(9, 16, "cpu")))
    d = sht.degree_power(x.double())
    assert d.dtype == torch.float64 and torch.allclose(d, a.double(), rtol=1e-4, atol=1e-6)


def test_the_bounds_reject_the_three_mutants():
    """what the GPU test asserts -- |power - reference| <= its bound, |loss - reference| within the bound carried through -- fails for a
    statement without the factor 2, with l (l + 1) shifted, or without the row l = m"""
    grid = (16, 32)
    x = _field(grid, planes=4).astype(np.float32)
    T = sht.legendre_table(*grid).astype(np.float32).astype(np.float64)
    P, dP = R.end_to_end(x, T)
    c = R.coeffs(T, R.operand(x, T.shape[0]))[0]
    assert np.all(np.abs(R.power(c) - P) <= dP)
    for mutant in (R.power(c, drop_factor=True), R.power(c, drop_diagonal=True)):
        assert np.any(np.abs(mutant - P) > dP)
    tar = x[2:].reshape(1, 2, *grid).astype(np.float64)                       # a red target, a white error: their spectra differ
    prd = tar + np.random.default_rng(3).standard_normal(tar.shape)
    for absolute in (False, True):
        for squared in (False, True):
            good = R.h1_loss(prd, tar, T, absolute, squared)
            bad = R.h1_loss(prd, tar, T, absolute, squared, shift=1)
            assert abs(bad - good) > 1e-2 * abs(good)          # the GPU test's derived bound on the loss is below 1e-3 relative (asserted there)


def _loss_inputs(B=2, C=3, grid=(9, 16)):
    rng = np.random.default_rng(5)
    return rng.standard_normal((B, C) + grid), rng.standard_normal((B, C) + grid) + 0.5


@pytest.mark.parametrize("squared", [False, True], ids=["norm", "squared"])
@pytest.mark.parametrize("absolute", [False, True], ids=["relative", "absolute"])
def test_h1_loss_against_the_numpy_restatement(absolute, squared):
    from swin_v2_weather_amd.utils.losses import GeometricH1Loss
    prd, tar = _loss_inputs()
    T = R.legendre(9, 16)
    tp, tt = torch.from_numpy(prd), torch.from_numpy(tar)
    for kw in (dict(), dict(size_average=True), dict(reduction=False), dict(alpha=0.25)):
        loss = GeometricH1Loss((9, 16), absolute=absolute, squared=squared, **kw).double()
        ref = R.h1_loss(prd, tar, T, absolute, squared, alpha=kw.get("alpha", 0.5), size_average=kw.get("size_average", False),
                        reduction=kw.get("reduction", True))
        assert np.allclose(loss(tp, tt).numpy(), ref, rtol=1e-11, atol=0), kw
    mask = np.array([0.25, 1.5])
    for kw in (dict(), dict(size_average=True), dict(reduction=False)):
        loss = GeometricH1Loss((9, 16), absolute=absolute, squared=squared, **kw).double()
        ref = R.h1_loss(prd, tar, T, absolute, squared, mask=mask, size_average=kw.get("size_average", False), reduction=kw.get("reduction", True))
        assert np.allclose(loss(tp, tt, torch.from_numpy(mask)).numpy(), ref, rtol=1e-11, atol=0), kw


def test_h1_loss_mask_broadcasts_as_torch_does():
    """the reference's dispatch would hand [1, C] channel weights to `mask`: [B] * [1, C] fails unless B is 1 or C, and so does this"""
    from swin_v2_weather_amd.utils.losses import GeometricH1Loss
    prd, tar = (torch.from_numpy(a) for a in _loss_inputs(B=2, C=3))
    with pytest.raises(RuntimeError):
        GeometricH1Loss((9, 16))(prd, tar, torch.ones(1, 3, dtype=torch.float64))
    assert GeometricH1Loss((9, 16), reduction=False)(prd[:1], tar[:1], torch.ones(1, 3, dtype=torch.float64)).shape == (1, 3)


@pytest.mark.parametrize("squared", [False, True], ids=["norm", "squared"])
@pytest.mark.parametrize("absolute", [False, True], ids=["relative", "absolute"])
def test_h1_loss_gradcheck(absolute, squared):
    from swin_v2_weather_amd.utils.losses import GeometricH1Loss
    prd, tar = (torch.from_numpy(a) for a in _loss_inputs(B=2, C=2))
    loss = GeometricH1Loss((9, 16), absolute=absolute, squared=squared).double()
    assert torch.autograd.gradcheck(lambda p: loss(p, tar), (prd.requires_grad_(True),))          # torch's defaults: eps 1e-6, atol 1e-5, rtol 1e-3


def test_loss_handler_still_refuses_geometric_h1():
    from types import SimpleNamespace
    from swin_v2_weather_amd.utils.losses import LossHandler
    params = SimpleNamespace(n_future=0, img_shape_x=9, img_shape_y=16, loss="geometric h1", channel_weights="constant", n_out_channels=2,
                             channel_names=["u10m", "v10m"], out_channels=[0, 1], dt=1)
    with pytest.raises(ValueError):
        LossHandler(params)


def test_small_scale_power_ratio_and_scorer_spectrum_on_the_cpu():
    from swin_v2_weather_amd.utils.weighted_acc_rmse import ForecastScorer, small_scale_power_ratio
    x = torch.from_numpy(_field((8, 32), planes=12)).float().reshape(2, 6, 8, 32)
    sc = ForecastScorer(8, 32, 2, "cpu")
    ps = sc.power_spectrum(x, x * 0.5, coff_prd=2, coff_tar=4)
    assert ps.pred.shape == ps.truth.shape == (2, 2, 8)
    assert torch.equal(ps.pred, sht.degree_power(x[:, 2:4])) and torch.equal(ps.truth, sht.degree_power(0.5 * x[:, 4:6]))
    assert sc.power_spectrum(x).truth is None
    r = small_scale_power_ratio(ps.pred, ps.truth)
    assert r.shape == (2, 2) and torch.allclose(r, ps.pred[..., 4:].sum(-1) / ps.truth[..., 4:].sum(-1))
    assert torch.allclose(small_scale_power_ratio(ps.truth * 0.25, ps.truth), torch.full((2, 2), 0.25))


def test_cli_flags():
    from swin_v2_weather_amd import inference
    ap = inference.build_parser()
    a = ap.parse_args(["--registry", "r", "--truth", "t.npy", "--spectrum", "--spectrum-out", "s.npz"])
    assert a.spectrum and a.spectrum_out == "s.npz"
    for bad in (["--spectrum-out", "s.npz"], ["--truth", "t.npy", "--spectrum", "--ensemble", "4", "--perturbation", "0.1"]):
        with pytest.raises(SystemExit):
            ap.parse_args(["--registry", "r"] + bad)
    assert len(inference.RolloutScores._fields) == 6 and inference.RolloutScores(1, 2, 3, 4, 5).spectrum is None          # the tuple is unchanged
    sc = inference.RolloutScores(torch.ones(2, 2), None, None, None, None).with_spectrum(
        inference.RolloutSpectrum(None, None, torch.full((2, 3, 2), 0.5)))
    assert len(sc) == 6 and sc.spectrum.ratio.shape == (2, 3, 2)
    assert "ssr_u10m" in inference.lead_time_table(sc, [("u10m", 0)]).splitlines()[0]


def test_abi_host_side():
    from swin_v2_weather_amd import _lib as L
    assert "sht.hip" in L.SOURCES and L.ABI_VERSION == 113
    lib = L.load()
    assert lib.swv2_version() == 113
    for planes, lmax, mmax in ((1, 2, 3), (146, 720, 721), (5, 24, 9), (17, 19, 8), (3, 8, 17)):
        assert lib.swv2_sht_ws_bytes(planes, lmax, mmax) == -(-min(mmax, lmax) // L.SHT_MRUN) * planes * lmax * 4
    for bad in ((0, 8, 8), (4, 0, 8), (4, 8, 0), (-1, 8, 8), (4, -8, 8), (4, 8, -3)):
        assert lib.swv2_sht_ws_bytes(*bad) == 0
    # refused before any launch (no device is touched): null pointers, bad sizes, a short workspace
    assert lib.swv2_sht_power(None, None, None, None, 1, 8, 8, 5, None, 0, None) == -1
    assert lib.swv2_sht_power(16, 16, 16, None, 0, 8, 8, 5, 16, 1 << 20, None) == -1
    assert lib.swv2_sht_power(16, 16, 16, None, 2, 8, 8, 5, 16, lib.swv2_sht_ws_bytes(2, 8, 5) - 1, None) == -1
    assert lib.swv2_sht_adjoint(16, None, 16, 16, 2, 8, 8, 5, None) == -1
    assert lib.swv2_sht_adjoint(16, 16, 16, 16, 2, 8, -8, 5, None) == -1
    assert lib.swv2_sht_repack(None, 16, 2, 8, 5, 1.0, 0, None) == -1 and lib.swv2_sht_repack(16, 16, 0, 8, 5, 1.0, 1, None) == -1
