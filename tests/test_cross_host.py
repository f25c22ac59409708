"""Host side of the cross spectra (no GPU): cross_power_torch against the independent fp64 statement of tests/cross_reference.py, the
identities that pin the cross spectrum and the adjusted spectral MSE, coherence_scale, LossHandler's amse strings against the formula written
out in numpy, the strings that keep raising, the command line's refusals, and the bounds against three mutants of the reference."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from swin_v2_weather_amd.utils import sht
from tests import cross_reference as X
from tests import sht_reference as R

GRIDS = [(9, 16), (12, 9), (16, 32)]


def _fields(grid, planes=3, seed=0):
    rng = np.random.default_rng(seed + grid[0])
    a = rng.standard_normal((planes,) + grid).cumsum(-1) / 4 + rng.standard_normal((planes, 1, 1))
    return a, 0.5 * a + rng.standard_normal((planes,) + grid)


def _spectra_torch(a, b, grid):
    return torch.stack(sht.cross_power_torch(torch.tensor(a), torch.tensor(b), torch.tensor(sht.legendre_table(*grid)))).numpy()


def _close(got, want, scale, tol=1e-12):
    assert np.max(np.abs(got - want)) <= tol * np.max(np.abs(scale)), (np.max(np.abs(got - want)), np.max(np.abs(scale)))


@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: f"{g[0]}x{g[1]}")
def test_statement_against_the_independent_reference(grid):
    a, b = _fields(grid)
    T = R.legendre(*grid)
    g = np.random.default_rng(1).standard_normal((3, a.shape[0], grid[0]))
    S, _, gx, _, _ = X.end_to_end(a, b, T, g)
    at, bt = torch.tensor(a, requires_grad=True), torch.tensor(b, requires_grad=True)
    got = torch.stack(sht.cross_power_torch(at, bt, torch.tensor(sht.legendre_table(*grid))))
    for k in range(3):
        _close(got[k].detach().numpy(), S[k], S[:2])
    (got * torch.tensor(g)).sum().backward()                 # autograd through the statement is the adjoint the kernels are held to
    _close(at.grad.numpy(), gx[0], gx[0])
    _close(bt.grad.numpy(), gx[1], gx[1])
    # cross_power on tensors the kernels do not take is the statement
    for x, y in zip(sht.cross_power(torch.tensor(a), torch.tensor(b)), got):
        assert torch.equal(x, y.detach())
    with pytest.raises(ValueError):
        sht.cross_power(torch.tensor(a), torch.tensor(b)[:2])


@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: f"{g[0]}x{g[1]}")
def test_identities_of_the_cross_spectrum(grid):
    a, b = _fields(grid)
    Paa, Pbb, Cab = _spectra_torch(a, b, grid)
    _, _, Caa = _spectra_torch(a, a, grid)
    _close(Caa, Paa, Paa)                                    # C_aa = P_aa
    _close(_spectra_torch(b, a, grid)[2], Cab, Paa)          # C_ab = C_ba
    assert np.all(Cab ** 2 <= Paa * Pbb * (1 + 1e-12))       # Cauchy-Schwarz, degree by degree
    table = torch.tensor(sht.legendre_table(*grid))
    _close(Paa + Pbb - 2 * Cab, sht.degree_power_torch(torch.tensor(a - b), table).numpy(), Paa + Pbb)
    coh = sht.spectral_coherence(*(torch.tensor(v) for v in (Paa, Pbb, Cab)))
    assert coh.dtype == torch.float64 and np.allclose(coh.numpy(), X.coherence(np.stack([Paa, Pbb, Cab])), rtol=1e-12, atol=0, equal_nan=True)


def test_coherence_is_nan_without_power_and_is_not_clamped():
    P = torch.tensor([1.0, 0.0, 4.0, 1.0], dtype=torch.float32)
    Q = torch.tensor([1.0, 2.0, 0.0, 1.0], dtype=torch.float32)
    C = torch.tensor([0.5, 0.0, 0.0, 1.0000001], dtype=torch.float32)
    coh = sht.spectral_coherence(P, Q, C)
    assert coh.dtype == torch.float64 and coh[0] == 0.5 and torch.isnan(coh[1]) and torch.isnan(coh[2]) and coh[3] > 1.0


def test_coherence_scale_on_hand_made_vectors():
    nan = float("nan")
    cases = [([0.0, 0.9, 0.8, 0.5, 0.4, 0.9], 3),           # degree 0 is not looked at; 0.5 itself passes; a later rise does not count
             ([1.0, 0.4, 0.9, 0.9], 0),                      # degree 1 already fails
             ([1.0, 0.9, nan, 0.9], 1),                      # a NaN counts as failing
             ([1.0, nan, 0.9, 0.9], 0),
             ([1.0, 0.9, 0.9, 0.9], 3),                      # never falls through: the last degree
             ([nan, 0.6, 0.6, 0.2], 2)]
    for v, want in cases:
        assert int(sht.coherence_scale(torch.tensor(v, dtype=torch.float64))) == want, v
    both = sht.coherence_scale(torch.tensor([cases[0][0], cases[0][0]], dtype=torch.float64).reshape(1, 2, 6), level=0.85)
    assert both.shape == (1, 2) and both.dtype == torch.int64 and both.tolist() == [[1, 1]]


# ---- the adjusted spectral MSE ------------------------------------------------------------------------------------------------------
def _amse(a, b, grid, absolute=True):
    from swin_v2_weather_amd.utils.losses import GeometricAMSELoss
    return GeometricAMSELoss(grid, absolute=absolute)(torch.tensor(a)[None], torch.tensor(b)[None])[0].numpy()


@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: f"{g[0]}x{g[1]}")
def test_amse_identities(grid):
    a, b = _fields(grid)
    table = torch.tensor(sht.legendre_table(*grid))
    Pa = sht.degree_power_torch(torch.tensor(a), table).numpy()
    mse = sht.degree_power_torch(torch.tensor(a - b), table).numpy().sum(-1)          # the spectral MSE, sum_l P_x + P_y - 2 C
    tot = Pa.sum(-1)
    assert np.all(np.abs(_amse(a, a, grid)) <= 1e-12 * tot)                           # AMSE(x, x) = 0
    for s in (0.25, 1.0, 3.0):                                                        # AMSE(x, s x) = (1 - s)^2 sum P_x
        _close(_amse(a, s * a, grid), (1 - s) ** 2 * tot, tot * max(1.0, s * s))
    S = _spectra_torch(a, b, grid)
    _close(X.amse(S, True, geometric_mean=True), mse, mse)                            # max -> sqrt(P_x P_y): the spectral MSE itself
    got = _amse(a, b, grid)
    assert np.all(got >= mse * (1 - 1e-12)) and np.any(got > mse * 1.001)             # never below it; above it when the powers differ
    rolled = np.roll(a, 3, axis=-1)                                                   # a rotation in longitude: P_x = P_y degree by degree
    _close(_amse(a, rolled, grid), sht.degree_power_torch(torch.tensor(a - rolled), table).numpy().sum(-1), tot)
    # the class against the reference's formula and gradient, both forms
    for absolute in (True, False):
        _close(_amse(a, b, grid, absolute), X.amse(S, absolute), X.amse(S, absolute))
        St = torch.tensor(S, requires_grad=True)
        from swin_v2_weather_amd.utils.losses import amse_from_spectra
        amse_from_spectra(St[0], St[1], St[2], absolute).sum().backward()
        _close(St.grad.numpy(), X.amse_grad(S, absolute), X.amse_grad(S, absolute))


def test_amse_of_a_degree_without_power():
    """a degree with P_x P_y == 0 contributes P_x + P_y - 2 C, and its gradient is finite"""
    from swin_v2_weather_amd.utils.losses import amse_from_spectra
    Px = torch.tensor([[4.0, 0.0, 1.0, 0.0]], dtype=torch.float64, requires_grad=True)
    Py = torch.tensor([[1.0, 2.0, 0.0, 0.0]], dtype=torch.float64, requires_grad=True)
    C = torch.tensor([[2.0, 0.0, 0.0, 0.0]], dtype=torch.float64, requires_grad=True)
    v = amse_from_spectra(Px, Py, C, absolute=True)
    assert float(v.detach()) == (2.0 - 1.0) ** 2 + 2 * 4.0 * (1 - 2.0 / 2.0) + 2.0 + 1.0 + 0.0
    v.sum().backward()
    assert all(bool(torch.isfinite(t.grad).all()) for t in (Px, Py, C))
    assert Px.grad[0, 1:].tolist() == [1.0, 1.0, 1.0] and C.grad[0, 1:].tolist() == [-2.0, -2.0, -2.0]
    S = np.stack([t.detach().numpy() for t in (Px, Py, C)])
    assert np.allclose(X.amse(S, True), v.detach().numpy()) and np.allclose(X.amse_grad(S, True)[0], Px.grad.numpy())


NAMES = ["u10m", "t2m", "z500"]


def _handler(loss, n_future=0, grid=(9, 16)):
    from swin_v2_weather_amd.utils.losses import LossHandler
    return LossHandler(SimpleNamespace(n_future=n_future, img_shape_x=grid[0], img_shape_y=grid[1], loss=loss, channel_weights="auto",
                                       n_out_channels=len(NAMES), channel_names=NAMES, out_channels=np.arange(len(NAMES)), dt=6,
                                       model_grid_type="equiangular"))


AMSE_STRINGS = ["amse", "weighted amse", "absolute amse", "weighted absolute amse", "weighted relative temp-std amse",
                "weighted absolute temp-std squared amse", "geometric amse"]


@pytest.mark.parametrize("n_future", [0, 1], ids=["single", "multistep"])
@pytest.mark.parametrize("loss", AMSE_STRINGS)
def test_loss_handler_amse_strings_against_numpy(loss, n_future):
    from swin_v2_weather_amd.utils.losses import load_stats
    grid, C, B = (9, 16), len(NAMES), 2
    flags = loss.split()
    lh = _handler(loss, n_future, grid)
    steps = n_future + 1
    rng = np.random.default_rng(11)
    tar = rng.standard_normal((B, C * steps) + grid)
    prd = tar + 0.5 * rng.standard_normal(tar.shape)
    # the channel weights written out: auto weights, normalised; the temp-std factor; the multistep weight per step
    cw = np.array([0.1, 1.0, 0.5]) if "weighted" in flags else np.ones(C)
    cw = cw / cw.sum()
    if "temp-std" in flags:
        gs, td = load_stats(SimpleNamespace(channel_names=NAMES, out_channels=np.arange(C)))
        tvw = gs.reshape(-1)[:C] / (np.sqrt(6) * td.reshape(-1)[:C] + 1e-6)
        cw = cw * (tvw ** 2 if "squared" in flags else tvw)
    T = R.legendre(*grid)
    S, _ = X.end_to_end(prd.reshape((-1,) + grid), tar.reshape((-1,) + grid), T)
    value = X.amse(S, "absolute" in flags).reshape(B, C * steps)
    for training in (True, False):
        lh.train(training)
        if not training and steps > 1:
            continue                                         # eval scores one step's channels: the weights have C entries
        chw = np.tile(cw, steps) / steps if training else cw
        want = (chw[None, :] * value).sum()
        pt = torch.tensor(prd, requires_grad=True)
        got = lh(pt, torch.tensor(tar))
        assert abs(float(got.detach()) - want) <= 1e-6 * abs(want), (loss, training, float(got.detach()), want)          # (the weight buffers are fp32)
        got.backward()
        assert bool(torch.isfinite(pt.grad).all()) and float(pt.grad.abs().sum()) > 0
    with lh.fused_with(object(), torch.tensor(tar)):         # a no-op for this family, as for l1: nothing is looked up on the model
        assert lh._fused is None


def test_l2_and_l1_keep_their_priority_over_amse():
    assert _handler("amse l2").p == 2 and _handler("amse l2").amse is None
    assert _handler("amse l1").p == 1 and _handler("l1 amse l2").p == 2
    assert _handler("weighted amse").p is None


@pytest.mark.parametrize("s", ["pole-masked amse", "geometric h1", "absolute geometric h1", "huber", "mse"])
def test_strings_that_keep_raising(s):
    with pytest.raises(ValueError) as e:
        _handler(s)
    if "pole-masked" not in s:
        assert "l2 and l1 families only" in str(e.value)     # its present message


# ---- scoring and the command line ---------------------------------------------------------------------------------------------------
def test_scorers_and_rollout_scores():
    from swin_v2_weather_amd import inference
    from swin_v2_weather_amd.utils.weighted_acc_rmse import ForecastScorer, RegriddedScorer
    grid = (9, 16)
    a, b = _fields(grid, planes=4)
    sc = ForecastScorer(grid[0], grid[1], 2, "cpu")
    coh = sc.spectral_coherence(torch.tensor(a, dtype=torch.float32).reshape(2, 2, *grid), torch.tensor(b, dtype=torch.float32).reshape(2, 2, *grid))
    assert coh.shape == (2, 2, grid[0]) and coh.dtype == torch.float64
    S, _ = X.end_to_end(a.astype(np.float32).astype(np.float64), b.astype(np.float32).astype(np.float64), R.legendre(*grid))
    assert np.allclose(coh.numpy().reshape(4, -1), X.coherence(S), atol=1e-4, equal_nan=True)          # (fp32 statement on the CPU)
    with pytest.raises(ValueError):
        RegriddedScorer.spectral_coherence(object())
    assert len(inference.RolloutScores._fields) == 6 and inference.RolloutScores(1, 2, 3, 4, 5).coherence is None          # the tuple is unchanged
    rs = inference.RolloutScores(torch.ones(2, 2), None, None, None, None)
    rs.coherence = inference.RolloutCoherence(torch.zeros(2, 2, 9, dtype=torch.float64), torch.tensor([[[3, 4]], [[1, 2]]]), 0.5)
    lines = inference.lead_time_table(rs, [("u10m", 0), ("v10m", 1)]).splitlines()
    assert "lcoh_u10m" in lines[0] and "lcoh_v10m" in lines[0] and lines[1].split()[-2:] == ["3.00000", "4.00000"]


def test_cli_flags_and_refusals():
    from swin_v2_weather_amd import inference
    ap = inference.build_parser()
    a = ap.parse_args(["--registry", "r", "--truth", "t.npy", "--coherence", "--spectrum", "--spectrum-out", "s.npz"])
    assert a.coherence and a.spectrum
    assert not ap.parse_args(["--registry", "r", "--truth", "t.npy"]).coherence
    for bad in (["--coherence"],                                                                      # needs --truth
                ["--truth", "t.npy", "--coherence", "--score-grid", "1.5"],                           # not on a coarser grid
                ["--truth", "t.npy", "--coherence", "--ensemble", "4", "--perturbation", "0.1"]):     # a single forecast
        with pytest.raises(SystemExit):
            ap.parse_args(["--registry", "r"] + bad)


def test_abi_host_side():
    from swin_v2_weather_amd import _lib as L
    assert L.ABI_VERSION == 113                              # the entry points are additive
    lib = L.load()
    assert lib.swv2_version() == 113
    for pairs, lmax, mmax in ((1, 2, 3), (146, 720, 721), (5, 24, 9), (17, 19, 8), (3, 8, 17)):
        assert lib.swv2_sht_cross_ws_bytes(pairs, lmax, mmax) == -(-min(mmax, lmax) // L.SHT_MRUN) * 3 * pairs * lmax * 4
    for bad in ((0, 8, 8), (4, 0, 8), (4, 8, 0), (-1, 8, 8)):
        assert lib.swv2_sht_cross_ws_bytes(*bad) == 0
    # refused before any launch (no device is touched): null pointers, bad sizes, too many pairs, a short workspace, the 2^31 offset limit
    big = 1 << 40
    assert lib.swv2_sht_cross_power(None, None, None, None, 1, 8, 8, 5, None, 0, None) == -1
    assert lib.swv2_sht_cross_power(16, 16, 16, None, 0, 8, 8, 5, 16, big, None) == -1
    assert lib.swv2_sht_cross_power(16, 16, 16, None, 32768, 8, 8, 5, 16, big, None) == -1
    assert b"pairs" in lib.swv2_last_error()
    assert lib.swv2_sht_cross_power(16, 16, 16, None, 2, 8, 8, 5, 16, lib.swv2_sht_cross_ws_bytes(2, 8, 5) - 1, None) == -1
    assert b"workspace" in lib.swv2_last_error()
    assert lib.swv2_sht_cross_power(16, 16, 16, None, 32767, 32768, 32768, 5, 16, big, None) == -1          # 4 pairs * nlat >= 2^31
    assert lib.swv2_sht_cross_adjoint(16, None, 16, 16, 2, 8, 8, 5, None) == -1
    assert lib.swv2_sht_cross_adjoint(16, 16, 16, 16, 2, 8, -8, 5, None) == -1
    assert lib.swv2_sht_cross_adjoint(16, 16, 16, 16, 32768, 8, 8, 5, None) == -1


# ---- the bounds tell a wrong kernel from a right one ------------------------------------------------------------------------------------
def test_the_bounds_reject_the_three_mutants():
    """what the GPU test asserts -- |C - reference| <= its bound, |dX - reference| <= its bound -- fails for a statement without the
    factor 2 of m >= 1 in C, with re paired with im in C, or with g_ab doubled in the adjoint; and passes for the reference itself rounded
    to fp32"""
    for grid, pairs in (((16, 32), 2), ((19, 15), 3)):
        a, b = _fields(grid, planes=pairs)
        T = sht.legendre_table(*grid).astype(np.float32).astype(np.float64)
        Xop = R.operand(X.stack_pairs(a.astype(np.float32), b.astype(np.float32)), T.shape[0]).astype(np.float32).astype(np.float64)
        c, mag = R.coeffs(T, Xop)
        dc = R.coeff_bound(mag, grid[0])
        S, dS = X.spectra(c), X.spectra_bound(c, dc)
        assert np.all(np.abs(X.cross(c).astype(np.float32) - S[2]) <= dS[2])
        for mutant in (X.cross(c, drop_factor=True), X.cross(c, swap_parts=True)):
            assert np.any(np.abs(mutant - S[2]) > dS[2])
        g = np.random.default_rng(2).standard_normal((3, pairs, grid[0]))
        dX, ddX = X.adjoint(T, c, g), X.adjoint_bound(T, c, dc, g)
        assert np.all(np.abs(dX.astype(np.float32) - dX) <= ddX)
        assert np.any(np.abs(X.adjoint(T, c, g, double_gab=True) - dX) > ddX)
