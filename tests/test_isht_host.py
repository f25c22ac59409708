"""No GPU: the inverse transform of utils/sht.py against its definition in fp64 (recovery through the forward statement, the truncation
identity, what irfft ignores), the noise spectrum and its variance identity on the table, perturb_initial_condition's spherical kind on
the CPU, the command line, the host side of swv2_sht_synth, and the bounds of tests/isht_reference.py against three mutants."""
import math

import numpy as np
import pytest
import torch

from tests import isht_reference as IR
from tests import sht_reference as R
from tests.test_sht_host import GRIDS
from swin_v2_weather_amd.utils import sht

BIG = [g for g in GRIDS if g[0] >= 8]
BIG_IDS = [f"{a}x{b}" for a, b in BIG]


def _band_limited(nlat, nlon, planes, rng):
    """complex coefficients [planes, lmax, mmax], non-zero for l <= (nlat - 1) // 2, m <= min(l, (nlon - 1) // 2); real at m = 0"""
    L0, M0, mmax = (nlat - 1) // 2, (nlon - 1) // 2, nlon // 2 + 1
    c = np.zeros((planes, nlat, mmax), complex)
    for l in range(L0 + 1):
        for m in range(min(l, M0) + 1):
            c[:, l, m] = rng.standard_normal(planes) + (1j * rng.standard_normal(planes) if m else 0.0)
    return c


def _tables(nlat, nlon):
    return torch.from_numpy(sht.legendre_table(nlat, nlon)), sht.inverse_weights(nlat, "cpu", torch.float64)


def test_inverse_weights_are_the_reciprocals_rounded_once_and_cached():
    w = sht.clenshaw_curtis_weights(19)
    assert np.all(w > 0)
    assert np.array_equal(sht.inverse_weights(19, "cpu", torch.float64).numpy(), 1.0 / w)
    assert np.array_equal(sht.inverse_weights(19, "cpu").numpy(), (1.0 / w).astype(np.float32))
    assert sht.inverse_weights(19, "cpu") is sht.inverse_weights(19, "cpu")


@pytest.mark.parametrize("grid", BIG, ids=BIG_IDS)
def test_the_statement_inverse_recovers_band_limited_coefficients(grid):
    nlat, nlon = grid
    c = _band_limited(nlat, nlon, 2, np.random.default_rng(nlat + nlon))
    T, rw = _tables(nlat, nlon)
    x = sht.inverse_real_sht_torch(torch.from_numpy(c), T, rw, nlon)
    assert x.shape == (2, nlat, nlon) and x.dtype == torch.float64
    got = sht.real_sht_torch(x, T).numpy()
    exact = np.arange(nlat) + (nlat - 1) // 2 <= nlat - 1          # the degrees the rule resolves against a field of degree (nlat - 1) // 2
    assert np.abs(got - c)[:, exact].max() < 1e-12
    # the same field from the independent statement of the synthesis (layouts of the kernels)
    cl = np.stack([c.real, c.imag], axis=2).transpose(3, 0, 2, 1).reshape(c.shape[2], 4, nlat)
    ref = IR.field(IR.synth(R.legendre(nlat, nlon), 1.0 / R.weights(nlat), cl, None, (1.0, 1.0), nlon), nlon)
    assert np.abs(ref - x.numpy()).max() < 1e-11
    assert torch.equal(sht.inverse_real_sht(torch.from_numpy(c), nlon), x)          # on the CPU the public function is the statement


@pytest.mark.parametrize("grid", BIG, ids=BIG_IDS)
def test_truncation_at_half_the_rows_is_the_identity_on_band_limited_fields(grid):
    nlat, nlon = grid
    c = _band_limited(nlat, nlon, 3, np.random.default_rng(7 * nlat + nlon))
    T, rw = _tables(nlat, nlon)
    x = sht.inverse_real_sht_torch(torch.from_numpy(c), T, rw, nlon)
    y = sht.spectral_truncate(x, (nlat - 1) // 2)
    err = float((y - x).abs().max())
    print(f"{grid}: spectral_truncate identity error {err:.2e}")
    assert err < 1e-11
    assert torch.equal(y, sht.spectral_filter(x, (torch.arange(nlat) <= (nlat - 1) // 2).double()))
    # a response per plane is applied plane by plane
    h = torch.from_numpy(np.random.default_rng(1).random((3, nlat)))
    per = sht.spectral_filter(x, h)
    for p in range(3):
        assert torch.allclose(per[p], sht.spectral_filter(x[p], h[p]), rtol=0, atol=1e-12)
    with pytest.raises(ValueError):
        sht.spectral_filter(x, h[:2])


def test_the_identity_response_is_not_the_identity_map():
    """what the module's docstring says of lmax = nlat: degrees above nlat - 1 - L alias"""
    nlat, nlon = 16, 32
    x = torch.from_numpy(np.random.default_rng(0).standard_normal((nlat, nlon)))
    assert float((sht.spectral_filter(x, torch.ones(nlat, dtype=torch.float64)) - x).abs().max()) > 1e-3


@pytest.mark.parametrize("nlon", [16, 15])
def test_imaginary_parts_at_m0_and_nyquist_are_ignored(nlon):
    nlat = 9
    rng = np.random.default_rng(nlon)
    c = _band_limited(nlat, nlon, 1, rng)
    mmax = c.shape[-1]
    c[:, 3:, mmax - 1] = rng.standard_normal(nlat - 3)          # something real at the last order (the Nyquist one for nlon = 16)
    dirty = c.copy()
    dirty[:, :, 0] += 1j * rng.standard_normal(nlat)
    if nlon % 2 == 0:
        dirty[:, :, nlon // 2] += 1j * rng.standard_normal(nlat)
    T, rw = _tables(nlat, nlon)
    a, b = (sht.inverse_real_sht_torch(torch.from_numpy(v), T, rw, nlon) for v in (c, dirty))
    assert float((a - b).abs().max()) < 1e-13
    z = rng.standard_normal((mmax, 2, nlat))
    sig = torch.from_numpy(sht.gaussian_noise_spectrum(nlat, nlon, 3000.0))
    zz = z.copy()
    zz[0, 1] = np.nan
    if nlon % 2 == 0:
        zz[nlon // 2, 1] = np.nan
    zz[~R.tri(mmax, nlat)[:, None, :].repeat(2, 1)] = np.nan     # and nothing below the diagonal is used
    a, b = (sht.spherical_noise_torch(torch.from_numpy(v), sig, T, rw, nlon) for v in (z, zz))
    assert bool(torch.isfinite(b).all()) and torch.equal(a, b)


@pytest.mark.parametrize("grid", GRIDS, ids=[f"{a}x{b}" for a, b in GRIDS])
def test_noise_spectrum_normalisation_and_support(grid):
    nlat, nlon = grid
    l = np.arange(nlat)
    top = min(nlat - 1, (nlon - 1) // 2)
    for zero_mean in (True, False):
        if zero_mean and top < 1:
            with pytest.raises(ValueError):
                sht.gaussian_noise_spectrum(nlat, nlon, 1000.0)
            continue
        for km in (200.0, 1500.0, 20000.0):
            s = sht.gaussian_noise_spectrum(nlat, nlon, km, zero_mean=zero_mean)
            assert s.dtype == np.float64 and s.shape == (nlat,)
            assert abs(np.sum(s * s * (2 * l + 1)) / (4 * math.pi) - 1.0) < 1e-12
            lo = 1 if zero_mean else 0
            assert np.all(s[:lo] == 0) and np.all(s[top + 1:] == 0) and np.all(s >= 0)
            if km > 10000.0:                                     # (three Earth radii: the tail underflows in fp64, nothing more to compare)
                continue
            assert np.all(s[lo:top + 1] > 0)
            r = s[lo + 1:top + 1] ** 2 / s[lo:top] ** 2              # the Gaussian shape: sigma_l^2 / sigma_{l-1}^2 = exp(-l (length / a)^2)
            assert np.allclose(r, np.exp(-l[lo + 1:top + 1] * (km / 6371.0) ** 2), rtol=1e-10, atol=0)
    with pytest.raises(ValueError):
        sht.gaussian_noise_spectrum(nlat, nlon, 0.0)


def test_sigma_beyond_the_orders_the_longitudes_carry_is_refused():
    nlat, nlon = 24, 16
    z = torch.zeros(nlon // 2 + 1, 2, nlat)
    s = np.zeros(nlat)
    s[(nlon - 1) // 2] = 1.0
    assert sht.spherical_noise(z, s, nlon).shape == (1, nlat, nlon)
    s[(nlon - 1) // 2 + 1] = 1e-30
    with pytest.raises(ValueError):
        sht.spherical_noise(z, s, nlon)
    with pytest.raises(ValueError):
        sht.spherical_noise(z, np.zeros(nlat - 1), nlon)
    with pytest.raises(ValueError):
        sht.spherical_noise(torch.zeros(nlon // 2, 2, nlat), np.zeros(nlat), nlon)


@pytest.mark.parametrize("grid", BIG, ids=BIG_IDS)
def test_variance_identity_on_the_table(grid):
    """the addition theorem as spherical_noise uses it: with f_0 = 1, f_m = sqrt(1/2) and the irfft's weights (1 at m = 0, a cosine and a
    sine of amplitude 2 each at m >= 1, so 4 f_m^2 = 2), sum_m f_m^2 v_m Pbar_l^m(theta_k)^2 = (2 l + 1) / (4 pi) at every row k"""
    nlat, nlon = grid
    P = sht.legendre_table(nlat, nlon) / sht.clenshaw_curtis_weights(nlat)
    top = min(nlat - 1, (nlon - 1) // 2)
    v = np.full(P.shape[0], 0.5 * 4.0)
    v[0] = 1.0
    for l in range(top + 1):
        var = np.einsum("m,mk->k", v[:l + 1], P[:l + 1, l] ** 2)
        assert np.abs(var - (2 * l + 1) / (4 * math.pi)).max() < 1e-12 * (2 * l + 1), l
    # and so the statement's field has the variance  sum_l sigma_l^2 (2 l + 1) / (4 pi) = 1  at every point: its covariance diagonal, exactly
    sig = sht.gaussian_noise_spectrum(nlat, nlon, 2500.0)
    var = np.einsum("l,m,mlk->k", sig ** 2, v, P ** 2 * R.tri(P.shape[0], nlat)[:, :, None])
    assert np.abs(var - 1.0).max() < 1e-12


def test_spherical_noise_statement_is_the_reference_synthesis():
    nlat, nlon, planes = 19, 15, 3
    rng = np.random.default_rng(4)
    z = rng.standard_normal((nlon // 2 + 1, 2 * planes, nlat))
    sig = sht.gaussian_noise_spectrum(nlat, nlon, 4000.0)
    T, rw = _tables(nlat, nlon)
    got = sht.spherical_noise_torch(torch.from_numpy(z), torch.from_numpy(sig), T, rw, nlon).numpy()
    ref = IR.from_coefficients(R.legendre(nlat, nlon), 1.0 / R.weights(nlat), z, sig, (1.0, math.sqrt(0.5)), nlon)[0]
    assert got.shape == (planes, nlat, nlon) and np.abs(got - ref).max() < 1e-12
    assert torch.equal(sht.spherical_noise(torch.from_numpy(z), sig, nlon), torch.from_numpy(got))


def test_perturb_default_is_the_inline_formula_bit_for_bit():
    from swin_v2_weather_amd import inference
    B, Cin, H, W, M, nf, amp, seed = 2, 6, 8, 16, 3, 4, 0.25, 17
    x0 = torch.randn(B, Cin, H, W, generator=torch.Generator().manual_seed(1))
    want = x0.repeat(M, 1, 1, 1)
    want[B:, :nf] += amp * torch.randn((M - 1) * B, nf, H, W, generator=torch.Generator().manual_seed(seed))
    assert torch.equal(inference.perturb_initial_condition(x0, M, amp, seed, nf), want)
    assert torch.equal(inference.perturb_initial_condition(x0, M, amp, seed, nf, "white", None), want)          # the new keywords go last
    for kw in (dict(kind="white", length_scale_km=500.0), dict(kind="spherical"), dict(kind="red", length_scale_km=500.0)):
        with pytest.raises(ValueError):
            inference.perturb_initial_condition(x0, M, amp, seed, nf, **kw)


def test_perturb_spherical_follows_the_draw_rule_on_the_cpu():
    from swin_v2_weather_amd import inference
    B, Cin, H, W, M, nf, amp, seed, km = 2, 6, 16, 32, 3, 4, 0.25, 17, 3000.0
    x0 = torch.randn(B, Cin, H, W, generator=torch.Generator().manual_seed(1))
    y = inference.perturb_initial_condition(x0, M, amp, seed, nf, kind="spherical", length_scale_km=km)
    assert y.shape == (M * B, Cin, H, W)
    assert torch.equal(y[:B], x0) and torch.equal(y[:, nf:], x0.repeat(M, 1, 1, 1)[:, nf:])
    gen = torch.Generator().manual_seed(seed)
    sigma = sht.gaussian_noise_spectrum(H, W, km)
    wq = torch.from_numpy(sht.clenshaw_curtis_weights(H))
    for r in range((M - 1) * B):                                  # one row at a time, ascending, from the one generator
        z = torch.randn(W // 2 + 1, 2 * nf, H, generator=gen)
        noise = sht.spherical_noise(z, sigma, W)
        assert torch.equal(y[B + r, :nf], x0[r % B, :nf] + amp * noise)
        # zero global mean: the quadrature of the field is its l = 0 coefficient, which the spectrum leaves out (fp32 arithmetic: the sum of
        # H W terms of size ~1 errs by far less than 1e-4)
        mean = (noise.double().mean(-1) * wq).sum(-1) / 2.0
        assert float(mean.abs().max()) < 1e-5
        assert 0.2 < float(noise.std()) < 2.0
    assert torch.equal(y, inference.perturb_initial_condition(x0, M, amp, seed, nf, kind="spherical", length_scale_km=km))
    assert not torch.equal(y, inference.perturb_initial_condition(x0, M, amp, seed + 1, nf, kind="spherical", length_scale_km=km))
    assert torch.equal(inference.perturb_initial_condition(x0, 1, amp, seed, nf, kind="spherical", length_scale_km=km), x0)
    # neighbouring points are correlated, unlike white noise: the lag-one correlation along a row near the equator
    d = (y[B:, :nf] - x0.repeat(M - 1, 1, 1, 1)[:, :nf])[:, :, H // 2]
    assert float((d * d.roll(1, -1)).mean() / (d * d).mean()) > 0.5


def test_cli_flag_and_refusals():
    from swin_v2_weather_amd import inference
    ap = inference.build_parser()
    base = ["--registry", "r", "--truth", "t.npy", "--ensemble", "4", "--perturbation", "0.1"]
    assert ap.parse_args(base).perturbation_scale is None
    assert ap.parse_args(base + ["--perturbation-scale", "750"]).perturbation_scale == 750.0
    for bad in (["--registry", "r", "--perturbation-scale", "750"], ["--registry", "r", "--truth", "t.npy", "--perturbation-scale", "750"],
                base + ["--perturbation-scale", "0"], base + ["--perturbation-scale", "-3"]):
        with pytest.raises(SystemExit):
            ap.parse_args(bad)
    import inspect
    sig = inspect.signature(inference.ensemble_rollout).parameters
    assert sig["perturbation_kind"].default == "white" and sig["length_scale_km"].default is None
    assert list(inspect.signature(inference.perturb_initial_condition).parameters)[-2:] == ["kind", "length_scale_km"]


def test_abi_host_side_of_the_synthesis():
    from swin_v2_weather_amd import _lib as L
    assert L.ABI_VERSION == 113                                   # additive: the number stayed (113 is swv2_loss_sums)
    lib = L.load()
    ok = dict(table=16, rw=16, c=16, h=None, hs=0, f0=1.0, fm=1.0, S=16, planes=2, nlat=8, lmax=8, mmax=5, nlon=8)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.swv2_sht_synth(a["table"], a["rw"], a["c"], a["h"], a["hs"], a["f0"], a["fm"], a["S"], a["planes"], a["nlat"], a["lmax"],
                                  a["mmax"], a["nlon"], None)

    # refused before any launch (no device is touched)
    for bad in (dict(table=None), dict(rw=None), dict(c=None), dict(S=None), dict(planes=0), dict(nlat=-8), dict(lmax=0), dict(mmax=0),
                dict(planes=(1 << 20) + 1), dict(nlat=(1 << 15) + 1), dict(mmax=65536), dict(hs=1), dict(hs=7), dict(h=16, hs=-8), dict(nlon=0),
                dict(nlon=-4)):
        assert call(**bad) == -1, bad
        assert b"sht_synth" in lib.swv2_last_error(), bad


def test_ops_wrapper_refuses_cpu_tensors_and_wrong_shapes():
    from swin_v2_weather_amd import _lib as L, ops
    t, rw, c = torch.zeros(5, 8, 8), torch.ones(8), torch.zeros(5, 4, 8)
    with pytest.raises(L.Swv2Error):
        ops.sht_synth(t, rw, c, nlon=8)


def test_the_bounds_reject_the_three_mutants():
    """what the GPU test asserts -- |S - reference| <= dS element by element, |field - reference| <= its bound -- fails for a synthesis
    without the sqrt(1/2), without 1 / w_k, or without the row l = m"""
    nlat, nlon, planes = 16, 32, 3
    rng = np.random.default_rng(11)
    T = sht.legendre_table(nlat, nlon).astype(np.float32).astype(np.float64)
    rw = (1.0 / sht.clenshaw_curtis_weights(nlat)).astype(np.float32).astype(np.float64)
    z = rng.standard_normal((nlon // 2 + 1, 2 * planes, nlat)).astype(np.float32).astype(np.float64)
    sig = sht.gaussian_noise_spectrum(nlat, nlon, 2000.0).astype(np.float32).astype(np.float64)
    sc = (1.0, float(np.float32(math.sqrt(0.5))))
    x, dx, S, dS = IR.from_coefficients(T, rw, z, sig, sc, nlon)
    assert np.all(np.isfinite(dS)) and dx.max() < 1e-4 * np.abs(x).max()
    mutants = [IR.synth(T, rw, z, sig, (1.0, 1.0), nlon), IR.synth(T, rw, z, sig, sc, nlon, drop_rw=True),
               IR.synth(T, rw, z, sig, sc, nlon, drop_diagonal=True)]
    for mu in mutants:
        assert np.any(np.abs(mu - S) > dS)
        assert np.any(np.abs(IR.field(mu, nlon) - x) > dx)
    # and the exact rows: zeros with a zero bound
    assert np.all(S[0, 1::2] == 0) and np.all(dS[0, 1::2] == 0) and np.all(S[nlon // 2, 1::2] == 0) and np.all(dS[nlon // 2, 1::2] == 0)
