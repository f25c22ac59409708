"""GPU (-m gpu): swv2_sht_synth through the C ABI, judged element by element against the fp64 statement of tests/isht_reference.py from
the library's own fp32 table, inverse weights, coefficients and response (every bound is derived there), then the Python layer on top:
real_sht, inverse_real_sht, spectral_filter, spherical_noise, perturb_initial_condition(kind="spherical") and ensemble_rollout."""
import functools
import math

import numpy as np
import pytest
import torch

from tests import isht_reference as IR
from tests import sht_reference as R
from tests.plane_harness import SENTINEL, Guarded, dev, lib  # noqa: F401  (dev, lib: fixtures)
from tests.test_sht_gpu import IDS, SHAPES, _case, worst

pytestmark = pytest.mark.gpu

SQRT_HALF = float(np.float32(math.sqrt(0.5)))          # the scale as the kernel receives it
SCALES = [(1.0, 1.0), (1.0, SQRT_HALF)]
MODES = ["null", "shared", "per_plane"]


@functools.lru_cache(maxsize=None)
def _inputs(nlat, nlon, planes):
    """one shape's inputs, computed once: the fp32 table and inverse weights as the library rounds them, fp32 coefficients in the kernels'
    layout with NaN wherever the synthesis must not look (below the diagonal, the imaginary rows of m = 0 and nlon / 2), a response per plane"""
    from swin_v2_weather_amd.utils import sht
    rng = np.random.default_rng(5 * nlat + 3 * nlon + planes)
    T32 = sht.legendre_table(nlat, nlon).astype(np.float32)
    rw32 = (1.0 / sht.clenshaw_curtis_weights(nlat)).astype(np.float32)
    mmax, lmax = T32.shape[0], nlat
    c = (rng.standard_normal((mmax, 2 * planes, lmax)) / (1.0 + np.arange(lmax))).astype(np.float32)          # a red spectrum
    use = R.tri(mmax, lmax)[:, None, :] & IR.real_rows(mmax, 2 * planes, nlon)[:, :, None]
    c[~use] = np.nan
    h = ((0.25 + rng.random((planes, lmax))) * np.where(rng.random((planes, lmax)) < 0.3, -1, 1)).astype(np.float32)
    h[:, lmax // 2] = 0.0                                      # a degree that is filtered out altogether
    for v in (T32, rw32, c, h):
        v.setflags(write=False)
    return T32, rw32, c, h


@functools.lru_cache(maxsize=None)
def _reference(nlat, nlon, planes, mode, scales):
    T32, rw32, c, h = _inputs(nlat, nlon, planes)
    hh = {"null": None, "shared": h[0], "per_plane": h}[mode]
    T, rw, c64 = T32.astype(np.float64), rw32.astype(np.float64), c.astype(np.float64)
    S = IR.synth(T, rw, c64, hh, scales, nlon)
    dS = IR.synth_bound(T, rw, c64, np.zeros_like(c64), hh, scales, nlon, S)
    S.setflags(write=False), dS.setflags(write=False)
    return hh, S, dS


def _synth(lib, dev, T32, rw32, c, hh, scales, planes, nlon):
    from swin_v2_weather_amd import _lib as L
    mmax, lmax, nlat = T32.shape
    T, rw, cd = (torch.tensor(a).to(dev) for a in (T32, rw32, c))
    hd = None if hh is None else torch.tensor(hh).to(dev)
    G = Guarded(dev, S=mmax * 2 * planes * nlat)
    L.check(lib.swv2_sht_synth(T.data_ptr(), rw.data_ptr(), cd.data_ptr(), None if hd is None else hd.data_ptr(),
                               0 if hh is None or hh.ndim == 1 else lmax, scales[0], scales[1], G["S"].data_ptr(), planes, nlat, lmax, mmax, nlon,
                               torch.cuda.current_stream().cuda_stream), "swv2_sht_synth")
    torch.cuda.synchronize()
    return G


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_synthesis_element_by_element_against_fp64(dev, lib, shape, mode):
    nlat, nlon, planes = shape
    T32, rw32, c, _ = _inputs(*shape)
    mmax = T32.shape[0]
    for scales in SCALES:
        hh, S, dS = _reference(nlat, nlon, planes, mode, scales)
        G = _synth(lib, dev, T32, rw32, c, hh, scales, planes, nlon)
        assert G.guards_intact(), "the kernel wrote outside its output"
        assert G.written("S"), "output slots left unwritten"
        got = G["S"].cpu().numpy().reshape(mmax, 2 * planes, nlat)
        assert np.all(np.isfinite(got)), "a coefficient that must not be read was read"
        assert np.all(got[0, 1::2] == 0) and np.all(got[nlat:] == 0)                 # imaginary rows of m = 0; m >= lmax
        if nlon % 2 == 0:
            assert np.all(got[nlon // 2, 1::2] == 0)
        r = worst(np.abs(got.astype(np.float64) - S), dS)                             # (asserts exact zeros wherever the bound is zero)
        print(f"{shape} {mode} scales {scales}: worst error / bound  S {r:.3f}")
        assert r <= 1.0
        G2 = _synth(lib, dev, T32, rw32, c, hh, scales, planes, nlon)
        assert torch.equal(G2.ints("S"), G.ints("S")), "two runs differ"


# ---- the Python layer ---------------------------------------------------------------------------------------------------------------
def _layout(c):
    """complex [planes, lmax, mmax] -> the kernels' layout [mmax, 2 planes, lmax] (fp64)"""
    planes, lmax, mmax = c.shape
    return np.stack([c.real, c.imag], axis=1).transpose(3, 0, 1, 2).reshape(mmax, 2 * planes, lmax).astype(np.float64)


def _tables64(nlat, nlon):
    T32, rw32, _, _ = _inputs(nlat, nlon, 1)
    return T32.astype(np.float64), rw32.astype(np.float64)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_real_sht_against_fp64_with_zeros_below_the_diagonal(dev, lib, shape):
    from swin_v2_weather_amd.utils import sht
    nlat, nlon, planes = shape
    _, x, _, _, _ = _case(*shape)
    T, _ = _tables64(nlat, nlon)
    c, dc = IR.analysis(x.astype(np.float64), T)
    got = sht.real_sht(torch.tensor(x).to(dev))
    assert got.shape == (planes, nlat, nlon // 2 + 1) and got.dtype == torch.complex64
    gl = _layout(got.cpu().numpy())
    tri = np.broadcast_to(R.tri(T.shape[0], nlat)[:, None, :], gl.shape)
    assert np.all(gl[~tri] == 0), "real_sht returns zeros for l < m"
    r = worst(np.abs(gl - c)[tri], dc[tri])
    print(f"{shape}: worst error / bound  real_sht {r:.3f}")
    assert r <= 1.0


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_inverse_real_sht_against_fp64(dev, lib, shape):
    """from given coefficients (dc = 0); what lies below the diagonal and the imaginary parts irfft ignores are NaN in the input"""
    from swin_v2_weather_amd.utils import sht
    nlat, nlon, planes = shape
    _, _, c, _ = _inputs(*shape)
    T, rw = _tables64(nlat, nlon)
    want, bound, _, _ = IR.from_coefficients(T, rw, c.astype(np.float64), None, (1.0, 1.0), nlon)
    cc = c.reshape(c.shape[0], planes, 2, nlat)
    cd = torch.complex(torch.tensor(cc[:, :, 0]), torch.tensor(cc[:, :, 1])).permute(1, 2, 0).contiguous().to(dev)
    got = sht.inverse_real_sht(cd, nlon)
    assert got.shape == (planes, nlat, nlon) and got.dtype == torch.float32
    r = worst(np.abs(got.cpu().numpy().astype(np.float64) - want), np.broadcast_to(bound, want.shape))
    print(f"{shape}: worst error / bound  inverse_real_sht {r:.3f}")
    assert r <= 1.0
    with pytest.raises(ValueError):
        sht.inverse_real_sht(cd, nlon + 2)


@pytest.mark.parametrize("per_plane", [False, True], ids=["shared", "per_plane"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_spectral_filter_against_the_end_to_end_bound(dev, lib, shape, per_plane):
    from swin_v2_weather_amd.utils import sht
    nlat, nlon, planes = shape
    _, x, _, _, _ = _case(*shape)
    _, _, _, h = _inputs(*shape)
    hh = h if per_plane else h[0]
    T, rw = _tables64(nlat, nlon)
    want, bound = IR.filter_end_to_end(x.astype(np.float64), T, rw, hh.astype(np.float64))
    xd = torch.tensor(x).to(dev)
    got = sht.spectral_filter(xd, torch.tensor(hh).to(dev))
    assert got.shape == xd.shape and got.dtype == torch.float32
    r = worst(np.abs(got.cpu().numpy().astype(np.float64) - want), np.broadcast_to(bound, want.shape))
    print(f"{shape} per_plane={per_plane}: worst error / bound  spectral_filter {r:.3f}")
    assert r <= 1.0
    if not per_plane:
        # the truncation is the response 1[l <= lcut]; the statement on the same device with the same fp32 tables obeys the same bound
        lcut = (nlat - 1) // 2
        step = (np.arange(nlat) <= lcut).astype(np.float64)
        tw, tb = IR.filter_end_to_end(x.astype(np.float64), T, rw, step)
        assert worst(np.abs(sht.spectral_truncate(xd, lcut).cpu().numpy().astype(np.float64) - tw), np.broadcast_to(tb, tw.shape)) <= 1.0
        st = sht.spectral_filter_torch(xd, torch.tensor(hh).to(dev), sht.device_table(nlat, nlon, dev), sht.inverse_weights(nlat, dev))
        assert worst(np.abs(st.cpu().numpy().astype(np.float64) - want), np.broadcast_to(bound, want.shape)) <= 1.0


def test_filter_of_a_channel_block_view_with_a_response_per_plane(dev, lib):
    from swin_v2_weather_amd.utils import sht
    nlat, nlon, planes = 16, 32, 4
    _, x, _, _, _ = _case(nlat, nlon, planes)
    _, _, _, h = _inputs(nlat, nlon, planes)
    T, rw = _tables64(nlat, nlon)
    want, bound = IR.filter_end_to_end(x.astype(np.float64), T, rw, h.astype(np.float64))
    wide = torch.full((2, 7, nlat, nlon), float("nan"), device=dev)
    wide[:, 3:5] = torch.tensor(x).to(dev).reshape(2, 2, nlat, nlon)
    view = wide[:, 3:5]
    assert sht.on_kernels(view) and not view.is_contiguous()
    got = sht.spectral_filter(view, torch.tensor(h).to(dev).reshape(2, 2, nlat))
    assert got.shape == (2, 2, nlat, nlon)
    assert worst(np.abs(got.cpu().numpy().astype(np.float64).reshape(want.shape) - want), np.broadcast_to(bound, want.shape)) <= 1.0
    c = sht.real_sht(view)
    assert c.shape == (2, 2, nlat, nlon // 2 + 1) and torch.equal(c.reshape(4, nlat, -1), sht.real_sht(torch.tensor(x).to(dev)))


def test_fp64_requires_grad_and_strided_inputs_take_the_statement(dev, lib, monkeypatch):
    from swin_v2_weather_amd import ops
    from swin_v2_weather_amd.utils import sht
    nlat, nlon, planes = 16, 32, 4
    _, x, _, _, _ = _case(nlat, nlon, planes)
    _, _, _, h = _inputs(nlat, nlon, planes)
    xd, hd = torch.tensor(x).to(dev), torch.tensor(h[0]).to(dev)
    on_kernels = sht.spectral_filter(xd, hd)

    def refuse(*a, **k):
        raise AssertionError("the kernel path was taken")

    for name in ("sht_synth", "sht_power", "sht_repack"):
        monkeypatch.setattr(ops, name, refuse)
    with pytest.raises(AssertionError):
        sht.spectral_filter(xd, hd)                              # (the patch bites: this input does go to the kernels)
    y64 = sht.spectral_filter(xd.double(), hd.double())
    assert y64.dtype == torch.float64 and torch.allclose(y64.float(), on_kernels, rtol=0, atol=1e-4 * float(on_kernels.abs().max()))
    xg = xd.clone().requires_grad_(True)
    yg = sht.spectral_filter(xg, hd)
    yg.square().sum().backward()
    assert xg.grad is not None and bool(torch.isfinite(xg.grad).all())
    with torch.no_grad():
        assert sht.on_kernels(xg) and sht._kernel_field(xg)      # without a gradient to serve the same tensor is the kernels'
    strided = torch.tensor(x).to(dev).transpose(-1, -2).contiguous().transpose(-1, -2)
    assert not sht.on_kernels(strided)
    assert torch.allclose(sht.spectral_filter(strided, hd), on_kernels, rtol=0, atol=1e-4 * float(on_kernels.abs().max()))
    assert sht.real_sht(xd.double()).dtype == torch.complex128
    cg = sht.real_sht(xg)
    assert cg.requires_grad
    assert sht.inverse_real_sht(cg, nlon).requires_grad and sht.inverse_real_sht(cg.detach().to(torch.complex128), nlon).dtype == torch.float64
    zg = torch.randn(nlon // 2 + 1, 2, nlat, device=dev, dtype=torch.float64)
    assert sht.spherical_noise(zg, sht.gaussian_noise_spectrum(nlat, nlon, 2000.0), nlon).dtype == torch.float64


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_spherical_noise_against_the_fp64_statement_from_the_same_normals(dev, lib, shape):
    """the reference takes what the kernel takes: the same z, sigma rounded to fp32, sqrt(1/2) rounded to fp32"""
    from swin_v2_weather_amd.utils import sht
    nlat, nlon, planes = shape
    T, rw = _tables64(nlat, nlon)
    z = torch.randn(nlon // 2 + 1, 2 * planes, nlat, device=dev, generator=torch.Generator(device=dev).manual_seed(nlat + planes))
    sigma = sht.gaussian_noise_spectrum(nlat, nlon, 1500.0)
    want, bound, _, _ = IR.from_coefficients(T, rw, z.cpu().numpy().astype(np.float64), sigma.astype(np.float32).astype(np.float64),
                                             (1.0, SQRT_HALF), nlon)
    got = sht.spherical_noise(z, sigma, nlon)
    assert got.shape == (planes, nlat, nlon) and got.dtype == torch.float32
    r = worst(np.abs(got.cpu().numpy().astype(np.float64) - want), np.broadcast_to(bound, want.shape))
    print(f"{shape}: worst error / bound  spherical_noise {r:.3f}")
    assert r <= 1.0
    assert torch.equal(got, sht.spherical_noise(z, sigma, nlon))
    dirty = z.clone()                                            # entries the draw does not use
    dirty[0, 1::2] = float("nan")
    dirty[torch.tensor(~R.tri(z.shape[0], nlat), device=dev)[:, None, :].expand_as(z)] = float("nan")
    assert torch.equal(got, sht.spherical_noise(dirty, sigma, nlon))


def test_perturb_spherical_on_the_device(dev, lib):
    from swin_v2_weather_amd import inference
    from swin_v2_weather_amd.utils import sht
    B, Cin, H, W, M, nf, amp, seed, km = 2, 6, 16, 32, 3, 4, 0.25, 17, 3000.0
    x0 = torch.randn(B, Cin, H, W, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    y = inference.perturb_initial_condition(x0, M, amp, seed, nf, kind="spherical", length_scale_km=km)
    assert y.shape == (M * B, Cin, H, W)
    assert torch.equal(y[:B], x0) and torch.equal(y[:, nf:], x0.repeat(M, 1, 1, 1)[:, nf:])          # control and invariants: bit-identical
    assert torch.equal(y, inference.perturb_initial_condition(x0, M, amp, seed, nf, kind="spherical", length_scale_km=km))
    assert not torch.equal(y, inference.perturb_initial_condition(x0, M, amp, seed + 1, nf, kind="spherical", length_scale_km=km))
    gen = torch.Generator(device=dev).manual_seed(seed)
    sigma = sht.gaussian_noise_spectrum(H, W, km)
    for r in range((M - 1) * B):                                 # the stated draw rule, row by row from the one generator
        z = torch.randn(W // 2 + 1, 2 * nf, H, generator=gen, device=dev)
        assert torch.equal(y[B + r, :nf], x0[r % B, :nf] + amp * sht.spherical_noise(z, sigma, W))
    white = inference.perturb_initial_condition(x0, M, amp, seed, nf)
    assert torch.equal(white[B:, :nf], x0.repeat(M - 1, 1, 1, 1)[:, :nf] +
                       amp * torch.randn((M - 1) * B, nf, H, W, generator=torch.Generator(device=dev).manual_seed(seed), device=dev))


def test_two_step_ensemble_rollout_with_spherical_perturbations_is_rollout_of_the_perturbed_batch(dev, lib, tmp_path):
    from swin_v2_weather_amd import inference
    from swin_v2_weather_amd.utils.weighted_acc_rmse import ForecastScorer
    from tests.test_ensemble_gpu import _registry_model
    model = _registry_model(dev, tmp_path)
    M, B, Cout, H, W, steps, amp, seed, km = 3, 2, 5, 48, 72, 2, 0.05, 11, 2500.0
    g = torch.Generator(device=dev).manual_seed(3)
    x0 = torch.randn(B, 9, H, W, device=dev, generator=g)
    cz = torch.rand(B, steps - 1, H, W, device=dev, generator=g) * 2 - 1
    truth = torch.randn(B, steps, Cout, H, W, device=dev, generator=g)
    scorer = ForecastScorer(H, W, Cout, dev)
    xe = inference.perturb_initial_condition(x0, M, amp, seed, 5, kind="spherical", length_scale_km=km)
    assert torch.equal(xe[:B], x0) and torch.equal(xe[B:, 5:], x0.repeat(M - 1, 1, 1, 1)[:, 5:]) and not torch.equal(xe[B:, :5], x0.repeat(M - 1, 1, 1, 1)[:, :5])
    y = inference.rollout(model, xe, steps, cz.repeat(M, 1, 1, 1), n_invar=3)
    kept = inference.ensemble_rollout(model, x0, truth, steps, M, amp, seed, cz, 3, scorer, keep_forecast=True, perturbation_kind="spherical",
                                      length_scale_km=km)
    assert torch.equal(kept.forecast, y)
    white = inference.ensemble_rollout(model, x0, truth, steps, M, amp, seed, cz, 3, scorer, keep_forecast=True)
    assert not torch.equal(white.forecast, y) and torch.equal(white.forecast[:B], y[:B])          # the control is the same forecast
    assert bool((kept.spread > 0).all())
