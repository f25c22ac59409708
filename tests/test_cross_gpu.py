"""GPU (-m gpu): swv2_sht_cross_power / swv2_sht_cross_adjoint through the C ABI, judged element by element against the fp64 statement of
tests/cross_reference.py from the kernels' own operand and the library's own fp32 table (every bound is derived there), then the Python
layer on top of them: cross_power value and gradients, GeometricAMSELoss, ForecastScorer.spectral_coherence, score_rollout."""
import functools

import numpy as np
import pytest
import torch

from tests import cross_reference as X
from tests import sht_reference as R
from tests.plane_harness import SENTINEL, Guarded, dev, lib  # noqa: F401  (dev, lib: fixtures)

pytestmark = pytest.mark.gpu

# (nlat, nlon, pairs)
SHAPES = [(2, 4, 1),           # degenerate smallest
          (8, 32, 3),          # mmax > lmax
          (24, 16, 5),         # mmax < lmax
          (33, 64, 2),         # one past a 32 tile in l and k
          (65, 128, 3),        # crosses 64
          (19, 15, 17),        # odd everything; 68 columns: the last pair alone beyond the tile edge at 64
          (96, 192, 20)]       # several tiles each way; 80 columns
IDS = ["x".join(map(str, s)) for s in SHAPES]


def worst(err, bound):
    """largest error / bound; an error where the bound is zero must be zero"""
    err, bound = np.asarray(err, np.float64), np.asarray(bound, np.float64)
    assert np.all(err[bound == 0] == 0), "an element that must be exact is not"
    return float(np.max(err[bound > 0] / bound[bound > 0])) if np.any(bound > 0) else 0.0


@functools.lru_cache(maxsize=None)
def _case(nlat, nlon, pairs):
    """one shape's inputs and fp64 answers, computed once: the fp32 table as the library rounds it, fields with a red spectrum and an offset
    per plane (b = a mixed with another such field: coherent, not equal), the operand X (fp32), the gradient g [3, pairs, lmax]"""
    from swin_v2_weather_amd.utils import sht
    rng = np.random.default_rng(nlat * 1000 + nlon + pairs)
    T32 = sht.legendre_table(nlat, nlon).astype(np.float32)

    def red():
        return rng.standard_normal((pairs, nlat, nlon)).cumsum(-1) / np.sqrt(nlon) + rng.standard_normal((pairs, 1, 1))

    a = red()
    b = (0.6 * a + 0.8 * red()).astype(np.float32)
    a = a.astype(np.float32)
    X32 = R.operand(X.stack_pairs(a, b), T32.shape[0]).astype(np.float32)
    g = ((0.5 + rng.random((3, pairs, nlat))) * np.where(rng.random((3, pairs, nlat)) < 0.3, -1, 1)).astype(np.float32)
    T, Xd, gd = T32.astype(np.float64), X32.astype(np.float64), g.astype(np.float64)
    c, mag = R.coeffs(T, Xd)
    dc = R.coeff_bound(mag, nlat)
    ref = dict(c=c, dc=dc, S=X.spectra(c), dS=X.spectra_bound(c, dc), dX=X.adjoint(T, c, gd), ddX=X.adjoint_bound(T, c, dc, gd))
    for v in (T32, a, b, X32, g, *ref.values()):
        v.setflags(write=False)
    return T32, a, b, X32, g, ref


def _run(lib, dev, T32, X32, g, pairs, keep=True):
    from swin_v2_weather_amd import _lib as L
    mmax, lmax, nlat = T32.shape
    wsb = lib.swv2_sht_cross_ws_bytes(pairs, lmax, mmax)
    assert wsb == -(-min(mmax, lmax) // L.SHT_MRUN) * 3 * pairs * lmax * 4
    T, Xd, gd = (torch.tensor(a).to(dev) for a in (T32, X32, g))
    G = Guarded(dev, ws=wsb // 4, spectra=3 * pairs * lmax, coef=mmax * 4 * pairs * lmax, dX=mmax * 4 * pairs * nlat)
    st = torch.cuda.current_stream().cuda_stream
    L.check(lib.swv2_sht_cross_power(T.data_ptr(), Xd.data_ptr(), G["spectra"].data_ptr(), G["coef"].data_ptr() if keep else None, pairs, nlat, lmax,
                                     mmax, G["ws"].data_ptr(), wsb, st), "swv2_sht_cross_power")
    if keep:
        L.check(lib.swv2_sht_cross_adjoint(T.data_ptr(), G["coef"].data_ptr(), gd.data_ptr(), G["dX"].data_ptr(), pairs, nlat, lmax, mmax, st),
                "swv2_sht_cross_adjoint")
    torch.cuda.synchronize()
    return G


def _plain_power(lib, dev, T32, X32, planes):
    """swv2_sht_power on the same operand: [planes, lmax] as int32 bits"""
    from swin_v2_weather_amd import _lib as L
    mmax, lmax, nlat = T32.shape
    wsb = lib.swv2_sht_ws_bytes(planes, lmax, mmax)
    T, Xd = torch.tensor(T32).to(dev), torch.tensor(X32).to(dev)
    G = Guarded(dev, ws=wsb // 4, power=planes * lmax)
    L.check(lib.swv2_sht_power(T.data_ptr(), Xd.data_ptr(), G["power"].data_ptr(), None, planes, nlat, lmax, mmax, G["ws"].data_ptr(), wsb,
                               torch.cuda.current_stream().cuda_stream), "swv2_sht_power")
    torch.cuda.synchronize()
    assert G.guards_intact()
    return G.ints("power").reshape(planes, lmax)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_kernels_element_by_element_against_fp64(dev, lib, shape):
    nlat, nlon, pairs = shape
    T32, _, _, X32, g, ref = _case(*shape)
    mmax, lmax, _ = T32.shape
    N = 4 * pairs
    G = _run(lib, dev, T32, X32, g, pairs)
    assert G.guards_intact(), "a kernel wrote outside its outputs"
    assert G.written("spectra") and G.written("dX"), "output slots left unwritten"
    tri = np.broadcast_to(R.tri(mmax, lmax)[:, None, :], (mmax, N, lmax))
    raw = G.ints("coef").cpu().numpy().reshape(mmax, N, lmax)
    assert np.all(raw[tri] != SENTINEL), "a coefficient with l >= m was left unwritten"
    assert np.all(raw[~tri] == SENTINEL), "a coefficient with l < m was written (those rows are neither read nor multiplied)"
    c = np.where(tri, G["coef"].cpu().numpy().reshape(mmax, N, lmax).astype(np.float64), 0.0)
    S = G["spectra"].cpu().numpy().reshape(3, pairs, lmax).astype(np.float64)
    dX = G["dX"].cpu().numpy().reshape(mmax, N, nlat).astype(np.float64)
    rc = worst(np.abs(c - ref["c"]), ref["dc"])
    rp = worst(np.abs(S[:2] - ref["S"][:2]), ref["dS"][:2])
    rx = worst(np.abs(S[2] - ref["S"][2]), ref["dS"][2])
    rd = worst(np.abs(dX - ref["dX"]), ref["ddX"])
    print(f"{shape}: worst error / bound  coefficients {rc:.3f}  auto spectra {rp:.3f}  cross spectrum {rx:.3f}  dX {rd:.3f}")
    assert rc <= 1.0 and rp <= 1.0 and rx <= 1.0 and rd <= 1.0
    # the auto spectra carry the bits of swv2_sht_power on the same 2 pairs planes
    plain = _plain_power(lib, dev, T32, X32, 2 * pairs)
    got = G.ints("spectra").reshape(3, pairs, lmax)
    assert torch.equal(got[0], plain[0::2]) and torch.equal(got[1], plain[1::2])
    # the forward without the coefficient buffer gives the same spectra, and a second run the same bits everywhere
    G0 = _run(lib, dev, T32, X32, g, pairs, keep=False)
    assert G0.guards_intact() and not G0.written("coef") and bool((G0.ints("coef") == SENTINEL).all())
    assert torch.equal(G0.ints("spectra"), G.ints("spectra"))
    G2 = _run(lib, dev, T32, X32, g, pairs)
    for k in ("spectra", "coef", "dX"):
        assert torch.equal(G2.ints(k), G.ints(k)), f"{k}: two runs differ"


@pytest.mark.parametrize("row", [0, 1, 2], ids=["g_aa=0", "g_bb=0", "g_ab=0"])
def test_adjoint_with_one_gradient_row_all_zero(dev, lib, row):
    shape = (33, 64, 2)
    T32, _, _, X32, g, ref = _case(*shape)
    g0 = g.copy()
    g0[row] = 0.0
    T, gd = T32.astype(np.float64), g0.astype(np.float64)
    G = _run(lib, dev, T32, X32, g0, shape[2])
    assert G.guards_intact() and G.written("dX")
    dX = G["dX"].cpu().numpy().reshape(ref["dX"].shape).astype(np.float64)
    r = worst(np.abs(dX - X.adjoint(T, ref["c"], gd)), X.adjoint_bound(T, ref["c"], ref["dc"], gd))
    print(f"row {row} zero: worst error / bound  dX {r:.3f}")
    assert r <= 1.0


# ---- the Python layer ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _e2e(nlat, nlon, pairs):
    T32, a, b, _, g, _ = _case(nlat, nlon, pairs)
    out = X.end_to_end(a.astype(np.float64), b.astype(np.float64), T32.astype(np.float64), g.astype(np.float64))
    for v in out:
        for w in (v if isinstance(v, tuple) else (v,)):
            w.setflags(write=False)
    return out


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_cross_power_value_and_gradients_against_fp64(dev, lib, shape):
    from swin_v2_weather_amd.utils import sht
    _, a, b, _, g, _ = _case(*shape)
    S, dS, gx, dgx, _ = _e2e(*shape)
    ad, bd = (torch.tensor(v).to(dev).requires_grad_(True) for v in (a, b))
    assert sht.on_kernels(ad) and sht.on_kernels(bd)
    got = torch.stack(sht.cross_power(ad, bd))
    (got * torch.tensor(g).to(dev)).sum().backward()
    rs = worst(np.abs(got.detach().cpu().numpy().astype(np.float64) - S), dS)
    ra = worst(np.abs(ad.grad.cpu().numpy().astype(np.float64) - gx[0]), dgx[0])
    rb = worst(np.abs(bd.grad.cpu().numpy().astype(np.float64) - gx[1]), dgx[1])
    print(f"{shape}: worst error / bound  spectra {rs:.3f}  gradient to a {ra:.3f}  to b {rb:.3f}")
    assert rs <= 1.0 and ra <= 1.0 and rb <= 1.0
    with torch.no_grad():                                    # without a gradient to serve no coefficients are kept: same bits
        assert torch.equal(torch.stack(sht.cross_power(ad.detach(), bd.detach())), got.detach())
    # an input that needs no gradient gets none, and the other one's is unchanged
    a2 = torch.tensor(a).to(dev).requires_grad_(True)
    (torch.stack(sht.cross_power(a2, bd.detach())) * torch.tensor(g).to(dev)).sum().backward()
    assert torch.equal(a2.grad, ad.grad)
    # the statement on the same device with the same fp32 table obeys the same bounds
    st = torch.stack(sht.cross_power_torch(ad.detach(), bd.detach(), sht.device_table(shape[0], shape[1], dev)))
    assert worst(np.abs(st.cpu().numpy().astype(np.float64) - S), dS) <= 1.0


@functools.lru_cache(maxsize=None)
def _loss_case():
    """fields with power in every degree: white noise plus an offset per plane; the forecast = target + noise of comparable amplitude.
    (17 x 32 with a modest offset: the FFT's term of the bound grows with sum |x| and with log2 nlon, and on 33 x 64 the weakest degree
    stands only 500 times above its bound, short of the 1000 the first-order argument asks for)"""
    rng = np.random.default_rng(78)
    B, C, nlat, nlon = 2, 3, 17, 32
    tar = (rng.standard_normal((B, C, nlat, nlon)) + 0.3 * rng.standard_normal((B, C, 1, 1))).astype(np.float32)
    prd = (tar + 0.7 * rng.standard_normal((B, C, nlat, nlon))).astype(np.float32)
    from swin_v2_weather_amd.utils import sht
    T = sht.legendre_table(nlat, nlon).astype(np.float32).astype(np.float64)
    return prd, tar, T


@pytest.mark.parametrize("absolute", [False, True], ids=["relative", "absolute"])
def test_amse_loss_value_and_gradient(dev, lib, absolute):
    """value[b, c] within the first-order bound carried from the spectra's; prd.grad within the bound of the adjoint for the fp64
    coefficients d value / d (P_x, P_y, C) plus the adjoint's magnitude sum for what those coefficients can move by"""
    from swin_v2_weather_amd.utils.losses import GeometricAMSELoss
    prd, tar, T = _loss_case()
    B, C, nlat, nlon = prd.shape
    p64, t64 = (v.reshape(B * C, nlat, nlon).astype(np.float64) for v in (prd, tar))
    S, dS = X.end_to_end(p64, t64, T)
    assert np.all(S[:2] >= 1e3 * dS[:2]), "the inputs must keep every degree's power far above its bound (the bound is first order)"
    ref, bound = X.amse(S, absolute), X.amse_bound(S, dS, absolute)
    assert np.all(bound < 1e-2 * np.abs(ref))                # (what test_cross_host.py's mutants of the loss are told apart by)
    gS = X.amse_grad(S, absolute)
    _, _, gx, dgx, _ = X.end_to_end(p64, t64, T, gS)
    # the coefficients gS are formed in fp32 from spectra off by up to dS: what they can move by goes through the adjoint's magnitude sum
    mg = X.end_to_end(p64, t64, T, X.amse_grad_spread(S, dS, absolute))[4]
    gbound = dgx[0] + mg[0]
    loss = GeometricAMSELoss((nlat, nlon), absolute=absolute).to(dev)
    p = torch.tensor(prd).to(dev).requires_grad_(True)
    val = loss(p, torch.tensor(tar).to(dev))
    assert val.shape == (B, C)
    val.sum().backward()
    rv = worst(np.abs(val.detach().cpu().numpy().astype(np.float64).reshape(-1) - ref), bound)
    rg = worst(np.abs(p.grad.cpu().numpy().astype(np.float64).reshape(B * C, nlat, nlon) - gx[0]), gbound)
    print(f"absolute={absolute}: value {val.detach().cpu().numpy().reshape(-1)[:2]} (fp64 {ref[:2]})  error / bound  value {rv:.5f}  gradient {rg:.5f}")
    assert rv <= 1.0 and rg <= 1.0


def test_coherence_of_a_channel_block_view(dev, lib):
    from swin_v2_weather_amd.utils import sht
    from swin_v2_weather_amd.utils.weighted_acc_rmse import ForecastScorer
    nlat, nlon, pairs = 24, 16, 5
    _, a, b, _, _, _ = _case(nlat, nlon, pairs)
    a, b = a[:4], b[:4]
    wide = torch.full((2, 7, nlat, nlon), float("nan"), device=dev)
    wide[:, 3:5] = torch.tensor(a).to(dev).reshape(2, 2, nlat, nlon)
    tar = torch.zeros(2, 4, nlat, nlon, device=dev)
    tar[:, 2:4] = torch.tensor(b).to(dev).reshape(2, 2, nlat, nlon)
    va, vb = wide[:, 3:5], tar[:, 2:4]
    assert sht.on_kernels(va) and not va.is_contiguous()
    got = sht.cross_power(va, vb)
    want = sht.cross_power(va.contiguous(), vb.contiguous())
    assert all(torch.equal(x, y) for x, y in zip(got, want)) and got[0].shape == (2, 2, nlat)
    coh = ForecastScorer(nlat, nlon, 2, dev).spectral_coherence(va, vb)
    assert coh.dtype == torch.float64 and coh.shape == (2, 2, nlat)
    T = sht.legendre_table(nlat, nlon).astype(np.float32).astype(np.float64)
    S, dS = X.end_to_end(a.astype(np.float64), b.astype(np.float64), T)
    assert worst(np.abs(torch.stack(got).cpu().numpy().reshape(3, 4, nlat).astype(np.float64) - S), dS) <= 1.0


def test_score_rollout_coherence_is_the_scorer_on_the_kept_forecast(dev, lib, tmp_path):
    from swin_v2_weather_amd import inference
    from swin_v2_weather_amd.utils.sht import coherence_scale
    from swin_v2_weather_amd.utils.weighted_acc_rmse import ForecastScorer
    from tests.test_score_gpu import _registry_model
    model = _registry_model(dev, tmp_path)
    B, Cout, H, W, steps = 2, 5, 48, 72, 3
    g = torch.Generator(device=dev).manual_seed(3)
    x0 = torch.randn(B, 9, H, W, device=dev, generator=g)
    cz = torch.rand(B, steps - 1, H, W, device=dev, generator=g) * 2 - 1
    truth = torch.randn(B, steps, Cout, H, W, device=dev, generator=g)
    scorer = ForecastScorer(H, W, Cout, dev)
    kept = inference.score_rollout(model, x0, truth, steps, cz, n_invar=3, scorer=scorer, keep_forecast=True, coherence=True)
    plain = inference.score_rollout(model, x0, truth, steps, cz, n_invar=3, scorer=scorer, keep_forecast=True)
    assert plain.coherence is None and torch.equal(plain.forecast, kept.forecast) and torch.equal(plain.rmse, kept.rmse)
    assert len(kept) == 6
    co = kept.coherence
    assert co.coherence.shape == (steps, Cout, H) and co.coherence.dtype == torch.float64 and co.scale.shape == (steps, B, Cout)
    same = lambda x, y: torch.equal(torch.nan_to_num(x, nan=7.0), torch.nan_to_num(y, nan=7.0))      # noqa: E731  (NaN: a degree without power)
    for s in range(steps):
        want = scorer.spectral_coherence(kept.forecast[:, s], truth[:, s])
        assert same(co.coherence[s], want.mean(dim=0)) and torch.equal(co.scale[s], coherence_scale(want, co.level))
    ring = inference.score_rollout(model, x0, truth, steps, cz, n_invar=3, scorer=scorer, coherence=True)
    assert same(ring.coherence.coherence, co.coherence) and torch.equal(ring.coherence.scale, co.scale)
