"""GPU (-m gpu): swv2_sht_power / swv2_sht_adjoint through the C ABI, judged element by element against the fp64 statement of
tests/sht_reference.py from the kernels' own operand and the library's own fp32 table (every bound is derived there), then the
Python layer on top of them: degree_power value and gradient, GeometricH1Loss, ForecastScorer.power_spectrum, score_rollout."""
import functools

import numpy as np
import pytest
import torch

from tests import sht_reference as R
from tests.plane_harness import SENTINEL, Guarded, dev, lib  # noqa: F401  (dev, lib: fixtures)

pytestmark = pytest.mark.gpu

# (nlat, nlon, planes)
SHAPES = [(2, 4, 1),           # degenerate smallest
          (8, 32, 3),          # mmax > lmax
          (24, 16, 5),         # mmax < lmax
          (16, 32, 4),         # the ERA5 aspect
          (33, 64, 2),         # one past a 32 tile in l and k
          (65, 128, 3),        # crosses 64
          (19, 15, 17),        # odd everything; the columns do not fill a tile
          (96, 192, 40)]       # several tiles each way; 80 columns
IDS = ["x".join(map(str, s)) for s in SHAPES]


def worst(err, bound):
    """largest error / bound; an error where the bound is zero must be zero"""
    err, bound = np.asarray(err, np.float64), np.asarray(bound, np.float64)
    assert np.all(err[bound == 0] == 0), "an element that must be exact is not"
    return float(np.max(err[bound > 0] / bound[bound > 0])) if np.any(bound > 0) else 0.0


@functools.lru_cache(maxsize=None)
def _case(nlat, nlon, planes):
    """one shape's inputs and fp64 answers, computed once: the fp32 table as the library rounds it, a field with a red spectrum and an
    offset per plane, the kernels' operand X (fp32, formed on the CPU in fp64 and rounded), the gradient g, and the reference from them"""
    from swin_v2_weather_amd.utils import sht
    rng = np.random.default_rng(nlat * 1000 + nlon + planes)
    T32 = sht.legendre_table(nlat, nlon).astype(np.float32)
    x = rng.standard_normal((planes, nlat, nlon)).cumsum(-1) / np.sqrt(nlon) + rng.standard_normal((planes, 1, 1))
    x = x.astype(np.float32)
    X32 = R.operand(x, T32.shape[0]).astype(np.float32)
    g = (0.5 + rng.random((planes, nlat))).astype(np.float32) * np.where(rng.random((planes, nlat)) < 0.3, -1, 1).astype(np.float32)
    T, X = T32.astype(np.float64), X32.astype(np.float64)
    c, mag = R.coeffs(T, X)
    dc = R.coeff_bound(mag, nlat)
    P = R.power(c)
    ref = dict(c=c, dc=dc, P=P, dP=R.power_bound(c, dc, P), dX=R.adjoint(T, c, g.astype(np.float64)),
               ddX=R.adjoint_bound(T, c, dc, g.astype(np.float64)))
    for v in (T32, x, X32, g, *ref.values()):
        v.setflags(write=False)
    return T32, x, X32, g, ref


def _run(lib, dev, T32, X32, g, planes, keep=True):
    from swin_v2_weather_amd import _lib as L
    mmax, lmax, nlat = T32.shape
    wsb = lib.swv2_sht_ws_bytes(planes, lmax, mmax)
    assert wsb == -(-min(mmax, lmax) // L.SHT_MRUN) * planes * lmax * 4
    T, X, gd = (torch.tensor(a).to(dev) for a in (T32, X32, g))
    G = Guarded(dev, ws=wsb // 4, power=planes * lmax, coef=mmax * 2 * planes * lmax, dX=mmax * 2 * planes * nlat)
    st = torch.cuda.current_stream().cuda_stream
    L.check(lib.swv2_sht_power(T.data_ptr(), X.data_ptr(), G["power"].data_ptr(), G["coef"].data_ptr() if keep else None, planes, nlat, lmax, mmax,
                               G["ws"].data_ptr(), wsb, st), "swv2_sht_power")
    if keep:
        L.check(lib.swv2_sht_adjoint(T.data_ptr(), G["coef"].data_ptr(), gd.data_ptr(), G["dX"].data_ptr(), planes, nlat, lmax, mmax, st),
                "swv2_sht_adjoint")
    torch.cuda.synchronize()
    return G


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_kernels_element_by_element_against_fp64(dev, lib, shape):
    nlat, nlon, planes = shape
    T32, _, X32, g, ref = _case(*shape)
    mmax, lmax, _ = T32.shape
    G = _run(lib, dev, T32, X32, g, planes)
    assert G.guards_intact(), "a kernel wrote outside its outputs"
    assert G.written("power") and G.written("dX"), "output slots left unwritten"
    tri = np.broadcast_to(R.tri(mmax, lmax)[:, None, :], (mmax, 2 * planes, lmax))
    raw = G.ints("coef").cpu().numpy().reshape(mmax, 2 * planes, lmax)
    assert np.all(raw[tri] != SENTINEL), "a coefficient with l >= m was left unwritten"
    assert np.all(raw[~tri] == SENTINEL), "a coefficient with l < m was written (those rows are neither read nor multiplied)"
    c = np.where(tri, G["coef"].cpu().numpy().reshape(mmax, 2 * planes, lmax).astype(np.float64), 0.0)
    P = G["power"].cpu().numpy().reshape(planes, lmax).astype(np.float64)
    dX = G["dX"].cpu().numpy().reshape(mmax, 2 * planes, nlat).astype(np.float64)
    rc, rp, rx = worst(np.abs(c - ref["c"]), ref["dc"]), worst(np.abs(P - ref["P"]), ref["dP"]), worst(np.abs(dX - ref["dX"]), ref["ddX"])
    print(f"{shape}: worst error / bound  coefficients {rc:.3f}  power {rp:.3f}  dX {rx:.3f}")
    assert rc <= 1.0 and rp <= 1.0 and rx <= 1.0
    # the forward without the coefficient buffer gives the same power, and a second run the same bits everywhere
    G0 = _run(lib, dev, T32, X32, g, planes, keep=False)
    assert G0.guards_intact() and not G0.written("coef") and bool((G0.ints("coef") == SENTINEL).all())
    assert torch.equal(G0.ints("power"), G.ints("power"))
    G2 = _run(lib, dev, T32, X32, g, planes)
    for k in ("power", "coef", "dX"):
        assert torch.equal(G2.ints(k), G.ints(k)), f"{k}: two runs differ"


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_repack_both_ways_bit_for_bit(dev, lib, shape):
    """swv2_sht_repack is a transposing copy with one fp32 product per element: X[m][2 p + ri][k] = scale F[p][k][m][ri] and back"""
    from swin_v2_weather_amd import _lib as L
    nlat, nlon, planes = shape
    mmax = nlon // 2 + 1
    rng = np.random.default_rng(7)
    F = rng.standard_normal((planes, nlat, mmax, 2)).astype(np.float32)
    scale = np.float32(2.0 * np.pi)
    G = Guarded(dev, X=F.size, back=F.size)
    Fd = torch.tensor(F).to(dev)
    st = torch.cuda.current_stream().cuda_stream
    L.check(lib.swv2_sht_repack(Fd.data_ptr(), G["X"].data_ptr(), planes, nlat, mmax, float(scale), 0, st), "swv2_sht_repack")
    L.check(lib.swv2_sht_repack(G["X"].data_ptr(), G["back"].data_ptr(), planes, nlat, mmax, 0.5, 1, st), "swv2_sht_repack")
    torch.cuda.synchronize()
    assert G.guards_intact() and G.written("X") and G.written("back")
    want = (scale * F).transpose(2, 0, 3, 1).reshape(mmax, 2 * planes, nlat)
    assert np.array_equal(G["X"].cpu().numpy().reshape(want.shape), want)
    assert np.array_equal(G["back"].cpu().numpy().reshape(F.shape), np.float32(0.5) * (scale * F))


# ---- the Python layer ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _e2e(nlat, nlon, planes):
    """the fp64 answers from the field itself (the FFT's share included): power, gradient of sum(g * power), their bounds"""
    T32, x, _, g, _ = _case(nlat, nlon, planes)
    out = R.end_to_end(x.astype(np.float64), T32.astype(np.float64), g.astype(np.float64))
    for v in out:
        v.setflags(write=False)
    return out


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_degree_power_value_and_gradient_against_fp64(dev, lib, shape):
    from swin_v2_weather_amd.utils import sht
    _, x, _, g, _ = _case(*shape)
    P, dP, gx, dgx, _ = _e2e(*shape)
    xd = torch.tensor(x).to(dev).requires_grad_(True)
    assert sht.on_kernels(xd)
    got = sht.degree_power(xd)
    (got * torch.tensor(g).to(dev)).sum().backward()
    rp = worst(np.abs(got.detach().cpu().numpy().astype(np.float64) - P), dP)
    rg = worst(np.abs(xd.grad.cpu().numpy().astype(np.float64) - gx), dgx)
    print(f"{shape}: worst error / bound  power {rp:.3f}  gradient {rg:.3f}")
    assert rp <= 1.0 and rg <= 1.0
    with torch.no_grad():                                    # without a gradient to serve no coefficients are kept: same bits
        assert torch.equal(sht.degree_power(xd.detach()), got.detach())
    # the statement on the same device with the same fp32 table obeys the same bounds (it is what the probe times the kernels against)
    st = sht.degree_power_torch(xd.detach(), sht.device_table(shape[0], shape[1], dev))
    assert worst(np.abs(st.cpu().numpy().astype(np.float64) - P), dP) <= 1.0


def _loss_bound(P, dP, lw, alpha, squared):
    """norm and its bound per sample from the degree power [B, C, lmax] and its bound: l2 = sum P and h1 = sum l (l + 1) P are sums of
    non-negative terms (n u relative each, n = C lmax terms), sqrt and the two products add 4 roundings"""
    B = P.shape[0]
    n = P[0].size
    l2, h1 = P.reshape(B, -1).sum(-1), (P * lw).reshape(B, -1).sum(-1)
    d2 = dP.reshape(B, -1).sum(-1) + n * 2.0 ** -23 * l2
    d1 = (dP * lw).reshape(B, -1).sum(-1) + (n + 1) * 2.0 ** -23 * h1
    if squared:
        v = alpha * l2 + (1 - alpha) * h1
        return v, alpha * d2 + (1 - alpha) * d1 + 4 * 2.0 ** -23 * v, d2 / l2 + d1 / h1
    v = alpha * np.sqrt(l2) + (1 - alpha) * np.sqrt(h1)
    # sqrt(a + d) - sqrt(a) <= d / (2 sqrt(a) (1 - d / a)) for d < a
    dv = alpha * d2 / (2 * np.sqrt(l2) * (1 - d2 / l2)) + (1 - alpha) * d1 / (2 * np.sqrt(h1) * (1 - d1 / h1)) + 4 * 2.0 ** -23 * v
    return v, dv, d2 / l2 + d1 / h1


@functools.lru_cache(maxsize=None)
def _loss_case():
    rng = np.random.default_rng(77)
    B, C, nlat, nlon = 2, 3, 33, 64
    prd = (rng.standard_normal((B, C, nlat, nlon)).cumsum(-1) / 8).astype(np.float32)
    tar = (rng.standard_normal((B, C, nlat, nlon)).cumsum(-1) / 8 + 0.5).astype(np.float32)
    from swin_v2_weather_amd.utils import sht
    T = sht.legendre_table(nlat, nlon).astype(np.float32).astype(np.float64)
    return prd, tar, T


@pytest.mark.parametrize("squared", [False, True], ids=["norm", "squared"])
@pytest.mark.parametrize("absolute", [False, True], ids=["relative", "absolute"])
def test_h1_loss_value_and_gradient(dev, lib, absolute, squared):
    """value within the bound carried from the power's; prd.grad within the bound of the adjoint for the fp64 coefficients d loss / d P
    plus their own relative error times the magnitude sum"""
    from swin_v2_weather_amd.utils.losses import GeometricH1Loss
    prd, tar, T = _loss_case()
    B, C, nlat, nlon = prd.shape
    alpha = 0.5
    lw = np.arange(nlat) * (np.arange(nlat) + 1.0)
    diff32 = prd - tar                                       # the loss forms the difference in fp32: exact inputs of the transform
    Pd, dPd = (a.reshape(B, C, nlat) for a in R.end_to_end(diff32.reshape(B * C, nlat, nlon).astype(np.float64), T))
    Pt, dPt = (a.reshape(B, C, nlat) for a in R.end_to_end(tar.reshape(B * C, nlat, nlon).astype(np.float64), T))
    vd, dvd, rd = _loss_bound(Pd, dPd, lw, alpha, squared)
    vt, dvt, rt = _loss_bound(Pt, dPt, lw, alpha, squared)
    if absolute:
        ref, bound, rel_g = vd.sum(), dvd.sum() + B * 2.0 ** -23 * vd.sum(), rd
        scale = np.ones(B)
    else:
        q = vd / vt
        dq = (dvd + q * dvt) / (vt - dvt) + 2.0 ** -23 * q
        ref, bound, rel_g = q.sum(), dq.sum() + B * 2.0 ** -23 * q.sum(), rd + dvt / (vt - dvt)
        scale = 1.0 / vt
    assert bound < 1e-3 * abs(ref)                           # (what test_sht_host.py::test_the_bounds_reject_the_three_mutants relies on)
    l2, h1 = Pd.reshape(B, -1).sum(-1), (Pd * lw).reshape(B, -1).sum(-1)
    if squared:
        gP = scale[:, None, None] * (alpha + (1 - alpha) * lw)[None, None, :] * np.ones((B, C, 1))
    else:
        gP = scale[:, None, None] * (alpha / (2 * np.sqrt(l2))[:, None, None] + (1 - alpha) * lw[None, None, :] / (2 * np.sqrt(h1))[:, None, None]) * \
            np.ones((B, C, 1))
    _, _, gx, dgx, mgx = R.end_to_end(diff32.reshape(B * C, nlat, nlon).astype(np.float64), T, gP.reshape(B * C, nlat))
    gbound = dgx + (rel_g + 16 * 2.0 ** -23)[:, None, None, None].repeat(C, 1).reshape(B * C, 1, 1) * mgx
    loss = GeometricH1Loss((nlat, nlon), absolute=absolute, squared=squared, alpha=alpha).to(dev)
    p = torch.tensor(prd).to(dev).requires_grad_(True)
    val = loss(p, torch.tensor(tar).to(dev))
    val.backward()
    rv = abs(float(val.detach()) - ref) / bound
    rg = worst(np.abs(p.grad.cpu().numpy().astype(np.float64).reshape(B * C, nlat, nlon) - gx), gbound)
    print(f"absolute={absolute} squared={squared}: loss {float(val.detach()):.7g} (fp64 {ref:.9g})  error / bound  value {rv:.3f}  gradient {rg:.3f}")
    assert rv <= 1.0 and rg <= 1.0


def test_power_spectrum_of_a_channel_block_view(dev, lib):
    from swin_v2_weather_amd.utils import sht
    from swin_v2_weather_amd.utils.weighted_acc_rmse import ForecastScorer
    nlat, nlon, planes = 16, 32, 4
    T32, x, _, _, _ = _case(nlat, nlon, planes)
    P, dP = (a.reshape(2, 2, nlat) for a in _e2e(nlat, nlon, planes)[:2])
    wide = torch.full((2, 7, nlat, nlon), float("nan"), device=dev)
    wide[:, 3:5] = torch.tensor(x).to(dev).reshape(2, 2, nlat, nlon)
    tar = torch.zeros(2, 4, nlat, nlon, device=dev)
    tar[:, 2:4] = 2.0 * wide[:, 3:5]
    assert sht.on_kernels(wide[:, 3:5]) and not wide[:, 3:5].is_contiguous()
    ps = ForecastScorer(nlat, nlon, 2, dev).power_spectrum(wide, tar, coff_prd=3, coff_tar=2)
    assert ps.pred.shape == ps.truth.shape == (2, 2, nlat)
    assert worst(np.abs(ps.pred.cpu().numpy().astype(np.float64) - P), dP) <= 1.0
    assert worst(np.abs(ps.truth.cpu().numpy().astype(np.float64) - 4.0 * P), 4.0 * dP) <= 1.0          # (scaling by 2 is exact)
    assert ForecastScorer(nlat, nlon, 2, dev).power_spectrum(wide, coff_prd=3).truth is None


def test_score_rollout_spectrum_is_the_scorer_on_the_kept_forecast(dev, lib, tmp_path):
    from swin_v2_weather_amd import inference
    from swin_v2_weather_amd.utils.weighted_acc_rmse import ForecastScorer, small_scale_power_ratio
    from tests.test_score_gpu import _registry_model
    model = _registry_model(dev, tmp_path)
    B, Cout, H, W, steps = 2, 5, 48, 72, 3
    g = torch.Generator(device=dev).manual_seed(3)
    x0 = torch.randn(B, 9, H, W, device=dev, generator=g)
    cz = torch.rand(B, steps - 1, H, W, device=dev, generator=g) * 2 - 1
    truth = torch.randn(B, steps, Cout, H, W, device=dev, generator=g)
    scorer = ForecastScorer(H, W, Cout, dev)
    kept = inference.score_rollout(model, x0, truth, steps, cz, n_invar=3, scorer=scorer, keep_forecast=True, spectrum=True)
    plain = inference.score_rollout(model, x0, truth, steps, cz, n_invar=3, scorer=scorer, keep_forecast=True)
    assert plain.spectrum is None and torch.equal(plain.forecast, kept.forecast) and torch.equal(plain.rmse, kept.rmse)
    sp = kept.spectrum
    assert sp.pred.shape == sp.truth.shape == (steps, Cout, H) and sp.ratio.shape == (steps, B, Cout)
    for s in range(steps):
        ps = scorer.power_spectrum(kept.forecast[:, s], truth[:, s])
        assert torch.equal(sp.pred[s], ps.pred.mean(dim=0)) and torch.equal(sp.truth[s], ps.truth.mean(dim=0))
        assert torch.equal(sp.ratio[s], small_scale_power_ratio(ps.pred, ps.truth))
    ring = inference.score_rollout(model, x0, truth, steps, cz, n_invar=3, scorer=scorer, spectrum=True)
    assert torch.equal(ring.spectrum.pred, sp.pred) and torch.equal(ring.spectrum.ratio, sp.ratio)
