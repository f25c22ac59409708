"""fp64 numpy statement of the cross spectra of plane pairs (swv2_sht_cross_power / swv2_sht_cross_adjoint), of the spectral coherence and
of the adjusted spectral MSE, written independently of swin_v2_weather_amd/utils/sht.py and utils/losses.py on top of
tests/sht_reference.py (weights, Legendre functions, operand, coefficients and their bound dc are taken from there unchanged).

Layouts are those of include/swv2.h: the operand holds the planes a_0, b_0, a_1, b_1, ..., so column 4 p + (0, 1, 2, 3) is (re a, im a,
re b, im b) of pair p; spectra and their gradients are [3, pairs, lmax] = (P_aa, P_bb, C_ab).

Bounds (u = 2^-24, U23 = 2 u, TINY = 2^-149 as in sht_reference; none is fitted to a result).

Auto spectra.  P_aa and P_bb are sht_reference.power_bound on the planes 2 p and 2 p + 1: the kernel forms them by the same chain.

Cross spectrum.  C = sum_m w_m (re_a re_b + im_a im_b).  With the coefficients off by at most dc each, a product moves by at most
|c_a| dc_b + |c_b| dc_a + dc_a dc_b.  The epilogue rounds the first product, then fmaf(im_a, im_b, .), then fmaf(w_m, ., sum): 3 roundings
per term, and the sum over m (runs, then the fold) has at most mmax additions.  The terms are of either sign, so every rounding is relative
to the sum of magnitudes M = sum_m w_m ((|re_a| + d)(|re_b| + d) + (|im_a| + d)(|im_b| + d)), not to C:
    dC = sum_m w_m sum_{re, im} (|c_a| dc_b + |c_b| dc_a + dc_a dc_b)  +  (mmax + 3) U23 M  +  4 (mmax + 1) TINY

Adjoint.  dX[n] = sum_{l >= m} T A,  A = s c[n] + t c[n ^ 2],  s = 2 w_m g_self, t = w_m g_ab.  The kernel's operand (csrc/sht.hip,
CrossScale): s and t exact (powers of two times g), t c[n ^ 2] rounded once, one fma joins it with s c[n]: 2 roundings relative to
magA = |s| (|c[n]| + dc[n]) + |t| (|c[n ^ 2]| + dc[n ^ 2]); the forward's error enters as |s| dc[n] + |t| dc[n ^ 2]; then the fma chain of
lmax - m terms as in sht_reference.adjoint_bound:
    ddX = (lmax - m + 2) U23 sum_l |T| magA  +  sum_l |T| (|s| dc[n] + |t| dc[n ^ 2])  +  (lmax - m + 2) TINY

End to end from the fields the FFT's term enters dc and the way back exactly as in sht_reference.end_to_end.

AMSE.  With gx, gy, gc = dA / d(P_x, P_y, C) in fp64 the value moves by at most sum_l (|gx| dP_x + |gy| dP_y + |gc| dC) to first order
(the tests assert min_l P >= 1000 dP on the reference before they rely on it), and the fp32 evaluation of the formula itself (three
square roots, a division and seven more operations per degree: at most 16 roundings, each relative to an intermediate no larger than
E_l = 2 (P_x + P_y) + 4 max(P_x, P_y), then a sum of lmax terms) adds (16 + lmax) U23 sum_l E_l.
"""
import numpy as np

from tests import sht_reference as R

U23, TINY = R.U23, R.TINY


def stack_pairs(a, b):
    """a, b [pairs, nlat, nlon] -> [2 pairs, nlat, nlon] in the order a_0, b_0, a_1, b_1, ..."""
    return np.stack([a, b], axis=1).reshape((-1,) + a.shape[1:])


def _parts(c):
    """[mmax, 4 pairs, lmax] -> (a, b), each [mmax, pairs, 2 (re, im), lmax]"""
    mmax, N, lmax = c.shape
    q = c.reshape(mmax, N // 4, 2, 2, lmax)
    return q[:, :, 0], q[:, :, 1]


def cross(c, drop_factor=False, swap_parts=False):
    """C[p, l] = sum_m w_m (re_a re_b + im_a im_b).  The switches build mutants the bound test must reject: the factor 2 of m >= 1 dropped;
    re paired with im."""
    ca, cb = _parts(c)
    if swap_parts:
        cb = cb[:, :, ::-1]
    w = np.ones(c.shape[0]) if drop_factor else R.wm(c.shape[0])
    return np.einsum("m,mpl->pl", w, (ca * cb).sum(2))


def spectra(c):
    """[3, pairs, lmax] = (P_aa, P_bb, C_ab)"""
    P = R.power(c)
    return np.stack([P[0::2], P[1::2], cross(c)])


def cross_bound(c, dc):
    mmax = c.shape[0]
    (ca, cb), (da, db) = _parts(np.abs(c)), _parts(dc)
    move = (ca * db + cb * da + da * db).sum(2)
    mag = ((ca + da) * (cb + db)).sum(2)
    w = R.wm(mmax)
    return np.einsum("m,mpl->pl", w, move) + (mmax + 3) * U23 * np.einsum("m,mpl->pl", w, mag) + 4 * (mmax + 1) * TINY


def spectra_bound(c, dc):
    dP = R.power_bound(c, dc, R.power(c))
    return np.stack([dP[0::2], dP[1::2], cross_bound(c, dc)])


def _scales(g, mmax, double_gab=False):
    """s, t [mmax, 4 pairs, lmax]: the factors of c[n] and of c[n ^ 2] in the adjoint's operand"""
    w = R.wm(mmax)[:, None, None]
    g_self = np.stack([g[0], g[0], g[1], g[1]], axis=1).reshape(-1, g.shape[-1])             # [4 pairs, lmax]
    g_ab = np.repeat(g[2], 4, axis=0) * (2.0 if double_gab else 1.0)
    return 2.0 * w * g_self[None], w * g_ab[None]


def _partner(c):
    mmax, N, lmax = c.shape
    return c.reshape(mmax, N // 4, 2, 2, lmax)[:, :, ::-1].reshape(mmax, N, lmax)


def adjoint(T, c, g, double_gab=False):
    """dX[m, n, k] = sum_{l >= m} T[m, l, k] (2 w_m g_self c[m, n, l] + w_m g_ab c[m, n ^ 2, l]); double_gab builds the third mutant"""
    s, t = _scales(g, c.shape[0], double_gab)
    return np.einsum("mlk,mnl->mnk", T, s * c + t * _partner(c))


def adjoint_bound(T, c, dc, g):
    mmax, lmax, _ = T.shape
    mask = R.tri(mmax, lmax)[:, None, :]
    s, t = (np.abs(v) * mask for v in _scales(g, mmax))
    n_terms = np.maximum(lmax - np.arange(mmax), 0)[:, None, None] + 2
    aT, ac = np.abs(T), np.abs(c)
    magA = s * (ac + dc) + t * (_partner(ac) + _partner(dc))
    return (n_terms * U23 * np.einsum("mlk,mnl->mnk", aT, magA) + np.einsum("mlk,mnl->mnk", aT, s * dc + t * _partner(dc)) + n_terms * TINY)


def end_to_end(a, b, T, g=None):
    """from the fields a, b [pairs, nlat, nlon] and the table T (fp64): spectra [3, pairs, lmax], their bound, and with g [3, pairs, lmax]
    the gradients of sum(g * spectra) with respect to a and b, their bounds, and the sums of the magnitudes of their terms"""
    x = stack_pairs(a, b)
    planes, nlat, nlon = x.shape
    mmax = T.shape[0]
    c, mag = R.coeffs(T, R.operand(x, mmax))
    dxf = np.repeat(R.fft_bound(x), 2, axis=0)
    dc = R.coeff_bound(mag, nlat, np.einsum("mlk,nk->mnl", np.abs(T), dxf) * R.tri(mmax, T.shape[1])[:, None, :])
    S, dS = spectra(c), spectra_bound(c, dc)
    if g is None:
        return S, dS
    dX, ddX = adjoint(T, c, g), adjoint_bound(T, c, dc, g)
    ang = 2.0 * np.pi * np.outer(np.arange(mmax), np.arange(nlon)) / nlon
    dXr = dX.reshape(mmax, planes, 2, nlat)
    gx = 2.0 * np.pi / nlon * (np.einsum("mpk,mj->pkj", dXr[:, :, 0], np.cos(ang)) - np.einsum("mpk,mj->pkj", dXr[:, :, 1], np.sin(ang)))
    bnd = ddX.reshape(mmax, planes, 2, nlat).sum(2) + R.fft_const(nlon) * (np.abs(dXr).sum(2) + 2.0 ** 24 * TINY)
    dgx = 2.0 * np.pi / nlon * bnd.sum(0)[:, :, None] * np.ones(nlon)
    s, t = _scales(g, mmax)
    sa = np.abs(s * c) + np.abs(t * _partner(c))
    mgx = 2.0 * np.pi / nlon * np.einsum("mlk,mnl->mnk", np.abs(T), sa).reshape(mmax, planes, 2, nlat).sum((0, 2))[:, :, None] * np.ones(nlon)
    return S, dS, (gx[0::2], gx[1::2]), (dgx[0::2], dgx[1::2]), (mgx[0::2], mgx[1::2])


def coherence(S):
    Paa, Pbb, C = S
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(Paa * Pbb == 0, np.nan, C / np.sqrt(Paa * Pbb))


def amse(S, absolute, geometric_mean=False):
    """[3, ..., lmax] -> [...]: sum_l (sqrt Px - sqrt Py)^2 + 2 max(Px, Py) (1 - C / sqrt(Px Py)), Px + Py - 2 C where Px Py == 0; relative:
    over sum_l Py.  geometric_mean replaces max by sqrt(Px Py): the spectral MSE itself (an identity the host tests use)."""
    Px, Py, C = S
    zero = Px * Py == 0
    r = np.sqrt(np.where(zero, 1.0, Px * Py))
    big = r if geometric_mean else np.maximum(Px, Py)
    term = np.where(zero, Px + Py - 2.0 * C, (np.sqrt(Px) - np.sqrt(Py)) ** 2 + 2.0 * big * (1.0 - C / r))
    A = term.sum(-1)
    return A if absolute else A / Py.sum(-1)


def amse_grad(S, absolute):
    """d value / d (Px, Py, C), [3, ..., lmax]"""
    Px, Py, C = S
    zero = Px * Py == 0
    sx, sy = np.sqrt(np.where(zero, 1.0, Px)), np.sqrt(np.where(zero, 1.0, Py))
    r = sx * sy
    coh, big = C / r, np.maximum(Px, Py)
    gx = (sx - sy) / sx + 2.0 * (Px >= Py) * (1.0 - coh) + big * C / (r * np.where(zero, 1.0, Px))
    gy = (sy - sx) / sy + 2.0 * (Py > Px) * (1.0 - coh) + big * C / (r * np.where(zero, 1.0, Py))
    gc = -2.0 * big / r
    g = np.stack([np.where(zero, 1.0, gx), np.where(zero, 1.0, gy), np.where(zero, -2.0, gc)])
    if absolute:
        return g
    tot = Py.sum(-1, keepdims=True)
    g = g / tot
    g[1] -= (amse(S, True) / tot[..., 0] ** 2)[..., None]
    return g


def amse_bound(S, dS, absolute):
    """first-order bound of the value from the spectra's bounds, plus the fp32 evaluation of the formula (the module's docstring)"""
    Px, Py, _ = S
    lmax = Px.shape[-1]
    E = (2.0 * (Px + Py) + 4.0 * np.maximum(Px, Py)).sum(-1)
    dA = (np.abs(amse_grad(S, True)) * dS).sum((0, -1)) + (16 + lmax) * U23 * E
    if absolute:
        return dA
    tot, dtot = Py.sum(-1), dS[1].sum(-1) + lmax * U23 * Py.sum(-1)
    A = amse(S, True)
    return (dA + A / tot * dtot) / (tot - dtot) + U23 * A / tot


def amse_grad_spread(S, dS, absolute):
    """[3, ..., lmax]: how far d value / d (Px, Py, C) can move while the spectra stay within their bounds -- the largest deviation over
    the eight corners S + (+-dS_x, +-dS_y, +-dS_C) (each coefficient is monotone in each spectrum over a box this small, a switch of
    max(Px, Py) inside the box included: then the corners differ by the jump), plus the 16 roundings of its own fp32 evaluation"""
    g = amse_grad(S, absolute)
    spread = np.zeros_like(g)
    for sx in (-1.0, 1.0):
        for sy in (-1.0, 1.0):
            for sc in (-1.0, 1.0):
                sign = np.array([sx, sy, sc]).reshape((3,) + (1,) * (S.ndim - 1))
                spread = np.maximum(spread, np.abs(amse_grad(S + sign * dS, absolute) - g))
    return spread + 16 * U23 * np.abs(g)
