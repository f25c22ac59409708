"""fp64 numpy statement of the spherical-harmonics synthesis (swv2_sht_synth), of the filter and the correlated noise built on it, with
the per-element bounds the fp32 kernels are held to.  The forward half, the table and the constants are those of tests/sht_reference.py.

Layouts are those of include/swv2.h: coefficients [mmax, 2 planes, lmax], S [mmax, 2 planes, nlat], rweights [nlat] = 1 / w_k.

    S[m, n, k] = rw[k] sum_{l >= m} T[m, l, k] s[m, n, l] c[m, n, l]          s = f_m h[n // 2, l],  f_0 = scale_m0, else scale_m
    x[p, k, j] = sum_m v_m (S_re cos(m phi_j) - S_im sin(m phi_j))            v_0 = 1, v_m = 2, v_{nlon / 2} = 1;  phi_j = 2 pi j / nlon

(the second line is irfft(S, n=nlon, norm="forward") written out: the imaginary parts at m = 0 and nlon / 2 meet sin = 0.)

Bounds (none is fitted to a result; u = 2^-24, TINY = 2^-149 as in sht_reference).

Synthesis.  The sum is the adjoint's fma chain with the operand scale s in place of 2 w_m g: s c carries 2 roundings (f_m h, then the
product with c) and, when the coefficients are given, dc = 0.  So R.adjoint_bound applies with that s -- it is handed T f_m / (2 w_m)
and g = h, whose product |T| |2 w_m g| is |T| |s| -- then the factor rw[k], then one more rounding of the product with rw[k]:
    dS = rw[k] adjoint_bound + 2^-24 |S| + TINY
End to end the forward's dc (R.coeff_bound with the FFT's share, as in R.end_to_end) enters through adjoint_bound's dc.
Inverse FFT.  irfft is an FFT of the same length as the forward one: R.fft_const(nlon) relative to the sum of the magnitudes entering,
sum_m (|S_re| + |S_im|), plus the propagated dS; both doubled for m >= 1 (a bound: the Nyquist term counts once in the value).
    dx = sum_m d_m (fft_const (|S_re| + |S_im|) + dS_re + dS_im) + fft_const 2^24 TINY,   d_0 = 1, else 2
"""
import numpy as np

from tests import sht_reference as R

U24 = 2.0 ** -24


def planes_response(h, planes, lmax):
    """None, [lmax] or [planes, lmax] -> [planes, lmax] fp64"""
    if h is None:
        return np.ones((planes, lmax))
    return np.broadcast_to(np.asarray(h, np.float64), (planes, lmax)).copy()


def m_scale(mmax, scales):
    f = np.full(mmax, float(scales[1]))
    f[0] = float(scales[0])
    return f


def real_rows(mmax, N, nlon):
    """[mmax, N]: False where the row counts as zeros -- the imaginary rows (n odd) of m = 0 and, nlon even, of m = nlon / 2"""
    keep = np.ones((mmax, N), bool)
    keep[0, 1::2] = False
    if nlon % 2 == 0 and nlon // 2 < mmax:
        keep[nlon // 2, 1::2] = False
    return keep


def clean(c, nlon):
    """the coefficients as the synthesis uses them: zero below the diagonal (whatever is stored there, NaN included) and in the rows
    real_rows() rules out"""
    mmax, N, lmax = c.shape
    use = R.tri(mmax, lmax)[:, None, :] & real_rows(mmax, N, nlon)[:, :, None]
    return np.where(use, c, 0.0)


def synth(T, rw, c, h, scales, nlon, drop_rw=False, drop_diagonal=False):
    """S [mmax, 2 planes, nlat].  The two switches build mutants the bound test must reject."""
    mmax, N, lmax = c.shape
    s = m_scale(mmax, scales)[:, None, None] * np.repeat(planes_response(h, N // 2, lmax), 2, axis=0)[None]
    cc = clean(c, nlon)
    if drop_diagonal:
        cc = cc * (np.arange(lmax)[None, :] != np.arange(mmax)[:, None])[:, None, :]
    S = np.einsum("mlk,mnl->mnk", T, s * cc)
    return S if drop_rw else S * rw


def synth_bound(T, rw, c, dc, h, scales, nlon, S):
    mmax, N, lmax = c.shape
    Tq = T * (m_scale(mmax, scales) / (2.0 * R.wm(mmax)))[:, None, None]
    use = real_rows(mmax, N, nlon)[:, :, None]
    b = R.adjoint_bound(Tq, clean(c, nlon), np.where(use, dc, 0.0) * np.ones_like(c), planes_response(h, N // 2, lmax))
    b = np.where(use, b, 0.0)                                                  # rows that are not computed at all: exact zeros
    b = np.where((np.arange(mmax) < lmax)[:, None, None], b, 0.0)              # m >= lmax: no degree, exact zeros
    return np.where(b > 0, rw * b + U24 * np.abs(S) + R.TINY, 0.0)


def field(S, nlon):
    """x [planes, nlat, nlon] = irfft(S, n=nlon, norm="forward"), written out"""
    mmax, N, nlat = S.shape
    v = np.full(mmax, 2.0)
    v[0] = 1.0
    if nlon % 2 == 0 and nlon // 2 < mmax:
        v[nlon // 2] = 1.0
    ang = 2.0 * np.pi * np.outer(np.arange(mmax), np.arange(nlon)) / nlon
    Sr = S.reshape(mmax, N // 2, 2, nlat)
    return np.einsum("m,mpk,mj->pkj", v, Sr[:, :, 0], np.cos(ang)) - np.einsum("m,mpk,mj->pkj", v, Sr[:, :, 1], np.sin(ang))


def field_bound(S, dS, nlon):
    """[planes, nlat, 1]: the same for every longitude"""
    mmax, N, nlat = S.shape
    d = np.full(mmax, 2.0)
    d[0] = 1.0
    t = (R.fft_const(nlon) * np.abs(S) + dS).reshape(mmax, N // 2, 2, nlat).sum(2)
    return (np.einsum("m,mpk->pk", d, t) + R.fft_const(nlon) * 2.0 ** 24 * R.TINY)[:, :, None]


def analysis(x, T):
    """from the field x [planes, nlat, nlon] (fp64 of fp32 values): coefficients and their bound, the FFT's share included (R.end_to_end)"""
    planes, nlat, nlon = x.shape
    mmax = T.shape[0]
    c, mag = R.coeffs(T, R.operand(x, mmax))
    dxf = np.repeat(R.fft_bound(x), 2, axis=0)
    dc = R.coeff_bound(mag, nlat, np.einsum("mlk,nk->mnl", np.abs(T), dxf) * R.tri(mmax, T.shape[1])[:, None, :])
    return c, dc


def filter_end_to_end(x, T, rw, h):
    """spectral_filter from the field: value [planes, nlat, nlon] and bound [planes, nlat, 1]"""
    nlon = x.shape[-1]
    c, dc = analysis(x, T)
    S = synth(T, rw, c, h, (1.0, 1.0), nlon)
    return field(S, nlon), field_bound(S, synth_bound(T, rw, c, dc, h, (1.0, 1.0), nlon, S), nlon)


def from_coefficients(T, rw, c, h, scales, nlon):
    """synthesis and irfft from given coefficients (dc = 0): the field, its bound, and S with its bound"""
    S = synth(T, rw, c, h, scales, nlon)
    dS = synth_bound(T, rw, c, np.zeros_like(c), h, scales, nlon, S)
    return field(S, nlon), field_bound(S, dS, nlon), S, dS
