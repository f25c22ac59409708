"""Real spherical-harmonics transform on the equiangular grid, and the degree power built on it.

What `torch_harmonics.RealSHT(nlat, nlon, grid='equiangular')` computes with its defaults (lmax = nlat, mmax = nlon // 2 + 1,
orthonormal harmonics with the Condon-Shortley phase, Clenshaw-Curtis quadrature on the nlat rows 0 .. pi, both poles included),
stated from its mathematical definition: torch_harmonics is not available to this project, so nothing here was compared with it;
tests/test_sht_host.py pins weights, normalisation, phase and orthonormality by closed forms in fp64.

    X[..., k, m]  = 2 pi * rfft(x, norm="forward")[..., k, m]                    m < mmax
    c[..., l, m]  = sum_k table[m, l, k] X[..., k, m]                            table = w_k * Pbar_l^m(cos theta_k), 0 for l < m
    P[..., l]     = |c[l, 0]|^2 + 2 sum_{m >= 1} |c[l, m]|^2                     the degree power

The rule is exact only while the degrees of field and harmonic add up to at most nlat - 1; beyond that the reference's choice of
lmax = nlat aliases, and so does this (mirrored, not repaired).

Tables are fp64 numpy, rounded to fp32 once when handed to a device.  `real_sht_torch` / `degree_power_torch` are the readable
statement (any device, any dtype, differentiable by autograd).  `degree_power` takes contiguous fp32 CUDA tensors through
csrc/sht.hip: torch's rfft for the longitudes, then one autograd node over swv2_sht_repack (the transposing copy into the kernels'
operand layout [mmax, 2 planes, nlat], times 2 pi), swv2_sht_power and, in backward, swv2_sht_adjoint and the repack the other way.
The node's input is the rfft's output, so autograd itself carries the gradient back through the rfft.

Two fields degree by degree: `cross_power(a, b)` returns the degree powers of both and their cross spectrum
C_ab[l] = sum_m w_m Re(c_a[l, m] conj(c_b[l, m])); `cross_power_torch` is its statement, and fp32 CUDA tensors with contiguous planes take
swv2_sht_cross_power / swv2_sht_cross_adjoint on the pair stacked plane by plane (one rfft, one autograd node).  `spectral_coherence` is
C_ab / sqrt(P_aa P_bb), the anomaly correlation of every degree, and `coherence_scale` the degree down to which it holds a level.

The way back, stated the same way (pinned by its definition in fp64, tests/test_isht_host.py; never compared with torch_harmonics):

    S[..., k, m]  = sum_{l >= m} Pbar_l^m(cos theta_k) c[..., l, m]              Pbar = table / w_k
    x[..., k, j]  = irfft(S, n=nlon, norm="forward")[..., k, j]                  (the 2 pi lives in the forward)

`inverse_real_sht`, `real_sht`, `spectral_filter` / `spectral_truncate` and `spherical_noise` each have their `_torch` statement beside
them; fp32 CUDA tensors with contiguous planes that need no gradient (at most 65535 planes a call) run on csrc/sht.hip
(swv2_sht_synth: the adjoint's product on the same table with a per-degree response and 1 / w_k in its epilogue), everything else runs
the statement; a failure on the kernel path raises.

What the grid allows.  With lmax = nlat the analysis aliases at degrees l > nlat - 1 - L for a field of degree L, so analysis followed
by synthesis with the identity response is NOT the identity map.  spectral_truncate(x, (nlat - 1) // 2) returns x for every field
band-limited to l <= (nlat - 1) // 2, m <= (nlon - 1) // 2 (7e-13 at worst in fp64 over the grids of tests/test_isht_host.py).
"""
import math

import numpy as np
import torch


def clenshaw_curtis_weights(nlat: int) -> np.ndarray:
    """fp64 weights of the Clenshaw-Curtis rule in x = cos(theta) on theta_k = k pi / (nlat - 1), k = 0 .. nlat - 1 (row 0: north pole)"""
    if nlat < 2:
        raise ValueError("the equiangular grid with both poles has at least 2 rows")
    N = nlat - 1
    theta = np.pi * np.arange(nlat) / N
    w = np.ones(nlat)
    for j in range(1, N // 2 + 1):
        b = 1.0 if 2 * j == N else 2.0
        w -= b / (4.0 * j * j - 1.0) * np.cos(2.0 * j * theta)
    c = np.full(nlat, 2.0)
    c[0] = c[-1] = 1.0
    return c / N * w


def legendre_table(nlat: int, nlon: int) -> np.ndarray:
    """fp64 [mmax, lmax, nlat]: w_k * Pbar_l^m(cos theta_k), orthonormal with the Condon-Shortley phase; zero for l < m and m >= lmax"""
    lmax, mmax = nlat, nlon // 2 + 1
    x = np.cos(np.pi * np.arange(nlat) / (nlat - 1))
    w = clenshaw_curtis_weights(nlat)
    nm = max(lmax, mmax)
    P = np.zeros((nm, lmax, nlat))              # unsigned, [m, l, k]
    P[0, 0] = 1.0 / math.sqrt(4.0 * math.pi)
    for l in range(1, lmax):
        P[l, l] = np.sqrt((2 * l + 1) * (1 + x) * (1 - x) / (2.0 * l)) * P[l - 1, l - 1]
        P[l - 1, l] = math.sqrt(2 * l + 1) * x * P[l - 1, l - 1]
    for l in range(2, lmax):
        m = np.arange(0, l - 1).reshape(-1, 1)
        a = np.sqrt((2 * l - 1) * (2 * l + 1) / ((l - m) * (l + m)))
        b = np.sqrt((l + m - 1) * (l - m - 1) * (2 * l + 1) / ((l - m) * (l + m) * (2.0 * l - 3)))
        P[:l - 1, l] = x * a * P[:l - 1, l - 1] - b * P[:l - 1, l - 2]
    P = P[:mmax]
    P[1::2] *= -1.0
    return P * w


def real_sht_torch(x: torch.Tensor, table: torch.Tensor) -> torch.Tensor:
    """x [..., nlat, nlon] real, table [mmax, lmax, nlat] -> complex c [..., lmax, mmax]"""
    mmax = table.shape[0]
    X = 2.0 * math.pi * torch.fft.rfft(x, dim=-1, norm="forward")[..., :mmax]
    return torch.einsum("mlk,...km->...lm", table.to(X.dtype), X)


def degree_power_torch(x: torch.Tensor, table: torch.Tensor) -> torch.Tensor:
    """[..., nlat, nlon] -> [..., lmax]: |c_l0|^2 + 2 sum_{m >= 1} |c_lm|^2 (losses.py:275-277), every m >= 1 doubled, the last included"""
    c = torch.view_as_real(real_sht_torch(x, table))
    c2 = c[..., 0] ** 2 + c[..., 1] ** 2
    return c2[..., :, 0] + 2 * torch.sum(c2[..., :, 1:], dim=-1)


_TABLES = {}


def device_table(nlat: int, nlon: int, device, dtype=torch.float32) -> torch.Tensor:
    """the table of a grid on a device, built once per (nlat, nlon, device, dtype)"""
    device = torch.device(device)
    key = (nlat, nlon, device.type, device.index, dtype)
    t = _TABLES.get(key)
    if t is None:
        t = _TABLES[key] = torch.from_numpy(legendre_table(nlat, nlon)).to(device=device, dtype=dtype).contiguous()
    return t


_RWEIGHTS = {}


def inverse_weights(nlat: int, device, dtype=torch.float32) -> torch.Tensor:
    """[nlat]: 1 / w_k of the Clenshaw-Curtis weights (all positive), divided in fp64 and rounded once; cached like device_table"""
    device = torch.device(device)
    key = (nlat, device.type, device.index, dtype)
    t = _RWEIGHTS.get(key)
    if t is None:
        t = _RWEIGHTS[key] = torch.from_numpy(1.0 / clenshaw_curtis_weights(nlat)).to(device=device, dtype=dtype).contiguous()
    return t


def longitude_transform(x: torch.Tensor) -> torch.Tensor:
    """[..., nlat, nlon] fp32 of any strides (the rfft reads a channel-block view in place) -> [planes, nlat, mmax, 2] fp32: the real view of
    rfft(x, norm="forward"), planes = the leading dimensions flattened (the rfft has nlon // 2 + 1 = mmax outputs: nothing is cut)"""
    F = torch.view_as_real(torch.fft.rfft(x, dim=-1, norm="forward"))
    return F.reshape(-1, F.shape[-3], F.shape[-2], 2)


def spectral_operand(x: torch.Tensor) -> torch.Tensor:
    """[..., nlat, nlon] fp32 -> the kernels' operand [mmax, 2 planes, nlat] (column 2 p: real part of plane p, 2 p + 1: imaginary) =
    2 pi rfft(x), moved by swv2_sht_repack"""
    from .. import ops
    F = longitude_transform(x)
    return ops.sht_repack(F, F.shape[0], F.shape[1], F.shape[2], 2.0 * math.pi)


class _DegreePower(torch.autograd.Function):
    """power [planes, lmax] of F = rfft(x) as longitude_transform leaves it: swv2_sht_repack (times 2 pi) and swv2_sht_power; backward
    swv2_sht_adjoint and the repack the other way.  Keeps the coefficients only when a gradient can be asked for."""

    @staticmethod
    def forward(ctx, F, table):
        from .. import ops
        planes, nlat, mmax, _ = F.shape
        keep = F.requires_grad
        power, coef = ops.sht_power(table, ops.sht_repack(F, planes, nlat, mmax, 2.0 * math.pi), keep_coeffs=keep)
        if keep:
            ctx.save_for_backward(table, coef)
        return power

    @staticmethod
    def backward(ctx, g):
        from .. import ops
        table, coef = ctx.saved_tensors
        mmax, lmax, nlat = table.shape
        dX = ops.sht_adjoint(table, coef, g.contiguous().float())
        return ops.sht_repack(dX, dX.shape[1] // 2, nlat, mmax, 2.0 * math.pi, backward=True), None


def on_kernels(x: torch.Tensor) -> bool:
    """fp32 CUDA tensors with contiguous planes (a contiguous tensor, or a channel-block view of one) of at least 2 x 2 points"""
    return (x.is_cuda and x.dtype == torch.float32 and x.dim() >= 2 and x.numel() > 0 and x.shape[-2] >= 2 and x.shape[-1] >= 2 and
            x.stride(-1) == 1 and x.stride(-2) == x.shape[-1])


def degree_power(x: torch.Tensor) -> torch.Tensor:
    """[..., nlat, nlon] -> [..., lmax = nlat]: the degree power of every plane.  fp32 CUDA tensors with contiguous planes run on
    csrc/sht.hip (a failure there raises: nothing falls back); every other tensor takes degree_power_torch in its own dtype on its own
    device."""
    nlat, nlon = x.shape[-2:]
    if not on_kernels(x):
        return degree_power_torch(x, device_table(nlat, nlon, x.device, x.dtype if x.dtype.is_floating_point else torch.float32))
    table = device_table(nlat, nlon, x.device)
    return _DegreePower.apply(longitude_transform(x), table).reshape(x.shape[:-2] + (nlat,))


# ---- two fields degree by degree: cross spectrum, coherence -----------------------------------------------------------------------------
def cross_power_torch(a: torch.Tensor, b: torch.Tensor, table: torch.Tensor):
    """a, b [..., nlat, nlon] -> (P_aa, P_bb, C_ab), each [..., lmax]: the degree powers of both and the cross spectrum
    C_ab[l] = Re(c_a[l, 0] conj(c_b[l, 0])) + 2 sum_{m >= 1} Re(c_a[l, m] conj(c_b[l, m])), every m >= 1 doubled as in degree_power_torch"""
    ca, cb = torch.view_as_real(real_sht_torch(a, table)), torch.view_as_real(real_sht_torch(b, table))

    def summed(t):
        return t[..., :, 0] + 2 * torch.sum(t[..., :, 1:], dim=-1)

    return (summed(ca[..., 0] ** 2 + ca[..., 1] ** 2), summed(cb[..., 0] ** 2 + cb[..., 1] ** 2),
            summed(ca[..., 0] * cb[..., 0] + ca[..., 1] * cb[..., 1]))


class _CrossPower(torch.autograd.Function):
    """spectra [3, pairs, lmax] of F = rfft of the pair stacked as [pairs, 2, nlat, nlon], as longitude_transform leaves it (planes a_0,
    b_0, a_1, ...): swv2_sht_repack (times 2 pi) and swv2_sht_cross_power; backward swv2_sht_cross_adjoint and the repack the other way.
    Keeps the coefficients only when a gradient can be asked for.  As with _DegreePower autograd itself carries the gradient back
    through the rfft and the stack, so an input that needs no gradient gets none."""

    @staticmethod
    def forward(ctx, F, table):
        from .. import ops
        planes, nlat, mmax, _ = F.shape
        keep = F.requires_grad
        spectra, coef = ops.sht_cross_power(table, ops.sht_repack(F, planes, nlat, mmax, 2.0 * math.pi), keep_coeffs=keep)
        if keep:
            ctx.save_for_backward(table, coef)
        return spectra

    @staticmethod
    def backward(ctx, g):
        from .. import ops
        table, coef = ctx.saved_tensors
        mmax, lmax, nlat = table.shape
        dX = ops.sht_cross_adjoint(table, coef, g.contiguous().float())
        return ops.sht_repack(dX, dX.shape[1] // 2, nlat, mmax, 2.0 * math.pi, backward=True), None


def cross_power(a: torch.Tensor, b: torch.Tensor):
    """a, b [..., nlat, nlon] of one shape -> (P_aa, P_bb, C_ab), each [..., lmax = nlat].  Two fp32 CUDA tensors with contiguous planes on
    one device (at most 32767 planes each) run on csrc/sht.hip: the pair stacked, one rfft, one autograd node over swv2_sht_cross_power (a
    failure there raises: nothing falls back); everything else takes cross_power_torch in a's dtype on a's device."""
    if a.shape != b.shape:
        raise ValueError(f"cross_power: {tuple(a.shape)} against {tuple(b.shape)}")
    nlat, nlon = a.shape[-2:]
    if not (on_kernels(a) and on_kernels(b) and a.device == b.device):
        return cross_power_torch(a, b.to(device=a.device, dtype=a.dtype), device_table(nlat, nlon, a.device, _float_dtype(a)))
    table = device_table(nlat, nlon, a.device)
    pair = torch.stack((a, b), dim=-3)                       # [..., 2, nlat, nlon]: the one copy; views are read where they lie
    s = _CrossPower.apply(longitude_transform(pair), table)
    lead = a.shape[:-2] + (nlat,)
    return s[0].reshape(lead), s[1].reshape(lead), s[2].reshape(lead)


def spectral_coherence(P_aa: torch.Tensor, P_bb: torch.Tensor, C_ab: torch.Tensor) -> torch.Tensor:
    """C_ab / sqrt(P_aa P_bb) in fp64: the anomaly correlation of every degree.  NaN where P_aa P_bb == 0; not clamped (rounding may
    carry a value past +-1 by an ulp or so, and it is reported as it is)"""
    den = P_aa.double() * P_bb.double()
    return torch.where(den == 0, torch.full_like(den, float("nan")), C_ab.double() / torch.sqrt(den))


def coherence_scale(coh: torch.Tensor, level: float = 0.5) -> torch.Tensor:
    """coh [..., lmax] -> int64 [...]: the largest L >= 1 with coh[l] >= level for every 1 <= l <= L (the effective resolution, in
    degrees of the expansion); 0 when coh[1] already fails.  A NaN counts as failing; degree 0 (the mean) is not looked at."""
    ok = (coh[..., 1:] >= level).to(torch.int64)             # (NaN >= level is False)
    return torch.cumprod(ok, dim=-1).sum(dim=-1)

# ---- the way back: synthesis, filter, correlated noise ----------------------------------------------------------------------------------
EARTH_RADIUS_KM = 6371.0


def inverse_real_sht_torch(c: torch.Tensor, table: torch.Tensor, rweights: torch.Tensor, nlon: int) -> torch.Tensor:
    """complex c [..., lmax, mmax], table [mmax, lmax, nlat], rweights [nlat] = 1 / w_k -> real x [..., nlat, nlon]"""
    S = torch.einsum("mlk,...lm->...km", (table * rweights).to(c.dtype), c)
    return torch.fft.irfft(S, n=nlon, dim=-1, norm="forward")


def _plain(t: torch.Tensor) -> bool:
    return not (t.requires_grad and torch.is_grad_enabled())


def _float_dtype(t: torch.Tensor):
    return t.dtype if t.dtype.is_floating_point else torch.float32


def _field_of(S: torch.Tensor, lead, nlon: int) -> torch.Tensor:
    """S [mmax, 2 planes, nlat] in the operand layout -> the field [*lead, nlat, nlon]: the repack the other way and irfft"""
    from .. import ops
    mmax, N, nlat = S.shape
    F = torch.view_as_complex(ops.sht_repack(S, N // 2, nlat, mmax, 1.0, backward=True))
    return torch.fft.irfft(F, n=nlon, dim=-1, norm="forward").reshape(tuple(lead) + (nlat, nlon))


def inverse_real_sht(c: torch.Tensor, nlon: int) -> torch.Tensor:
    """complex c [..., lmax = nlat, mmax = nlon // 2 + 1] -> x [..., nlat, nlon], the inverse convention of real_sht.  Entries l < m
    count as zeros, the imaginary parts at m = 0 and (nlon even) m = nlon / 2 as irfft counts them: not at all.  complex64 CUDA tensors
    that are contiguous and need no gradient run swv2_sht_repack (view_as_real(c) has the rfft's layout with lmax for nlat),
    swv2_sht_synth, the repack back and torch's irfft; everything else inverse_real_sht_torch."""
    nlat, mmax = c.shape[-2:]
    if mmax != nlon // 2 + 1:
        raise ValueError(f"inverse_real_sht: {mmax} orders for nlon = {nlon} (mmax = nlon // 2 + 1)")
    planes = c.numel() // max(nlat * mmax, 1)
    if not (c.is_cuda and c.dtype == torch.complex64 and c.is_contiguous() and _plain(c) and nlat >= 2 and nlon >= 2 and 0 < planes <= 65535):
        real = torch.float64 if c.dtype == torch.complex128 else torch.float32
        return inverse_real_sht_torch(c, device_table(nlat, nlon, c.device, real), inverse_weights(nlat, c.device, real), nlon)
    from .. import ops
    coef = ops.sht_repack(torch.view_as_real(c), planes, nlat, mmax, 1.0)
    S = ops.sht_synth(device_table(nlat, nlon, c.device), inverse_weights(nlat, c.device), coef, nlon=nlon)
    return _field_of(S, c.shape[:-2], nlon)


def _kernel_field(x: torch.Tensor) -> bool:
    return on_kernels(x) and _plain(x) and x.numel() // (x.shape[-2] * x.shape[-1]) <= 65535


def real_sht(x: torch.Tensor) -> torch.Tensor:
    """x [..., nlat, nlon] -> complex c [..., lmax, mmax], zeros for l < m.  On the kernels: rfft, repack, swv2_sht_power into a zeroed
    coefficient buffer, the repack back; else real_sht_torch."""
    nlat, nlon = x.shape[-2:]
    if not _kernel_field(x):
        return real_sht_torch(x, device_table(nlat, nlon, x.device, _float_dtype(x)))
    from .. import ops
    table = device_table(nlat, nlon, x.device)
    X = spectral_operand(x)
    _, coef = ops.sht_power(table, X, keep_coeffs=True, zero_coeffs=True)
    c = ops.sht_repack(coef, X.shape[1] // 2, nlat, table.shape[0], 1.0, backward=True)          # lmax = nlat: the same kernel serves
    return torch.view_as_complex(c).reshape(x.shape[:-2] + (nlat, table.shape[0]))


def spectral_filter_torch(x: torch.Tensor, response: torch.Tensor, table: torch.Tensor, rweights: torch.Tensor) -> torch.Tensor:
    c = real_sht_torch(x, table)
    return inverse_real_sht_torch(response.to(table.dtype).unsqueeze(-1) * c, table, rweights, x.shape[-1])


def spectral_filter(x: torch.Tensor, response: torch.Tensor) -> torch.Tensor:
    """inverse_real_sht(response * real_sht(x)): x [..., nlat, nlon], response [lmax] or one per plane [..., lmax].  On the kernels the data
    stay in their layouts: rfft, repack, swv2_sht_power keeping the coefficients, swv2_sht_synth with the response, the repack back, irfft.
    With lmax = nlat a response of ones is not the identity map (the module's docstring)."""
    nlat, nlon = x.shape[-2:]
    if response.shape[-1] != nlat or (response.dim() > 1 and response.shape[:-1] != x.shape[:-2]):
        raise ValueError(f"spectral_filter: response {tuple(response.shape)} for a field {tuple(x.shape)} (lmax = nlat)")
    response = response.to(x.device)
    if not (_kernel_field(x) and _plain(response)):
        dt = _float_dtype(x)
        return spectral_filter_torch(x, response, device_table(nlat, nlon, x.device, dt), inverse_weights(nlat, x.device, dt))
    from .. import ops
    table = device_table(nlat, nlon, x.device)
    _, coef = ops.sht_power(table, spectral_operand(x), keep_coeffs=True)
    h = response.float().reshape((-1, nlat) if response.dim() > 1 else (nlat,)).contiguous()
    S = ops.sht_synth(table, inverse_weights(nlat, x.device), coef, h, nlon=nlon)
    return _field_of(S, x.shape[:-2], nlon)


def spectral_truncate(x: torch.Tensor, lcut: int) -> torch.Tensor:
    """spectral_filter with the response 1[l <= lcut]"""
    h = (torch.arange(x.shape[-2], device=x.device) <= lcut).to(_float_dtype(x))
    return spectral_filter(x, h)


def gaussian_noise_spectrum(nlat: int, nlon: int, length_scale_km: float, zero_mean: bool = True) -> np.ndarray:
    """fp64 sigma_l [lmax] of isotropic Gaussian-correlated noise on the sphere: sigma_l^2 ~ exp(-l (l + 1) (length / a)^2 / 2), a = 6371 km,
    on the degrees 1 (0 without zero_mean) .. min(lmax - 1, (nlon - 1) // 2), zero elsewhere, scaled to sum_l sigma_l^2 (2 l + 1) / (4 pi) = 1:
    unit variance at every point, by the addition theorem"""
    if not length_scale_km > 0:
        raise ValueError(f"gaussian_noise_spectrum: length scale {length_scale_km} km")
    l = np.arange(nlat, dtype=np.float64)
    top = min(nlat - 1, (nlon - 1) // 2)
    keep = (l >= (1 if zero_mean else 0)) & (l <= top)
    if not keep.any():
        raise ValueError(f"gaussian_noise_spectrum: the grid {nlat} x {nlon} resolves no degree to put the noise on")
    e = -0.5 * l * (l + 1.0) * (length_scale_km / EARTH_RADIUS_KM) ** 2
    s2 = np.where(keep, np.exp(e - e[keep].max()), 0.0)          # (the largest term is 1: no underflow of the whole spectrum)
    return np.sqrt(s2 / np.sum(s2 * (2.0 * l + 1.0) / (4.0 * math.pi)))


def _noise_sigma(sigma, lmax: int, nlon: int) -> np.ndarray:
    s = np.asarray(sigma.detach().cpu() if isinstance(sigma, torch.Tensor) else sigma, dtype=np.float64)
    if s.shape != (lmax,):
        raise ValueError(f"spherical_noise: sigma {s.shape} for lmax = {lmax}")
    if np.any(s[(nlon - 1) // 2 + 1:] != 0.0):
        raise ValueError(f"spherical_noise: sigma_l is non-zero beyond l = {(nlon - 1) // 2}, the orders nlon = {nlon} points carry without aliasing")
    return s


def spherical_noise_torch(z: torch.Tensor, sigma: torch.Tensor, table: torch.Tensor, rweights: torch.Tensor, nlon: int) -> torch.Tensor:
    """the statement of spherical_noise: z [mmax, 2 planes, lmax] -> [planes, nlat, nlon] under table [mmax, lmax, nlat]"""
    mmax, N, lmax = z.shape
    f = torch.full((mmax,), math.sqrt(0.5), dtype=table.dtype, device=z.device)
    f[0] = 1.0
    zc = z.to(table.dtype).reshape(mmax, N // 2, 2, lmax)
    im_ok = torch.ones(mmax, dtype=torch.bool, device=z.device)
    im_ok[0] = False
    if nlon % 2 == 0 and nlon // 2 < mmax:
        im_ok[nlon // 2] = False
    im = torch.where(im_ok[:, None, None], zc[:, :, 1], torch.zeros_like(zc[:, :, 1]))
    c = torch.complex(zc[:, :, 0], im) * (f[:, None, None] * sigma.to(table.dtype)[None, None, :])
    tri = torch.arange(lmax, device=z.device)[None, :] >= torch.arange(mmax, device=z.device)[:, None]
    c = torch.where(tri[:, None, :], c, torch.zeros_like(c))                                             # l < m: not part of the draw's use
    return inverse_real_sht_torch(c.permute(1, 2, 0), table, rweights, nlon)


def _spherical_noise(z, sig, nlon):
    """spherical_noise with sigma [lmax] already checked and on z's device in fp32"""
    mmax, N, lmax = z.shape
    if not (z.is_cuda and z.dtype == torch.float32 and z.is_contiguous() and _plain(z) and lmax >= 2 and nlon >= 2 and 0 < N // 2 <= 65535):
        dt = _float_dtype(z)
        return spherical_noise_torch(z, sig, device_table(lmax, nlon, z.device, dt), inverse_weights(lmax, z.device, dt), nlon)
    from .. import ops
    S = ops.sht_synth(device_table(lmax, nlon, z.device), inverse_weights(lmax, z.device), z, sig, scales=(1.0, math.sqrt(0.5)), nlon=nlon)
    return _field_of(S, (N // 2,), nlon)


def spherical_noise(z: torch.Tensor, sigma, nlon: int) -> torch.Tensor:
    """z [mmax, 2 planes, lmax = nlat] standard normals in the coefficient layout, sigma [lmax] (gaussian_noise_spectrum) ->
    [planes, nlat, nlon]: the real field with coefficients c_l0 = sigma_l z_re (variance sigma_l^2) and c_lm = sigma_l (z_re + i z_im) / sqrt 2
    (sigma_l^2 / 2 each part); entries l < m of z are not used.  Its variance at every point is sum_l sigma_l^2 (2 l + 1) / (4 pi).
    On the kernels: swv2_sht_synth with the response sigma and the scales (1, sqrt 1/2), the repack back, irfft."""
    if z.dim() != 3 or z.shape[1] % 2 or z.shape[0] != nlon // 2 + 1:
        raise ValueError(f"spherical_noise: z {tuple(z.shape)} is not [mmax = {nlon // 2 + 1}, 2 planes, lmax]")
    s = _noise_sigma(sigma, z.shape[2], nlon)
    return _spherical_noise(z, torch.from_numpy(s).to(device=z.device, dtype=_float_dtype(z)), nlon)
