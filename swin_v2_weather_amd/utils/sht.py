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
