"""LossHandler with the reference's surface and semantics (utils/losses.py:30-232) on the fused quadrature kernels.

The O(B*C*H*W) work -- the latitude-weighted sums of (prd - tar)^2 and tar^2 per (sample, channel) plane and the
gradient d loss / d prd -- is two HIP entry points (swv2_loss_sums / swv2_loss_grad, csrc/loss_l2.hip); the remaining arithmetic is on
[B, C] tensors.  Supported: the 'l2' family used by every entry of config/swin.yaml ('l2', 'squared geometric l2',
'weighted absolute|relative temp-std squared geometric l2') and the 'l1' family (every string with the word l1 and
without l2: losses.py:114-120 builds the same class with p = 1).

l1: S0 = sum q[h] |prd - tar|, S1 = sum q[h] |tar| per plane, loss = sum_bc chw[c] (S0 or S0 / S1).  The reference never
forwards `squared` for p = 1 and x ** (1 / 1) is the identity, so 'l1', 'geometric l1' and 'squared geometric l1' are one
number; the word `squared` still squares the temp-std channel factor.  `geometric_l1_torch` is the readable definition
(any device, any dtype, differentiable by autograd); on CUDA fp32 tensors with W % 4 == 0 value and gradient come from
one autograd node over swv2_l1_sums / swv2_l1_finalize / swv2_l1_grad (csrc/loss_l1.hip), in training, validation and
rollouts alike.  The head epilogue evaluates squared residuals, so `fused_with` is a no-op for l1.

Quadrature: the 'naive' rule, or Gauss-Legendre rows (utils/grids.py) when model_grid_type is 'legendre_gauss' and the
string contains `geometric` (losses.py:102-120), for l1 and l2 alike: the kernels take per-row weights.
pole-masked (an undefined name in the reference) raises, and so do the geometric h1 strings of LossHandler; the class behind them,
GeometricH1Loss, is here on its own (utils/sht.py, csrc/sht.hip).

amse: every string with the word amse and neither l2 nor l1 (those two keep their priority, as in the reference's if / elif) is the
adjusted spectral MSE, GeometricAMSELoss below, per (sample, channel): loss = sum_bc chw[c] value[b, c] with the channel weights, the
temp-std factor and the multistep weight of the l1 family.  `fused_with` is a no-op for it as for l1.
"""
import math

import os

import numpy as np
import torch
from torch import nn

from .. import ops
from .grids import legendre_gauss_quadrature_weights, naive_quadrature_weights


def geometric_l1_torch(prd, tar, quad_rows, chw, absolute):
    """The geometric l1 loss in plain torch (losses.py:188-240 with p = 1): prd, tar [B, C, H, W], quad_rows [H] normalised row
    weights, chw [C] (or [1, C]) channel weights -> sum_bc chw[c] S0[b, c] (absolute) or chw[c] S0[b, c] / S1[b, c], with
    S0 = sum_hw q[h] |prd - tar| and S1 = sum_hw q[h] |tar|.  In the inputs' dtype, on their device."""
    q = quad_rows.to(device=prd.device, dtype=prd.dtype).reshape(1, 1, -1, 1)
    B = prd.shape[0]
    norms = torch.sum(torch.abs(prd - tar) * q, dim=(-2, -1)).reshape(B, -1)
    if not absolute:
        norms = norms / torch.sum(torch.abs(tar) * q, dim=(-2, -1)).reshape(B, -1)
    return torch.sum(chw.to(device=prd.device, dtype=prd.dtype).reshape(1, -1) * norms)


class GeometricH1Loss(nn.Module):
    """The weighted H1 loss on the sphere (reference utils/losses.py:244-338): with P[b, c, l] the degree power of prd - tar
    (utils/sht.py::degree_power; HIP kernels on contiguous fp32 CUDA tensors), per sample

        l2 = sum_{c, l} P          h1 = sum_{c, l} l (l + 1) P
        norm = alpha sqrt(l2) + (1 - alpha) sqrt(h1)        (squared: alpha l2 + (1 - alpha) h1)

    absolute: the norms [B]; relative: divided by the same norm of tar, then times `mask` when one is given.  reduction sums (or, with
    size_average, averages: the mean, or sum / sum(mask) in the relative form with a mask) over what is left; reduction=False returns
    it.  `p` is accepted and unused, and the absolute form ignores `mask`, both as in the reference.  Everything after the degree
    power is torch on [B, C, lmax]; `retval * mask` broadcasts or fails exactly as torch does for the reference.

    LossHandler does not build this class: its 'geometric h1' strings raise.  The reference's dispatch hands the channel weights
    [1, C] to `mask`, and the relative form then multiplies [B] by [1, C], which torch rejects unless B is 1 or C (and mis-weights when
    it does not reject).  The transform is pinned by its definition, not compared with torch_harmonics (utils/sht.py)."""

    def __init__(self, img_shape, p=2., size_average=False, reduction=True, absolute=False, squared=False, alpha=0.5):
        super().__init__()
        self.img_shape = tuple(img_shape)
        self.reduction, self.size_average, self.absolute, self.squared, self.alpha = reduction, size_average, absolute, squared, alpha
        h1_weights = torch.arange(self.img_shape[0]).float()                  # lmax = nlat
        self.register_buffer("h1_weights", h1_weights * (h1_weights + 1))

    def _norms(self, field):
        from .sht import degree_power
        if tuple(field.shape[-2:]) != self.img_shape:
            raise ValueError(f"GeometricH1Loss for a {self.img_shape} grid got a field of {tuple(field.shape[-2:])}")
        num_examples = field.size()[0]
        norm2 = degree_power(field)
        l2_norm2 = norm2.reshape(num_examples, -1).sum(dim=-1)
        h1_norm2 = (norm2 * self.h1_weights.to(norm2.dtype)).reshape(num_examples, -1).sum(dim=-1)
        if not self.squared:
            return self.alpha * torch.sqrt(l2_norm2) + (1 - self.alpha) * torch.sqrt(h1_norm2)
        return self.alpha * l2_norm2 + (1 - self.alpha) * h1_norm2

    def abs(self, prd, tar):
        all_norms = self._norms(prd - tar)
        if self.reduction:
            return torch.mean(all_norms) if self.size_average else torch.sum(all_norms)
        return all_norms

    def rel(self, prd, tar, mask=None):
        retval = self._norms(prd - tar) / self._norms(tar)
        if mask is not None:
            retval = retval * mask
        if self.reduction:
            if self.size_average:
                retval = torch.mean(retval) if mask is None else torch.sum(retval) / torch.sum(mask)
            else:
                retval = torch.sum(retval)
        return retval

    def forward(self, prd, tar, mask=None):
        return self.abs(prd, tar) if self.absolute else self.rel(prd, tar, mask)


def amse_from_spectra(Px, Py, C, absolute=False):
    """[..., lmax] degree powers of forecast and target and their cross spectrum -> [...]: the adjusted spectral MSE

        A = sum_l [ (sqrt Px - sqrt Py)^2 + 2 max(Px, Py) (1 - C / sqrt(Px Py)) ]        (a degree with Px Py == 0: Px + Py - 2 C)

    or, relative, A / sum_l Py.  Plain torch in the inputs' dtype; autograd differentiates it (the masked degrees are taken out before
    the square roots, so no 0 * inf reaches a gradient)."""
    zero = (Px * Py) == 0
    one = torch.ones_like(Px)
    px, py = torch.where(zero, one, Px), torch.where(zero, one, Py)
    amp = (torch.sqrt(px) - torch.sqrt(py)) ** 2
    coh = 2 * torch.maximum(px, py) * (1 - C / torch.sqrt(px * py))
    A = torch.where(zero, Px + Py - 2 * C, amp + coh).sum(dim=-1)
    return A if absolute else A / Py.sum(dim=-1)


class GeometricAMSELoss(nn.Module):
    """The adjusted spectral MSE on the sphere (Subich et al. 2025, "Fixing the double penalty in data-driven weather forecasting through
    a modified spherical harmonic loss function"), per (sample, channel) plane: with P_x, P_y [b, c, l] the degree powers of prd and tar
    and C their cross spectrum (utils/sht.py::cross_power; HIP kernels on fp32 CUDA tensors with contiguous planes),

        A = sum_l [ (sqrt P_x - sqrt P_y)^2 + 2 max(P_x, P_y) (1 - C / sqrt(P_x P_y)) ]   (a degree with P_x P_y == 0: P_x + P_y - 2 C)
        value[b, c] = A (absolute)   or   A / sum_l P_y[l] (relative)

    The spectral MSE of a degree, P_x + P_y - 2 C, split into an amplitude term and a coherence term, the latter weighted by the larger
    of the two powers and not by their geometric mean: a forecast is no longer rewarded for losing small-scale power.  forward returns
    [B, C]; everything after cross_power is torch on [B, C, lmax].

    Written from the paper's formula: the authors' code is not available to this project, so nothing here was compared with it.  The
    loss is pinned by its identities (tests/test_cross_host.py): AMSE(x, x) = 0; AMSE(x, s x) = (1 - s)^2 sum P_x for s > 0; with max
    replaced by sqrt(P_x P_y) it is sum degree_power(x - y), the spectral MSE, which it never falls below; and it equals it when P_x = P_y."""

    def __init__(self, img_shape, absolute=False):
        super().__init__()
        self.img_shape = tuple(img_shape)
        self.absolute = absolute

    def forward(self, prd, tar):
        from .sht import cross_power
        if tuple(prd.shape[-2:]) != self.img_shape or prd.shape != tar.shape:
            raise ValueError(f"GeometricAMSELoss for a {self.img_shape} grid got fields of {tuple(prd.shape)} and {tuple(tar.shape)}")
        Px, Py, C = cross_power(prd, tar)
        return amse_from_spectra(Px, Py, C, self.absolute)


class _GeoL1(torch.autograd.Function):
    """The l1 LossHandler value as one node: l1_sums (one pass over prd / tar), l1_finalize (the slices, the [B, C] arithmetic and
    the backward coefficients), and in backward one l1_grad pass.  `ws`: the caller's workspace for this shape."""

    @staticmethod
    def forward(ctx, prd, tar, qw, chw, absolute, ws):
        prd, tar = prd.contiguous(), tar.contiguous()
        B, C, H, W = prd.shape
        ops.l1_sums(prd, tar, qw, ws)
        _, loss, coef = ops.l1_finalize(ws, B, C, H, W, chw, absolute)
        ctx.save_for_backward(prd, tar, qw, coef)
        return loss.view(())

    @staticmethod
    def backward(ctx, gout):
        prd, tar, qw, coef = ctx.saved_tensors
        dprd = torch.empty_like(prd)
        ops.l1_grad(prd, tar, qw, (coef * gout).contiguous(), dprd)
        return dprd, None, None, None, None, None


class _QuadSums(torch.autograd.Function):
    """sums[b, c] = (sum_hw q[h] (prd - tar)^2, sum_hw q[h] tar^2); backward: dprd = 2 dS0[b,c] q[h] (prd - tar).  `ws`: the
    caller's workspace for this shape (ops.loss_workspace), or None"""

    @staticmethod
    def forward(ctx, prd, tar, qw, ws=None):
        prd, tar = prd.contiguous().float(), tar.contiguous().float()
        B, C = prd.shape[:2]
        sums = torch.empty(B, C, 2, dtype=torch.float32, device=prd.device)
        ops.loss_sums(prd, tar, qw, sums, ws)
        ctx.save_for_backward(prd, tar, qw)
        return sums

    @staticmethod
    def backward(ctx, dsums):
        prd, tar, qw = ctx.saved_tensors
        coef = (2.0 * dsums[..., 0]).contiguous().float()
        dprd = torch.empty_like(prd)
        ops.loss_grad(prd, tar, qw, coef, dprd)
        return dprd, None, None, None


class _GeoL2(torch.autograd.Function):
    """The whole LossHandler value as one node: loss_sums (one pass over prd / tar), loss_finalize (the [B, C] arithmetic +
    the backward coefficients), and in backward one loss_grad pass.  Same value and gradient as _QuadSums + torch ops.  `ws` as
    for _QuadSums."""

    @staticmethod
    def forward(ctx, prd, tar, qw, chw, absolute, squared, ws=None):
        prd, tar = prd.contiguous().float(), tar.contiguous().float()
        B, C = prd.shape[:2]
        buf = torch.empty(B * C * 3 + 1, dtype=torch.float32, device=prd.device)      # sums | coef | loss: one allocation, all written
        sums, coef, loss = buf[:B * C * 2].view(B, C, 2), buf[B * C * 2:B * C * 3], buf[B * C * 3:]
        ops.loss_sums(prd, tar, qw, sums, ws)
        ops.loss_finalize(sums, chw, absolute, squared, loss, coef)
        ctx.save_for_backward(prd, tar, qw, coef)
        return loss.view(())

    @staticmethod
    def backward(ctx, gout):
        prd, tar, qw, coef = ctx.saved_tensors
        dprd = torch.empty_like(prd)
        ops.loss_grad(prd, tar, qw, (coef * gout).contiguous(), dprd)
        return dprd, None, None, None, None, None, None


class _FusedGeoL2(torch.autograd.Function):
    """LossHandler value from the quadrature sums the head's un-patchify epilogue produced (SWV2_EPI_UNPATCH_LOSS): one
    loss_finalize launch; backward hands d loss / d sums[..., 0] to the head's backward, which scales the stored residual."""

    @staticmethod
    def forward(ctx, sums, chw, absolute, squared):
        loss, coef = ops.loss_finalize_sums(sums, chw, absolute, squared)
        ctx.layers = sums.shape[0]
        ctx.save_for_backward(coef)
        return loss.view(())

    @staticmethod
    def backward(ctx, gout):
        (coef,) = ctx.saved_tensors
        ds = torch.zeros((ctx.layers,) + tuple(coef.shape) + (2,), dtype=torch.float32, device=coef.device)
        ds[..., 0] = 0.5 * gout * coef               # coef = 2 d loss / d S0 (every layer of the sums alike); the relative
        return ds, None, None, None                  # losses' d / d S1 has no consumer (the target needs no gradient)


class _LossCtx:
    """one forward's hand-over between LossHandler.fused_with and the model head"""

    def __init__(self, tar, qw):
        self.tar, self.qw, self.y, self.sums = tar, qw, None, None

    def fits(self, x, net):
        t = self.tar
        return (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and not t.requires_grad and t.dim() == 4 and
                t.shape[0] == x.shape[0] and t.shape[1] == net.out_chans and tuple(t.shape[2:]) == tuple(x.shape[2:]) and
                self.qw.numel() == t.shape[2] and t.shape[3] % 4 == 0 and (t.shape[2] // 4) * (t.shape[3] // 4) >= 32 and
                t.numel() < 2 ** 32 and x.numel() < 2 ** 32)

    def offer(self, y, sums):
        self.y, self.sums = y, sums

    # rollouts (MultiStepWrapper): every step's head offers the sums of its Cout channels of the concatenated prediction
    def fits_step(self, x, net, result, coff):
        t = self.tar
        return (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and not t.requires_grad and t.dim() == 4 and
                t.shape[0] == x.shape[0] and t.shape[1] == result.shape[1] and coff + net.out_chans <= t.shape[1] and
                tuple(t.shape[2:]) == tuple(x.shape[2:]) and self.qw.numel() == t.shape[2] and t.shape[3] % 4 == 0 and
                (t.shape[2] // 4) * (t.shape[3] // 4) >= 32 and t.numel() < 2 ** 32 - 1024 and x.numel() < 2 ** 32 - 1024 and
                # what the fused rollout path itself needs (else the two-pass loss, as before -- ADVICE r5): the dump offset is a C int,
                # swv2_loss_resid_to_image stages 16 rows of Cout * 16 (+ 8) bf16 in 64 KB of LDS, and the concatenated prediction must
                # carry the epilogue's scratch behind it
                result.numel() < 2 ** 31 - 1024 and 16 * (net.out_chans * 16 + 8) * 2 <= 65536 and self._slack_behind(result) >= ops.L.LOSS_DUMP_BYTES)

    @staticmethod
    def _slack_behind(t):
        """allocated bytes behind the last element of a (view of a) tensor"""
        base = t._base if t._base is not None else t
        return base.data_ptr() + base.numel() * base.element_size() - (t.data_ptr() + t.numel() * t.element_size())

    def offer_step(self, result, coff, sums):
        if self.steps is None or self.result_ptr != result.data_ptr():
            self.steps, self.result_ptr, self.result_shape = [], result.data_ptr(), tuple(result.shape)
        self.steps.append((coff, sums))

    steps, result_ptr, result_shape = None, None, None

    def rollout_sums(self, prd, n_out):
        """[SLICES, B, S * Cout, 2] if every channel block of `prd` (the rollout's concatenated prediction) was offered, else None"""
        if not self.steps or prd.data_ptr() != self.result_ptr or tuple(prd.shape) != self.result_shape:
            return None
        steps = sorted(self.steps, key=lambda cs: cs[0])
        if [c for c, _ in steps] != list(range(0, prd.shape[1], n_out)) or any(s.shape[2] != n_out for _, s in steps):
            return None
        return torch.cat([s for _, s in steps], dim=2)


def _core_net(model):
    """the SwinTransformerV2Cr under DDP (`.module`) and the step wrappers (`.model`)"""
    m, seen = model, 0
    while seen < 4 and not hasattr(m, "_features_bhwc"):
        m = getattr(m, "module", None) or getattr(m, "model", None)
        if m is None:
            return None
        seen += 1
    return m if hasattr(m, "_features_bhwc") else None


def auto_channel_weights(channel_names, n_out):
    """losses.py:57-68"""
    w = torch.ones(n_out, dtype=torch.float32)
    for c, chn in enumerate(channel_names):
        if chn in ['u10m', 'v10m', 'u100m', 'v100m', 'tp', 'sp', 'msl', 'tcwv']:
            w[c] = 0.1
        elif chn in ['t2m', '2d']:
            w[c] = 1.0
        elif chn[0] in ['z', 'u', 'v', 't', 'r', 'q']:
            w[c] = 0.001 * float(chn[1:])
        else:
            w[c] = 0.01
    return w


def load_stats(params):
    """(global_stds, time_diff_stds) as [1, N, 1, 1] float32 arrays (losses.py:91-92 loads them from params.*_path).
    Without the ERA5 statistics files (synthetic-data runs: no dataset in the image) the stand-ins of SURVEY.md 8(d) are
    used: unit global stds and a fixed, seeded positive vector of time-difference stds."""
    import os
    gp, tp = str(getattr(params, 'global_stds_path', '')), str(getattr(params, 'time_diff_stds_path', ''))
    if os.path.isfile(gp) and os.path.isfile(tp):
        return np.load(gp).astype(np.float32), np.load(tp).astype(np.float32)
    n = max(len(getattr(params, 'channel_names', [])), int(np.max(np.asarray(params.out_channels))) + 1)
    rng = np.random.RandomState(333)
    return np.ones((1, n, 1, 1), np.float32), (0.05 + 0.45 * rng.rand(1, n, 1, 1)).astype(np.float32)


class LossHandler(nn.Module):
    """Wrapper class that handles computing losses: `LossHandler(params)(prd, tar, inp)` (losses.py:30-150)."""

    def __init__(self, params):
        super().__init__()
        self.n_future = params.n_future
        self.img_shape = (params.img_shape_x, params.img_shape_y)
        self.loss_type = params.loss
        flags = set(params.loss.split())
        if 'pole-masked' in flags:
            raise ValueError("pole-masked losses hit an undefined name in the reference (grids.py:97-99)")
        if 'l2' in flags:                      # l2 wins when both words occur, as the reference's if / elif (losses.py:107-120)
            self.p = 2
        elif 'l1' in flags:
            self.p = 1
        elif 'amse' in flags:
            self.p = None                      # neither quadrature family: the spectral loss below
        else:
            raise ValueError(f"Unknown / unsupported loss function: {self.loss_type} (l2 and l1 families only)")
        if 'weighted' in flags:
            if params.channel_weights == 'auto':
                cw = auto_channel_weights(params.channel_names, params.n_out_channels)
            else:
                cw = torch.Tensor(params.channel_weights).float()
        else:
            cw = torch.ones(params.n_out_channels, dtype=torch.float32)
        cw = cw.reshape(1, -1, 1, 1)
        cw = cw / torch.sum(cw)
        self.absolute = 'absolute' in flags
        # plain 'l2' never forwards `squared` (losses.py:112-113), and is sphere-weighted all the same (quirk 9)
        self.squared = ('squared' in flags) and ('geometric' in flags)
        if 'temp-std' in flags:
            eps = 1e-6
            oc = np.asarray(params.out_channels)
            gs_np, td_np = load_stats(params)
            gstd = torch.from_numpy(gs_np).reshape(1, -1, 1, 1)[:, oc]
            tstd = np.sqrt(params.dt) * torch.from_numpy(td_np).reshape(1, -1, 1, 1)[:, oc]
            tvw = gstd / (tstd + eps)
            if 'squared' in flags:
                tvw = tvw ** 2
            cw = cw * tvw
        self.register_buffer('channel_weights', cw.float())
        # the non-geometric strings never forward the rule (losses.py:112-113, 119-120): naive rows whatever the grid
        rule = naive_quadrature_weights
        if getattr(params, 'model_grid_type', 'equiangular') == 'legendre_gauss' and 'geometric' in flags:
            rule = legendre_gauss_quadrature_weights
        self.register_buffer('quad_rows', rule(self.img_shape[0], self.img_shape[1], True).contiguous())
        self.amse = GeometricAMSELoss(self.img_shape, absolute=self.absolute) if self.p is None else None
        self._l1_ws = {}                       # (device, B, C) -> the l1 kernels' workspace of that shape, made once and reused
        self._l2_ws = {}                       # the same for swv2_loss_sums
        ms = torch.ones(self.n_future + 1, dtype=torch.float32) / float(self.n_future + 1)
        self.register_buffer('multistep_weight', ms.reshape(-1, 1, 1, 1))

    _fused = None

    def fused_with(self, model, tar: torch.Tensor):
        """`with loss_obj.fused_with(model, tar): gen = model(inp)` then `loss_obj(gen, tar, inp)` as usual: the model's head
        evaluates this loss's quadrature sums in the epilogue that writes `gen` and keeps the weighted residual for its own
        backward, so the prediction is not read back by the loss (2 passes) nor a gradient of its size written and re-read
        (losses.py:188-206 on the output of swinv2_global.py:784-802).  Purely an accelerator: same value, same gradients;
        when the shapes do not fit (rollouts, skip inputs that need gradients, eval) the two-pass kernels run instead."""
        import contextlib

        @contextlib.contextmanager
        def cm():
            # (l1, amse: the head epilogue evaluates squared residuals -- no hand-over, the two-pass l1 kernels / the spectral loss run)
            net = _core_net(model) if (self.p == 2 and self.training and os.environ.get("SWV2_LOSS_IN_HEAD", "1") != "0") else None
            # (rollouts: every step's head takes its channel block of the target; SWV2_LOSS_IN_HEAD_ROLLOUT=0 keeps the two-pass kernels)
            if net is None or (self.n_future != 0 and os.environ.get("SWV2_LOSS_IN_HEAD_ROLLOUT", "1") == "0"):
                yield
                return
            lc = _LossCtx(tar, self.quad_rows)
            net._loss_ctx, self._fused = lc, lc
            try:
                yield
            finally:
                net._loss_ctx = None
        return cm()

    def _chw_now(self):
        """[1, C (n_future + 1)] in training (the multistep weight per step), [1, C] in eval (losses.py:145-148)"""
        chw = self.channel_weights
        if self.training:
            return (chw * self.multistep_weight).reshape(1, -1)
        return chw.reshape(1, -1)

    def _forward_l1(self, prd, tar):
        chw = self._chw_now()
        on_kernels = (prd.is_cuda and tar.is_cuda and prd.device == tar.device == self.quad_rows.device and
                      prd.dtype == tar.dtype == torch.float32 and prd.dim() == 4 and prd.shape == tar.shape and
                      not tar.requires_grad and prd.shape[3] % 4 == 0 and prd.shape[2] == self.quad_rows.numel() and
                      chw.numel() == prd.shape[1] and prd.shape[0] * prd.shape[1] <= 65535 and prd.shape[2] * prd.shape[3] < 2 ** 30)
        if not on_kernels:
            return geometric_l1_torch(prd, tar, self.quad_rows, chw, self.absolute)
        return _GeoL1.apply(prd, tar, self.quad_rows, chw.reshape(-1).contiguous().float(), self.absolute,
                            self._workspace(self._l1_ws, ops.l1_workspace, prd))

    @staticmethod
    def _workspace(cache, make, prd):
        B, C, H, W = prd.shape
        key = (prd.device, B, C)
        if key not in cache:
            cache[key] = make(B * C, H, W, prd.device)
        return cache[key]

    def forward(self, prd: torch.Tensor, tar: torch.Tensor, inp: torch.Tensor = None):
        lc, self._fused = self._fused, None
        if self.p == 1:
            return self._forward_l1(prd, tar)
        if self.p is None:
            return torch.sum(self._chw_now().to(prd.dtype) * self.amse(prd, tar))
        rsums = None
        if lc is not None and lc.steps and lc.tar is tar and self.training and prd.dtype == torch.float32:
            rsums = lc.rollout_sums(prd, prd.shape[1] // (self.n_future + 1))
        if rsums is not None or (lc is not None and lc.y is not None and lc.tar is tar and self.training and
                                 (lc.y is prd or (prd.data_ptr() == lc.y.data_ptr() and prd.shape == lc.y.shape and prd.dtype == lc.y.dtype))):
            # (the product of two constant buffers: cached, one tiny launch per step less; re-made when a buffer moved or changed)
            key = (self.channel_weights.data_ptr(), self.channel_weights._version, self.multistep_weight.data_ptr(), self.multistep_weight._version)
            if getattr(self, "_chw_key", None) != key:
                self._chw_flat = (self.channel_weights * self.multistep_weight).reshape(-1).contiguous().float()
                self._chw_key = key
            return _FusedGeoL2.apply(lc.sums if rsums is None else rsums, self._chw_flat, self.absolute, self.squared)
        chw = self._chw_now()
        ws = self._workspace(self._l2_ws, ops.loss_workspace, prd)
        if prd.is_cuda and prd.requires_grad and not tar.requires_grad and os.environ.get("SWV2_LOSS_FUSED", "1") != "0":
            return _GeoL2.apply(prd, tar, self.quad_rows, chw.reshape(-1).contiguous().float(), self.absolute, self.squared, ws)
        sums = _QuadSums.apply(prd, tar, self.quad_rows, ws)
        norms = sums[..., 0]
        if not self.absolute:
            norms = norms / sums[..., 1]
        if not self.squared:
            norms = torch.sqrt(norms)
        return torch.sum(chw * norms)
