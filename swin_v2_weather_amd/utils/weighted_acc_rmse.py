"""Forecast verification: the reference's metric functions under their names (utils/weighted_acc_rmse.py there), ForecastScorer (RMSE /
ACC, MAE, top-quantile error, degree spectra, ensemble scores and events of channel blocks of wide tensors, read where they lie) and
RegriddedScorer (the same on a coarser grid: cut the blocks, regrid them, hand them to an inner ForecastScorer).

Blocks that ops.py's operand contract accepts (CUDA fp32, DESIGN "Blocks of planes read in place") go through the HIP kernels, one
streaming pass per score family; anything else -- CPU tensors (the host tests, the gloo trainer), odd widths, other dtypes -- runs the
plain-torch statement of the same sums.  Each view of the operands is cut and checked once: _channel_blocks and _member_blocks."""
import os
from collections import namedtuple

import numpy as np
import torch


def weighted_rmse_torch(pred: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    """[n, c, h, w] x2 -> [c]: mean over the batch of sqrt(mean_hw(w_lat (pred - target)^2)), with
    w_lat = num_lat cos(lat_j) / sum_j cos(lat_j), lat_j = 90 - 180 j / (num_lat - 1) degrees (pi ~ 3.1416 as there)."""
    num_lat = pred.shape[2]
    j = torch.arange(0, num_lat, device=pred.device)
    coslat = torch.cos(3.1416 / 180.0 * (90.0 - j * 180.0 / float(num_lat - 1)))
    weight = (num_lat * coslat / coslat.sum()).reshape(1, 1, -1, 1)
    return torch.sqrt(torch.mean(weight * (pred - target) ** 2.0, dim=(-1, -2))).mean(dim=0)


# ---- forecast scoring: RMSE and anomaly correlation per channel (reference utils/weighted_acc_rmse.py:50-115) ----------------
# On the kernel path the sums come from ONE pass of swv2_score_sums (csrc/score.hip) instead of torch's ten.
_WEIGHTS = {}


def latitude_weights(num_lat: int, device=None) -> torch.Tensor:
    """[num_lat] fp32: num_lat cos(3.1416 / 180 lat_j) / sum_j cos(..), lat_j = 90 - 180 j / (num_lat - 1).  Computed ONCE on the CPU
    in fp32 and copied, cached per device: the CPU and GPU paths use bit-identical weights.  The tensor returned IS the cached one:
    read it, never modify it in place."""
    dev = torch.device(device) if device is not None else torch.device("cpu")
    key = (int(num_lat), dev)
    if key not in _WEIGHTS:
        if (int(num_lat), torch.device("cpu")) not in _WEIGHTS:
            j = torch.arange(0, num_lat)
            coslat = torch.cos(3.1416 / 180.0 * (90.0 - j * 180.0 / float(num_lat - 1)))
            _WEIGHTS[(int(num_lat), torch.device("cpu"))] = num_lat * coslat / coslat.sum()
        _WEIGHTS[key] = _WEIGHTS[(int(num_lat), torch.device("cpu"))].to(dev)
    return _WEIGHTS[key]


def _row_weights(t: torch.Tensor, weighted: bool) -> torch.Tensor:
    if weighted:
        return latitude_weights(t.shape[2], t.device)
    key = ("ones", int(t.shape[2]), t.device)
    if key not in _WEIGHTS:
        _WEIGHTS[key] = torch.ones(t.shape[2], dtype=torch.float32, device=t.device)
    return _WEIGHTS[key]


def _on_kernels(pred: torch.Tensor, target: torch.Tensor) -> bool:
    if not (pred.is_cuda and target.is_cuda and pred.shape == target.shape):
        return False
    from .. import ops
    return ops.score_planes_ok(pred) and ops.score_planes_ok(target)


def _ensemble_on_kernels(ens: torch.Tensor, target: torch.Tensor, device) -> bool:
    """members [M, B, C, H, W] and truth [B, C, H, W] that swv2_ens_sums / swv2_event_ens_sums take in place, on the scorer's device"""
    if not (ens.is_cuda and target.is_cuda and ens.device == device == target.device):
        return False
    from .. import ops
    return ops.ens_members_ok(ens) and ops.score_planes_ok(target)


def _channel_blocks(who, C, H, W, prd, tar, coff_prd, coff_tar):
    """the [B, C, H, W] channel blocks of prd and tar at their offsets, as views"""
    p, t = prd[:, coff_prd:coff_prd + C], tar[:, coff_tar:coff_tar + C]
    if p.shape != t.shape or p.shape[1:] != (C, H, W):
        raise ValueError(f"{who}: blocks {tuple(p.shape)} / {tuple(t.shape)}, expected [B, {C}, {H}, {W}]")
    return p, t


def _member_blocks(who, C, H, W, ens, tar, n_members, coff_ens, coff_tar):
    """the member view: ens [M B, Cany, H, W] with a member-major batch (row m B + b) or [M, B, Cany, H, W] -> (channels coff_ens .. + C of
    it as [M, B, C, H, W], channels coff_tar .. + C of tar as [B, C, H, W]), both views"""
    M = int(n_members)
    if ens.dim() == 4:
        if M < 1 or ens.shape[0] % M:
            raise ValueError(f"{who}: a batch of {ens.shape[0]} rows does not hold {M} members")
        ens = ens.unflatten(0, (M, ens.shape[0] // M))                    # always a view: row m B + b -> [m, b]
    e, t = ens[:, :, coff_ens:coff_ens + C], tar[:, coff_tar:coff_tar + C]
    if e.dim() != 5 or e.shape[0] != M or M < 2 or e.shape[1:] != t.shape or t.shape[1:] != (C, H, W):
        raise ValueError(f"{who}: members {tuple(e.shape)} / truth {tuple(t.shape)}, expected [{M} >= 2, B, {C}, {H}, {W}] / [B, {C}, {H}, {W}]")
    return e, t


def _as_climatology(x, C, H, W, device):
    """a climatology given as an array or tensor -> contiguous fp32 [C, H, W] on device, or None"""
    if x is None:
        return None
    if isinstance(x, np.ndarray):
        x = torch.from_numpy(np.array(x, dtype=np.float32))          # (a copy: the array may be read-only)
    x = torch.as_tensor(x, dtype=torch.float32).to(device).contiguous()
    if x.shape != (C, H, W):
        raise ValueError(f"climatology {tuple(x.shape)}, expected {(C, H, W)}")
    return x


def _torch_sums(pred, target, w, clim=None):
    """the four sums of csrc/score.hip in plain torch, in the inputs' dtype: [n, c] each"""
    w = w.to(pred.dtype).reshape(1, 1, -1, 1)
    pa, ta = (pred, target) if clim is None else (pred - clim, target - clim)
    d = pred - target
    return tuple(torch.sum(w * a * b, dim=(-1, -2)) for a, b in ((d, d), (pa, ta), (pa, pa), (ta, ta)))


def _acc_channels(pred, target, weighted: bool):
    w = _row_weights(pred, weighted)
    if _on_kernels(pred, target):
        from .. import ops
        return ops.forecast_scores(pred, target, w)[2]
    _, s_pt, s_pp, s_tt = _torch_sums(pred, target, w)
    return s_pt / torch.sqrt(s_pp * s_tt)


def weighted_rmse_torch_channels(pred: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    """[n, c, h, w] x2 -> [n, c]: sqrt(mean_hw(w_lat (pred - target)^2)).  Like the other drop-in names below this is a stateless call: on
    the kernel path it takes a fresh workspace (n c slices 16 bytes, from torch's caching allocator) every time and computes all four
    sums for the one it returns; a loop that scores many steps should hold a ForecastScorer, which owns and reuses its workspace."""
    w = _row_weights(pred, True)
    if _on_kernels(pred, target):
        from .. import ops
        return ops.forecast_scores(pred, target, w)[1]
    return torch.sqrt(torch.mean(w.to(pred.dtype).reshape(1, 1, -1, 1) * (pred - target) ** 2.0, dim=(-1, -2)))


def weighted_acc_torch_channels(pred: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    """[n, c, h, w] x2 (anomalies) -> [n, c]: sum(w p t) / sqrt(sum(w p p) sum(w t t))"""
    return _acc_channels(pred, target, True)


def weighted_acc_torch(pred: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    return torch.mean(weighted_acc_torch_channels(pred, target), dim=0)


def unweighted_acc_torch_channels(pred: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    return _acc_channels(pred, target, False)


def unweighted_acc_torch(pred: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    return torch.mean(unweighted_acc_torch_channels(pred, target), dim=0)


# ---- forecast extremes: top-quantile error (reference utils/weighted_acc_rmse.py:36-47, 117-126) -----------------------------------
# torch.quantile sorts every plane; the 100 levels need at most 200 order statistics, the same ranks in every plane.  On CUDA fp32 inputs
# with contiguous planes and H * W % 4 == 0 they come from swv2_plane_order_stats (csrc/quantile.hip: a five-pass radix select, exact);
# anything else runs torch.quantile.
def quantile_levels(qlim=3, qcut=0.1, qs=100) -> torch.Tensor:
    """[qs] fp32: 1 - logspace(-qlim, -qcut, qs), the reference's levels, log-spaced toward the upper tail (0.2057 .. 0.999)"""
    return 1.0 - torch.logspace(-qlim, -qcut, steps=qs)


def quantile_ranks(n: int, q: torch.Tensor):
    """The order statistics torch.quantile(x, q) of n values reads, WITH ITS ARITHMETIC: pos = q * (n - 1) in fp32, lo = floor(pos),
    hi = ceil(pos), weight = pos - lo (an fp64 product gives other floors at n = 721 * 1440).  All on the CPU ->
    (ranks [K] int32: the distinct lo and hi, ascending; i_lo, i_hi [len(q)] int64: where each level's two ranks sit in `ranks`;
    weight [len(q)] fp32)."""
    q = torch.as_tensor(q, dtype=torch.float32, device="cpu").reshape(-1)
    if q.numel() == 0 or bool(((q < 0) | (q > 1)).any()):
        raise ValueError("quantile_ranks: levels must lie in [0, 1]")
    pos = q * (n - 1)
    lo, hi = pos.floor(), pos.ceil()
    weight = pos - lo
    lo, hi = lo.long().clamp_(0, n - 1), hi.long().clamp_(0, n - 1)
    ranks = torch.unique(torch.cat([lo, hi]))                  # sorted
    return ranks.int(), torch.searchsorted(ranks, lo), torch.searchsorted(ranks, hi), weight


class _QuantilePlan:
    """the ranks of quantile_ranks and the gather indices on one device"""

    def __init__(self, n, q, device):
        ranks, i_lo, i_hi, weight = quantile_ranks(n, q)
        self.K = ranks.numel()
        self.ranks, self.i_lo, self.i_hi = ranks.to(device), i_lo.to(device), i_hi.to(device)
        self.weight = weight.to(device).reshape(-1, 1, 1)

    def quantiles(self, x, ws=None):
        from .. import ops
        v, nan_count = ops.plane_order_stats(x, self.ranks, ws)
        out = torch.lerp(v[self.i_lo], v[self.i_hi], self.weight)
        return out.masked_fill_((nan_count > 0).unsqueeze(0), float("nan"))           # as torch.quantile: a NaN poisons its plane


def _quantiles_on_kernels(x: torch.Tensor) -> bool:
    if not (x.is_cuda and x.dim() == 4):
        return False
    from .. import ops
    return ops.quantile_planes_ok(x)


def plane_quantiles(x: torch.Tensor, q: torch.Tensor) -> torch.Tensor:
    """[B, C, H, W], levels [Q] -> [Q, B, C]: torch.quantile(x.view(B, C, H W), q, dim=-1) (linear interpolation).  A stateless call (a
    fresh workspace each time on the kernel path); a loop should hold a ForecastScorer."""
    q = torch.as_tensor(q, dtype=torch.float32).reshape(-1)
    if _quantiles_on_kernels(x):
        from .. import ops
        step = ops.QUANTILE_MAX_RANKS // 2                     # two ranks per level at most: every chunk of levels fits one call
        parts = [_QuantilePlan(x.shape[2] * x.shape[3], q[i:i + step], x.device).quantiles(x) for i in range(0, q.numel(), step)]
        return parts[0] if len(parts) == 1 else torch.cat(parts, dim=0)
    B, Cc = x.shape[:2]
    return torch.quantile(x.reshape(B, Cc, -1), q.to(device=x.device, dtype=x.dtype), dim=-1)


def top_quantiles_error_torch(pred: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    """[n, c, h, w] x2 -> [n, c]: the mean over the 100 levels of quantile(pred) - quantile(target), per plane: negative where the
    forecast blurs its extremes"""
    q = quantile_levels()
    return torch.mean(plane_quantiles(pred, q) - plane_quantiles(target, q), dim=0)


def top_quantiles_error(pred, target):
    """the numpy form, CPU only: [n, h, w] (or [h, w]) x2 -> [n], levels 1 - logspace(-5, -0.1, 100) in fp64"""
    pred, target = np.asarray(pred), np.asarray(target)
    if pred.ndim == 2:
        pred = np.expand_dims(pred, 0)
    if target.ndim == 2:
        target = np.expand_dims(target, 0)
    qtile = 1.0 - np.logspace(-5, -0.1, num=100)
    return np.mean(np.quantile(pred, q=qtile, axis=(1, 2)) - np.quantile(target, q=qtile, axis=(1, 2)), axis=0)


def load_climatology(params, means=None, stds=None):
    """The normalised climatology ACC needs, [C, H, W] fp32 numpy: (time_means[:, out_channels, :H, :W] - means) / stds with the
    reference's files (`time_means_path` [1, Call, Hfull, Wfull]; means / stds [1, Call, 1, 1] from `global_means_path` /
    `global_stds_path` unless given; a missing stats file means unit stds / zero means, as validation treats synthetic fields).
    None when `time_means_path` is not a file."""
    def get(k):
        return params[k] if k in params else None
    path = get("time_means_path")
    if path is None or not os.path.isfile(str(path)):
        return None
    H, W = get("img_size")
    chans = np.asarray(get("out_channels"))
    tm = np.load(str(path))[:, chans, :H, :W].astype(np.float32)

    def stat(given, key, default):
        if given is None:
            f = get(key)
            if f is None or not os.path.isfile(str(f)):
                return np.float32(default)
            given = np.load(str(f))
        return np.asarray(given, dtype=np.float32)[:, chans]
    return np.ascontiguousarray(((tm - stat(means, "global_means_path", 0.0)) / stat(stds, "global_stds_path", 1.0))[0], dtype=np.float32)


Scores = namedtuple("Scores", "rmse acc rmse_mean acc_mean sums")
MaeScores = namedtuple("MaeScores", "mae mae_mean sums")
EnsembleScores = namedtuple("EnsembleScores", "sums hist ens_rmse spread crps fair_crps ens_rmse_mean spread_mean crps_mean fair_crps_mean")
PowerSpectrum = namedtuple("PowerSpectrum", "pred truth")

# forecast events: contingency tables and Brier scores (the statements and the fp64 scores live in utils/events.py)
from .events import (EVENT_MAX_K, EnsembleEventScores, EventScores, EventSpec, brier_scores, contingency_scores,  # noqa: E402,F401
                     ensemble_event_sums_torch, event_table_torch, expand_thresholds, quantile_thresholds, reliability_scores)
from .events import (FSS_MAX_S, NeighbourhoodScores, box_sizes, check_scales, fss_rows_torch, fss_scores, useful_scale)  # noqa: E402,F401
from .events import EnsembleNeighbourhoodScores, fss_ens_rows_torch, fss_ens_scores  # noqa: E402,F401


def small_scale_power_ratio(pred: torch.Tensor, truth: torch.Tensor) -> torch.Tensor:
    """degree power [..., lmax] x2 -> [...]: sum_{l >= lmax // 2} pred / sum_{l >= lmax // 2} truth, the share of the truth's power in the
    upper half of the degrees that the forecast keeps.  This project's own scalar for the blurring of long rollouts (1: as sharp as the
    analysis, below 1: blurred); the reference has no counterpart."""
    lo = pred.shape[-1] // 2
    return pred[..., lo:].sum(dim=-1) / truth[..., lo:].sum(dim=-1)


class ForecastScorer:
    """Latitude-weighted RMSE and ACC of [B, C, H, W] forecasts against the verifying analysis, both normalised as the model sees them.
    Owns the row weights, the normalised climatology [C, H, W] (None: no ACC) and the kernel workspace; `stds` [C] puts the batch-mean
    RMSE into physical units.  One pass over prediction, truth and climatology per call on CUDA (csrc/score.hip), plain torch elsewhere.
    weights: an [H] row-weight vector in place of latitude_weights(H) (default None: the reference's cos(lat) weights, as ever)."""

    def __init__(self, H, W, n_channels, device, climatology=None, stds=None, weights=None):
        self.H, self.W, self.C = int(H), int(W), int(n_channels)
        if weights is None:
            self.w = latitude_weights(self.H, device)
        else:                                             # another convention's row weights [H] (RegriddedScorer: the target's cell areas)
            self.w = torch.as_tensor(weights, dtype=torch.float32).reshape(-1).to(device).contiguous()
            if self.w.numel() != self.H:
                raise ValueError(f"{self.w.numel()} row weights for {self.H} rows")
        self.device = self.w.device                       # resolved: "cuda" names the current device, whose tensors say cuda:<index>
        self.clim = _as_climatology(climatology, self.C, self.H, self.W, self.device)
        self.scale = None if stds is None else torch.as_tensor(stds, dtype=torch.float32).reshape(-1).to(self.device).contiguous()
        if self.scale is not None and self.scale.numel() != self.C:
            raise ValueError(f"{self.scale.numel()} stds for {self.C} channels")
        self._qplan = None
        self._ws = {}                                     # (kind, ...) -> the kernel workspace of that call shape, made once and reused

    def _workspace(self, key, make, *args):
        if key not in self._ws:
            self._ws[key] = make(*args, self.device)
        return self._ws[key]

    def _threshold_chunks(self, thr, key, make, *args):
        """thr [1 or B, C, K] in chunks of EVENT_MAX_K thresholds -> (the chunk, contiguous; its K; the workspace of that call shape)"""
        for k0 in range(0, thr.shape[2], EVENT_MAX_K):
            tk = thr[:, :, k0:k0 + EVENT_MAX_K].contiguous()
            K = tk.shape[2]
            yield tk, K, self._workspace(key + (K,), make, *args, K)

    def score(self, prd, tar, coff_prd=0, coff_tar=0) -> Scores:
        """channels coff_prd .. + C of prd against channels coff_tar .. + C of tar (scored in place, no copy) ->
        Scores(rmse [B, C], acc [B, C] | None, rmse_mean [C] (x stds), acc_mean [C] | None, sums [B, C, 4])"""
        p, t = _channel_blocks("score", self.C, self.H, self.W, prd, tar, coff_prd, coff_tar)
        if _on_kernels(p, t) and p.device == self.device:
            from .. import ops
            B = p.shape[0]
            ws = self._workspace(("score", B), ops.score_workspace, B * self.C, self.H, self.W)
            ops.score_sums(p, t, self.w, ws, self.clim)
            sums, rmse, acc, rmse_mean, acc_mean = ops.score_finalize(ws, B, self.C, self.H, self.W, self.scale)
        else:
            w = self.w.to(p.device)
            clim = None if self.clim is None else self.clim.to(device=p.device, dtype=p.dtype)
            s = _torch_sums(p, t, w, clim)
            sums = torch.stack(s, dim=-1)
            rmse = torch.sqrt(s[0] / float(self.H * self.W))
            acc = s[1] / torch.sqrt(s[2] * s[3])
            rmse_mean, acc_mean = rmse.mean(dim=0), acc.mean(dim=0)
            if self.scale is not None:
                rmse_mean = rmse_mean * self.scale.to(device=p.device, dtype=p.dtype)
        if self.clim is None:
            acc = acc_mean = None
        return Scores(rmse, acc, rmse_mean, acc_mean, sums)

    def mae(self, prd, tar, coff_prd=0, coff_tar=0) -> MaeScores:
        """latitude-weighted mean absolute error of channels coff_prd .. + C of prd against channels coff_tar .. + C of tar (read in
        place) -> MaeScores(mae [B, C] = S0 / (H W), mae_mean [C] = mean_b mae (x stds), sums [B, C, 2] = (S0, S1)) with
        S0 = sum w[h] |prd - tar|, S1 = sum w[h] |tar|.  One pass of swv2_l1_sums (csrc/loss_l1.hip) on CUDA, plain torch elsewhere."""
        p, t = _channel_blocks("mae", self.C, self.H, self.W, prd, tar, coff_prd, coff_tar)
        n = float(self.H * self.W)
        if _on_kernels(p, t) and p.device == self.device:
            from .. import ops
            B = p.shape[0]
            ws = self._workspace(("l1", B), ops.l1_workspace, B * self.C, self.H, self.W)
            ops.l1_sums(p, t, self.w, ws)
            sums = ops.l1_finalize(ws, B, self.C, self.H, self.W)[0]
        else:
            w = self.w.to(device=p.device, dtype=p.dtype).reshape(1, 1, -1, 1)
            sums = torch.stack((torch.sum(w * torch.abs(p - t), dim=(-1, -2)), torch.sum(w * torch.abs(t), dim=(-1, -2))), dim=-1)
        mae = sums[..., 0] / n
        mae_mean = mae.mean(dim=0)
        if self.scale is not None:
            mae_mean = mae_mean * self.scale.to(device=p.device, dtype=p.dtype)
        return MaeScores(mae, mae_mean, sums)

    def power_spectrum(self, prd, tar=None, coff_prd=0, coff_tar=0) -> PowerSpectrum:
        """spherical-harmonic degree power (utils/sht.py::degree_power: csrc/sht.hip on CUDA fp32) of channels coff_prd .. + C of prd and,
        with tar, of channels coff_tar .. + C of tar, both read in place -> PowerSpectrum(pred [B, C, lmax = H], truth [B, C, lmax] | None),
        in the scorer's normalised units (squared)"""
        from .sht import degree_power
        p = prd[:, coff_prd:coff_prd + self.C]
        if p.shape[1:] != (self.C, self.H, self.W):
            raise ValueError(f"power_spectrum: block {tuple(p.shape)}, expected [B, {self.C}, {self.H}, {self.W}]")
        if tar is None:
            return PowerSpectrum(degree_power(p), None)
        p, t = _channel_blocks("power_spectrum", self.C, self.H, self.W, prd, tar, coff_prd, coff_tar)
        return PowerSpectrum(degree_power(p), degree_power(t))

    def spectral_coherence(self, prd, tar, coff_prd=0, coff_tar=0) -> torch.Tensor:
        """the anomaly correlation of every degree, C / sqrt(P_prd P_tar) (utils/sht.py::cross_power and spectral_coherence: csrc/sht.hip on
        CUDA fp32), of channels coff_prd .. + C of prd against channels coff_tar .. + C of tar, both read in place -> [B, C, lmax = H] in
        fp64; NaN where a power is zero, not clamped"""
        from .sht import cross_power, spectral_coherence
        p, t = _channel_blocks("spectral_coherence", self.C, self.H, self.W, prd, tar, coff_prd, coff_tar)
        return spectral_coherence(*cross_power(p, t))

    def quantile_error(self, prd, tar, coff_prd=0, coff_tar=0) -> torch.Tensor:
        """top_quantiles_error_torch of channels coff_prd .. + C of prd against channels coff_tar .. + C of tar (read in place) -> [B, C].
        The rank tensor and the workspace (one per B) are made once and reused."""
        p, t = _channel_blocks("quantile_error", self.C, self.H, self.W, prd, tar, coff_prd, coff_tar)
        q = quantile_levels()
        if not (_quantiles_on_kernels(p) and _quantiles_on_kernels(t) and p.device == self.device == t.device):
            return torch.mean(plane_quantiles(p, q) - plane_quantiles(t, q), dim=0)
        from .. import ops
        if self._qplan is None:
            self._qplan = _QuantilePlan(self.H * self.W, q, self.device)
        B = p.shape[0]
        ws = self._workspace(("quantile", B), ops.quantile_workspace, B * self.C, self.H, self.W, self._qplan.K)
        return torch.mean(self._qplan.quantiles(p, ws) - self._qplan.quantiles(t, ws), dim=0)

    def ensemble_score(self, ens, tar, n_members, coff_ens=0, coff_tar=0) -> EnsembleScores:
        """n_members forecasts against one truth.  ens: [M B, Cany, H, W] with a member-major batch (row m B + b) or [M, B, Cany, H, W];
        channels coff_ens .. + C of it against channels coff_tar .. + C of tar [B, Cany', H, W], all read in place (a ring slot of
        inference.ensemble_rollout) -> EnsembleScores(sums [B, C, 4] = (S_mse, S_var, S_1, S_2), hist [B, C, M + 1] int32, ens_rmse, spread,
        crps, fair_crps [B, C], and their batch means [C]; the scorer's stds multiply ens_rmse_mean, spread_mean and crps_mean).  One
        workspace per (M, B) is kept and reused."""
        e, t = _member_blocks("ensemble_score", self.C, self.H, self.W, ens, tar, n_members, coff_ens, coff_tar)
        if _ensemble_on_kernels(e, t, self.device):
            from .. import ops
            M, B = e.shape[:2]
            ws = self._workspace(("ensemble", M, B), ops.ens_workspace, B * self.C, self.H, self.W, M)
            ops.ens_sums(e, t, self.w, ws)
            sums, hist, er, sp, cr, fc, means = ops.ens_finalize(ws, M, B, self.C, self.H, self.W, self.scale)
            return EnsembleScores(sums, hist, er, sp, cr, fc, means[0], means[1], means[2], means[3])
        return ensemble_scores_torch(e, t, self.w, self.scale)

    # ---- forecast events (utils/events.py, csrc/events.hip) ----
    def _event_base(self, who, anomaly, base):
        if anomaly:
            if base is not None:
                raise ValueError(f"{who}: anomaly=True takes the scorer's climatology as the base field; give one of the two")
            if self.clim is None:
                raise ValueError(f"{who}: anomaly=True needs a scorer with a climatology")
            return self.clim
        if base is None:
            return None
        base = torch.as_tensor(base, dtype=torch.float32).to(self.device).contiguous()
        if base.shape != (self.C, self.H, self.W):
            raise ValueError(f"{who}: base field {tuple(base.shape)}, expected {(self.C, self.H, self.W)}")
        return base

    def event_thresholds(self, spec, tar, coff_tar=0):
        """the thresholds an EventSpec names for this truth: kind "anomaly" -> its levels [K] (offsets from the climatology, normalised
        units; score with anomaly=True), kind "quantile" -> quantile_thresholds of channels coff_tar .. + C of tar [B, C, K]"""
        if spec.kind == "anomaly":
            return torch.as_tensor(spec.levels, dtype=torch.float32).reshape(-1)
        if spec.kind == "quantile":
            return quantile_thresholds(tar[:, coff_tar:coff_tar + self.C], spec.levels)
        raise ValueError(f"EventSpec.kind {spec.kind!r}: \"anomaly\" or \"quantile\"")

    def event_score(self, prd, tar, thresholds, anomaly=False, base=None, below=False, coff_prd=0, coff_tar=0) -> EventScores:
        """The 2 x 2 contingency table of the event "x > theta" ("x < theta" with below) in channels coff_prd .. + C of prd against channels
        coff_tar .. + C of tar (read in place), for thresholds [K], [C, K] or [B, C, K] in the scorer's normalised units; theta = threshold,
        or base + threshold with a base field [C, H, W] (anomaly=True: the scorer's climatology) -> EventScores(table [B, C, K, 4] =
        (a, b, c, d) with the scorer's row weights, n_invalid [B, C] int32: the points with a NaN, which enter no cell, scores: the dict of
        contingency_scores per sample [B, C, K], pooled: the same from the tables summed over the batch [C, K], both fp64).  One pass of
        swv2_event_sums per 8 thresholds on CUDA fp32, event_table_torch elsewhere."""
        p, t = _channel_blocks("event_score", self.C, self.H, self.W, prd, tar, coff_prd, coff_tar)
        base = self._event_base("event_score", anomaly, base)
        B = p.shape[0]
        thr = expand_thresholds(thresholds, B, self.C, p.device)
        if _on_kernels(p, t) and p.device == self.device:
            from .. import ops
            tables = []
            for tk, K, ws in self._threshold_chunks(thr, ("event", B), ops.event_workspace, B * self.C, self.H, self.W):
                ops.event_sums(p, t, tk, self.w, ws, base, below)
                tab, ninv = ops.event_finalize(ws, K, B, self.C, self.H, self.W)
                tables.append(tab)
            table = tables[0] if len(tables) == 1 else torch.cat(tables, dim=2)
        else:
            table, ninv = event_table_torch(p, t, thr, self.w, None if base is None else base.to(p.device), below)
        return EventScores(table, ninv, contingency_scores(table), contingency_scores(table.to(torch.float64).sum(dim=0)))

    def _chunked_rows(self, thr, sc, key, make, call):
        """rows [B, C, K, S, H, 3] of one of the two neighbourhood kernels, run per 8 scales and 8 thresholds: make(planes, H, W, S, K,
        device) -> the workspace of a call shape (kept under key + (S, K)), call(thresholds, scales, workspace) -> (rows, n_invalid)"""
        per_s = []
        for s0 in range(0, len(sc), FSS_MAX_S):
            sk = sc[s0:s0 + FSS_MAX_S]
            per_k = []
            for tk, K, ws in self._threshold_chunks(thr, key + (len(sk),), make, self.H, self.W, len(sk)):
                r, ninv = call(tk, sk, ws)
                per_k.append(r)
            per_s.append(per_k[0] if len(per_k) == 1 else torch.cat(per_k, dim=2))
        return (per_s[0] if len(per_s) == 1 else torch.cat(per_s, dim=3)), ninv

    def _fss_rows(self, p, t, thr, sc, base, below):
        """(rows, n_invalid) of one forecast block p against t for every scale of sc: swv2_fss_rows on CUDA fp32, fss_rows_torch elsewhere"""
        if _on_kernels(p, t) and p.device == self.device:
            from .. import ops
            planes = p.shape[0] * self.C
            return self._chunked_rows(thr, sc, ("fss", p.shape[0]), lambda H, W, S, K, device: ops.fss_workspace(planes, H, W, K, S, device),
                                      lambda tk, sk, ws: ops.fss_rows(p, t, tk, sk, ws, base, below))
        return fss_rows_torch(p, t, thr, sc, None if base is None else base.to(p.device), below)

    def ensemble_neighbourhood_score(self, ens, tar, n_members, thresholds, scales, anomaly=False, base=None, below=False, coff_ens=0,
                                     coff_tar=0, members=False) -> EnsembleNeighbourhoodScores:
        """The probabilistic fractions skill score of n_members forecasts (ens as ensemble_score takes it, read in place): the neighbourhood
        ensemble probability -- the box mean of the member fraction c / M -- against the analysis' fraction, for the events of
        ensemble_event_score and the scales of neighbourhood_score -> EnsembleNeighbourhoodScores(rows [B, C, K, S, H, 3] int64 =
        (sum_w (N_f - M n_o)^2, sum_w N_f^2, sum_w n_o^2), n_invalid [B, C] int32: the points with a NaN in any member, the truth or the
        base, which are events nowhere; scores: fss_ens_scores per sample (pfss, fbs [B, C, K, S], fss_uniform, base_rate [B, C, K]) plus
        useful_scale; pooled: the same from the rows summed over the batch).  Scale 0 is always computed and stays out of what is
        reported where `scales` does not name it.  members=True adds, from swv2_fss_rows / fss_rows_torch (one forecast against one field):
        member_rows = sum_m rows(member m vs analysis), dispersion_rows = sum_{m >= 1} rows(member m vs member 0), and member_scores /
        dispersion_scores: their pooled fss_scores (fss = eFSS / dFSS of Dey et al. 2014) with useful_scale.  swv2_fss_ens_rows per 8
        thresholds and 8 scales on CUDA fp32, fss_ens_rows_torch elsewhere.  Boxes count grid points; ties between members are not
        randomised."""
        e, t = _member_blocks("ensemble_neighbourhood_score", self.C, self.H, self.W, ens, tar, n_members, coff_ens, coff_tar)
        base = self._event_base("ensemble_neighbourhood_score", anomaly, base)
        asked = check_scales(scales, self.W)
        sc = asked if asked[0] == 0 else (0,) + asked
        M, B = e.shape[:2]
        thr = expand_thresholds(thresholds, B, self.C, t.device)
        if _ensemble_on_kernels(e, t, self.device):
            from .. import ops
            rows, ninv = self._chunked_rows(thr, sc, ("fss_ens", M, B),
                                            lambda H, W, S, K, device: ops.fss_ens_workspace(B * self.C, H, W, M, K, S, device),
                                            lambda tk, sk, ws: ops.fss_ens_rows(e, t, tk, sk, ws, base, below))
        else:
            rows, ninv = fss_ens_rows_torch(e, t, thr, sc, None if base is None else base.to(t.device), below)

        def cut(r):
            return r if sc is asked else r[:, :, :, 1:]

        def scores(r, fields, m=None):
            s = fss_scores(r, self.w, sc, self.W, fields) if m is None else fss_ens_scores(r, self.w, sc, self.W, m, fields)
            name = "fss" if m is None else "pfss"
            if sc is not asked:
                s[name], s["fbs"] = s[name][..., 1:], s["fbs"][..., 1:]
            s["useful_scale"] = useful_scale(s[name], s["fss_uniform"], asked)
            return s
        extra = ()
        if members:
            mr = dr = None
            for m in range(M):
                r = self._fss_rows(e[m], t, thr, sc, base, below)[0]
                mr = r if mr is None else mr + r
                if m:
                    r = self._fss_rows(e[m], e[0], thr, sc, base, below)[0]
                    dr = r if dr is None else dr + r
            extra = (cut(mr), cut(dr), scores(mr.sum(dim=0), B * M), scores(dr.sum(dim=0), B * (M - 1)))
        return EnsembleNeighbourhoodScores(cut(rows), ninv, scores(rows, 1, M), scores(rows.sum(dim=0), B, M), *extra)

    def neighbourhood_score(self, prd, tar, thresholds, scales, anomaly=False, base=None, below=False, coff_prd=0,
                            coff_tar=0) -> NeighbourhoodScores:
        """The fractions skill score of the event of event_score (same blocks, thresholds, base field and direction) over boxes of
        half-width r grid points for every r of `scales` (strictly ascending, 0 .. 32, 2 r + 1 <= W; periodic in longitude, clipped at the
        poles) -> NeighbourhoodScores(rows [B, C, K, S, H, 3] int64 = (sum_w (n_f - n_o)^2, sum_w n_f^2, sum_w n_o^2), n_invalid [B, C]
        int32: the points with a NaN, which are events in neither field, scores: the dict of fss_scores per sample (fss, fbs [B, C, K, S],
        fss_uniform, base_rate [B, C, K]) plus useful_scale [B, C, K], pooled: the same from the rows summed over the batch; fp64, with
        the scorer's row weights).  Scale 0 carries the base rate: it is always computed, and stays out of rows and scores where `scales`
        does not name it.  swv2_fss_rows per 8 thresholds and 8 scales on CUDA fp32, fss_rows_torch elsewhere."""
        p, t = _channel_blocks("neighbourhood_score", self.C, self.H, self.W, prd, tar, coff_prd, coff_tar)
        base = self._event_base("neighbourhood_score", anomaly, base)
        asked = check_scales(scales, self.W)
        sc = asked if asked[0] == 0 else (0,) + asked
        B = p.shape[0]
        thr = expand_thresholds(thresholds, B, self.C, p.device)
        rows, ninv = self._fss_rows(p, t, thr, sc, base, below)

        def scores(r, fields=1):
            s = fss_scores(r, self.w, sc, self.W, fields)
            if sc is not asked:
                s["fss"], s["fbs"] = s["fss"][..., 1:], s["fbs"][..., 1:]
            s["useful_scale"] = useful_scale(s["fss"], s["fss_uniform"], asked)
            return s
        return NeighbourhoodScores(rows if sc is asked else rows[:, :, :, 1:], ninv, scores(rows), scores(rows.sum(dim=0), B))

    def ensemble_event_score(self, ens, tar, n_members, thresholds, anomaly=False, base=None, below=False, coff_ens=0,
                             coff_tar=0) -> EnsembleEventScores:
        """The exceedance probabilities n / M of n_members forecasts (ens as ensemble_score takes it) against the event in the truth, for
        thresholds as event_score takes them -> EnsembleEventScores(sums [B, C, K, 3] = (S_e, S_f, S_o), wv [B, C], hist
        [B, C, K, 2, M + 1] int32 point counts ([0]: forecasts of n / M, [1]: those with the event observed), n_invalid [B, C], scores:
        brier_scores per sample [B, C, K], pooled: the same from the sums added over the batch [C, K], reliability: reliability_scores of
        the counts added over the batch [C, K]; all fp64).  The reliability table and the ROC area are point counts: they carry no area
        weights.  One pass of swv2_event_ens_sums per 8 thresholds on CUDA fp32, ensemble_event_sums_torch elsewhere."""
        e, t = _member_blocks("ensemble_event_score", self.C, self.H, self.W, ens, tar, n_members, coff_ens, coff_tar)
        base = self._event_base("ensemble_event_score", anomaly, base)
        M, B = e.shape[:2]
        thr = expand_thresholds(thresholds, B, self.C, t.device)
        if _ensemble_on_kernels(e, t, self.device):
            from .. import ops
            parts = []
            for tk, K, ws in self._threshold_chunks(thr, ("ens_event", M, B), ops.ens_event_workspace, B * self.C, self.H, self.W, M):
                ops.ens_event_sums(e, t, tk, self.w, ws, base, below)
                parts.append(ops.ens_event_finalize(ws, M, K, B, self.C, self.H, self.W))
            sums, hist = (parts[0][i] if len(parts) == 1 else torch.cat([q[i] for q in parts], dim=2) for i in (0, 2))
            wv, ninv = parts[0][1], parts[0][3]
        else:
            sums, wv, hist, ninv = ensemble_event_sums_torch(e, t, thr, self.w, None if base is None else base.to(t.device), below)
        hp = hist.to(torch.int64).sum(dim=0)
        return EnsembleEventScores(sums, wv, hist, ninv, brier_scores(sums, wv, M),
                                   brier_scores(sums.to(torch.float64).sum(dim=0), wv.to(torch.float64).sum(dim=0), M),
                                   reliability_scores(hp[..., 0, :], hp[..., 1, :]))


# ---- ensemble scores: CRPS, spread, ensemble-mean RMSE, rank histogram (what Earth2MIP reports for perturbed-initial-condition runs) ----
# M members x_m against the truth y, per grid point (every term from differences of inputs, so the rounding error of a sum is relative to
# that sum of non-negative terms and not to the magnitude of the fields):
#     xbar = mean_m x_m    s2 = sum_m (x_m - xbar)^2 / (M - 1)    e1 = sum_m |x_m - y|    e2 = sum_{m<n} |x_m - x_n|    rank = #{m : x_m < y}
# per plane, with row weights w[h] and N = H W:
#     S_mse = sum w (xbar - y)^2    S_var = sum w s2    S_1 = sum w e1    S_2 = sum w e2    hist[r] = #{points of rank r}
#     ens_rmse = sqrt(S_mse / N)    spread = sqrt(S_var / N)    crps = (S_1 / M - S_2 / M^2) / N    fair_crps = (S_1 / M - S_2 / (M (M - 1))) / N
# On the kernel path the sums come from ONE pass of swv2_ens_sums (csrc/ensemble.hip: the M values of a grid point in registers);
# anything else runs ensemble_scores_torch.


def spread_skill_ratio(spread: torch.Tensor, ens_rmse: torch.Tensor, n_members: int) -> torch.Tensor:
    """sqrt((M + 1) / M) spread / ens_rmse: 1 for a statistically consistent ensemble"""
    return float(np.sqrt((n_members + 1.0) / n_members)) * spread / ens_rmse


def ensemble_scores_torch(ens: torch.Tensor, tar: torch.Tensor, w=None, scale=None) -> EnsembleScores:
    """ens [M, B, C, H, W], tar [B, C, H, W], w [H] (default: the latitude weights) -> EnsembleScores, in plain torch on any device and
    for any W: sort over the member axis, e2 from the gaps of the sorted members, the variance from deviations.  scale [C] multiplies the
    first three batch means."""
    M, B, Cc, H, W = ens.shape
    if M < 2 or tar.shape != ens.shape[1:]:
        raise ValueError(f"ensemble_scores_torch: members {tuple(ens.shape)} / truth {tuple(tar.shape)}, expected [M >= 2, B, C, H, W] / [B, C, H, W]")
    w = (latitude_weights(H, ens.device) if w is None else w).to(device=ens.device, dtype=ens.dtype).reshape(1, 1, -1, 1)
    n = float(H * W)
    d = ens - tar.unsqueeze(0)
    e1 = d.abs().sum(dim=0)
    rank = (ens < tar.unsqueeze(0)).sum(dim=0)
    a = ens - ens[0:1]
    abar = a.mean(dim=0)
    vv = ((a - abar.unsqueeze(0)) ** 2).sum(dim=0)
    em = d[0] + abar
    gaps = torch.diff(torch.sort(ens, dim=0).values, dim=0)
    i = torch.arange(1, M, device=ens.device, dtype=ens.dtype)
    e2 = ((i * (M - i)).reshape(-1, 1, 1, 1, 1) * gaps).sum(dim=0)
    s_mse, s_vv, s_1, s_2 = (torch.sum(w * t, dim=(-1, -2)) for t in (em * em, vv, e1, e2))
    s_var = s_vv / (M - 1.0)
    hist = torch.zeros(B, Cc, M + 1, dtype=torch.int64, device=ens.device)
    hist.scatter_add_(2, rank.reshape(B, Cc, H * W), torch.ones(B, Cc, H * W, dtype=torch.int64, device=ens.device))
    ens_rmse, spread = torch.sqrt(s_mse / n), torch.sqrt(s_var / n)
    spread = torch.where(torch.isnan(s_1), s_1, spread)        # a NaN in the truth poisons the plane's spread too, as every other score
    crps, fair = (s_1 / M - s_2 / float(M * M)) / n, (s_1 / M - s_2 / float(M * (M - 1))) / n
    means = [v.mean(dim=0) for v in (ens_rmse, spread, crps, fair)]
    if scale is not None:
        sc = scale.to(device=ens.device, dtype=ens.dtype)
        means = [m * sc for m in means[:3]] + means[3:]
    return EnsembleScores(torch.stack((s_mse, s_var, s_1, s_2), dim=-1), hist.to(torch.int32), ens_rmse, spread, crps, fair, *means)


class RegriddedScorer:
    """ForecastScorer on a coarser grid: every call regrids the named channel blocks of the wide tensors where they lie (utils/regrid.py::
    Regridder: csrc/regrid.hip on CUDA fp32, the dense statement elsewhere) into coarse buffers kept per call shape, and hands those to an
    inner ForecastScorer(Hd, Wd, C, weights = the target's cell areas, the climatology regridded once here).  The published tables of
    this model family (WeatherBench 2 scorecards: 1.5 degrees, cell-area weights) are on such a grid.  score, mae, quantile_error and
    ensemble_score keep ForecastScorer's signatures; .C, .H, .W and .clim are the SOURCE grid's (what score_rollout and
    ensemble_rollout read), .grid is the target, .inner the coarse scorer.  power_spectrum raises: spectra are taken on the native grid."""

    def __init__(self, regridder, n_channels, climatology=None, stds=None):
        self.regridder, self.C = regridder, int(n_channels)
        (self.H, self.W), self.grid, self.device = regridder.src.shape, regridder.dst, regridder.device
        self.clim = _as_climatology(climatology, self.C, self.H, self.W, self.device)
        Hd, Wd = self.grid.shape
        self.inner = ForecastScorer(Hd, Wd, self.C, self.device, climatology=None if self.clim is None else regridder(self.clim),
                                    stds=stds, weights=regridder.area_weights)
        self._buf = {}

    def _coarse(self, name, x):
        """x [..., C, H, W] (a view of the caller's tensor) regridded into this scorer's buffer of that name and shape"""
        key = (name, tuple(x.shape[:-2]), x.dtype, x.device)
        if key not in self._buf:
            self._buf[key] = torch.empty(tuple(x.shape[:-2]) + self.grid.shape, dtype=x.dtype, device=x.device)
        return self.regridder(x, out=self._buf[key])

    def _pair(self, who, prd, tar, coff_prd, coff_tar):
        p, t = _channel_blocks(who, self.C, self.H, self.W, prd, tar, coff_prd, coff_tar)
        return self._coarse("prd", p), self._coarse("tar", t)

    def _members(self, who, ens, tar, n_members, coff_ens, coff_tar):
        e, t = _member_blocks(who, self.C, self.H, self.W, ens, tar, n_members, coff_ens, coff_tar)
        return self._coarse("ens", e), self._coarse("tar", t), e.shape[0]

    def score(self, prd, tar, coff_prd=0, coff_tar=0) -> Scores:
        return self.inner.score(*self._pair("score", prd, tar, coff_prd, coff_tar))

    def mae(self, prd, tar, coff_prd=0, coff_tar=0) -> MaeScores:
        return self.inner.mae(*self._pair("mae", prd, tar, coff_prd, coff_tar))

    def quantile_error(self, prd, tar, coff_prd=0, coff_tar=0) -> torch.Tensor:
        return self.inner.quantile_error(*self._pair("quantile_error", prd, tar, coff_prd, coff_tar))

    def ensemble_score(self, ens, tar, n_members, coff_ens=0, coff_tar=0) -> EnsembleScores:
        return self.inner.ensemble_score(*self._members("ensemble_score", ens, tar, n_members, coff_ens, coff_tar))

    def event_thresholds(self, spec, tar, coff_tar=0):
        """ForecastScorer.event_thresholds; the quantiles are those of the REGRIDDED truth"""
        t = tar[:, coff_tar:coff_tar + self.C]
        return self.inner.event_thresholds(spec, self._coarse("tar", t) if spec.kind == "quantile" else t)

    def event_score(self, prd, tar, thresholds, anomaly=False, base=None, below=False, coff_prd=0, coff_tar=0) -> EventScores:
        """ForecastScorer.event_score on the coarse grid: the FIELDS are regridded first and the events are then taken there, against the
        regridded climatology (anomaly=True) or a base field given on the coarse grid, with the cell-area weights.  This is not the
        regridding of the events: a cell's mean exceeds a threshold less often than its points do."""
        return self.inner.event_score(*self._pair("event_score", prd, tar, coff_prd, coff_tar), thresholds, anomaly=anomaly, base=base, below=below)

    def neighbourhood_score(self, prd, tar, thresholds, scales, anomaly=False, base=None, below=False, coff_prd=0,
                            coff_tar=0) -> NeighbourhoodScores:
        """ForecastScorer.neighbourhood_score on the coarse grid: regrid first, then take the neighbourhoods there (the scales count
        grid points of the COARSE grid)"""
        return self.inner.neighbourhood_score(*self._pair("neighbourhood_score", prd, tar, coff_prd, coff_tar), thresholds, scales, anomaly=anomaly,
                                              base=base, below=below)

    def ensemble_event_score(self, ens, tar, n_members, thresholds, anomaly=False, base=None, below=False, coff_ens=0,
                             coff_tar=0) -> EnsembleEventScores:
        """ForecastScorer.ensemble_event_score on the coarse grid; as event_score, the fields are regridded, not the events"""
        return self.inner.ensemble_event_score(*self._members("ensemble_event_score", ens, tar, n_members, coff_ens, coff_tar), thresholds,
                                               anomaly=anomaly, base=base, below=below)

    def ensemble_neighbourhood_score(self, ens, tar, n_members, thresholds, scales, anomaly=False, base=None, below=False, coff_ens=0,
                                     coff_tar=0, members=False) -> EnsembleNeighbourhoodScores:
        """ForecastScorer.ensemble_neighbourhood_score on the coarse grid: regrid first, then take the neighbourhoods there (the scales
        count grid points of the COARSE grid)"""
        return self.inner.ensemble_neighbourhood_score(*self._members("ensemble_neighbourhood_score", ens, tar, n_members, coff_ens, coff_tar),
                                                       thresholds, scales, anomaly=anomaly, base=base, below=below, members=members)

    def power_spectrum(self, *args, **kwargs):
        raise ValueError("RegriddedScorer: degree spectra are taken on the model's own grid; use a ForecastScorer for power_spectrum")

    def spectral_coherence(self, *args, **kwargs):
        raise ValueError("RegriddedScorer: degree spectra are taken on the model's own grid; use a ForecastScorer for spectral_coherence")
