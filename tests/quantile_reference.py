"""The statement the quantile tests compare against, and the bounds they allow.

Statement: every plane sorted by torch.sort on the CPU in fp32 (NaNs last), then torch.quantile's own rank arithmetic

    pos = q * (N - 1) in fp32      lo = floor(pos)      hi = ceil(pos)      weight = pos - lo      value = lerp(v_lo, v_hi, weight)

On the CPU this equals torch.quantile bit for bit (tests/test_quantile_host.py checks it), and so the reference's
top_quantiles_error_torch.

Bounds, none of them taken from the code under test:
  order statistics      equal as floats to the sorted plane's entries, no tolerance (-0.0 == +0.0 counts as equal).
  interpolated value    4 fp32 ulp of max(|v_lo|, |v_hi|): the lerp is three roundings (the difference, the product, the sum) of
                        quantities bounded by twice that maximum, which also covers an fma-contracted against an uncontracted lerp and
                        torch's second form b - (b - a)(1 - w) for w >= 0.5.  Exact (bound 0) where lo == hi.
  the [n, c] error      the mean over the levels of the two operands' bounds, plus gamma(100) times the mean of the absolute level gaps
                        for the fp32 mean over the 100 levels (any order of additions); the reference value itself is the fp64 mean of the
                        fp32 reference quantiles' gaps.
"""
import numpy as np
import torch

from tests.plane_reference import U, gamma, worst  # noqa: F401  (re-exported)


def levels(qlim=3, qcut=0.1, qs=100):
    return 1.0 - torch.logspace(-qlim, -qcut, steps=qs)


def sorted_planes(x):
    """[B, C, H, W] (numpy or CPU tensor) -> [B, C, H W] fp32 CPU tensor, every plane ascending, NaNs last"""
    x = x.detach().clone().float() if isinstance(x, torch.Tensor) else torch.from_numpy(np.array(x, dtype=np.float32))     # (a copy)
    return torch.sort(x.reshape(x.shape[0], x.shape[1], -1), dim=-1).values


def rank_arithmetic(n, q):
    """-> (lo, hi int64 [Q], weight fp32 [Q]) with torch.quantile's fp32 arithmetic"""
    q = torch.as_tensor(q, dtype=torch.float32)
    pos = q * (n - 1)
    assert pos.dtype == torch.float32
    lo, hi = pos.floor(), pos.ceil()
    return lo.long(), hi.long(), pos - lo


def order_stats(x, ranks):
    """[K, B, C]: the entries `ranks` of every sorted plane"""
    return sorted_planes(x)[..., torch.as_tensor(ranks, dtype=torch.long)].permute(2, 0, 1).contiguous()


def quantiles(x, q, srt=None):
    """-> (reference [Q, B, C] fp32 numpy, bound [Q, B, C] fp64 numpy); a plane with a NaN is NaN at every level (bound 0)"""
    srt = sorted_planes(x) if srt is None else srt
    lo, hi, w = rank_arithmetic(srt.shape[-1], q)
    v_lo, v_hi = srt[..., lo].permute(2, 0, 1), srt[..., hi].permute(2, 0, 1)
    ref = torch.lerp(v_lo, v_hi, w.reshape(-1, 1, 1))
    ref = ref.masked_fill(torch.isnan(srt).any(-1).unsqueeze(0), float("nan")).numpy()
    m = np.maximum(np.abs(v_lo.numpy()), np.abs(v_hi.numpy()))
    bound = 4.0 * np.spacing(m).astype(np.float64)
    bound[(lo == hi).numpy()] = 0.0
    bound[np.isnan(ref)] = 0.0
    return ref, bound


def top_quantiles_error(pred, target):
    """-> (reference [B, C] fp64, bound [B, C] fp64)"""
    q = levels()
    (p, bp), (t, bt) = quantiles(pred, q), quantiles(target, q)
    gap = p.astype(np.float64) - t.astype(np.float64)
    return gap.mean(axis=0), (bp + bt).mean(axis=0) + gamma(100) * np.abs(gap).mean(axis=0)
