"""fp64 numpy statements of three small entry points and the error bounds the tests hold the fp32 kernels to: swv2_batch_sum and
swv2_merge_ln_bwd (csrc/rowops.hip), swv2_loss_finalize (csrc/loss_l2.hip).  Shared by tests/test_rows_exact_host.py and
tests/test_rows_exact_gpu.py, inputs included.  u = 2^-24 is one fp32 rounding, gamma(k) = k u / (1 - k u) >= (1 + u)^k - 1.  The library is
built with `hipcc -O3 -std=c++17` alone: `/` and `sqrtf` are correctly rounded (one rounding each), a * b + c may or may not be one fma,
and every count below holds for both.

swv2_batch_sum.  out[i] = (out[i] +) in[0][i] + in[1][i] + ... in that order, fp32 additions only: no bound, numpy reproduces the bits
(`batch_sum`).

swv2_merge_ln_bwd.  Row m of the 2 x 2 gather (linear_reference.merge_rows, MERGE_ORDER) has K = 4 C columns; with the STORED fp32
mean[m], rstd[m] (swv2_merge_stats' outputs are inputs here), x^ = (x - mean) rstd, gg = dn gamma:
        s1 = sum_k gg / K      s2 = sum_k gg x^ / K      dx = rstd (gg - s1 - x^ s2)      dgamma += sum_m dn x^      dbeta += sum_m dn
    x^       the subtraction and the product: gamma(2) |x^|.
    gg       one product (dn is bf16, exact in fp32).
    s1, s2   lane l adds its n = ceil(K / 64) terms k = l, l + 64, ... in order (s2 by fma), `wave_sum` (common.h) adds 6 levels of
             __shfl_xor partners (lanes without a term hold 0), the division by K rounds once:
                 ds1 = gamma(n + 6 + 1 + 1) sum_k |gg| / K             (the last 1: gg's own rounding)
                 ds2 = gamma(n + 6 + 1 + 3) sum_k |gg x^| / K          (the 3: gg 1, x^ 2)
    dx       gg passes its own rounding, two subtractions and the product with rstd (4); s1 the two subtractions and the product (3, and
             ds1); x^ s2 carries x^ (2), its product, one subtraction and the product with rstd (5, and |x^| ds2); a fused x^ s2 only
             drops one.  |dx - dx_ref| <= rstd (gamma(5) (|gg| + |s1| + |x^ s2|) + (1 + gamma(5)) (ds1 + |x^| ds2)).
    dgamma   M float atomics in arrival order onto the baseline: every partial sum is at most |base| + sum |term|, so whatever the order
             the additions cost gamma(M) of that; a term dn x^ carries 3 roundings:  gamma(M + 3) (|base| + sum_m |dn x^|).
    dbeta    the terms are exact:  gamma(M) (|base| + sum_m |dn|).

swv2_loss_finalize.  With S0 = sum_l sums[l][i][0], S1 = sum_l sums[l][i][1] (all >= 0, added in order), w = chw[i % C], den = 1 (absolute)
or S1, r = S0 / den, f = r (squared) or sqrt(r), f' = 1 or 1 / (2 f):      loss = sum_i w f      coef[i] = 2 w f' / den
    S0, S1   gamma(layers) each (positive terms: relative).
    r        k_r = 2 layers + 1 roundings (both sums and the division).
    f        k_f = k_r (squared) or layers + 2 (sqrt halves a relative error: (2 layers + 1) / 2 < layers + 1, and rounds once).
    coef     2 w is exact; f' = 0.5f / f: k_f + 1 (squared: 0); the product, the division and den's gamma(layers):
                 |coef - ref| <= gamma(k) |ref|,  k = layers + 2 (squared), 2 layers + 5 (sqrt)       -- a few u
    loss     a thread adds ceil(BC / 256) terms, `wave_sum` 6 levels, the four waves 2 more (3 allowed: the count tests/test_l1_loss_gpu.py
             uses), each term w f carries k_f + 1:     |loss - ref| <= gamma(ceil(BC / 256) + 6 + 3 + k_f + 1) sum_i |w f|
    A plane with S0 = 0: f = 0, the plane adds 0; squared variants have the finite coef 2 w / den, sqrt variants 2 w (0.5 / 0) / den = +-inf
    with the sign of w, which is also what autograd gives for the plain-torch statement (utils/losses.py: sqrt at 0 has the derivative inf).
"""
import math

import numpy as np
import torch

from tests.linear_reference import MERGE_ORDER, merge_rows

U = 2.0 ** -24
BATCH_SUM_CAP = 8192 * 256 * 4       # elements one pass of the capped grid covers
MERGE_ROW_CAP = 4096 * 4             # merged rows one pass of the capped grid covers
LOSS_PART_SLICES = 8


def gamma(k):
    return k * U / (1.0 - k * U)


def d(x):
    return np.asarray(x, dtype=np.float64)


def ratio(err, bound):
    """largest error / bound over the elements (an exact 0 <= 0 counts as 0); inf when anything is not finite"""
    err, bound = np.atleast_1d(np.abs(d(err))), np.atleast_1d(d(bound))
    if not (np.all(np.isfinite(err)) and np.all(np.isfinite(bound))):
        return float("inf")
    return float(np.max(np.where(err == 0, 0.0, err / np.where(bound == 0, np.finfo(np.float64).tiny, bound))))


# ---------------------------------------------------------------------------------------------------------------
# swv2_batch_sum
# ---------------------------------------------------------------------------------------------------------------
def batch_sum(inp, base=None):
    """inp fp32 [B][n], base fp32 [n] or None -> the kernel's bits: fp32 additions, baseline (or 0) first, then b = 0 .. B - 1"""
    s = np.zeros(inp.shape[1], np.float32) if base is None else base.astype(np.float32).copy()
    for b in range(inp.shape[0]):
        s = s + inp[b]
    assert s.dtype == np.float32
    return s


# ---------------------------------------------------------------------------------------------------------------
# swv2_merge_ln_bwd
# ---------------------------------------------------------------------------------------------------------------
MERGE_SHAPES = [(1, 6, 10, 8), (2, 8, 12, 16), (2, 6, 10, 24), (3, 4, 6, 128), (1, 4, 4, 192), (1, 258, 256, 8)]


def rows_of(x, order=MERGE_ORDER):
    """[B][H][W][C] numpy -> [M][4 C] in the gather's column order"""
    return merge_rows(torch.from_numpy(np.ascontiguousarray(x)), order).numpy()


def scatter_rows(rows, shape, order=MERGE_ORDER):
    """the way back: [M][4 C] -> [B][H][W][C]"""
    B, H, W, C = shape
    out = np.empty(shape, rows.dtype)
    r = rows.reshape(B, H // 2, W // 2, 4, C)
    for blk, (hp, wp) in enumerate(order):
        out[:, hp::2, wp::2, :] = r[:, :, :, blk, :]
    return out


def bf16_values(x):
    """fp32 -> (the nearest bf16 values as fp32, their 16-bit patterns as uint16)"""
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(torch.bfloat16)
    return t.float().numpy(), t.view(torch.int16).numpy().view(np.uint16)


def merge_inputs(shape, integer=False):
    """-> dict(x [B][H][W][C] fp32, dn [M][4 C] fp32 bf16 VALUES, dn_bits uint16, gamma [4 C], base_g, base_b [4 C]); integer: small integers
    throughout (the exact case; its mean = 0, rstd = 1 are the caller's).  x carries a per-pixel offset of a few sigma, as
    linear_reference.merge_case adds: the rows' means are far from 0 and x - mean cancels."""
    B, H, W, C = shape
    rng = np.random.default_rng(B * 1000003 + H * 10007 + W * 101 + C)
    M, K = B * (H // 2) * (W // 2), 4 * C
    if integer:
        x = rng.integers(-3, 4, shape).astype(np.float32)
        dn = rng.integers(-4, 5, (M, K)).astype(np.float32)
        g = rng.integers(-2, 3, K).astype(np.float32)
        bg, bb = rng.integers(-50, 51, K).astype(np.float32), rng.integers(-50, 51, K).astype(np.float32)
    else:
        x = (rng.standard_normal(shape) + 3.0 * rng.standard_normal((B, H, W, 1))).astype(np.float32)
        dn = (np.exp(rng.uniform(-5, 0, (M, K))) * rng.choice([-1.0, 1.0], (M, K))).astype(np.float32)
        g = (np.exp(rng.uniform(math.log(1e-2), math.log(2.0), K)) * rng.choice([-1.0, 1.0], K)).astype(np.float32)
        # baselines of the sums' own size (|sum_m| grows with M), never near 0: a lost baseline is far outside gamma(M) (|base| + sum |term|)
        bg, bb = ((max(1.0, 0.05 * M) * rng.uniform(0.5, 2.0, K) * rng.choice([-1.0, 1.0], K)).astype(np.float32) for _ in range(2))
    dn, bits = bf16_values(dn)
    return dict(x=x, dn=dn, dn_bits=bits, gamma=g, base_g=bg, base_b=bb)


def merge_ln_bwd(x, dn, g, mean, rstd, base_g, base_b, order=MERGE_ORDER):
    """-> (dx [B][H][W][C], dgamma, dbeta [4 C]) in fp64 and their bounds (bdx, bdg, bdb), from the fp32 inputs as stored"""
    xr = d(rows_of(x, order))
    M, K = xr.shape
    mu, rs = d(mean).reshape(-1, 1), d(rstd).reshape(-1, 1)
    xh = (xr - mu) * rs
    gg = d(dn) * d(g)
    s1, s2 = gg.mean(1, keepdims=True), (gg * xh).mean(1, keepdims=True)
    dxr = rs * (gg - s1 - xh * s2)
    n = -(-K // 64)
    ds1 = gamma(n + 8) * np.abs(gg).mean(1, keepdims=True)
    ds2 = gamma(n + 10) * np.abs(gg * xh).mean(1, keepdims=True)
    bdx = rs * (gamma(5) * (np.abs(gg) + np.abs(s1) + np.abs(xh * s2)) + (1 + gamma(5)) * (ds1 + np.abs(xh) * ds2))
    tg = d(dn) * xh
    dg, db = d(base_g) + tg.sum(0), d(base_b) + d(dn).sum(0)
    bdg = gamma(M + 3) * (np.abs(d(base_g)) + np.abs(tg).sum(0))
    bdb = gamma(M) * (np.abs(d(base_b)) + np.abs(d(dn)).sum(0))
    return (scatter_rows(dxr, x.shape, order), dg, db), (scatter_rows(np.broadcast_to(bdx, dxr.shape).copy(), x.shape, order), bdg, bdb)


# ---------------------------------------------------------------------------------------------------------------
# swv2_loss_finalize
# ---------------------------------------------------------------------------------------------------------------
FINALIZE_SHAPES = [(1, 1), (2, 3), (2, 73), (1, 256), (1, 257), (8, 73)]
VARIANTS = [(a, s) for a in (0, 1) for s in (0, 1)]          # (absolute, squared)


def finalize_inputs(B, C, layers, zero_plane=None):
    """-> (sums fp32 [layers][B C][2], chw fp32 [C]).  layers = 8: log-uniform magnitudes over 1e-6 .. 1e3 per (layer, plane, sum), so the
    layers are unequal; chw has large and small weights of both signs.  zero_plane: a plane whose S0 is 0 in every layer."""
    rng = np.random.default_rng(B * 7919 + C * 31 + layers)
    sums = np.exp(rng.uniform(math.log(1e-6), math.log(1e3), (layers, B * C, 2))).astype(np.float32)
    chw = (np.exp(rng.uniform(math.log(1e-3), math.log(1e2), C)) * rng.choice([-1.0, 1.0], C)).astype(np.float32)
    if zero_plane is not None:
        sums[:, zero_plane, 0] = 0.0
    return sums, chw


def loss_finalize(sums, chw, absolute, squared):
    """sums [layers][BC][2], chw [C] -> (loss, bound_loss, coef [BC], bound_coef [BC]) in fp64.  A plane with S0 = 0 under a sqrt variant
    has coef = +-inf (sign of w) and bound nan there: compare its class, not its distance."""
    layers, BC, _ = sums.shape
    S = d(sums).sum(0)
    w = d(chw)[np.arange(BC) % chw.size]
    den = np.ones(BC) if absolute else S[:, 1]
    r = S[:, 0] / den
    k_f = 2 * layers + 1 if squared else layers + 2
    with np.errstate(divide="ignore", invalid="ignore"):
        f, df = (r, np.ones(BC)) if squared else (np.sqrt(r), 0.5 / np.sqrt(r))
        coef = 2.0 * w * df / den
        bcoef = gamma(layers + 2 if squared else 2 * layers + 5) * np.abs(coef)
    loss = float(np.sum(w * f))
    bloss = gamma(math.ceil(BC / 256) + 6 + 3 + k_f + 1) * float(np.sum(np.abs(w * f)))
    return loss, bloss, coef, bcoef


def torch_l2_coef(sums, chw, absolute, squared):
    """2 d loss / d S0 by autograd through the plain-torch l2 statement of utils/losses.py (LossHandler.forward: norms = S0 (/ S1), sqrt
    unless squared, sum(chw norms)) in float64 on the layer sums"""
    S = torch.from_numpy(d(sums).sum(0)).requires_grad_(True)
    BC = S.shape[0]
    w = torch.from_numpy(d(chw))[torch.arange(BC) % chw.size]
    norms = S[:, 0]
    if not absolute:
        norms = norms / S[:, 1]
    if not squared:
        norms = torch.sqrt(norms)
    torch.sum(w * norms).backward()
    return 2.0 * S.grad[:, 0].numpy()
