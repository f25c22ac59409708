"""fp64 numpy statement of the l1 loss family as `swv2_l1_sums` / `swv2_l1_finalize` / `swv2_l1_grad` (csrc/loss_l1.hip),
`utils/losses.LossHandler` (p = 1) and `ForecastScorer.mae` define it, and the error bounds the tests hold the fp32 code to.  Shared by
tests/test_l1_loss_gpu.py and tests/test_l1_loss_host.py.

Everything is built from exactly what the kernels read: the fp32 prediction, target, row weights and channel weights, taken as exact.
    S0 = sum q |p - t|    S1 = sum q |t|    norm = S0 (absolute) or S0 / S1    loss = sum_bc chw[c] norm[b, c]
    coef[b, c] = chw[c] (absolute) or chw[c] / S1[b, c]    dprd = coef q[h] sign(p - t)    mae = S0 / (H W)

Bounds, u = 2^-24, g(k) = k u / (1 - k u) (tests/plane_reference.py).

Sums:  |S_k - S_k^ref| <= g(n + C_TERM) A_k,  A_k = sum |q| |a| in fp64 (a = p - t or t).  |q|, not q: the scorer's pole rows carry a
    slightly negative fp32 weight (tests/score_reference.py), so the terms are not all of one sign.
    C_TERM = 2 per-term roundings, counted in loss_l1.hip's l1_vec as written:
        S0  d = p - t: 1 (relative to |d| itself, however much cancels);  |d| exact;  the fma (q |d| + s, the product unrounded): 1     = 2
        S1  |t| exact;  the fma: 1                                                                                                   = 1, held to 2
    n = chain_length(H, W, slices): the longest chain of fp32 additions a term passes through under the kernel's plan
        4 ceil(v / 256)    the thread's running sum: v 16-byte vectors in the largest slice, 256 threads, 4 fma per vector and sum
        6                  wave64 butterfly
        2                  the four waves through LDS, (w0 + w1) + (w2 + w3)
        ceil(slices / 64)  swv2_l1_finalize: lane l adds the slices l, l + 64, ... in ascending order
        6                  wave64 butterfly
    The plain-torch paths sum in an order this file does not know: n = H W, any order of a sum of H W terms; their terms are q * |d|
    with a rounded product: 2 roundings too.

coef:  absolute: chw[c] itself, exact.  Relative: chw / S1 with one division: |coef - ref| <= |ref| ((1 + u) / (1 - x1) - 1), x1 = dS1 / S1 < 1.
norm:  absolute: S0, bound dS0.  Relative: one division of the two sums: (|S0| + dS0) (1 + u) / (S1 - dS1) - |S0| / S1.
loss:  the term chw norm: 1 rounding (none where the compiler fuses it into the addition); the additions: wave v's running sum over the
    planes v, v + 16, ... in ascending order, ceil(B C / 16), then the binary tree over the sixteen waves: 4.  With k = ceil(B C / 16) + 5:
        |loss - ref| <= (1 + g(k)) sum |chw| dnorm + g(k) sum |chw| |norm|.
    The torch statement adds the B C terms in an unknown order: k = B C + 1.
dprd:  no bound: exactly +-fp32(coef_got q[h]) (ONE fp32 product of the kernel's own coef) or 0, the sign from the fp64 difference of
    the fp32 inputs, which is exact.
mae:   S0 / (H W): one division: dS0 / (H W) + u |mae|.  Batch means: tests/score_reference.py::batch_mean, from the code's OWN values.
"""
import math

import numpy as np

from tests.plane_reference import BLOCKS, U, gamma, plan_slices, slice_bounds, worst  # noqa: F401  (re-exported)
from tests.score_reference import batch_mean  # noqa: F401  (re-exported)

C_TERM = 2


def chain_length(H: int, W: int, slices: int) -> int:
    v = max((hi - lo) // 4 for lo, hi in slice_bounds(H * W, slices))
    return 4 * math.ceil(v / 256) + 6 + 2 + math.ceil(slices / 64) + 6


def sums(prd, tar, q):
    """fp32 arrays [B, C, H, W] x2, [H] -> (S [B, C, 2], A [B, C, 2]) in fp64: the sums and the sums of magnitudes"""
    p, t, q = prd.astype(np.float64), tar.astype(np.float64), q.astype(np.float64).reshape(1, 1, -1, 1)
    terms = (np.abs(p - t), np.abs(t))
    S = np.stack([(q * a).sum(axis=(2, 3)) for a in terms], axis=-1)
    A = np.stack([(np.abs(q) * a).sum(axis=(2, 3)) for a in terms], axis=-1)
    return S, A


def sum_bounds(A, n: int):
    return gamma(n + C_TERM) * A


def loss(S, dS, chw, absolute: bool, k: int = None):
    """reference sums [B, C, 2] and their bounds, chw [C] fp32 -> (loss, loss bound, coef [B, C], coef bound [B, C]) in fp64;
    k: the roundings of a term on its way into the loss (default: the kernel's ceil(B C / 16) + 5)"""
    B, C = S.shape[:2]
    cw = np.broadcast_to(chw.astype(np.float64).reshape(1, C), (B, C))
    S0, S1, d0, d1 = S[..., 0], S[..., 1], dS[..., 0], dS[..., 1]
    if absolute:
        norm, dnorm, coef, dcoef = S0, d0, cw.copy(), np.zeros((B, C))
    else:
        assert np.all(S1 - d1 > 0), "degenerate plane: S1 is not above its own error bound"
        norm = S0 / S1
        dnorm = (np.abs(S0) + d0) * (1 + U) / (S1 - d1) - np.abs(S0) / S1
        coef = cw / S1
        dcoef = np.abs(coef) * ((1 + U) / (1 - d1 / S1) - 1)
    k = math.ceil(B * C / 16) + 5 if k is None else k
    bound = (1 + gamma(k)) * (np.abs(cw) * dnorm).sum() + gamma(k) * (np.abs(cw) * np.abs(norm)).sum()
    return float((cw * norm).sum()), float(bound), coef, dcoef


def grad(prd, tar, q, coef):
    """d loss / d prd in fp64 from fp64 coef [B, C]: coef q[h] sign(p - t)"""
    sg = np.sign(prd.astype(np.float64) - tar.astype(np.float64))
    return coef[:, :, None, None] * q.astype(np.float64).reshape(1, 1, -1, 1) * sg


def grad_bits(prd, tar, q, coef_got):
    """what swv2_l1_grad must store, bit for bit: +-fp32(coef_got[b, c] * q[h]) or 0 by the exact sign; fp32 arrays in, fp32 out"""
    c = (coef_got.astype(np.float32)[:, :, None] * q.astype(np.float32)[None, None, :])[..., None]          # one fp32 product
    sg = np.sign(prd.astype(np.float64) - tar.astype(np.float64))
    return np.where(sg > 0, c, np.where(sg < 0, -c, np.float32(0.0))).astype(np.float32)


def mae(S, dS, H: int, W: int):
    """-> (mae [B, C], bound [B, C])"""
    m = S[..., 0] / (H * W)
    return m, dS[..., 0] / (H * W) + U * np.abs(m)


def judge_sums(got_sums, prd, tar, q, n: int, tag=""):
    """element-by-element verdict on sums [B, C, 2] (numpy fp32); prints and returns the worst error / bound"""
    S, A = sums(prd, tar, q)
    r = worst(np.abs(got_sums.astype(np.float64) - S), sum_bounds(A, n))
    print(f"{tag} n = {n}: worst error / bound  sums {r:.3f}")
    return r
