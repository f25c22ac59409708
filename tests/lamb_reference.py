"""fp64 numpy statement of LAMB as `swv2_lamb_grad_norm` / `swv2_lamb_multi` and `utils/optim.HipLamb` define it (apex FusedLAMB), and the
error bounds the tests hold the fp32 kernels to.  Shared by tests/test_lamb_gpu.py and tests/test_lamb_host.py.

Everything is built from exactly what the kernels read: the fp32 inputs and the fp32 VALUE of every scalar argument (`Hyper` rounds
them on the way in; 1 - beta2 formed from the double 0.999 instead of fp32(0.999) is off by 3e-5 relative and misses v by 18 x its
bound).  Every output is judged from the kernel's own upstream values, so that no error is counted twice:
    m, v      with the clip divisor c formed in fp64 from the kernel's stored |g|^2, and the stored bc1, bc2
    u_ref     from the kernel's stored NEW m, v and the old p
    r         from the kernel's stored |p|^2 and |u|^2
    p         with the kernel's stored r

Bounds, u = 2^-24 (one fp32 rounding), D = SWV2_LAMB_SUM_DEPTH = 64.  Roundings counted in csrc/lamb.hip as written (an fma counts once):
    |g|^2, |p|^2   (D + 2) u of the fp64 sum.  Each term: (g inv) 1, its square 1 (|p|^2: the square only); then at most D additions
                   (the header of lamb.hip lists them: 17 + 6 + 2 per chunk, then h + 8 + 6 + 2 (+ 1) over the chunk partials, <= 62).
    |u|^2          (D + 2 + 2 * 16) u of sum u_ref^2: as above plus twice the relative error of u, which the p row below allows 16 u.
    c              2 u of sqrt(|g|^2) / max_grad_norm (sqrt, divide); exactly 1 when G <= max_grad_norm.
    bc1, bc2       exactly fp32(1 - beta^step) from the fp32 beta, 1 with bias_correction off (checked to 2 u: the C and the Python pow).
    r              4 u of sqrt(|p|^2) / sqrt(|u|^2) of the stored values (3 roundings: two square roots, one divide); exactly 1 in
                   the degenerate cases (weight_decay = 0 without use_nvlamb, |p| = 0, |u| = 0).
    m              8 u (|beta1 m| + |b3 g^|).  adam_w_mode: c 2, s = inv / c 1, g s 1, b3 g^ 1, the fma 1: <= 6 on the second term, 1 on the
                   first.  L2 mode forms g^ = g s + wd p in fp64 from the stored |g|^2 and rounds once (its two terms may cancel, so fp32
                   terms would not be small against g^): 1 + 1 + 1 = 3.
    v              12 u (beta2 v + (1 - beta2) g^^2).  g^ 4 as above, twice, + 2 products + the fma: <= 11 on the second term, 1 on the first.
    a              (m rbc1) / (sqrt(v rbc2) + eps), rbc = 1 / bc: numerator 2, denominator 2 / 2 + 1 + 1 <= 3, divide 1: 6 u |a|.
    p              2 u |p_ref| + lr r (16 u |a| + 8 u |weight_decay p|).  u = fma(wd, p, a): 6 u |a| + u |u| <= 7 u |a| + u |wd p|;
                   lr r 1 and the fma p - (lr r) u 1 more on the product and 1 on the result: lr r (9 u |a| + 3 u |wd p|) + u |p_ref|.
The issue's constants (8, 12, 16 / 8, D + 2, D + 34, 4) are kept: the counts above sit inside every one of them.
"""
from dataclasses import dataclass

import numpy as np

U = 2.0 ** -24
D = 64


def f32(x) -> float:
    return float(np.float32(x))


@dataclass
class Hyper:
    lr: float = 1e-3
    beta1: float = 0.9
    beta2: float = 0.999
    eps: float = 1e-6
    weight_decay: float = 0.01
    grad_inv_scale: float = 1.0
    max_grad_norm: float = 1.0
    step: int = 1
    adam_w_mode: bool = True
    bias_correction: bool = True
    grad_averaging: bool = True
    use_nvlamb: bool = False

    def __post_init__(self):
        for k in ("lr", "beta1", "beta2", "eps", "weight_decay", "grad_inv_scale", "max_grad_norm"):
            setattr(self, k, f32(getattr(self, k)))

    @property
    def b3(self):
        return 1.0 - self.beta1 if self.grad_averaging else 1.0

    def bias_corrections(self):
        if not self.bias_correction:
            return 1.0, 1.0
        return f32(1.0 - self.beta1 ** self.step), f32(1.0 - self.beta2 ** self.step)

    @property
    def uses_ratio(self):
        return self.use_nvlamb or self.weight_decay != 0.0


def d(x):
    return np.asarray(x, dtype=np.float64)


def grad_norm2(grads, grad_inv_scale):
    """sum over ALL gradients of (g * grad_inv_scale)^2"""
    return float(sum(np.sum((d(g) * f32(grad_inv_scale)) ** 2) for g in grads))


def clip_divisor(gnorm2, max_grad_norm):
    G = np.sqrt(float(gnorm2))
    return G / f32(max_grad_norm) if G > f32(max_grad_norm) else 1.0


def moments(p, g, m, v, h: Hyper, c):
    """(m_ref, v_ref, bound_m, bound_v, g^) from the old p, m, v, the gradient and the clip divisor c"""
    p, g, m, v = d(p), d(g), d(m), d(v)
    gh = g * h.grad_inv_scale / c
    if not h.adam_w_mode:
        gh = gh + h.weight_decay * p
    t1, t2 = h.beta1 * m, h.b3 * gh
    v_ref = h.beta2 * v + (1.0 - h.beta2) * gh * gh
    return t1 + t2, v_ref, 8 * U * (np.abs(t1) + np.abs(t2)), 12 * U * v_ref, gh


def update(p, m_new, v_new, h: Hyper, bc=None):
    """(a, u) from the NEW moments and the OLD parameter"""
    bc1, bc2 = bc if bc is not None else h.bias_corrections()
    p = d(p)
    a = (d(m_new) / bc1) / (np.sqrt(d(v_new) / bc2) + h.eps)
    return a, (a + h.weight_decay * p if h.adam_w_mode else a)


def trust_ratio(p2, u2, h: Hyper):
    if h.uses_ratio and p2 != 0 and u2 != 0:
        return float(np.sqrt(float(p2)) / np.sqrt(float(u2)))
    return 1.0


def apply(p, a, u, r, h: Hyper):
    """(p_ref, bound_p)"""
    p = d(p)
    p_ref = p - h.lr * r * u
    return p_ref, 2 * U * np.abs(p_ref) + h.lr * r * (16 * U * np.abs(a) + 8 * U * np.abs(h.weight_decay * p))


def step(ps, gs, ms, vs, h: Hyper):
    """one whole step in fp64 from fp32 (or any) inputs: lists of new (p, m, v) and the diagnostics (|g|^2, c, [(|p|^2, |u|^2, r)])"""
    g2 = grad_norm2(gs, h.grad_inv_scale)
    c = clip_divisor(g2, h.max_grad_norm)
    out_p, out_m, out_v, diag = [], [], [], []
    for p, g, m, v in zip(ps, gs, ms, vs):
        m1, v1, _, _, _ = moments(p, g, m, v, h, c)
        a, u = update(p, m1, v1, h)
        p2, u2 = float(np.sum(d(p) ** 2)), float(np.sum(u ** 2))
        r = trust_ratio(p2, u2, h)
        out_p.append(apply(p, a, u, r, h)[0]); out_m.append(m1); out_v.append(v1); diag.append((p2, u2, r))
    return out_p, out_m, out_v, (g2, c, diag)
