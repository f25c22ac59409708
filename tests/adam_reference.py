"""fp64 numpy statement of one Adam step as `swv2_adam_multi` / `swv2_adam_step` (csrc/rowops.hip) and `utils/optim.HipAdam` define it, the
same step with the scalars `torch.optim.Adam` forms, and the elementwise error bounds the tests hold the fp32 kernels to.  Shared by
tests/test_adam_host.py and tests/test_adam_gpu.py, inputs included (`CASES`, `case_inputs`), so that the host twins run on the GPU test's inputs.

One step is (p, g, m, v, lr, beta1, beta2, eps, step, inv) -> (p', m', v'):
    g^ = g inv          m' = beta1 m + (1 - beta1) g^          v' = beta2 v + (1 - beta2) g^ g^
    bc1 = 1 - beta1^step    step_size = lr / bc1    bc2_sqrt = sqrt(1 - beta2^step)
    p' = p - step_size m' / (sqrt(v') / bc2_sqrt + eps)

`step_abi`: every hyper-parameter enters as the fp32 VALUE the C ABI receives (`float lr, beta1, beta2, eps, grad_inv_scale`); the scalars
are then formed exactly (fp64) from those values.  `step_torch`: torch's scalars.  torch keeps the hyper-parameters as Python doubles, forms
1 - beta1, 1 - beta2, lr / (1 - beta1^step) and sqrt(1 - beta2^step) in double and hands each to an fp32 kernel, which rounds it once
(`cast`; with `cast=float` nothing is rounded and the statement is torch's float64 Adam, which test_adam_host.py checks to 1e-12 against
`torch.optim.Adam` itself).  exp_avg is a lerp, m + w (g^ - m) with w = cast(1 - beta1): beta1 never enters it.  The gap between the two
statements is what the float ABI costs; no bound below contains it.

p' is judged from the kernel's own stored m', v' (the rule of tests/lamb_reference.py), so no error is counted twice and errors do not
compound through a chain of steps: each step starts from the state the kernel itself left.

Bounds.  u = 2^-24 is one fp32 rounding, gamma(k) = k u / (1 - k u) >= (1 + u)^k - 1.  The library is compiled with `hipcc -O3 -std=c++17`
and nothing else (`_lib.build_library`, called by `__graft_entry__.build()`): no fast-math flag, and hipcc's default
`-fhip-fp32-correctly-rounded-divide-sqrt` stays on, so `sqrtf` and `/` are correctly rounded (the kernels' code shows it: v_sqrt_f32
followed by the one-ulp correction, v_div_scale / v_div_fmas / v_div_fixup) and count ONE rounding each, not two.  fp contraction is on
(hipcc's default), so a * b + c may be one fma or two roundings; every count below holds for either.  The inputs of the tests keep every
intermediate in fp32's normal range, so no absolute (subnormal) term is needed; an exact 0 has error 0.
    g^           one rounding.
    m'           t1 = beta1 m, t2 = (1 - beta1) g^.  t2 carries g^ (1), the subtraction 1.f - beta1 (1; exact for beta1 >= 1/2), and then either
                 its own product (1) and the fma (1), or the fma alone with t1's product rounded instead; t1 its product (0 or 1) and the
                 final rounding (1).  For either contraction and for none:  |m' - m_ref| <= gamma(2) |t1| + gamma(4) |t2|.
    v'           t1 = beta2 v, t2 = (1 - beta2) g^ g^ formed as ((1 - beta2) g^) g^: g^ twice (2), 1.f - beta2 (1), two products (2; one of
                 them may be the fma), the final rounding (1):  |v' - v_ref| <= gamma(2) |t1| + gamma(6) |t2|.
    host scalars powf is allowed 2 ulp = 4 u relative.  In bc = 1 - beta^t an error of u in beta^t is u beta^t / (1 - beta^t) relative to bc;
                 the subtraction rounds once more:       e_bc(beta, t) = 4 u beta^t / (1 - beta^t) + u
                 step_size = lr / bc1, one division:     e1 = e_bc(beta1, t) + u
                 bc2_sqrt = sqrtf(bc2), sqrt halves a relative error and rounds once:   e2 = e_bc(beta2, t) / 2 + u
    the update   x = step_size m' / (sqrt(v') / bc2_sqrt + eps) from the stored m', v': sqrtf 1, the division by bc2_sqrt 1, + eps 1 (both
                 addends are positive, so the denominator's relative error is at most its larger part's), the product step_size m' 1, the
                 division 1; no fma can form across a division.  Relative error of x:
                     E = (1 + gamma(5)) (1 + e1) (1 + e2 / (1 - e2)) - 1
    p'           p - x rounds once:  |p' - p_ref| <= E |x| + u (|p_ref| + E |x|).
"""
import math

import numpy as np

U = 2.0 ** -24
CHUNK = 4096
SIZES = [1, 5, 4095, 4096, 4097, 3 * 4096 + 5, 70 * 4096 + 123]
GRID_CAP = 8192 * 256            # adam_kernel: threads in the capped grid


def f32(x) -> float:
    return float(np.float32(x))


def d(x):
    return np.asarray(x, dtype=np.float64)


def gamma(k):
    return k * U / (1.0 - k * U)


# ---------------------------------------------------------------------------------------------------------------
# the scalars
# ---------------------------------------------------------------------------------------------------------------
def abi_scalars(lr, beta1, beta2, eps, step, inv=1.0):
    """what the kernels' arithmetic means, exactly, given the fp32 values of the arguments"""
    lr, b1, b2, eps, inv = (f32(x) for x in (lr, beta1, beta2, eps, inv))
    return dict(b1=b1, w1=1.0 - b1, b2=b2, w2=1.0 - b2, step_size=lr / (1.0 - b1 ** step), bc2_sqrt=math.sqrt(1.0 - b2 ** step), eps=eps,
                inv=inv)


def torch_scalars(lr, beta1, beta2, eps, step, inv=1.0, cast=f32):
    """torch.optim.Adam's: Python doubles, each rounded by `cast` where torch hands it to an fp32 kernel.  exp_avg.lerp_(g, 1 - beta1) is
    m + w (g - m) = (1 - w) m + w g; exp_avg_sq.mul_(beta2).addcmul_(g, g, value=1 - beta2); the gradient scale is this project's own
    argument (torch's path is handed gradients multiplied by fp32(inv) beforehand)."""
    w1 = cast(1.0 - beta1)
    return dict(b1=1.0 - w1, w1=w1, b2=cast(beta2), w2=cast(1.0 - beta2), step_size=cast(lr / (1.0 - beta1 ** step)),
                bc2_sqrt=cast(math.sqrt(1.0 - beta2 ** step)), eps=cast(eps), inv=f32(inv))


def scalar_errors(beta1, beta2, step):
    """(e1, e2): the relative error allowed to the host's fp32 step_size and bc2_sqrt against `abi_scalars`"""
    def e_bc(b, t):
        bt = f32(b) ** t
        return 4 * U * bt / (1.0 - bt) + U
    return e_bc(beta1, step) + U, e_bc(beta2, step) / 2 + U


# ---------------------------------------------------------------------------------------------------------------
# the step
# ---------------------------------------------------------------------------------------------------------------
def moments(g, m, v, s):
    """(m_ref, v_ref, bound_m, bound_v) from the old moments and the un-scaled gradient; s: a scalars dict"""
    gh = d(g) * s["inv"]
    t1, t2 = s["b1"] * d(m), s["w1"] * gh
    q1, q2 = s["b2"] * d(v), s["w2"] * gh * gh
    return t1 + t2, q1 + q2, gamma(2) * np.abs(t1) + gamma(4) * np.abs(t2), gamma(2) * q1 + gamma(6) * q2


def update(p, m_new, v_new, s, e=(0.0, 0.0)):
    """(p_ref, bound_p) from the NEW moments (the kernel's stored ones) and the old parameter; e = scalar_errors(...)"""
    with np.errstate(invalid="ignore"):             # (a defective v' < 0 becomes a NaN, which `ratio` reports as outside)
        x = s["step_size"] * d(m_new) / (np.sqrt(d(v_new)) / s["bc2_sqrt"] + s["eps"])
    p_ref = d(p) - x
    E = (1 + gamma(5)) * (1 + e[0]) * (1 + e[1] / (1 - e[1])) - 1
    return p_ref, E * np.abs(x) + U * (np.abs(p_ref) + E * np.abs(x))


def step_abi(p, g, m, v, lr, beta1, beta2, eps, step, inv=1.0):
    """the whole step in fp64 with the C ABI's scalars: (p', m', v'), p' from the fp64 moments"""
    s = abi_scalars(lr, beta1, beta2, eps, step, inv)
    m1, v1, _, _ = moments(g, m, v, s)
    return update(p, m1, v1, s)[0], m1, v1


def step_torch(p, g, m, v, lr, beta1, beta2, eps, step, inv=1.0, cast=f32):
    s = torch_scalars(lr, beta1, beta2, eps, step, inv, cast)
    m1, v1, _, _ = moments(g, m, v, s)
    return update(p, m1, v1, s)[0], m1, v1


def ratio(err, bound):
    """largest error / bound over the elements (an exact 0 <= 0 counts as 0); inf when anything is not finite"""
    err, bound = np.atleast_1d(np.abs(d(err))), np.atleast_1d(d(bound))
    if not (np.all(np.isfinite(err)) and np.all(np.isfinite(bound))):
        return float("inf")
    return float(np.max(np.where(err == 0, 0.0, err / np.where(bound == 0, np.finfo(np.float64).tiny, bound))))


def judge(old, g, new, hyper, step, stmt="abi"):
    """{m, v, p: worst error / bound} of one step's stored results `new` = (p', m', v') against the statement, from the state `old` =
    (p, m, v) it started from; hyper = (lr, beta1, beta2, eps, inv).  stmt "torch": the same bounds around torch's statement."""
    lr, b1, b2, eps, inv = hyper
    s = abi_scalars(lr, b1, b2, eps, step, inv) if stmt == "abi" else torch_scalars(lr, b1, b2, eps, step, inv)
    m_ref, v_ref, bm, bv = moments(g, old[1], old[2], s)
    p_ref, bp = update(old[0], new[1], new[2], s, scalar_errors(b1, b2, step))
    return dict(m=ratio(new[1] - m_ref, bm), v=ratio(new[2] - v_ref, bv), p=ratio(new[0] - p_ref, bp))


def judge_against_torch(old, g, new, hyper, step):
    """{m, v, p: worst error / (bound + gap)} of the stored results against TORCH's statement, the bound being the one around the ABI's
    statement and the gap the elementwise distance between the two statements on these inputs"""
    lr, b1, b2, eps, inv = hyper
    sa, st = abi_scalars(lr, b1, b2, eps, step, inv), torch_scalars(lr, b1, b2, eps, step, inv)
    _, _, bm, bv = moments(g, old[1], old[2], sa)
    _, bp = update(old[0], new[1], new[2], sa, scalar_errors(b1, b2, step))
    m_t, v_t, _, _ = moments(g, old[1], old[2], st)
    p_t, _ = update(old[0], new[1], new[2], st)
    gaps = torch_gap(old, g, new, hyper, step)[1]
    return dict(m=ratio(new[1] - m_t, bm + gaps["m"]), v=ratio(new[2] - v_t, bv + gaps["v"]), p=ratio(new[0] - p_t, bp + gaps["p"]))


def torch_gap(old, g, new, hyper, step):
    """what the float ABI costs on these inputs: per output the largest |abi statement - torch statement| over the elements, in units of
    u times the statement's own magnitude (|beta1 m| + |(1 - beta1) g^| for m', whose two terms may cancel; v'; and for p the size of the
    update), and the elementwise gaps themselves"""
    lr, b1, b2, eps, inv = hyper
    sa, st = abi_scalars(lr, b1, b2, eps, step, inv), torch_scalars(lr, b1, b2, eps, step, inv)
    ma, va, _, _ = moments(g, old[1], old[2], sa)
    mt, vt, _, _ = moments(g, old[1], old[2], st)
    pa, _ = update(old[0], new[1], new[2], sa)
    pt, _ = update(old[0], new[1], new[2], st)
    x = np.abs(d(old[0]) - pa)
    rel = lambda gap, mag: float(np.max(np.where(mag > 0, gap / np.where(mag > 0, mag, 1.0), 0.0))) / U
    gaps = dict(m=np.abs(ma - mt), v=np.abs(va - vt), p=np.abs(pa - pt))
    mag_m = np.abs(sa["b1"] * d(old[1])) + np.abs(sa["w1"] * d(g) * sa["inv"])
    return dict(m=rel(gaps["m"], mag_m), v=rel(gaps["v"], va), p=rel(gaps["p"], x)), gaps


# ---------------------------------------------------------------------------------------------------------------
# the inputs of the GPU test (and of the host twins)
# ---------------------------------------------------------------------------------------------------------------
EPS = 1e-8
LRS = [2e-3, 1e-3, 3e-3, 5e-4]                      # lr changes between the chained steps
GSCALE = 1e-2                                       # |g inv| is log-uniform over GSCALE * (e^-6 .. 1): sqrt(v') reaches down to eps's size
CASES = {"b%s_inv%s_step%d" % (str(b2)[2:], "1" if inv == 1.0 else "1024th", s0): dict(betas=(0.9, b2), inv=inv, step0=s0)
         for b2 in (0.95, 0.999) for inv in (1.0, 1.0 / 1024) for s0 in (1, 1000)}


def carry_tail(x):
    """the last element of a tensor whose last chunk is partial is 100 x the largest other magnitude (tests/test_lamb_gpu.py)"""
    if x.size % CHUNK and x.size > 1:
        x[-1] = 100.0 * np.abs(x[:-1]).max()
    return x


def draw_p(rng, n):
    return carry_tail((0.02 * rng.standard_normal(n)).astype(np.float32))


def draw_g(rng, n, scale):
    """log-uniform magnitudes over e^-6 .. 1, times scale, random signs"""
    return carry_tail((scale * np.exp(rng.uniform(-6, 0, n)) * rng.choice([-1.0, 1.0], n)).astype(np.float32))


def zero_positions(n):
    """planted g = 0 (every step), m = v = 0 (at the start): p must not move there.  Never the carried tail element."""
    return np.arange(3, n - 1, 7)


def case_inputs(name, sizes=SIZES):
    """-> dict(p, m, v: lists of fp32 start tensors; grads[k][i]: the gradient of tensor i at chained step k; hypers[k] = (lr, beta1, beta2,
    eps, inv); steps[k])"""
    c = CASES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    inv, s0 = c["inv"], c["step0"]
    p = [draw_p(rng, n) for n in sizes]
    if s0 == 1:
        m, v = [np.zeros(n, np.float32) for n in sizes], [np.zeros(n, np.float32) for n in sizes]
    else:                                           # a run in progress: moments of the gradients' own size
        m = [(0.3 * GSCALE * rng.standard_normal(n)).astype(np.float32) for n in sizes]
        v = [(GSCALE ** 2 * np.exp(rng.uniform(-12, 0, n))).astype(np.float32) for n in sizes]
    grads = [[draw_g(rng, n, GSCALE / inv) for n in sizes] for _ in LRS]
    for i, n in enumerate(sizes):
        z = zero_positions(n)
        m[i][z], v[i][z] = 0.0, 0.0
        for gk in grads:
            gk[i][z] = 0.0
    return dict(p=p, m=m, v=v, grads=grads, hypers=[(lr, c["betas"][0], c["betas"][1], EPS, inv) for lr in LRS],
                steps=[s0 + k for k in range(len(LRS))])
