"""fp64 references, per-element error bounds and input generators for the window-attention core (csrc/attn*.hip).

Plain torch, no GPU: shared by tests/test_attn_exact_host.py (which checks the checkers) and tests/test_attn_exact_gpu.py (which
checks the kernels).  Every element of every output is compared; there is no floor and no share of elements left out.  Bounds are
sums of absolute values of the terms a kernel adds, so cancellation needs no exemption.

WHAT THE KERNELS READ (all tensors here are [Bw, h, L, d], un-padded, fp64 holding bf16 / fp32 values)
  q^, k^ (L2-normalised) and v as bf16; tau = logit_scale fp32, sigma = exp(min(tau, ln 100)) (clamped_logit_scale, csrc/attn_common.h); the CPB table as bf16(b log2 e) --
  the reference uses b' = bf16(fp32(b log2 e)) / log2 e; the shift mask of swv2.h in closed form: in the windows of the LAST window row
  (wi == nwh - 1: last_window_row, csrc/attn_common.h) a pair whose tokens lie on different sides of mask_thr gets -100 (finite, as in
  the reference).
  S = sigma q^.k^ + b' + m,  P = softmax(S),  o = P v,  lse = log2 sum exp(S)  (log2 domain, as stored).

BACKWARD, following the kernels' data flow from the STORED tensors it is handed (oh, lse, doh, rnorm):
  P = exp2(S log2 e - lse), delta = rowsum(dO * oh), dS = P (dO v^T - delta), dv = P^T dO,
  g_q = sigma dS k^, dq = rq (g_q - q^ (g_q . q^)) and the same for k with dS^T, q^ and rk,
  d logit_scale = [tau <= ln 100] sigma sum dS cos,  d bias = sum over windows of dS.

BOUNDS.  u = 2^-9 is the relative error of one round-to-nearest bf16 conversion, 2^-24 that of one fp32 operation.
  score error  eS = cS T + mask_eps |m|,  T = sigma sum_c |q^_c| |k^_c| + |b'|:
      row-maximum kernels (attn.hip, attn_wide.hip, attn_d256.hip): the MFMA adds d products in fp32, then one fma with sigma log2 e
      and one addition each for table and mask, then the subtraction of the maximum: (d + 3) operations of 2^-24 relative to the
      absolute sum, doubled for the hardware exp2's input/output ulp -> cS = (d + 8) 2^-23.
      operand-folded kernels (attn2.hip): sigma log2 e q^ is a two-part bf16 operand hi + lo, lo rounded at 2^-9 of |lo| <= 2^-8 |x|
      -> 2^-17 |x| per channel, the (sigma' + table maximum) reference enters the same way, fp32 accumulation on top -> cS = 2^-15.
      mask_eps = 2^-22 where the mask is added in fp32 (-100 log2 e is one constant: 2^-24, then the additions around it).
      Backward kernels that carry the mask inside the MFMA operands (swv2_attn_kernel_t.aug) hold c = -100 / sigma as hi + lo bf16
      parts (aug_key_operands, csrc/attn_common.h: the one place that builds them): |error| <= 2^-9 |lo| <= 2^-17 |c| (hi exact to 2^-8 |c|, lo to 2^-9 of that) -> mask_eps = 2^-17 there.
  e_q = max_k eS (a row's normaliser sees every key's error).
  o    : the exponentials feed the P.V product as bf16 (u each), regime 1 also sums the rounded ones (u), the row's exponent errors move
         numerator and normaliser by <= e_q each, o is stored as bf16 (u (|ref| + error)):
         |o - ref| <= 2^-8 |ref| + (2^-7 + 2 e_q) sum_k P |v|.
  lse  : log2 of a sum whose terms are off by e_q (and u when the rounded exponentials are summed: r = 1), stored as fp32:
         |lse - ref| <= log2 e (r 2^-8 + e_q) + 2^-22 (1 + |ref|).
  P in the backward: eP = e_q + 2^-22 (|lse| + |S log2 e|)   (fp32 lse, the fma and the subtraction; aug kernels: three-part bf16
         operands, 2^-24 each) + mask_eps |m| log2 e.
  dS   : A = |dO|.|v| + |dO|.|oh| bounds |dP| + |delta|; both are d-term fp32 sums (delta of aug kernels: three-part, 2^-24):
         e_qk = 2^-8 |dS| + (eP + (2d + 8) 2^-23) P A        (first term: bf16(dS) is what dq, dk and d logit_scale consume)
  dv   : bf16(P) (u) against bf16(dO), fp32 accumulation over L queries, bf16 store:
         2^-8 |ref| + sum_q (2^-8 + eP) P |dO| + L 2^-23 sum_q P |dO|.
  dq   : E_c = sigma sum_k e_qk |k^_kc| + L 2^-23 G_c, G_c = sigma sum_k |dS| |k^_kc|; through the projection
         2^-8 |ref| + rq (E_c + |q^_c| sum_c' |q^_c'| E_c') + (d + 8) 2^-23 rq (G_c + |q^_c| sum_c' |q^_c'| G_c').   dk: q and k exchanged.
  d logit_scale: sum sigma e_qk acos + N 2^-24 sigma sum |dS| acos, acos = sum_c |q^_c||k^_c| (the kernels form it as sum_k (sum_q dS q^).k^,
         so the absolute sum is over channels too), N = L + d + 64: L in-thread additions, d + 6 in the dot product and its lane
         reduction, <= 16 waves, <= 32 workgroups' atomics (the tests use <= 12).  Exactly 0 above the clamp.
         The absolute-value bound sits ~sqrt(Bw L^2) above a typical error, because it adds Bw L^2 rounding errors of bf16(dS) as if they had
         one sign.  On RANDOM data (the normal generator: continuous, independent q^, k^, v, dO) those roundings delta_qk, |delta_qk| <= a_qk / |cos| with
         a_qk = 2^-9 (|dS| + its error) |cos|, are independent and of either sign, and Hoeffding's inequality gives
         P(|sum delta cos| > t) <= 2 exp(-t^2 / (2 sum a^2)): t = 6 sqrt(sum a^2) is exceeded with probability 3e-8.  Second check there:
         sigma (6 sqrt(sum a_qk^2) + sum (1 + 2^-9)(eP + (2d + 8) 2^-23) P A acos + N 2^-24 sum |dS| acos) -- the systematic part (a row's lse
         or delta error has one sign along the row) stays a sum of absolute values.  Not applied to the structured generators, whose equal or
         mirrored values round alike.
  d bias: sum_w (eP + (2d + 8) 2^-23) P A + N 2^-24 sum_w |dS| with the UNROUNDED dS, N = Bw + 8 (a workgroup's windows, then atomics /
         the reduction over workgroups).
  underflow: fp32 and bf16 share the exponent range and the kernels may flush below 2^-126 (an exponential of a far-away key, a
         product with it, a stored result): every exponential carries an absolute 2^-126 on top of its relative error, every stored
         element another 2^-126.  TINY below; it matters only where the reference itself is below ~1e-35.
  padding: o rows >= L, columns >= d and lse rows >= L exactly 0; rows >= L of all three parts of dqkvh exactly 0; columns >= d of
         dqkvh may hold anything.
Worst measured ratios |error| / bound on an MI355X are recorded in LABNOTES.md; no constant above was fitted to them.
"""
import math
from types import SimpleNamespace

import torch

LOG2E = 1.4426950408889634
LN100 = math.log(100.0)
U8, U9 = 2.0 ** -8, 2.0 ** -9
CS_ROW_MAX = lambda d: (d + 8) * 2.0 ** -23          # noqa: E731
CS_FOLDED = 2.0 ** -15
MASK_EPS_F32, MASK_EPS_AUG = 2.0 ** -22, 2.0 ** -17
MASK_VALUE = -100.0
TINY = 2.0 ** -126


def bf16(x):
    return x.to(torch.bfloat16).to(x.dtype)


def mask_table(Bw, L, nwh, nww, mask_thr):
    """[Bw, 1, L, L] fp64: the closed-form shift mask of swv2.h (0 everywhere without one)"""
    m = torch.zeros(Bw, 1, L, L, dtype=torch.float64)
    if mask_thr > 0:
        reg = torch.arange(L) >= mask_thr
        cross = (reg[:, None] != reg[None, :]).double() * MASK_VALUE
        bw = torch.arange(Bw)
        last_row = ((bw % (nwh * nww)) // nww) == nwh - 1
        m[last_row] = cross
    return m


def forward_reference(qn, kn, v, tau, bias, nwh, nww, mask_thr):
    qn, kn, v = qn.double(), kn.double(), v.double()
    Bw, h, L, d = qn.shape
    sigma = torch.exp(torch.clamp(tau.double(), max=LN100))
    sg = sigma.view(1, h, 1, 1)
    cos = torch.einsum("bhqd,bhkd->bhqk", qn, kn)
    acos = torch.einsum("bhqd,bhkd->bhqk", qn.abs(), kn.abs())
    b = None
    S0 = sg * cos
    T = sg * acos
    if bias is not None:
        b = bf16(bias.float() * LOG2E).double() / LOG2E          # the fp32 product the packing kernel rounds (a double product flips rare bf16 ties)
        S0 = S0 + b.unsqueeze(0)
        T = T + b.abs().unsqueeze(0)
    m = mask_table(Bw, L, nwh, nww, mask_thr)
    S = S0 + m
    lse_nat = torch.logsumexp(S, -1)
    P = torch.exp(S - lse_nat.unsqueeze(-1))
    o = torch.einsum("bhqk,bhkd->bhqd", P, v)
    return SimpleNamespace(qn=qn, kn=kn, v=v, tau=tau, sigma=sigma, cos=cos, acos=acos, b=b, m=m, S0=S0, S=S, T=T, P=P, o=o,
                           lse=lse_nat * LOG2E, L=L, d=d, Bw=Bw, h=h)


def score_error(ref, cS, mask_eps=MASK_EPS_F32):
    """eS [Bw, h, L, L] (nat)"""
    return cS * ref.T + mask_eps * ref.m.abs()


def forward_bounds(ref, cS, rounded_sum):
    e_q = score_error(ref, cS).amax(-1)                                     # [Bw, h, L]
    pv = torch.einsum("bhqk,bhkd->bhqd", ref.P, ref.v.abs())
    bo = U8 * ref.o.abs() + (2.0 ** -7 + 2 * e_q).unsqueeze(-1) * pv + TINY * (1 + ref.v.abs().sum(2, keepdim=True))
    bl = LOG2E * ((U8 if rounded_sum else 0.0) + e_q) + 2.0 ** -22 * (1 + ref.lse.abs())
    return SimpleNamespace(o=bo, lse=bl, e_q=e_q)


def backward_reference(ref, oh, lse, doh, rq, rk, with_bias):
    """oh, doh [Bw, h, L, d]; lse [Bw, h, L] (log2 domain); rq, rk [Bw, h, L]: the stored tensors the kernel is handed"""
    oh, lse, doh, rq, rk = oh.double(), lse.double(), doh.double(), rq.double(), rk.double()
    sg = ref.sigma.view(1, ref.h, 1, 1)
    P = torch.exp2(ref.S * LOG2E - lse.unsqueeze(-1))
    delta = (doh * oh).sum(-1, keepdim=True)
    dP = torch.einsum("bhqd,bhkd->bhqk", doh, ref.v)
    dS = P * (dP - delta)
    dv = torch.einsum("bhqk,bhqd->bhkd", P, doh)
    gq = sg * torch.einsum("bhqk,bhkd->bhqd", dS, ref.kn)
    gk = sg * torch.einsum("bhqk,bhqd->bhkd", dS, ref.qn)
    dq = rq.unsqueeze(-1) * (gq - ref.qn * (gq * ref.qn).sum(-1, keepdim=True))
    dk = rk.unsqueeze(-1) * (gk - ref.kn * (gk * ref.kn).sum(-1, keepdim=True))
    gate = (ref.tau.float() <= torch.tensor(LN100, dtype=torch.float32)).double()      # the kernels compare in fp32
    dlogit = gate * ref.sigma * (dS * ref.cos).sum((0, 2, 3))
    dbias = dS.sum(0) if with_bias else None
    return SimpleNamespace(P=P, dS=dS, dv=dv, dq=dq, dk=dk, dlogit=dlogit, dbias=dbias, oh=oh, lse=lse, doh=doh, rq=rq, rk=rk, gate=gate)


def backward_bounds(ref, bw, cS, mask_eps, n_dbias=None):
    L, d, h = ref.L, ref.d, ref.h
    sg = ref.sigma.view(1, h, 1, 1)
    e_q = score_error(ref, cS, MASK_EPS_F32).amax(-1)
    eP = (e_q + 2.0 ** -22 * bw.lse.abs()).unsqueeze(-1) + 2.0 ** -22 * (ref.S0 * LOG2E).abs() + mask_eps * ref.m.abs() * LOG2E
    c1 = (2 * d + 8) * 2.0 ** -23
    A = torch.einsum("bhqd,bhkd->bhqk", bw.doh.abs(), ref.v.abs()) + (bw.doh.abs() * bw.oh.abs()).sum(-1, keepdim=True)
    ePA = (eP + c1) * bw.P * A + TINY * (1 + A)
    e_qk = U8 * bw.dS.abs() + ePA
    pdo = torch.einsum("bhqk,bhqd->bhkd", (U8 + eP + L * 2.0 ** -23) * bw.P, bw.doh.abs())
    b_dv = U8 * bw.dv.abs() + pdo + TINY * (1 + bw.doh.abs().sum(2, keepdim=True))

    def proj(e, G, x, r):
        ax = x.abs()
        E = e + L * 2.0 ** -23 * G
        t = E + ax * (ax * E).sum(-1, keepdim=True)
        f = (d + 8) * 2.0 ** -23 * (G + ax * (ax * G).sum(-1, keepdim=True))
        return r.unsqueeze(-1) * (t + f) + TINY
    aS = bw.dS.abs()
    b_dq = U8 * bw.dq.abs() + proj(sg * torch.einsum("bhqk,bhkd->bhqd", e_qk, ref.kn.abs()),
                                   sg * torch.einsum("bhqk,bhkd->bhqd", aS, ref.kn.abs()), ref.qn, bw.rq)
    b_dk = U8 * bw.dk.abs() + proj(sg * torch.einsum("bhqk,bhqd->bhkd", e_qk, ref.qn.abs()),
                                   sg * torch.einsum("bhqk,bhqd->bhkd", aS, ref.qn.abs()), ref.kn, bw.rk)
    n_ls = L + d + 64
    b_dl = bw.gate * ref.sigma * ((e_qk * ref.acos).sum((0, 2, 3)) + n_ls * 2.0 ** -24 * (aS * ref.acos).sum((0, 2, 3)))
    # the same sum with the ROUNDING part of e_qk counted statistically (check_backward(..., random_data=True)): see the docstring
    a_i = U9 * (aS + ePA) * ref.cos.abs()
    b_dls = bw.gate * ref.sigma * (6.0 * torch.sqrt((a_i * a_i).sum((0, 2, 3))) + ((1 + U9) * ePA * ref.acos).sum((0, 2, 3))
                                  + n_ls * 2.0 ** -24 * (aS * ref.acos).sum((0, 2, 3)))
    n_db = (ref.Bw + 8) if n_dbias is None else n_dbias
    b_db = ePA.sum(0) + n_db * 2.0 ** -24 * aS.sum(0)
    return SimpleNamespace(dv=b_dv, dq=b_dq, dk=b_dk, dlogit=b_dl, dlogit_stat=b_dls, dbias=b_db, e_qk=e_qk)


# ---------------------------------------------------------------------------------------------------------------
# checkers: every element; the worst ratio |error| / bound is returned (and must be <= 1)
# ---------------------------------------------------------------------------------------------------------------
def ratio(got, ref, bound):
    got, ref, bound = got.double(), ref.double(), bound.double()
    assert got.shape == ref.shape == bound.shape, (got.shape, ref.shape, bound.shape)
    err = (got - ref).abs()
    err = torch.where(torch.isfinite(got), err, torch.full_like(err, float("inf")))
    r = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, float("inf"))))
    return r


def check(name, got, ref, bound, report=None):
    r = ratio(got, ref, bound)
    worst = float(r.max())
    if report is not None:
        report[name] = max(report.get(name, 0.0), worst)
    if not worst <= 1.0:
        i = int(r.flatten().argmax())
        idx = tuple(int(x) for x in torch.unravel_index(torch.tensor(i), r.shape))
        raise AssertionError(f"{name}: |error| / bound = {worst:.3g} at {idx}: got {float(got.double()[idx]):.9g}, reference "
                             f"{float(ref.double()[idx]):.9g}, bound {float(bound.double()[idx]):.3g}; {int((r > 1).sum())} of {r.numel()} elements exceed")
    return worst


def check_forward(o, lse, ref, cS, rounded_sum, report=None):
    b = forward_bounds(ref, cS, rounded_sum)
    return check("o", o, ref.o, b.o, report), check("lse", lse, ref.lse, b.lse, report)


def check_backward(dq, dk, dv, dlogit, dbias, ref, bw, cS, mask_eps, report=None, random_data=False):
    b = backward_bounds(ref, bw, cS, mask_eps)
    out = [check("dv", dv, bw.dv, b.dv, report), check("dq", dq, bw.dq, b.dq, report), check("dk", dk, bw.dk, b.dk, report),
           check("dlogit", dlogit, bw.dlogit, b.dlogit, report)]
    if random_data:
        out.append(check("dlogit_stat", dlogit, bw.dlogit, b.dlogit_stat, report))
    if bw.dbias is not None:
        out.append(check("dbias", dbias, bw.dbias, b.dbias, report))
    return out


def check_padding_fwd(oh_full, lse_full, L, d):
    """oh_full [Bw, h, Lp, DP], lse_full [Bw, h, Lp] as the kernel left them (prefilled with a sentinel by the caller)"""
    assert bool((oh_full[:, :, L:, :] == 0).all()), "oh: rows >= L must be exactly 0"
    assert bool((oh_full[:, :, :, d:] == 0).all()), "oh: columns >= head_dim must be exactly 0"
    assert bool((lse_full[:, :, L:] == 0).all()), "lse: rows >= L must be exactly 0"


def check_padding_bwd(dqkvh_full, L):
    """dqkvh_full [Bw, h, 3, Lp, DP]: rows >= L of dq, dk and dv exactly 0 (columns >= head_dim may hold anything)"""
    for s, n in enumerate(("dq", "dk", "dv")):
        assert bool((dqkvh_full[:, :, s, L:, :] == 0).all()), f"{n}: rows >= L must be exactly 0"


# ---------------------------------------------------------------------------------------------------------------
# input generators: q^, k^, v, dO [Bw, h, L, d] fp32 holding bf16 values; tau [h] fp32; rq, rk [Bw, h, L] fp32
# ---------------------------------------------------------------------------------------------------------------
GENERATORS = ("normal", "counting", "peaked", "adversarial")
SIGMA_MID = 25600.0 / 373.0        # -100 / sigma lies midway between two bf16 values


def _unit(x):
    return x / x.norm(dim=-1, keepdim=True).clamp_min(1e-12)


def generate(kind, Bw, h, L, d, mask_thr, seed=0):
    g = torch.Generator().manual_seed(seed * 7919 + GENERATORS.index(kind))
    rn = lambda *s: torch.randn(*s, generator=g)          # noqa: E731
    logu = lambda *s: torch.exp(torch.rand(*s, generator=g) * math.log(1e3) - math.log(1e3))      # noqa: E731  log-uniform 1e-3 .. 1
    q, k = _unit(rn(Bw, h, L, d)), _unit(rn(Bw, h, L, d))
    v = rn(Bw, h, L, d) * logu(1, h, 1, d)
    dO = rn(Bw, h, L, d) * logu(1, h, 1, d)
    tau = math.log(10.0) + 0.5 * rn(h)
    if kind == "normal":
        tau[-1] = 5.0                                     # above the ln 100 clamp: sigma = 100, zero gradient
        if h >= 4:
            tau[0], tau[1] = math.log(27.0), math.log(30.0)     # the two sides of the fixed-maximum rule (sigma log2 e <= 40)
    elif kind == "counting":
        q = torch.zeros_like(q)
        v = (torch.arange(L).view(L, 1) % d == torch.arange(d).view(1, d)).float().expand(Bw, h, L, d).clone()
    elif kind == "peaked":
        q = k.clone()
        tau = torch.tensor([LN100, 5.0, math.log(27.0), math.log(30.0)])[torch.arange(h) % 4].clone()
    elif kind == "adversarial":
        # keys of region 0 near +a, of region 1 near -a; each query aligned with the OTHER region's keys and opposed to its own
        thr = mask_thr if mask_thr > 0 else L // 2
        a = _unit(rn(Bw, h, 1, d))
        sign = torch.where(torch.arange(L) >= thr, -1.0, 1.0).view(1, 1, L, 1)
        k = _unit(sign * a + 0.05 * rn(Bw, h, L, d))
        q = _unit(-sign * a + 0.05 * rn(Bw, h, L, d))
        # (-100 / sigma is exact in bf16 at sigma = 100 and 80: the midpoint value comes first so that two-head cases have it)
        tau = torch.log(torch.tensor([SIGMA_MID, 100.0, 80.0]))[torch.arange(h) % 3].clone()
    else:
        raise ValueError(kind)
    rq, rk = torch.rand(Bw, h, L, generator=g) + 0.5, torch.rand(Bw, h, L, generator=g) + 0.5
    return SimpleNamespace(qn=bf16(q.float()), kn=bf16(k.float()), v=bf16(v.float()), dO=bf16(dO.float()), tau=tau.float(), rq=rq.float(),
                           rk=rk.float())


def make_bias(h, L, seed=0):
    g = torch.Generator().manual_seed(1000 + seed)
    return torch.randn(h, L, L, generator=g)


# kernel layouts: [Bw, h, L, d] <-> zero-padded [Bw, h, (parts,) Lp, DP]
def pad_heads(parts, Lp, DP, dtype=torch.float32):
    Bw, h, L, d = parts[0].shape
    out = torch.zeros(Bw, h, len(parts), Lp, DP, dtype=dtype)
    for i, p in enumerate(parts):
        out[:, :, i, :L, :d] = p
    return out


def pad_rows(x, Lp):
    Bw, h, L = x.shape
    out = torch.zeros(Bw, h, Lp, dtype=x.dtype)
    out[:, :, :L] = x
    return out


# ---------------------------------------------------------------------------------------------------------------
# The case table of tests/test_attn_exact_gpu.py, pinned without a GPU by tests/test_host_and_cabi.py.
# fwd / bwd: the kernel the case is FILED under, "FAMILY<LT,DK,LFIX>" + the arithmetic variants of the first-generation backward
# (+aug: statistics and mask inside the MFMA operands, +biaslds: table image in LDS, +qg: q / dO fragments from global memory).
# bias: None, "raw" (fp32 table only) or "packed" (swv2_attn_pack_bias as well).  thr: "mid" = the shifted block's threshold
# (wh - wh // 2) * ww, or an explicit mask_thr (0 = no mask; "last" = L - 1).  nw = windows per sample (nwh, nww), B = 2 samples: the
# windows of the last window row carry the mask, the others do not, so a masked case runs both branches.
# fdbg / bdbg: swv2_attn_args.dbg of the two launches.  mc = max_chunks.  dest: where d bias goes (atomics / ws / partials).
# ---------------------------------------------------------------------------------------------------------------
DBG = {"FIRST_GEN": 16, "PLAIN_STATS": 8192, "BWD_TWO_PHASE": 32}


def _c(wh, ww, d, h, bias, fwd, bwd, thr="mid", nw=(2, 2), fdbg=0, bdbg=0, mc=64, dest="atomics"):
    return SimpleNamespace(wh=wh, ww=ww, L=wh * ww, d=d, h=h, bias=bias, fwd=fwd, bwd=bwd, thr=thr, nw=nw, fdbg=fdbg, bdbg=bdbg, mc=mc, dest=dest)


def case_id(c):
    s = f"{c.fwd}-{c.bwd}-L{c.L}-d{c.d}-h{c.h}-{c.bias or 'nobias'}-thr{c.thr}-{c.nw[0]}x{c.nw[1]}-mc{c.mc}"
    if c.bias:
        s += "-" + c.dest
    if c.fdbg or c.bdbg:
        s += f"-dbg{c.fdbg}.{c.bdbg}"
    return s.replace("FIRST_GEN", "FG")


def case_thr(c):
    return {"mid": (c.wh - c.wh // 2) * c.ww, "last": c.L - 1}.get(c.thr, c.thr)


FG, PS, TP = DBG["FIRST_GEN"], DBG["PLAIN_STATS"], DBG["BWD_TWO_PHASE"]
CASES = [
    # ---- 64-row layout: first generation only
    _c(3, 3, 4, 2, None, "FIRST_GEN<4,1,0>", "FIRST_GEN<4,1,0>+aug"),                               # under one key tile
    _c(4, 4, 16, 2, "raw", "FIRST_GEN<4,1,0>", "FIRST_GEN<4,1,0>+biaslds"),                         # exactly one tile
    _c(6, 9, 16, 4, None, "FIRST_GEN<4,1,54>", "FIRST_GEN<4,1,54>+aug", mc=3),
    _c(6, 9, 4, 2, "packed", "FIRST_GEN<4,1,54>", "FIRST_GEN<4,1,54>+aug+biaslds", dest="ws"),
    _c(6, 9, 16, 2, "raw", "FIRST_GEN<4,1,54>", "FIRST_GEN<4,1,54>+biaslds", bdbg=PS, mc=1),
    _c(8, 8, 16, 2, None, "FIRST_GEN<4,1,0>", "FIRST_GEN<4,1,0>+aug", thr=1),                      # no padding; first token alone in region 0
    _c(8, 8, 16, 2, "packed", "FIRST_GEN<4,1,0>", "FIRST_GEN<4,1,0>+biaslds", thr="last", dest="partials", mc=3),
    _c(3, 3, 20, 2, None, "FIRST_GEN<4,2,0>", "FIRST_GEN<4,2,0>+aug"),
    _c(8, 8, 32, 2, "raw", "FIRST_GEN<4,2,0>", "FIRST_GEN<4,2,0>+biaslds"),
    _c(8, 8, 32, 2, None, "FIRST_GEN<4,2,0>", "FIRST_GEN<4,2,0>", bdbg=PS),
    _c(4, 4, 36, 2, None, "FIRST_GEN<4,4,0>", "FIRST_GEN<4,4,0>"),
    _c(8, 8, 64, 2, "packed", "FIRST_GEN<4,4,0>", "FIRST_GEN<4,4,0>", dest="ws", mc=3),
    _c(3, 3, 68, 2, None, "FIRST_GEN<4,6,0>", "FIRST_GEN<4,6,0>"),
    _c(8, 8, 96, 2, "raw", "FIRST_GEN<4,6,0>", "FIRST_GEN<4,6,0>"),
    _c(4, 4, 100, 2, None, "FIRST_GEN<4,8,0>", "FIRST_GEN<4,8,0>"),
    _c(8, 8, 128, 2, "packed", "FIRST_GEN<4,8,0>", "FIRST_GEN<4,8,0>", dest="partials"),
    # ---- 176-row layout, 16-wide slots
    _c(5, 13, 4, 2, None, "FIRST_GEN<11,1,0>", "STREAM<11,1,0>+aug"),                               # tiles 5 .. 10 pure padding
    _c(5, 13, 16, 2, "raw", "FIRST_GEN<11,1,0>", "FIRST_GEN<11,1,0>+biaslds"),
    _c(3, 53, 16, 8, None, "FIRST_GEN<11,1,0>", "STREAM<11,1,0>+aug", nw=(3, 2), mc=1),             # last area below attn2.hip; 12 windows per workgroup
    _c(3, 53, 16, 2, "packed", "FIRST_GEN<11,1,0>", "FIRST_GEN<11,1,0>+biaslds", dest="ws", mc=3),
    _c(8, 20, 16, 2, None, "FWD3<11,1,0>", "STREAM<11,1,0>+aug", mc=3),
    _c(8, 20, 16, 2, "packed", "FWD3B<11,1,0>", "FIRST_GEN<11,1,0>+biaslds"),
    _c(9, 18, 16, 8, None, "FWD3<11,1,162>", "STREAM<11,1,162>+aug", nw=(3, 2)),
    _c(9, 18, 16, 2, None, "FIRST_GEN<11,1,162>", "FIRST_GEN<11,1,162>+aug", fdbg=FG, bdbg=TP, mc=3),
    _c(9, 18, 16, 2, None, "FWD3<11,1,162>", "FIRST_GEN<11,1,162>", thr=0, bdbg=PS),
    _c(9, 18, 16, 4, "packed", "FWD3B<11,1,162>", "FIRST_GEN<11,1,162>+aug+biaslds", dest="partials"),
    _c(9, 18, 16, 2, "raw", "FIRST_GEN<11,1,162>", "FIRST_GEN<11,1,162>+aug+biaslds", mc=3),
    _c(9, 18, 16, 2, "packed", "FWD3B<11,1,162>", "FIRST_GEN<11,1,162>+aug+biaslds", thr=0, dest="ws", mc=1),
    _c(5, 35, 16, 2, None, "FWD3<11,1,0>", "STREAM<11,1,0>+aug", thr=1),
    _c(5, 35, 16, 2, "packed", "FWD3B<11,1,0>", "FIRST_GEN<11,1,0>+biaslds", thr="last"),
    _c(11, 16, 16, 2, None, "FWD3<11,1,0>", "STREAM<11,1,0>+aug", thr="last"),                       # no padding
    _c(11, 16, 16, 2, "packed", "FWD3B<11,1,0>", "FIRST_GEN<11,1,0>+biaslds", nw=(1, 2)),          # one window row: every window masked
    _c(11, 16, 4, 2, None, "FIRST_GEN<11,1,0>", "FIRST_GEN<11,1,0>+aug", fdbg=FG, bdbg=TP),
    # ---- 176-row layout, 32-wide slots
    _c(5, 13, 20, 2, None, "FIRST_GEN<11,2,0>", "FIRST_GEN<11,2,0>+aug"),
    _c(8, 20, 32, 2, None, "FWD3W<11,2,0>", "FIRST_GEN<11,2,0>+aug", mc=3),
    _c(9, 18, 20, 2, None, "FWD3W<11,2,162>", "FIRST_GEN<11,2,162>+aug"),
    _c(9, 18, 32, 2, "raw", "FIRST_GEN<11,2,162>", "FIRST_GEN<11,2,162>"),
    _c(5, 35, 32, 2, None, "FWD3W<11,2,0>", "FIRST_GEN<11,2,0>+aug", thr=1),
    _c(11, 16, 32, 2, None, "FWD3W<11,2,0>", "FIRST_GEN<11,2,0>+aug", thr="last"),
    _c(11, 16, 32, 2, "packed", "FIRST_GEN<11,2,0>", "FIRST_GEN<11,2,0>", dest="ws"),
    _c(11, 16, 20, 2, None, "FIRST_GEN<11,2,0>", "FIRST_GEN<11,2,0>", fdbg=FG, bdbg=PS),
    # ---- 176-row layout, wider slots
    _c(5, 13, 36, 2, None, "FIRST_GEN<11,4,0>", "FIRST_GEN<11,4,0>"),
    _c(11, 16, 64, 2, "raw", "FIRST_GEN<11,4,0>", "FIRST_GEN<11,4,0>", mc=3),
    _c(5, 13, 68, 2, None, "WIDE<11,6,0>", "WIDE<11,6,0>"),
    _c(3, 53, 96, 2, None, "WIDE<11,6,0>", "WIDE<11,6,0>", mc=3),
    _c(8, 20, 96, 2, None, "WIDE<11,6,0>", "WIDE<11,6,0>"),
    _c(9, 18, 96, 2, None, "WIDE<11,6,162>", "WIDE<11,6,162>"),
    _c(9, 18, 68, 2, None, "WIDE<11,6,162>", "WIDE<11,6,162>", thr=0, mc=1),
    _c(5, 35, 68, 2, None, "WIDE<11,6,0>", "WIDE<11,6,0>", thr=1),
    _c(11, 16, 68, 2, None, "WIDE<11,6,0>", "WIDE<11,6,0>", thr="last"),
    _c(5, 13, 68, 2, "raw", "FIRST_GEN<11,6,0>", "FIRST_GEN<11,6,0>+qg"),
    _c(11, 16, 96, 2, None, "FIRST_GEN<11,6,0>", "FIRST_GEN<11,6,0>+qg", fdbg=FG, bdbg=FG),
    _c(5, 13, 100, 2, None, "FIRST_GEN<11,8,0>", "FIRST_GEN<11,8,0>+qg"),
    _c(11, 16, 128, 2, "packed", "FIRST_GEN<11,8,0>", "FIRST_GEN<11,8,0>+qg"),
    # ---- 256-channel heads
    _c(5, 13, 256, 2, None, "D256<11,16,0>", "D256<11,16,0>"),
    _c(9, 18, 256, 2, None, "D256<11,16,162>", "D256<11,16,162>", mc=3),
    _c(11, 16, 256, 2, None, "D256<11,16,0>", "D256<11,16,0>", thr="last"),
]

# ---- The first-generation matrix: EVERY instantiation of attn_fwd_kernel / attn_bwd_kernel (SWV2_ATTN_ROWS of csrc/attn.hip) x {no
# table, raw table, packed table} x {smallest, largest window area of its layout} (the rows specialised for one area have that area only).
# The launchers take another data path for each table form (bias converted in the kernel, or the packed register / LDS images), and a
# table at an L well below Lp is where a padded table row or column would leak.  SWV2_ATTN_FIRST_GEN on the forward and
# SWV2_ATTN_BWD_TWO_PHASE | SWV2_ATTN_FIRST_GEN on the backward select the first generation where another family is the default; they
# change nothing elsewhere.  The library refuses none of these combinations.  Backward variants per row, written out by hand:
# (without a table, with a table).
FIRST_GEN_ROWS = {
    (4, 1, 54): ("+aug", "+aug+biaslds"), (4, 1, 0): ("+aug", "+biaslds"), (4, 2, 0): ("+aug", "+biaslds"), (4, 4, 0): ("", ""),
    (4, 6, 0): ("", ""), (4, 8, 0): ("", ""),
    (11, 1, 162): ("+aug", "+aug+biaslds"), (11, 1, 0): ("+aug", "+biaslds"), (11, 2, 162): ("+aug", ""), (11, 2, 0): ("+aug", ""),
    (11, 4, 0): ("", ""), (11, 6, 0): ("+qg", "+qg"), (11, 8, 0): ("+qg", "+qg"),
}
_SLOT_DIMS = {1: (4, 16), 2: (20, 32), 4: (36, 64), 6: (68, 96), 8: (100, 128)}      # both ends of every head slot


def _matrix():
    out, n = [], 0
    for (LT, DK, LFIX), (v_none, v_tab) in FIRST_GEN_ROWS.items():
        if LFIX:
            shapes = [((6, 9) if LFIX == 54 else (9, 18), None)]
        else:
            shapes = [((3, 3) if LT == 4 else (5, 13), 0), ((8, 8) if LT == 4 else (11, 16), 1)]
        for (wh, ww), end in shapes:
            for form in (None, "raw", "packed"):
                d = _SLOT_DIMS[DK][n % 2 if end is None else end]
                name = f"FIRST_GEN<{LT},{DK},{LFIX}>"
                out.append(_c(wh, ww, d, 2, form, name, name + (v_tab if form else v_none), thr=("mid", 1, "last")[n % 3], fdbg=FG, bdbg=TP | FG,
                              mc=(64, 3, 1)[n % 3], dest=("atomics", "ws", "partials")[(n // 3 + n) % 3]))
                n += 1
    return out


CASES += _matrix()


def kernel_name(info, names, bwd):
    """swv2_attn_kernel_t -> the string a case is filed under"""
    s = f"{names[info.family]}<{info.LT},{info.DK},{info.LFIX}>"
    if bwd:
        s += ("+aug" if info.aug else "") + ("+biaslds" if info.bias_lds else "") + ("+qg" if info.qg else "")
    return s
