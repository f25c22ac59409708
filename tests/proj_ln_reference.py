"""fp64 references and per-element bound checkers for proj + LayerNorm1 (swv2_proj_ln_fwd / _bwd) and the row-table
LayerNorm (swv2_ln_residual_fwd / _bwd), shared by tests/test_proj_ln_exact_gpu.py (the kernels) and
tests/test_proj_ln_exact_host.py (the references and bounds themselves, no GPU).  Everything here is plain torch and runs on
whatever device its inputs live on.

Layouts: window rows m = w * Lp + t (t >= Lv: padded rows of a window); rowidx[m] = destination row or -1; oh / doh are
head-major [Bw][heads][Lp][slot] with the real head width in the first 3/4 of a slot (12 of 16, 24 of 32) and zeros behind it.

Bounds (derived, not measured; C = channels, K = heads * slot; the worst measured ratios stand beside the constants in
test_proj_ln_exact_gpu.py):
  a1     |a1 - v| <= 2^-8 |v| + K 2^-23 A          v = oh wp^T + bp, A = |oh| |wp|^T + |bp|.  bf16 round-to-nearest moves the fp32
                                                    value by <= 2^-8 of itself; K fp32 accumulations in any order lose <= K 2^-24 A (doubled)
  mean   |mean - mu| <= C 2^-23 mean_c |a1|         mu from the saved a1 in fp64; C fp32 additions, doubled
  rstd   |rstd / rho - 1| <= C 2^-22                rho = (var + eps)^-1/2 from the saved a1 in fp64
  y      |y - ref| <= 2^-20 (|x| + |s| (|a1 - mean| rstd |gamma| + |beta|))     ref from the SAVED a1, mean, rstd: about six fp32
                                                    roundings of the terms of this sum (6 * 2^-24 = 0.375 * 2^-20)
  da1    |da1 - ref| <= 2^-8 |ref| + C 2^-22 rstd (|g| + T1 + |xhat| T2)        d = s dy[dst], xhat = (a1 - mean) rstd, g = d gamma,
                                                    T1 = mean_c |g|, T2 = mean_c |g xhat|; ref = rstd (g - mean_c g - xhat mean_c (g xhat)),
                                                    exactly 0 on rows with a negative table entry
  doh    |doh - ref| <= 2^-8 |ref| + C 2^-23 sum_c |wpt| |da1|                  ref from the kernel's own bf16 da1
  dgamma |dgamma - base - sum_rows d xhat| <= C_FOLD sum_rows |d xhat| + 2^-24 |base|, dbeta alike with d; rows with a table entry
         >= 0, each once.  C_FOLD = 51 * 2^-24 follows from the fold's own order (see C_FOLD below)
2^-8 is bf16's unit roundoff (8 significant bits: a correctly rounded value at the bottom of a binade is 2^-8 of itself away), so
a1, da1 and doh reach their bound's first term by construction; what the fp32 arithmetic adds is reported apart ("beyond rounding").
"""
import math
import types

import torch

BF = torch.bfloat16
F64 = torch.float64
EPS32 = float(torch.tensor(1e-5, dtype=torch.float32))       # the eps the kernels read: 1e-5 rounded to fp32
SENT = -12288.0                                               # guard / prefill value: exact in bf16 and fp32, far from every result
RPS = 100                                                     # rows per sample: deliberately no multiple of Lv or of a tile height
# dgamma / dbeta: fp32 column reductions over rows.  The bar was first taken from the weight gradients (C32 = 2^-20 of
# test_wgrad_exact_gpu.py); the fused backward measured 0.31 of it on dbeta (C 32, 176 rows: the last row's large contribution passes
# through most of the fold), more than the quarter a borrowed bar is kept at, so it is derived from the fold's own order instead.
# A row's contribution passes through, at most:
#   proj_ln_bwd_kernel   NPASS fmas in the thread (<= 16) + the GROWS row groups summed through LDS (<= 32, one more for the two
#                        rounds of the 8-wave kernel); the largest sum over the instantiations is <32, MT 2>: 4 + 32 = 36
#   ln_residual_bwd      ceil(M / (512 * rows per workgroup)) rows in the thread (<= 5 in these tests) + 16 row groups through LDS
#   ln_partials_reduce   ceil(workgroups / 64) partial rows in a slice (<= 8) + 6 tree levels + the addition onto dgamma / dbeta
# i.e. <= 36 + 5 + 6 + 1 = 48 additions (unfused: 5 + 16 + 8 + 6 + 1 = 36), each rounding a partial sum of magnitude <= A by
# 2^-24, plus the roundings of the addends themselves: d = s * dy (1) and xhat = (a - mean) * rstd (2); the product enters by fma.
# 51 * 2^-24 * A to first order, and 2^-24 |base| for the baseline's share of the last addition.  Measured worst on an MI355X
# against this bar: fused dgamma 0.064, dbeta 0.097; unfused 0.053, 0.045; the row-table LayerNorm past its grid cap 0.004.
C_FOLD = 51 * 2.0 ** -24

# every (C, heads) swv2_proj_ln_supported admits (C 192: 32-wide slots; heads 1, 3, 8 of its 1 .. 8)
PAIRS = [(32, 2), (64, 2), (64, 4), (96, 2), (96, 4), (96, 6), (128, 2), (128, 4), (128, 6), (128, 8), (192, 1), (192, 3), (192, 8)]
# (Bw, Lp): one 64-row tile exactly | 2 tiles + 48 rows (C 192: 1 tile of 128 + 48) | 880 rows | 32 912 rows: the MT = 2 kernels
# (Bw * Lp >= 32 768) with a 16-row last tile
ROW_CASES = [(1, 64), (1, 176), (5, 176)]
BIG_CASE = (187, 176)
BIG_PAIRS = [(32, 2), (96, 6), (128, 8), (192, 8)]
LV = {64: 54, 176: 162}                                       # valid rows per window
GEOMETRY = [(C, h, Bw, Lp) for C, h in PAIRS for Bw, Lp in ROW_CASES] + [(C, h) + BIG_CASE for C, h in BIG_PAIRS]


def geometry_id(p):
    return "C%d-h%d-Bw%d-Lp%d" % tuple(p)


def slot(C):
    return 32 if C == 192 else 16


def head_major(dense, Bw, heads, Lp, HS):
    """[Bw * Lp][heads * HS] -> [Bw][heads][Lp][HS]"""
    return dense.view(Bw, Lp, heads, HS).permute(0, 2, 1, 3).contiguous()


def dense_rows(hm, Bw, heads, Lp, HS):
    """[Bw][heads][Lp][HS] -> [Bw * Lp][heads * HS]"""
    return hm.view(Bw, heads, Lp, HS).permute(0, 2, 1, 3).reshape(Bw * Lp, heads * HS)


def proj_map(heads, hd, HS):
    """the head-padding map the block uses: padded feature head * HS + j -> head * hd + j, or -1 for j >= hd"""
    j = torch.arange(HS)
    one = torch.where(j.view(1, -1) < hd, torch.arange(heads).view(-1, 1) * hd + j.view(1, -1), torch.full((1, 1), -1))
    return one.reshape(-1).to(torch.int32)


def prep_dense(wp, pmap):
    """what swv2_prep_weight makes of the fp32 proj weight [C][heads * hd] and the column map: bf16 [C][heads * HS]"""
    out = torch.zeros(wp.shape[0], pmap.numel(), dtype=wp.dtype, device=wp.device)
    real = pmap >= 0
    out[:, real] = wp[:, pmap[real].long()]
    return out.to(BF)


def row_table(M, valid, g):
    """int32 [M]: -1 where not valid, the valid rows a random permutation onto 0 .. (number of valid rows) - 1"""
    n = int(valid.sum())
    tab = torch.full((M,), -1, dtype=torch.int32)
    tab[valid] = torch.randperm(n, generator=g).to(torch.int32)
    return tab, n


def scale_cycle(rows, rps):
    """drop-path factors per sample, cycling through 0, 1.25, 1 (a single sample gets 1.25: a zero there would zero every gradient)"""
    n = -(-rows // rps)
    return torch.tensor([(0.0, 1.25, 1.0)[(i + (n == 1)) % 3] for i in range(n)], dtype=torch.float32)


def signed_log_uniform(n, lo, hi, g):
    mag = torch.exp(torch.empty(n).uniform_(math.log(lo), math.log(hi), generator=g))
    return mag * (torch.randint(0, 2, (n,), generator=g).float() * 2 - 1)


def last_live_dst(rowidx, M):
    """destination row of the last window row with a table entry >= 0"""
    if rowidx is None:
        return M - 1
    return int(rowidx[(rowidx >= 0).nonzero().flatten()[-1]])


def make_case(C, heads, Bw, Lp, mode, table=True, with_scale=True, seed=0):
    """the operands of one proj + LN1 case, on the CPU (case_to moves them).  mode "exact": integer operands for which no rounding
    can occur (oh rows with at most four entries of +-1 .. +-8, wp in -4 .. 4, bp in -8 .. 8: |a1| <= 4 * 8 * 4 + 8 = 136);
    "random": normal operands, gamma from 1e-3 to 2 in magnitude with random signs."""
    g = torch.Generator().manual_seed(1000003 * seed + 7919 * C + 131 * heads + 17 * Bw + Lp)
    HS = slot(C)
    hd, Lv, Mw, K = 3 * HS // 4, LV[Lp], Bw * Lp, heads * HS
    pmap = proj_map(heads, hd, HS)
    real = (pmap >= 0).nonzero().flatten()
    dense = torch.zeros(Mw, K, dtype=F64)
    if mode == "exact":
        cols = real[torch.randint(0, real.numel(), (Mw, 4), generator=g)]
        vals = torch.randint(1, 9, (Mw, 4), generator=g).double() * (torch.randint(0, 2, (Mw, 4), generator=g).double() * 2 - 1)
        dense.scatter_(1, cols, vals)
        wp = torch.randint(-4, 5, (C, heads * hd), generator=g).float()
        bp = torch.randint(-8, 9, (C,), generator=g).float()
    else:
        dense[:, real] = torch.randn(Mw, real.numel(), generator=g, dtype=F64)
        wp = torch.randn(C, heads * hd, generator=g)
        bp = torch.randn(C, generator=g)
    c = types.SimpleNamespace(C=C, heads=heads, Bw=Bw, Lp=Lp, Lv=Lv, Mw=Mw, HS=HS, hd=hd, K=K, rps=RPS, mode=mode, pmap=pmap)
    c.oh = head_major(dense.to(BF), Bw, heads, Lp, HS)
    c.wp, c.bp = wp, bp
    c.gamma, c.beta = signed_log_uniform(C, 1e-3, 2.0, g), torch.randn(C, generator=g)
    if table:
        c.rowidx, c.rows = row_table(Mw, (torch.arange(Mw) % Lp) < Lv, g)
    else:
        c.rowidx, c.rows = None, Mw
    c.x = torch.randn(c.rows, C, generator=g)
    c.scale = scale_cycle(c.rows, RPS) if with_scale else None
    if table and with_scale:              # the last valid window row goes to a sample that is not dropped (its table entry swapped)
        lv = (c.rowidx >= 0).nonzero().flatten()
        on = lv[c.scale[c.rowidx[lv].long() // RPS] != 0]
        if c.scale[int(c.rowidx[lv[-1]]) // RPS] == 0:
            c.rowidx[[int(lv[-1]), int(on[0])]] = c.rowidx[[int(on[0]), int(lv[-1])]]
    c.dy = torch.randn(c.rows, C, generator=g)
    c.dy[last_live_dst(c.rowidx, Mw)] *= 64.0        # a doubled or dropped last row moves dgamma / dbeta far beyond C_FOLD * A
    sgn = lambda: torch.randint(0, 2, (C,), generator=g).float() * 2 - 1          # noqa: E731
    c.base_g = torch.randint(1, 4, (C,), generator=g).float() * sgn()
    c.base_b = torch.randint(1, 4, (C,), generator=g).float() * sgn()
    return c


def case_to(c, device):
    return types.SimpleNamespace(**{k: (v.to(device) if torch.is_tensor(v) else v) for k, v in vars(c).items()})


# ---------------------------------------------------------------------------------------------------------------
# references (fp64) with their bounds
# ---------------------------------------------------------------------------------------------------------------
def table_of(rowidx, M, device):
    """(live [M] bool, dst [M] long, 0 where not live)"""
    if rowidx is None:
        return torch.ones(M, dtype=torch.bool, device=device), torch.arange(M, device=device)
    return rowidx >= 0, rowidx.long().clamp_min(0)


def sample_scale(scale, dst, rps):
    """fp64 [M]: scale[dst / rows_per_sample], 1 without a scale"""
    if scale is None:
        return torch.ones(dst.shape[0], dtype=F64, device=dst.device)
    return scale.double()[dst // rps]


def ref_proj(oh, wpb, bp, Bw, heads, Lp):
    """v = merge_heads(oh) wp^T + bp and A = |oh| |wp|^T + |bp| from the bf16 operands the kernel reads; -> (v, bound)"""
    HS = oh.shape[-1]
    o, w = dense_rows(oh, Bw, heads, Lp, HS).double(), wpb.double()
    v = o @ w.T + bp.double()
    A = o.abs() @ w.abs().T + bp.double().abs()
    return v, 2.0 ** -8 * v.abs() + heads * HS * 2.0 ** -23 * A


def rounding_share(ref):
    """the first term of the bf16 outputs' bounds: the rounding of the result itself"""
    return 2.0 ** -8 * ref.abs()


def ref_stats(a):
    """LayerNorm statistics of the saved bf16 rows -> (mu, bound of mean, rho, bound of rstd)"""
    a = a.double()
    Cc = a.shape[1]
    mu = a.mean(1)
    rho = ((a - mu.view(-1, 1)) ** 2).mean(1).add(EPS32).rsqrt()
    return mu, Cc * 2.0 ** -23 * a.abs().mean(1), rho, Cc * 2.0 ** -22 * rho


def ref_y(y0, a, mean, rstd, gamma, beta, res, scale, rowidx, rps, res_mod=0):
    """y[dst] = res[res_mod ? dst % res_mod : dst] + s (LN(a) gamma + beta) from the SAVED mean / rstd; rows no table entry names
    keep y0 (bound 0).  -> (ref, bound), shaped like y0"""
    a, mean, rstd, gamma, beta = a.double(), mean.double().view(-1, 1), rstd.double().view(-1, 1), gamma.double(), beta.double()
    live, dst = table_of(rowidx, a.shape[0], a.device)
    s = sample_scale(scale, dst, rps).view(-1, 1)
    rrow = dst % res_mod if res_mod else dst
    x = res.double()[rrow] if res is not None else torch.zeros_like(a)
    val = x + s * ((a - mean) * rstd * gamma + beta)
    bnd = 2.0 ** -20 * (x.abs() + s.abs() * ((a - mean).abs() * rstd * gamma.abs() + beta.abs()))
    ref, bound = y0.double().clone(), torch.zeros_like(y0, dtype=F64)
    ref[dst[live]], bound[dst[live]] = val[live], bnd[live]
    return ref, bound


def ref_ln_bwd(a, mean, rstd, gamma, dy, scale, rowidx, rps):
    """the LayerNorm backward written out, from the saved a, mean, rstd.  -> namespace(da, da_bound, dgamma, A_g, dbeta, A_b)
    (dgamma / dbeta without the baseline they are accumulated onto)"""
    a, mean, rstd, gamma = a.double(), mean.double().view(-1, 1), rstd.double().view(-1, 1), gamma.double()
    Cc = a.shape[1]
    live, dst = table_of(rowidx, a.shape[0], a.device)
    lv = live.double().view(-1, 1)
    d = sample_scale(scale, dst, rps).view(-1, 1) * dy.double()[dst] * lv
    xh = (a - mean) * rstd
    g = d * gamma
    da = rstd * (g - g.mean(1, keepdim=True) - xh * (g * xh).mean(1, keepdim=True)) * lv
    slack = Cc * 2.0 ** -22 * rstd * (g.abs() + g.abs().mean(1, keepdim=True) + xh.abs() * (g * xh).abs().mean(1, keepdim=True)) * lv
    return types.SimpleNamespace(da=da, da_bound=2.0 ** -8 * da.abs() + slack, dgamma=(d * xh).sum(0), A_g=(d * xh).abs().sum(0),
                                 dbeta=d.sum(0), A_b=d.abs().sum(0))


def fold_bound(A, base):
    """dgamma / dbeta: C_FOLD * A + 2^-24 |base| (nothing where A = 0: base + 0 is exact)"""
    return C_FOLD * A + 2.0 ** -24 * base.double().abs() * (A > 0)


def ref_doh(da, wpt, Bw, heads, Lp):
    """d(oh) = split_heads(da1 wp) from the bf16 da1 the kernel wrote and the bf16 wpt [heads * HS][C]; -> (ref, bound), head-major"""
    HS = wpt.shape[0] // heads
    d, w = da.double(), wpt.double()
    ref = d @ w.T
    bound = 2.0 ** -8 * ref.abs() + da.shape[1] * 2.0 ** -23 * (d.abs() @ w.abs().T)
    return head_major(ref, Bw, heads, Lp, HS), head_major(bound, Bw, heads, Lp, HS)


# ---------------------------------------------------------------------------------------------------------------
# checkers
# ---------------------------------------------------------------------------------------------------------------
WORST = {}          # name -> worst |err| / bound seen so far (reported by the GPU tests)


def within(got, ref, bound):
    """(number of elements with |got - ref| > bound or not finite, worst |err| / bound, index of the worst).  bound = 0: equality."""
    err = (got.double() - ref).abs()
    bad = ~(err <= bound)
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp_min(1e-300))
    ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, math.inf), ratio)
    flat = int(ratio.argmax())
    idx = tuple(int(i) for i in torch.unravel_index(torch.tensor(flat), ratio.shape)) if ratio.dim() else ()
    return int(bad.sum()), float(ratio.reshape(-1)[flat]), idx


def assert_within(name, got, ref, bound, what="", rnd=None, worst=None):
    """asserts |got - ref| <= bound on every element; -> worst |err| / bound.  rnd: the share of `bound` that is the bf16 rounding of
    the result itself; the worst of (|err| - rnd) / (bound - rnd) is then filed in WORST (or the table `worst`) under name + ' beyond
    rounding'"""
    worst = WORST if worst is None else worst
    nbad, ratio, idx = within(got, ref, bound)
    worst[name] = max(worst.get(name, 0.0), ratio if math.isfinite(ratio) and nbad == 0 else worst.get(name, 0.0))
    if rnd is not None and nbad == 0:
        ex = (((got.double() - ref).abs() - rnd).clamp_min(0) / (bound - rnd).clamp_min(1e-300)).max()
        worst[name + " beyond rounding"] = max(worst.get(name + " beyond rounding", 0.0), float(ex))
    assert nbad == 0, (f"{name} {what}: {nbad} elements out of bound, worst |err| / bound {ratio:.3g} at {idx}: got {float(got[idx]):.9g}, "
                       f"ref {float(ref[idx]):.9g}, bound {float(bound[idx]):.3g}")
    return ratio


def check_forward(name, c, wpb, a1, mean, rstd, y, y0, what=""):
    """every Part B forward bound on one run's outputs; -> {output: worst ratio}"""
    v, vb = ref_proj(c.oh, wpb, c.bp, c.Bw, c.heads, c.Lp)
    r = {"a1": assert_within(name + " a1", a1, v, vb, what, rounding_share(v))}
    r.update(check_ln_forward(name, a1, mean, rstd, y, y0, c.gamma, c.beta, c.x, c.scale, c.rowidx, c.rps, 0, what))
    return r


def check_ln_forward(name, a, mean, rstd, y, y0, gamma, beta, res, scale, rowidx, rps, res_mod=0, what=""):
    mu, mub, rho, rhob = ref_stats(a)
    r = {"mean": assert_within(name + " mean", mean, mu, mub, what), "rstd": assert_within(name + " rstd", rstd, rho, rhob, what)}
    yr, yb = ref_y(y0, a, mean, rstd, gamma, beta, res, scale, rowidx, rps, res_mod)
    r["y"] = assert_within(name + " y", y, yr, yb, what)
    return r


def check_ln_backward(name, a, mean, rstd, gamma, dy, scale, rowidx, rps, da, dgamma, dbeta, base_g, base_b, what=""):
    rf = ref_ln_bwd(a, mean, rstd, gamma, dy, scale, rowidx, rps)
    r = {"da1": assert_within(name + " da1", da, rf.da, rf.da_bound, what, rounding_share(rf.da))}
    live, _ = table_of(rowidx, a.shape[0], a.device)
    assert bool((da[~live].contiguous().view(torch.int16) == 0).all()), f"{name} {what}: da1 is not exactly +0 on rows with a negative table entry"
    # (the baseline is an integer: got - base is exact in fp64)
    r["dgamma"] = assert_within(name + " dgamma", dgamma.double() - base_g.double(), rf.dgamma, fold_bound(rf.A_g, base_g), what)
    r["dbeta"] = assert_within(name + " dbeta", dbeta.double() - base_b.double(), rf.dbeta, fold_bound(rf.A_b, base_b), what)
    return r


def check_doh(name, c, da, wpt, doh, what=""):
    ref, bound = ref_doh(da, wpt, c.Bw, c.heads, c.Lp)
    r = {"doh": assert_within(name + " doh", doh, ref, bound, what, rounding_share(ref))}
    live, _ = table_of(c.rowidx, c.Mw, doh.device)
    rows = dense_rows(doh, c.Bw, c.heads, c.Lp, c.HS)
    assert bool((rows[~live] == 0).all()), f"{name} {what}: doh is not exactly 0 on rows with a negative table entry"
    assert bool((rows[:, c.pmap.to(rows.device) < 0] == 0).all()), f"{name} {what}: doh is not exactly 0 in the padded head columns"
    return r
