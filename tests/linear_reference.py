"""Case builders, fp64 references and per-element bounds for the forward GEMM engine behind swv2_linear (csrc/gemm.hip,
csrc/gemm_common.h), shared by tests/test_linear_exact_gpu.py (the kernels) and tests/test_linear_exact_host.py (the references and
bounds themselves, no GPU).  Plain torch; runs on whatever device a case's tensors live on.  The helpers of the earlier exact suites
are reused, not copied (tests/mlp_reference.py: WORST, lut_of, host_gelu_lut, _chunked_matmul, and in the GPU file Guarded and
library_gelu_lut; tests/proj_ln_reference.py: assert_within, table_of, row generators; the bf16 row of the bounds is ref_linear's).

A case is a namespace: one operand (opk), one bf16 weight [N][K] as swv2_prep_weight returns it, one epilogue (epk), the kernel
swv2_linear_kernel must name for its descriptors (kernel, None = not asked) and the value of SWV2_GEMM_WIDE it runs under.
  dense_operand(c)  fp64 [M][K] of exactly what the loader hands to the matrix cores, with the absolute error of that statement
                    (None where IEEE fp32 torch operations reproduce the operand bit for bit)
  reference(c, o)   {output: (ref, bound, written)} from the case and -- where an output is judged against the kernel's own upstream
                    tensor -- from the run's outputs o
  emulate(c)        the same outputs from fp32 torch with the kernels' rounding points (bf16 operands, fp32 accumulation over 64
                    columns at a time), optionally with one of the defects of MUTANTS
  check_case(c, o)  every element of every output: written elements finite and within their bound, all others still the prefill

Bounds (derived, none fitted to a measurement).  K = columns of the operand, v = a w^T + bias in fp64,
A = |a| |w|^T + |bias|, E = K 2^-23 A (+ da |w|^T where the operand carries an error da):
  E            K products are exact in fp32 (bf16 x bf16 has 16 significant bits); K - 1 additions and the bias, each rounding a
               partial sum of magnitude <= A by 2^-24 of it, in any order: K 2^-24 A, doubled
  fp32 out     E + 2^-24 (|v| + |aux|)      the residual add rounds the result once; |aux| pays for a second rounding when bias and
                                            residual are added one after the other
  bf16 out     2^-8 |v| + E                 mlp_reference.ref_linear: 2^-8 is bf16's unit roundoff
  accumulate   E + 2^-24 |v| + 2^-24 |base| one fp32 addition onto the baseline: its result is within 2^-24 of |base| + |acc|
  q, k         v / max(n, 1e-12), n = |v| over the head's DP columns.  To first order an error dv, |dv| <= E, moves q by
               dv / n - v (v . dv) / n^3: P = E / n + |v| (|v| . E) / n^3.  The fp32 reciprocal norm is off by
               RN(DP) = (DP / 2 + 3) 2^-24 relative: DP fused multiply-adds each round a partial sum <= n^2 (DP 2^-24 on n^2, half
               of it on n), sqrtf and the division are correctly rounded (2^-24 each), one more for second-order terms; the product
               v rn rounds once more (2^-24) and the bf16 store 2^-8:  2^-8 |ref| + P + |ref| (RN + 2^-24)
  rnorm        rn (|v| . E / n^2 + RN(DP))  the same propagation through 1 / n
  wide heads   (DP 96, 128: the epilogue stores bf16(v) and adds squared-norm pieces into rnorm; swv2_qk_normalize finishes)
               squared norm: 2 |v| . E + 22 2^-24 n^2 (16 fmas per 16-column piece, at most 6 pieces added); then, from the
               kernel's OWN squared norm s and bf16 values: rn within 3 2^-24 of 1 / max(sqrt(s), 1e-12), q within
               (2^-8 + 2^-24) |ref| of bf16(v) rn
  merge stats  mean: 4C 2^-23 mean_k |x| (4C additions, doubled).  rstd = (q / 4C - mean^2 + eps)^-1/2 in ONE pass: the two terms
               carry 4C 2^-23 (mean_k x^2 + mean^2) between them, d rstd / rstd = d var / (2 (var + eps)), plus 4 2^-24 for the
               approximate rsqrtf, the division and the additions of eps and mean^2
  OP_MERGE_LN  a = (x - mean) rstd gamma + beta from the library's own mean / rstd; the kernel's fp32 evaluation rounds four
               times (5 2^-24 (|x - mean| rstd |gamma| + |beta|), ties included) and then to bf16: da = 2^-8 |a| + that
  OP_BF16_CSCALE  a = resid coef: one fp32 product, then bf16: da = (2^-8 + 2^-24) |a|
  loss sums    per 32-row group, slot and channel, from the kernel's own fp32 prediction y: every term q (y - t)^2 is built from
               7 roundings (the difference, four squares / three additions, the weight): 8 2^-24 of itself; the 16-row
               accumulation, the wave reduction (6 levels) and the lane sums add at most n_terms roundings of partial sums
               <= S = sum q (y - t)^2:  n_terms 2^-23 S + 8 2^-24 S  (n_terms = rows x 16 pixels of the group in that slot)
  loss_part_reduce  per slice (the groups g with g mod 8 = slice), the fp64 fold of the kernel's own partial sums; at most
                    ceil(groups / 8) + 8 additions: (that) 2^-24 sum |part|
  loss_resid   bf16(q (y - t)) from the kernel's own y: 2^-8 |ref| + 2^-23 (|y| + |t|) q  (the fp32 difference and product)
Exact cases (operands from small integers, every accumulator an integer below 2^24): E = 0, fp32 outputs equal the reference,
bf16 outputs equal its round-to-nearest-even bf16, q / k / rnorm keep only the rounding terms above.
"""
import math
import types

import torch

from tests import mlp_reference as MR
from tests import proj_ln_reference as P
from tests.proj_ln_reference import BF, F64, SENT, signed_log_uniform

NAN = float("nan")
U8, U24 = 2.0 ** -8, 2.0 ** -24
GROUP = 32                    # SWV2_LOSS_GROUP_ROWS
SLICES = 8                    # SWV2_LOSS_PART_SLICES
DUMP_BYTES = 2048             # SWV2_LOSS_DUMP_BYTES
(Q128, Q192, DX128, DMA, WIDE, T64, T128) = range(7)          # SWV2_LINEAR_*: asserted against _lib in the tests
KERNEL_NAMES = ("RESIDENT_QKV128", "RESIDENT_QKV192X3", "RESIDENT_DX128", "WIDE_DMA", "WIDE", "TILE64", "TILE128")
WORST = MR.WORST


def rn_rel(DP):
    return (DP / 2 + 3) * U24


def resid_pitch(n):
    return (n + 63) // 64 * 64


# ---------------------------------------------------------------------------------------------------------------
# operand values
# ---------------------------------------------------------------------------------------------------------------
def _gen(*key):
    s = 7
    for k in key:
        s = (s * 1000003 + int(k)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(s)


def _ints(shape, lo, hi, g):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def _scaled(rows, cols, g, lo=2.0 ** -6, hi=4.0):
    """normal values whose COLUMNS carry log-uniform scales over lo .. hi (as _colscale of test_wgrad_exact_gpu.py): most products are
    small against their neighbours"""
    sc = torch.exp(torch.empty(cols).uniform_(math.log(lo), math.log(hi), generator=g))
    return torch.randn(rows, cols, generator=g) * sc


def _values(rows, cols, exact, g):
    return _ints((rows, cols), -4, 4, g) if exact else _scaled(rows, cols, g)


def _weight(N, K, exact, g):
    """fp32 [N][K]: integers -4 .. 4, or normals whose ROWS carry log-uniform scales"""
    return _ints((N, K), -4, 4, g) if exact else _scaled(K, N, g, 2.0 ** -8, 1.0).T.contiguous() / math.sqrt(K)


def _bias(N, exact, g):
    return _ints((N,), -8, 8, g) if exact else signed_log_uniform(N, 1e-3, 1.0, g)


def gather_table(M, n_src, valid, g, drop=8):
    """int32 [M]: -1 where not valid and on about 1 / drop of the valid rows, the others random source rows in 0 .. n_src - 1"""
    tab = torch.randint(0, n_src, (M,), generator=g).to(torch.int32)
    tab[torch.rand(M, generator=g) < 1.0 / drop] = -1
    tab[~valid] = -1
    return tab


def scatter_table(M, valid, g, drop=8):
    """(int32 [M]: -1 where not valid and on about 1 / drop of the valid rows, the others distinct rows of an output of M rows in random
    order; M): the output rows that no entry names are never written"""
    live = valid & (torch.rand(M, generator=g) >= 1.0 / drop)
    if not bool(live.any()):
        live = valid.clone()
    tab = torch.full((M,), -1, dtype=torch.int32)
    tab[live] = torch.randperm(M, generator=g)[:int(live.sum())].to(torch.int32)
    return tab, M


def patch_rows(img):
    """[B][C][H][W] -> [B gh gw][C 16], column c * 16 + p * 4 + q (the conv weight's order)"""
    B, Cc, H, W = img.shape
    return img.reshape(B, Cc, H // 4, 4, W // 4, 4).permute(0, 2, 4, 1, 3, 5).reshape(B * (H // 4) * (W // 4), Cc * 16)


def unpatch_image(rows, B, Cc, H, W):
    """the inverse of patch_rows"""
    return rows.reshape(B, H // 4, W // 4, Cc, 4, 4).permute(0, 3, 1, 4, 2, 5).reshape(B, Cc, H, W)


def merge_rows(x, order):
    """[B][H][W][C] -> [B h2 w2][4 C]: block blk of the 4 C columns is pixel (2 i + order[blk][0], 2 j + order[blk][1])"""
    return torch.cat([x[:, hp::2, wp::2, :] for hp, wp in order], dim=-1).reshape(-1, 4 * x.shape[-1])


MERGE_ORDER = ((0, 0), (1, 0), (0, 1), (1, 1))          # (row, column) parity of blocks 0 .. 3; checked against the reference fixture


def heads_rows(src):
    """[Bw][h][S][Lp][DP] -> [Bw Lp][S h DP]"""
    Bw, h, S, Lp, DP = src.shape
    return src.permute(0, 3, 2, 1, 4).reshape(Bw * Lp, S * h * DP)


def dense_operand(c, lut=None):
    """-> (a fp64 [M][K], da fp64 [M][K] or None)"""
    k = c.opk
    if k in ("f32", "bf16", "gelu"):
        src = c.x.to(BF)
        src = (MR.lut_of(lut, src) if k == "gelu" else src).double()
        if c.rowidx_in is None:
            return src, None
        a = src[c.rowidx_in.long().clamp_min(0)]
        a[c.rowidx_in < 0] = 0
        return a, None
    if k == "heads":
        return heads_rows(c.x).double(), None
    if k == "patch":
        img = c.x[:, :c.Cin]
        if c.aux0 is not None:
            img = img + c.aux0[:, :c.Cin]                     # one IEEE fp32 addition, as the loader's
        return patch_rows(img.to(BF).double()), None
    if k == "merge":
        xr = merge_rows(c.x.double(), MERGE_ORDER)
        mu, rs = c.mean.double().view(-1, 1), c.rstd.double().view(-1, 1)
        a = (xr - mu) * rs * c.gamma.double() + c.beta.double()
        if c.exact:
            return a, None
        return a, U8 * a.abs() + 5 * U24 * ((xr - mu).abs() * rs * c.gamma.double().abs() + c.beta.double().abs())
    if k == "cscale":
        rows = torch.arange(c.M, device=c.x.device) // c.rps
        a = c.x[:, :c.K].double() * c.coef.double()[rows].repeat_interleave(16, dim=1)
        return a, (None if c.exact else (U8 + U24) * a.abs())
    raise ValueError(k)


def emulated_operand(c, lut=None):
    """the operand as fp32 torch arithmetic with the loader's rounding points makes it: fp32 [M][K] of bf16 values"""
    k = c.opk
    if k == "merge":
        xr = merge_rows(c.x, MERGE_ORDER)
        return ((xr - c.mean.view(-1, 1)) * c.rstd.view(-1, 1) * c.gamma + c.beta).to(BF).float()
    if k == "cscale":
        rows = torch.arange(c.M, device=c.x.device) // c.rps
        return (c.x[:, :c.K].float() * c.coef[rows].repeat_interleave(16, dim=1)).to(BF).float()
    return dense_operand(c, lut)[0].float()


# ---------------------------------------------------------------------------------------------------------------
# the product and the epilogues: fp64 reference with bounds
# ---------------------------------------------------------------------------------------------------------------
def product(c, lut=None, share=None):
    """-> (v, E): a w^T + bias in fp64 and the accumulation bound (0 in exact cases).  share: a dict that receives "op" = da |w|^T, the
    part of E that is the operand's own rounding (reached by construction where one product dominates an output)"""
    a, da = dense_operand(c, lut)
    w = c.w.double()
    v = a @ w.T
    A = a.abs() @ w.abs().T
    if c.bias is not None:
        v, A = v + c.bias.double(), A + c.bias.double().abs()
    if c.exact:
        assert da is None
        return v, torch.zeros_like(v)
    E = c.K * 2.0 ** -23 * A
    if da is not None:
        E = E + da @ w.abs().T
        if share is not None:
            share["op"] = da @ w.abs().T
    return v, E


def max_accumulator(c, lut=None):
    """the largest |partial sum| any summation order can meet: |a| |w|^T + |bias| (Part 1's premise: below 2^24)"""
    a, _ = dense_operand(c, lut)
    A = a.abs() @ c.w.double().abs().T
    if c.bias is not None:
        A = A + c.bias.double().abs()
    return float(A.max())


def _bf16_of(v):
    return v.float().to(BF).double()


def _row_major(c, v, E, bits, extra=None):
    """rows scattered through rowidx_out into [rows_out][ld]; -> (ref, bound, written)"""
    dev = v.device
    ref = torch.zeros(c.rows_out, c.ld, dtype=F64, device=dev)
    bound = torch.zeros_like(ref)
    written = torch.zeros(c.rows_out, c.ld, dtype=torch.bool, device=dev)
    live, dst = P.table_of(c.rowidx_out, c.M, dev)
    if bits == 16:
        r, b = (_bf16_of(v), torch.zeros_like(v)) if c.exact else (v, U8 * v.abs() + E)
    else:
        r, b = v, E if extra is None else E + extra
    ref[dst[live], :c.N], bound[dst[live], :c.N], written[dst[live], :c.N] = r[live], b[live], True
    return ref, bound, written


def _split_heads(t, c):
    """[M][S h DP] -> [Bw][h][S][Lp][DP]"""
    S = t.shape[1] // (c.h * c.DP)
    return t.view(c.Bw, c.Lp, S, c.h, c.DP).permute(0, 3, 2, 1, 4).contiguous()


def wide_heads(c):
    return c.DP > 64


def reference(c, o=None, lut=None):
    """{output: (ref, bound, written)}.  o: the run's outputs, for what is judged against the kernel's own upstream tensor"""
    share = {}
    v, E = product(c, lut, share)
    dev = v.device
    k = c.epk
    if k == "bf16":
        return {"out": _row_major(c, v, E, 16)}
    if k == "f32":
        if c.aux is None:
            r = _row_major(c, v, E, 32, U24 * v.abs() * (0 if c.exact else 1))
            if "op" in share:                                    # (OP_MERGE_LN, OP_BF16_CSCALE: no scatter, no pitch)
                assert c.rowidx_out is None and c.ld == c.N
                r = r + (share["op"],)
            return {"out": r}
        live, dst = P.table_of(c.rowidx_out, c.M, dev)
        ax = c.aux.double()[dst][:, :c.N]
        tot = v + ax
        return {"out": _row_major(c, tot, E, 32, U24 * (tot.abs() + ax.abs()) * (0 if c.exact else 1))}
    if k == "acc":
        live, dst = P.table_of(c.rowidx_out, c.M, dev)
        bs = c.base.double()[dst][:, :c.N]
        tot = v + bs
        return {"out": _row_major(c, tot, E, 32, U24 * (tot.abs() + bs.abs()) * (0 if c.exact else 1))}
    if k == "qkv":
        return _reference_qkv(c, v, E, o)
    if k in ("unpatch", "loss"):
        return _reference_head(c, v, E, o)
    raise ValueError(k)


def _reference_qkv(c, v, E, o):
    vh, Eh = _split_heads(v, c), _split_heads(E, c)
    valid = (torch.arange(c.Lp, device=v.device) < c.L).view(1, 1, 1, c.Lp, 1)
    vh, Eh = vh * valid, Eh * valid                              # padded window rows: exactly 0 everywhere
    qk, Eqk = vh[:, :, :2], Eh[:, :, :2]
    n2 = (qk * qk).sum(-1)
    all_w = torch.ones_like(vh, dtype=torch.bool)
    vb = (_bf16_of(vh), torch.zeros_like(vh)) if c.exact else (vh, U8 * vh.abs() + Eh)
    if wide_heads(c):
        r = {"qkvh_raw": (vb[0], vb[1], all_w),
             "ss": (n2, 2 * (qk.abs() * Eqk).sum(-1) + (0 if c.exact else 22 * U24) * n2, torch.ones_like(n2, dtype=torch.bool))}
        if o is not None:                                        # swv2_qk_normalize, from the kernel's own squared norms and bf16 values
            s = o["ss"].double()
            rn = 1.0 / s.sqrt().clamp_min(1e-12) * valid.view(1, 1, 1, c.Lp)
            raw = o["qkvh_raw"].double()
            ref = raw.clone()
            ref[:, :, :2] = raw[:, :, :2] * o["rnorm"].double().unsqueeze(-1)
            bound = torch.zeros_like(ref)
            bound[:, :, :2] = (U8 + U24) * ref[:, :, :2].abs()
            r["rnorm"] = (rn, 3 * U24 * rn, torch.ones_like(n2, dtype=torch.bool))
            r["qkvh"] = (ref, bound, all_w)
        return r
    n = n2.sqrt()
    nc = n.clamp_min(1e-12)
    rn = 1.0 / nc * valid.view(1, 1, 1, c.Lp)
    RN = (3 * U24) if c.exact else rn_rel(c.DP)
    dot = (qk.abs() * Eqk).sum(-1)
    ref, bound = vb[0].clone(), vb[1].clone()
    q = qk * rn.unsqueeze(-1)
    ref[:, :, :2] = q
    bound[:, :, :2] = U8 * q.abs() + Eqk / nc.unsqueeze(-1) + qk.abs() * (dot / nc ** 3).unsqueeze(-1) + q.abs() * (RN + U24)
    return {"qkvh": (ref, bound, all_w), "rnorm": (rn, rn * (dot / nc ** 2 + RN), torch.ones_like(n2, dtype=torch.bool))}


def loss_edges(M, T):
    """bool per 32-row group: its slot 1 is written (the row behind the group belongs to another sample, or is past M)"""
    return torch.tensor([(g * GROUP + GROUP >= M) or ((g * GROUP + GROUP) // T != (g * GROUP) // T) for g in range(-(-M // GROUP))])


def _reference_head(c, v, E, o):
    B, Cout, H, W, dev = c.B, c.Cout, c.H, c.W, v.device
    img = unpatch_image(v, B, Cout, H, W)
    bnd = unpatch_image(E, B, Cout, H, W)
    if c.skip is not None:
        sk = c.skip.double()[:, :Cout]
        img = img + sk
        bnd = bnd + (0 if c.exact else U24) * (img.abs() + sk.abs())
    r = {}
    for name, Ct, c0 in (("y", c.Ct, c.c0),) + ((("y2", c.C2, 0),) if c.C2 else ()):
        ref = torch.zeros(B, Ct, H, W, dtype=F64, device=dev)
        bound, written = torch.zeros_like(ref), torch.zeros(B, Ct, H, W, dtype=torch.bool, device=dev)
        ref[:, c0:c0 + Cout], bound[:, c0:c0 + Cout], written[:, c0:c0 + Cout] = img, bnd, True
        r[name] = (ref, bound, written)
    if c.epk != "loss" or o is None:
        return r
    # the loss, from the kernel's OWN fp32 prediction
    y = o["y"][:, c.c0:c.c0 + Cout].double()
    t = c.tar.double()[:, c.coff:c.coff + Cout]
    q = c.qw.double().view(1, 1, H, 1)
    T, M = c.T, c.M
    ng = -(-M // GROUP)
    e0 = patch_rows(q * (y - t) ** 2).view(M, Cout, 16).sum(-1)                 # [M][Cout]
    e1 = patch_rows(q * t ** 2).view(M, Cout, 16).sum(-1)
    rows = torch.arange(M, device=dev)
    grp, first_b = rows // GROUP, (rows // GROUP * GROUP) // T
    slot = (rows // T != first_b).long()
    part = torch.zeros(ng, 2, Cout, 2, dtype=F64, device=dev)
    nterm = torch.zeros(ng, 2, dtype=F64, device=dev)
    part.index_put_((grp, slot), torch.stack([e0, e1], -1), accumulate=True)
    nterm.index_put_((grp, slot), torch.full((M,), 16.0, dtype=F64, device=dev), accumulate=True)
    pw = torch.ones(ng, 2, Cout, 2, dtype=torch.bool, device=dev)
    pw[:, 1] = loss_edges(M, T).to(dev).view(-1, 1, 1)
    r["part"] = (part, (nterm.view(ng, 2, 1, 1) * 2.0 ** -23 + 8 * U24) * part, pw)
    rr = patch_rows(q * (y - t))
    rb = U8 * rr.abs() + 2.0 ** -23 * patch_rows(q * (y.abs() + t.abs()))
    RPp = resid_pitch(c.N)
    ref = torch.zeros(M, RPp, dtype=F64, device=dev)
    bound, written = torch.zeros_like(ref), torch.zeros(M, RPp, dtype=torch.bool, device=dev)
    ref[:, :c.N], bound[:, :c.N], written[:, :c.N] = rr, rb, True
    r["resid"] = (ref, bound, written)
    # swv2_loss_part_reduce: the fp64 fold of the kernel's own partial sums
    kp = o["part"].double()
    kp = torch.where(pw, kp, torch.zeros_like(kp))
    sums = torch.zeros(SLICES, B, c.Ctar, 2, dtype=F64, device=dev)
    sabs = torch.zeros_like(sums)
    gi = torch.arange(ng, device=dev)
    g_first = (gi * GROUP) // T                                                # sample of each group's first row
    strad = (g_first + 1 < B) & loss_edges(M, T).to(dev)                       # slot 1 belongs to the next sample
    for dst_t, src_t in ((sums, kp), (sabs, kp.abs())):
        view = dst_t[:, :, c.coff:c.coff + Cout]
        view.index_put_((gi % SLICES, g_first), src_t[:, 0], accumulate=True)
        view.index_put_((gi[strad] % SLICES, (g_first + 1)[strad]), src_t[strad][:, 1], accumulate=True)
    sw = torch.zeros(SLICES, B, c.Ctar, 2, dtype=torch.bool, device=dev)
    sw[:, :, c.coff:c.coff + Cout] = True
    r["sums"] = (sums, (-(-ng // SLICES) + 8) * U24 * sabs, sw)
    return r


# ---------------------------------------------------------------------------------------------------------------
# outputs: shapes, prefill; the checker
# ---------------------------------------------------------------------------------------------------------------
def output_specs(c):
    """{output: (shape, dtype, prefill: a value or a tensor)} of what the launch itself writes"""
    k = c.epk
    if k in ("bf16", "f32"):
        return {"out": ((c.rows_out, c.ld), BF if k == "bf16" else torch.float32, NAN)}
    if k == "acc":
        return {"out": ((c.rows_out, c.ld), torch.float32, c.base)}
    if k == "qkv":
        return {"qkvh": ((c.Bw, c.h, 3, c.Lp, c.DP), BF, NAN), "rnorm": ((c.Bw, c.h, 2, c.Lp), torch.float32, 0.0 if wide_heads(c) else NAN)}
    r = {"y": ((c.B, c.Ct, c.H, c.W), torch.float32, NAN)}
    if c.C2:
        r["y2"] = ((c.B, c.C2, c.H, c.W), torch.float32, NAN)
    if k == "loss":
        r["part"] = ((-(-c.M // GROUP), 2, c.Cout, 2), torch.float32, NAN)
        r["resid"] = ((c.M, resid_pitch(c.N)), BF, NAN)
    return r


def same_bits(a, b):
    """elementwise: the same bit pattern (NaN prefill included)"""
    it = torch.int16 if a.dtype == BF else torch.int32
    return a.contiguous().view(it) == b.contiguous().view(it)


def prefill_of(c, name, like):
    spec = output_specs(c).get(name)
    if name == "sums":
        return torch.full_like(like, SENT)
    if name in ("qkvh_raw", "ss"):
        return torch.zeros_like(like)
    pf = spec[2]
    return pf.to(like.device) if torch.is_tensor(pf) else torch.full_like(like, pf)


def check_case(c, o, lut=None, tag=None, worst=None):
    """every element of every output of one run; -> {output: worst |err| / bound}"""
    ref = reference(c, o, lut)
    tag = tag or c.family
    out = {}
    for name, (r, b, written, *rest) in ref.items():
        got = o[name]
        assert got.shape == r.shape, (c.name, name, got.shape, r.shape)
        keep = same_bits(got, prefill_of(c, name, got))
        nbad = int((~keep & ~written).sum())
        assert nbad == 0, f"{c.name} {name}: {nbad} elements the contract leaves alone were written"
        if name not in ("qkvh_raw", "ss"):                       # (snapshots taken between two launches: every element is written)
            nfin = int((~torch.isfinite(got.float()) & written).sum())
            assert nfin == 0, f"{c.name} {name}: {nfin} written elements are not finite"
        rnd = rest[0][written] if rest else None                # the operand's own rounding, or the bf16 rounding of the result
        if got.dtype == BF and not c.exact:
            rnd = U8 * r[written].abs()
        out[name] = P.assert_within(f"{tag} {name}", got[written], r[written], b[written], c.name, rnd, worst=WORST if worst is None else worst)
    return out


# ---------------------------------------------------------------------------------------------------------------
# fp32 emulation with the kernels' rounding points, and the host twins of kernel defects
# ---------------------------------------------------------------------------------------------------------------
MUTANTS = ("gather_next_row", "k_tail", "bias_slot", "rnorm_padded", "q_with_k_norm", "loss_slot_fold", "unpatch_pq", "skip_next_channel")


def _store(c, name, shape, dtype):
    """the output `name` as the launch finds it: its prefill"""
    pf = output_specs(c)[name][2]
    return pf.clone().to(dtype) if torch.is_tensor(pf) else torch.full(shape, pf, dtype=dtype)


def emulate(c, lut=None, mutate=None):
    """the launch in fp32 torch (CPU): {output: tensor}.  mutate: one of MUTANTS"""
    lut = MR.host_gelu_lut() if lut is None else lut
    a = emulated_operand(c, lut)
    tile = 64 if c.kernel in (T64, DX128) else 128
    if mutate == "gather_next_row" and c.rowidx_in is not None and c.opk in ("f32", "bf16"):
        # a row tile's last row reads the gather entry of the row behind it
        src = c.x.to(BF).float()
        m = torch.arange(tile - 1, c.M - 1, tile)
        idx = c.rowidx_in[m + 1].long()
        a[m] = torch.where((idx >= 0).view(-1, 1), src[idx.clamp_min(0)], torch.zeros(()))
    w = c.w.float()
    if mutate == "k_tail" and c.K % 64:
        a, w = a[:, :c.K // 64 * 64], w[:, :c.K // 64 * 64]
    acc = MR._chunked_matmul(a, w, 64) if a.shape[1] else torch.zeros(c.M, c.N)
    if c.bias is not None:
        b = c.bias
        if mutate == "bias_slot":                                # every column reads the bias 16 columns further on
            b = c.bias[(torch.arange(c.N) + 16) % c.N]
        acc = acc + b
    k = c.epk
    live, dst = P.table_of(c.rowidx_out, c.M, acc.device) if k in ("bf16", "f32", "acc") else (None, None)
    if k == "bf16":
        out = _store(c, "out", (c.rows_out, c.ld), BF)
        out[dst[live], :c.N] = acc[live].to(BF)
        return {"out": out}
    if k == "f32":
        out = _store(c, "out", (c.rows_out, c.ld), torch.float32)
        if c.aux is not None:
            acc = acc + c.aux[dst][:, :c.N]
        out[dst[live], :c.N] = acc[live]
        return {"out": out}
    if k == "acc":
        out = _store(c, "out", (c.rows_out, c.ld), torch.float32)
        out[dst[live], :c.N] = out[dst[live], :c.N] + acc[live]
        return {"out": out}
    if k == "qkv":
        return _emulate_qkv(c, acc, mutate)
    return _emulate_head(c, acc, mutate)


def _emulate_qkv(c, acc, mutate):
    vh = _split_heads(acc, c)
    valid = (torch.arange(c.Lp) < c.L).view(1, 1, 1, c.Lp, 1)
    vh = torch.where(valid, vh, torch.zeros(()))
    ss = (vh[:, :, :2] ** 2).sum(-1)
    if wide_heads(c):
        raw = vh.to(BF)
        rn = torch.where(valid.view(1, 1, 1, c.Lp), 1.0 / ss.sqrt().clamp_min(1e-12), torch.zeros(()))
        if mutate == "rnorm_padded":
            rn = 1.0 / ss.sqrt().clamp_min(1e-12)
        out = raw.clone()
        out[:, :, :2] = (raw[:, :, :2].float() * rn.unsqueeze(-1)).to(BF)
        return {"qkvh_raw": raw, "ss": ss, "qkvh": out, "rnorm": rn}
    rn = 1.0 / ss.sqrt().clamp_min(1e-12)
    rn_used = rn
    if mutate == "q_with_k_norm" and c.DP == 32:                 # q rows of the 32-wide slots scaled by k's reciprocal norm
        rn_used = rn[:, :, [1, 1]]
    out = vh.clone()
    out[:, :, :2] = vh[:, :, :2] * rn_used.unsqueeze(-1)
    rn_out = torch.where(valid.view(1, 1, 1, c.Lp), rn, torch.zeros(()))
    if mutate == "rnorm_padded":
        rn_out = rn
    return {"qkvh": out.to(BF), "rnorm": rn_out}


def _emulate_head(c, acc, mutate):
    B, Cout, H, W = c.B, c.Cout, c.H, c.W
    if mutate == "unpatch_pq":
        acc = acc.view(c.M, Cout, 4, 4).transpose(2, 3).reshape(c.M, c.N)
    img = unpatch_image(acc, B, Cout, H, W)
    if c.skip is not None:
        sk = c.skip[:, :Cout]
        if mutate == "skip_next_channel":
            sk = c.skip[:, (torch.arange(Cout) + 1) % c.skip.shape[1]]
        img = img + sk
    o = {}
    for name, Ct, c0 in (("y", c.Ct, c.c0),) + ((("y2", c.C2, 0),) if c.C2 else ()):
        o[name] = _store(c, name, (B, Ct, H, W), torch.float32)
        o[name][:, c0:c0 + Cout] = img
    if c.epk != "loss":
        return o
    t = c.tar[:, c.coff:c.coff + Cout]
    q = c.qw.view(1, 1, H, 1)
    d = img - t
    M, T, ng = c.M, c.T, -(-c.M // GROUP)
    e0 = patch_rows(q * (d * d)).view(M, Cout, 16).sum(-1)
    e1 = patch_rows(q * (t * t)).view(M, Cout, 16).sum(-1)
    rows = torch.arange(M)
    grp = rows // GROUP
    slot = (rows // T != (grp * GROUP) // T).long()
    if mutate == "loss_slot_fold":
        slot = torch.zeros_like(slot)
    part = torch.zeros(ng, 2, Cout, 2)
    part.index_put_((grp, slot), torch.stack([e0, e1], -1), accumulate=True)
    edges = loss_edges(M, T)
    o["part"] = torch.where(edges.view(-1, 1, 1, 1) | (torch.arange(2).view(1, 2, 1, 1) == 0), part, torch.full((), NAN))
    o["resid"] = _store(c, "resid", (M, resid_pitch(c.N)), BF)
    o["resid"][:, :c.N] = patch_rows(q * d).to(BF)
    kp = torch.nan_to_num(o["part"], nan=0.0)
    sums = torch.full((SLICES, B, c.Ctar, 2), SENT)
    view = sums[:, :, c.coff:c.coff + Cout]
    view.zero_()
    gi = torch.arange(ng)
    g_first = (gi * GROUP) // T
    strad = (g_first + 1 < B) & edges
    view.index_put_((gi % SLICES, g_first), kp[:, 0], accumulate=True)
    view.index_put_((gi[strad] % SLICES, (g_first + 1)[strad]), kp[strad][:, 1], accumulate=True)
    o["sums"] = sums
    return o


# ---------------------------------------------------------------------------------------------------------------
# case builders
# ---------------------------------------------------------------------------------------------------------------
def _case(name, family, kernel, opk, epk, M, K, N, exact, wide_env=None, **kw):
    c = types.SimpleNamespace(name=name + ("-exact" if exact else ""), family=family, kernel=kernel, opk=opk, epk=epk, M=M, K=K, N=N, exact=exact,
                              wide_env=wide_env, rowidx_in=None, rowidx_out=None, bias=None, aux=None, aux0=None, base=None, skip=None,
                              prep=None, rows_out=M, ld=N, C2=0)
    for k_, v_ in kw.items():
        setattr(c, k_, v_)
    return c


def _padded_weight(c, w_src, h, d, DP, parts, transpose, g):
    """the head-padded weight: w_src fp32 [parts h d][C] (or its use transposed), row (part h + head) DP + j <- part h d + head d + j,
    zero rows for j >= d; records the prep_weight arguments and the host construction"""
    j = torch.arange(DP)
    one = torch.where(j.view(1, -1) < d, torch.arange(h).view(-1, 1) * d + j.view(1, -1), torch.full((1, 1), -1)).reshape(-1)
    hmap = torch.cat([torch.where(one >= 0, one + p * h * d, one) for p in range(parts)]).to(torch.int32)
    real = hmap >= 0
    if not transpose:                                            # [parts h DP][C]
        w = torch.zeros(hmap.numel(), w_src.shape[1])
        w[real] = w_src[hmap[real].long()]
        c.prep = dict(transpose=False, row_map=hmap, out_rows=hmap.numel(), col_map=None, out_cols=None)
    else:                                                        # [C][parts h DP] = w_src^T with padded columns
        w = torch.zeros(w_src.shape[1], hmap.numel())
        w[:, real] = w_src.T[:, hmap[real].long()]
        c.prep = dict(transpose=True, row_map=None, out_rows=None, col_map=hmap, out_cols=hmap.numel())
    c.w_src, c.w, c.hmap = w_src, w.to(BF), hmap
    return real


def qkv_case(kernel, Cc, h, d, DP, Bw, Lp, L, exact, wide_env=None):
    """OP_F32 gathered through rowidx (-1 on the padded window rows and on about 1 / 8 of the valid ones) -> EPI_QKV_HEADS"""
    M, N = Bw * Lp, 3 * h * DP
    g = _gen(1, Cc, h, DP, Bw, Lp, L, exact)
    name = f"qkv-{KERNEL_NAMES[kernel]}-C{Cc}-h{h}x{d}in{DP}-Bw{Bw}-Lp{Lp}-L{L}" + ("-wide0" if wide_env == "0" else "")
    c = _case(name, KERNEL_NAMES[kernel], kernel, "f32", "qkv", M, Cc, N, exact, wide_env, Bw=Bw, Lp=Lp, L=L, h=h, d=d, DP=DP)
    n_src = Bw * L
    c.x = _values(n_src, Cc, exact, g)
    c.rowidx_in = gather_table(M, n_src, (torch.arange(M) % Lp) < L, g)
    real = _padded_weight(c, _weight(3 * h * d, Cc, exact, g), h, d, DP, 3, False, g)
    c.bias = torch.zeros(N)
    c.bias[real] = _bias(3 * h * d, exact, g)
    c.pad_cols = ~real
    return c


def dx_case(kernel, Cc, h, d, DP, Bw, Lp, L, exact, wide_env=None):
    """OP_HEADS with 3 parts -> EPI_F32 with the residual aux and the scatter rowidx (-1 entries)"""
    M, K = Bw * Lp, 3 * h * DP
    g = _gen(2, Cc, h, DP, Bw, Lp, L, exact)
    name = f"dx-{KERNEL_NAMES[kernel]}-C{Cc}-h{h}x{d}in{DP}-Bw{Bw}-Lp{Lp}-L{L}" + ("-wide0" if wide_env == "0" else "")
    c = _case(name, KERNEL_NAMES[kernel], kernel, "heads", "f32", M, K, Cc, exact, wide_env, Bw=Bw, Lp=Lp, L=L, h=h, d=d, DP=DP)
    real = _padded_weight(c, _weight(3 * h * d, Cc, exact, g), h, d, DP, 3, True, g)
    src = _values(M, K, exact, g) * real.float()                 # the padded head columns of d(qkv) are zeros, as the attention leaves them
    src[(torch.arange(M) % Lp) >= L] = 0
    c.x = src.view(Bw, Lp, 3, h, DP).permute(0, 3, 2, 1, 4).contiguous().to(BF)
    c.rowidx_out, c.rows_out = scatter_table(M, (torch.arange(M) % Lp) < L, g)
    c.aux = _ints((c.rows_out, Cc), -64, 64, g) if exact else torch.randn(c.rows_out, Cc, generator=g)
    return c


PLAIN_MS = (1, 63, 64, 65, 127, 128, 129, 257)
PLAIN_NS = (8, 96, 128, 136, 200, 288)
PLAIN_KS = (8, 64, 72, 1168)
PLAIN_VARIANTS = ("bf16_gather-f32", "gelu-f32_bias", "f32-acc", "f32-acc_scatter", "f32-bf16_scatter")


def plain_case(variant, M, N, K, exact):
    """the plain loaders and epilogues on the tile kernel, output pitch ld = N + 8"""
    g = _gen(3, PLAIN_VARIANTS.index(variant), M, N, K, exact)
    opk = {"bf16_gather": "bf16", "gelu": "gelu", "f32": "f32"}[variant.split("-")[0]]
    epk = {"f32": "f32", "f32_bias": "f32", "acc": "acc", "acc_scatter": "acc", "bf16_scatter": "bf16"}[variant.split("-")[1]]
    c = _case(f"plain-{variant}-M{M}-N{N}-K{K}", "TILE128", T128, opk, epk, M, K, N, exact, ld=N + 8)
    c.w_src = _weight(N, K, exact, g)
    c.w = c.w_src.to(BF)
    if opk == "gelu":
        # pre-activations whose bf16(GELU) is the value itself (exact cases: mlp_reference.EXACT_PRE, and -20 -> 0)
        c.x = (torch.tensor(MR.EXACT_PRE)[torch.randint(0, len(MR.EXACT_PRE), (M, K), generator=g)] if exact else _scaled(M, K, g)).to(BF)
        if exact:
            c.w = (c.w_src.sign()).to(BF)                        # |a| <= 32: K * 32 < 2^24
            c.w_src = c.w.float()
        c.bias = _bias(N, exact, g)
    elif opk == "bf16":
        n_src = M + 3
        c.x = _values(n_src, K, exact, g).to(BF)
        c.rowidx_in = gather_table(M, n_src, torch.ones(M, dtype=torch.bool), g, drop=5)
    else:
        c.x = _values(M, K, exact, g)
    if "scatter" in variant:
        c.rowidx_out, c.rows_out = scatter_table(M, torch.ones(M, dtype=torch.bool), g, drop=5)
    if epk == "acc":
        c.base = (_ints((c.rows_out, c.ld), -64, 64, g) if exact else torch.randn(c.rows_out, c.ld, generator=g) * 4.0)
    return c


def patch_case(Cin, H, W, Cc, second, inside, exact, B=2):
    """PatchEmbed: OP_PATCH -> EPI_BF16 with bias.  second: aux0 added on load; inside: the Cin planes are the first channels of a larger
    tensor (p[3] = Cin + 3) whose other channels hold NaN"""
    g = _gen(4, Cin, H, W, Cc, second, inside, exact)
    M = B * (H // 4) * (W // 4)
    c = _case(f"patch-Cin{Cin}-{H}x{W}-N{Cc}" + ("-second" if second else "") + ("-inside" if inside else ""), "TILE128", T128, "patch", "bf16",
              M, Cin * 16, Cc, exact, B=B, H=H, W=W, Cin=Cin)
    Ct = Cin + 3 if inside else Cin
    c.x = torch.full((B, Ct, H, W), NAN)
    c.x[:, :Cin] = _values(B * Cin * H, W, exact, g).view(B, Cin, H, W)
    c.Ctot = Ct
    if second:
        c.aux0 = torch.full((B, Cin + 2, H, W), NAN)
        c.aux0[:, :Cin] = _values(B * Cin * H, W, exact, g).view(B, Cin, H, W)
    c.w_src = _weight(Cc, Cin * 16, exact, g)
    if exact and second:
        c.w_src = c.w_src.clamp(-2, 2)                           # |x + aux0| <= 8
    c.w = c.w_src.to(BF)
    c.bias = _bias(Cc, exact, g)
    return c


def merge_case(Cc, H, W, exact, B=2):
    """PatchMerging: OP_MERGE_LN -> EPI_F32 (the module's epilogue), N = 2 C.  mean / rstd: the library's own (set by the GPU test
    before the launch; on the host their fp32 twins), or the caller's mean 0, rstd 1 in exact cases"""
    g = _gen(5, Cc, H, W, exact)
    M = B * (H // 2) * (W // 2)
    c = _case(f"merge-C{Cc}-{H}x{W}", "TILE128", T128, "merge", "f32", M, 4 * Cc, 2 * Cc, exact, B=B, H=H, W=W, C=Cc)
    if exact:
        c.x = _ints((B, H, W, Cc), -2, 2, g)
        c.gamma, c.beta = _ints((4 * Cc,), -2, 2, g), _ints((4 * Cc,), -4, 4, g)
        c.mean, c.rstd = torch.zeros(M), torch.ones(M)
    else:
        c.x = _scaled(B * H * W, Cc, g).view(B, H, W, Cc) + torch.randn(B, H, W, 1, generator=g)
        c.gamma, c.beta = signed_log_uniform(4 * Cc, 1e-2, 2.0, g), torch.randn(4 * Cc, generator=g) * 0.1
        xr = merge_rows(c.x, MERGE_ORDER)
        c.mean = xr.mean(1)
        c.rstd = ((xr * xr).mean(1) - c.mean * c.mean).clamp_min(0).add(1e-5).rsqrt()
    c.w_src = _weight(2 * Cc, 4 * Cc, exact, g)
    c.w = c.w_src.to(BF)
    return c


def ref_merge_stats(x):
    """-> (mu, bound, rho, bound) per merged row, fp64 (see "merge stats" in the module docstring)"""
    xr = merge_rows(x.double(), MERGE_ORDER)
    n = xr.shape[1]
    mu = xr.mean(1)
    var = ((xr - mu.view(-1, 1)) ** 2).mean(1)
    rho = (var + P.EPS32).rsqrt()
    dvar = n * 2.0 ** -23 * ((xr * xr).mean(1) + mu * mu)
    return mu, n * 2.0 ** -23 * xr.abs().mean(1), rho, rho * (dvar / (2 * (var + P.EPS32)) + 4 * U24)


def head_case(Cout, gh, gw, Cc, loss, skip, second, sliced, exact, B=3):
    """the head: OP_F32 -> EPI_UNPATCH / EPI_UNPATCH_LOSS.  skip: Cs = Cout + 2 channels; second: a second destination of Cout + 1
    channels per sample; sliced: out is channels 2 .. 2 + Cout of a tensor of Cout + 3 channels (p[4])"""
    g = _gen(6, Cout, gh, gw, Cc, loss, skip, second, sliced, exact)
    H, W, T = 4 * gh, 4 * gw, gh * gw
    M, N = B * T, Cout * 16
    name = f"head-{'loss' if loss else 'plain'}-Cout{Cout}-T{T}-K{Cc}" + ("-skip" if skip else "") + ("-second" if second else "") + ("-sliced" if sliced else "")
    c = _case(name, "TILE64" if loss else "TILE128", T64 if loss else T128, "f32", "loss" if loss else "unpatch", M, Cc, N, exact,
              B=B, H=H, W=W, T=T, Cout=Cout, Ct=Cout + 3 if sliced else Cout, c0=2 if sliced else 0, C2=Cout + 1 if second else 0)
    c.x = _values(M, Cc, exact, g)
    # the head weight: module rows n = (p * 4 + q) * Cout + c -> kernel rows c * 16 + p * 4 + q (row_map of prep_weight)
    c.w_src = _weight(N, Cc, exact, g)
    perm = (torch.arange(16).view(1, -1) * Cout + torch.arange(Cout).view(-1, 1)).reshape(-1).to(torch.int32)
    c.prep = dict(transpose=False, row_map=perm, out_rows=None, col_map=None, out_cols=None)
    c.w = c.w_src[perm.long()].to(BF)
    if skip:
        c.skip = _ints((B, Cout + 2, H, W), -64, 64, g) if exact else torch.randn(B, Cout + 2, H, W, generator=g)
    if loss:
        c.Ctar, c.coff = Cout + 2, 1
        c.tar = _ints((B, c.Ctar, H, W), -8, 8, g) if exact else torch.randn(B, c.Ctar, H, W, generator=g)
        c.qw = (torch.randint(1, 4, (H,), generator=g).float() * 0.25) if exact else (torch.rand(H, generator=g) + 0.1)
    return c


def cscale_case(Cout, T, Cc, exact, B=3):
    """the head's backward operand: OP_BF16_CSCALE (residual rows of the padded pitch, coef per (sample, channel)) -> EPI_F32"""
    g = _gen(7, Cout, T, Cc, exact)
    M, K = B * T, Cout * 16
    c = _case(f"cscale-Cout{Cout}-T{T}-N{Cc}", "TILE128", T128, "cscale", "f32", M, K, Cc, exact, rps=T, B=B)
    c.x = torch.full((M, resid_pitch(K)), NAN, dtype=BF)
    c.x[:, :K] = _values(M, K, exact, g).to(BF)
    c.coef = torch.exp2(torch.randint(-2, 3, (B, Cout), generator=g).float()) * (torch.randint(0, 2, (B, Cout), generator=g).float() * 2 - 1) \
        if exact else signed_log_uniform(B * Cout, 1e-2, 2.0, g).view(B, Cout)
    c.w_src = _weight(Cc, K, exact, g)
    c.w = c.w_src.to(BF)
    return c


def case_to(c, dev):
    def mv(v):
        if torch.is_tensor(v):
            return v.to(dev)
        return {k: mv(x) for k, x in v.items()} if isinstance(v, dict) else v
    return types.SimpleNamespace(**{k: mv(v) for k, v in vars(c).items()})


# ---- the lists the GPU file runs (and the host file asks swv2_linear_kernel about): (builder, arguments) without `exact` -----------
LP, LV = 176, 162
M_WIDE_BW = 27                 # 27 * 176 = 4752 rows >= 16 * 256, ragged last 256-row tile


def qkv_specs():
    r = [(qkv_case, (Q128, 128, 8, 12, 16, 2053, 16, 13)),                    # 32 768 + 80 rows: ragged last tile of the persistent walk
         (qkv_case, (Q128, 128, 8, 16, 16, 2048, 16, 16)),                    # 32 768 rows exactly; Lp = L
         (qkv_case, (Q192, 192, 8, 24, 32, 190, LP, LV)),                     # 33 440 rows
         # Bw * Lp = 176, 2 * 176 and 27 * 176 all name TILE128 (swv2_linear_kernel); TILE64 takes over once the 64-row tiles are about
         # 62 more than the 128-row tiles: 64 * 176 = 11 264 rows
         (qkv_case, (T128, 128, 8, 12, 16, 1, LP, LV)), (qkv_case, (T128, 128, 8, 12, 16, 27, LP, LV)),
         (qkv_case, (T64, 128, 8, 12, 16, 64, LP, LV)),
         (qkv_case, (T128, 192, 8, 24, 32, 2, LP, LV)), (qkv_case, (T64, 192, 8, 24, 32, 64, LP, LV))]
    for Cc, d, DP in ((512, 64, 64), (768, 96, 96), (1024, 128, 128)):
        r.append((qkv_case, (WIDE, Cc, 8, d, DP, M_WIDE_BW, LP, LV)))
        r.append((qkv_case, (T128, Cc, 8, d, DP, M_WIDE_BW, LP, LV, "0")))
    return r


def dx_specs():
    return [(dx_case, (DX128, 128, 8, 12, 16, 1027, 16, 13)),                  # 16 384 + 48 rows
            (dx_case, (DX128, 128, 8, 16, 16, 1024, 16, 16)),                  # 16 384 rows exactly
            (dx_case, (DMA, 192, 8, 24, 32, 94, LP, LV)),                      # 16 544 rows: partial column tile of the DMA kernel
            (dx_case, (T64, 192, 8, 24, 32, 94, LP, LV, "0")),
            (dx_case, (T128, 128, 8, 12, 16, 1, LP, LV)), (dx_case, (T128, 128, 8, 12, 16, 27, LP, LV)),
            (dx_case, (T64, 128, 8, 12, 16, 64, LP, LV)),
            (dx_case, (DMA, 512, 8, 64, 64, M_WIDE_BW, LP, LV)), (dx_case, (T128, 512, 8, 64, 64, M_WIDE_BW, LP, LV, "0"))]


def plain_specs():
    """every variant meets every M, every N and every K at least once"""
    return [(plain_case, (variant, M, PLAIN_NS[(i + vi) % 6], PLAIN_KS[(i + 2 * vi) % 4]))
            for vi, variant in enumerate(PLAIN_VARIANTS) for i, M in enumerate(PLAIN_MS)]


def patch_specs():
    return [(patch_case, a) for a in ((1, 8, 12, 32, False, False), (1, 24, 40, 96, True, True), (7, 8, 12, 96, True, False),
                                      (7, 24, 40, 32, False, True), (73, 8, 12, 96, False, True), (73, 24, 40, 136, True, False))]


def merge_specs():
    return [(merge_case, (Cc, H, W)) for Cc in (32, 128, 192) for H, W in ((4, 6), (18, 36))]


HEAD_GRIDS = ((4, 8), (8, 8), (12, 18))          # T = 32, 64 (group-aligned sample boundaries), 216 (straddling)


def head_specs(loss):
    r = []
    for i, Cout in enumerate((5, 9, 73)):
        for j, (gh, gw) in enumerate(HEAD_GRIDS):
            v = (i + j) % 3                                      # variants cycle so that every Cout and every T meets each
            r.append((head_case, (Cout, gh, gw, (96, 72, 128)[j], loss, v != 0, v == 1, v == 2)))
    r.append((head_case, (5, 12, 18, 96, loss, True, True, True)))
    if loss:        # 108 groups per sample: swv2_loss_part_reduce's unrolled loop (more than 12 * 8 groups) and all four of its sub-slices
        r.append((head_case, (5, 48, 72, 96, loss, True, False, False)))
    return r


def cscale_specs():
    return [(cscale_case, (5, 32, 96)), (cscale_case, (9, 216, 72)), (cscale_case, (73, 64, 128))]


def all_specs():
    return qkv_specs() + dx_specs() + plain_specs() + patch_specs() + merge_specs() + head_specs(False) + head_specs(True) + cscale_specs()


def build(spec, exact):
    fn, args = spec
    if fn in (qkv_case, dx_case):
        return fn(*args[:8], exact, *args[8:])
    return fn(*args, exact)


def spec_id(spec):
    fn, args = spec
    return fn.__name__[:-5] + "-" + "-".join((KERNEL_NAMES[a] if i == 0 and fn in (qkv_case, dx_case) else str(a)) for i, a in enumerate(args))


# ---------------------------------------------------------------------------------------------------------------
# descriptors (the same for the host's swv2_linear_kernel query and the GPU launch) and the host construction of prep_weight
# ---------------------------------------------------------------------------------------------------------------
def host_prep_weight(w_src, transpose=False, row_map=None, out_rows=None, col_map=None, out_cols=None):
    """what swv2_prep_weight makes: out[i][j] = W'[row_map[i]][col_map[j]] (0 where a map entry is negative or past the map), W' = w^T if
    transpose, as bf16"""
    wt = w_src.T if transpose else w_src
    R = out_rows if out_rows is not None else wt.shape[0]
    Cn = out_cols if out_cols is not None else wt.shape[1]
    rm = row_map.long() if row_map is not None else torch.arange(R, device=w_src.device)
    cm = col_map.long() if col_map is not None else torch.arange(Cn, device=w_src.device)
    out = wt[rm.clamp_min(0)][:, cm.clamp_min(0)] * ((rm >= 0).view(-1, 1) & (cm >= 0).view(1, -1))
    return out.to(BF)


def descriptors(c, ops, L, outs):
    """(operand, epilogue, N) of the case's launch; outs: {output: tensor} as output_specs names them (CPU tensors serve the selection
    query, which dereferences nothing)"""
    k = c.opk
    if k == "f32":
        a = ops.operand(L.OP_F32, c.x, c.M, c.K, c.K, c.rowidx_in)
    elif k in ("bf16", "gelu"):
        a = ops.operand(L.OP_BF16_GELU if k == "gelu" else L.OP_BF16, c.x, c.M, c.K, c.K, c.rowidx_in)
    elif k == "heads":
        a = ops.operand(L.OP_HEADS, c.x, c.M, c.K, 3, p=(c.h, 0, c.Lp, c.DP))
    elif k == "patch":
        a = ops.operand(L.OP_PATCH, c.x, c.M, c.K, c.aux0.shape[1] if c.aux0 is not None else 0, aux=(c.aux0, None, None, None),
                        p=(c.Cin, c.H, c.W, c.Ctot if c.Ctot != c.Cin else 0))
    elif k == "merge":
        a = ops.operand(L.OP_MERGE_LN, c.x, c.M, c.K, 0, aux=(c.mean, c.rstd, c.gamma, c.beta), p=(c.H, c.W, c.C, 0))
    else:
        a = ops.operand(L.OP_BF16_CSCALE, c.x, c.M, c.K, c.x.shape[1], aux=(c.coef, None, None, None), p=(c.rps, 0, c.coef.shape[1], 0))
    e = c.epk
    if e in ("bf16", "f32", "acc"):
        kind = {"bf16": L.EPI_BF16, "f32": L.EPI_F32, "acc": L.EPI_F32_ACC}[e]
        ep = ops.epilogue(kind, outs["out"], ld=c.ld, bias=c.bias, aux=c.aux, rowidx=c.rowidx_out)
    elif e == "qkv":
        ep = ops.epilogue(L.EPI_QKV_HEADS, outs["qkvh"], bias=c.bias, aux_out=outs["rnorm"], p=(c.h, 0, c.Lp, c.DP, c.L))
    else:
        y = outs["y"]
        out = y[:, c.c0:] if c.Ct != c.Cout else y             # (a view: the first element of channel c0 of sample 0)
        p = (c.Cout, c.H, c.W, c.skip.shape[1] if c.skip is not None else 0, c.Ct if c.Ct != c.Cout else 0)
        if e == "unpatch":
            ep = ops.epilogue(L.EPI_UNPATCH, out, aux=c.skip, aux_out=outs.get("y2"), ld=c.C2, p=p)
        else:
            loss = (c.tar, c.qw, outs["part"], outs["resid"], c.coff) + ((y,) if c.Ct != c.Cout else ())
            if y.is_cuda:
                ep = ops.epilogue(L.EPI_UNPATCH_LOSS, out, aux=c.skip, aux_out=outs.get("y2"), ld=c.C2, p=p, loss=loss)
            else:               # (ops.epilogue insists on device tensors for the loss: the host's selection query fills the same fields)
                ep = ops.epilogue(L.EPI_UNPATCH_LOSS, out, aux=c.skip, aux_out=outs.get("y2"), ld=c.C2, p=p)
                ep.loss_tar, ep.loss_qw, ep.loss_part, ep.loss_resid = (t.data_ptr() for t in loss[:4])
                ep.q[0], ep.q[1], ep.q[2] = c.Ctar, c.coff, (y.numel() - c.c0 * c.H * c.W if c.Ct != c.Cout else 0)
    return a, ep, c.N
