"""fp64 references and per-element bound checkers for the fused MLP pair (swv2_mlp_fwd / swv2_mlp_bwd, csrc/mlp.hip) and the
unfused fc1 / dh epilogues (EPI_BF16_GELU, EPI_GELU_GRAD), shared by tests/test_mlp_exact_gpu.py (the kernels) and
tests/test_mlp_exact_host.py (the references and bounds themselves, no GPU).  Plain torch; runs on whatever device its inputs
live on.  LayerNorm statistics, y, da2 and the dgamma / dbeta references are those of tests/proj_ln_reference.py without a row table.

Every reference is fp64 of exactly what the next stage of the kernel reads, and every output is judged against the kernel's own
saved upstream tensor, so one stage's rounding is not charged to the next.  With K1 = C, K2 = hidden:
  hpre   |hpre - v| <= 2^-8 |v| + K1 2^-23 (|bf16(x)| |w1|^T + |b1|)      v = bf16(x) w1^T + b1
  a2     |a2 - v| <= 2^-8 |v| + K2 2^-23 (|act| |w2|^T + |b2|)            v = act w2^T + b2, act = gelu_lut[bits of the kernel's hpre]:
                                                                         the library's own bf16(GELU), itself held to fp64 by ref_gelu
  mean, rstd, y                                                          as proj + LN1: C 2^-23 mean_c |a2|, C 2^-22 relative,
                                                                         2^-20 (|x| + |s| (|a2 - mean| rstd |gamma| + |beta|))
  da2    |da2 - ref| <= 2^-8 |ref| + C 2^-22 rstd (|g| + T1 + |xhat| T2) as da1 of proj + LN1
  dh     |dh - ref| <= 2^-8 |ref| + C 2^-23 (|da2| |w2|) |GELU'| + B' |G| ref = G GELU'_64(hpre), G = (kernel's da2) w2 in fp64.  The
                                                                         middle term is the fp32 accumulation of G (C terms, doubled),
                                                                         the last the fp32 GELU' (gelu_grad_bar)
  dx     |dx - ref| <= 2^-23 |dy| + K2 2^-23 (|dh| |w1|)                  ref = dy + (kernel's dh) w1
  dgamma |dgamma - base - sum_rows d xhat| <= C_FOLD_MLP sum_rows |d xhat| + 2^-24 |base|, dbeta alike with d (see C_FOLD_MLP)
2^-8 is bf16's unit roundoff: hpre, a2, da2 and dh reach their bound's first term by construction; what the fp32 arithmetic adds
is reported apart ("beyond rounding").
"""
import math
import types

import torch

from tests import proj_ln_reference as P
from tests.proj_ln_reference import BF, F64, SENT, RPS, within, rounding_share, case_to, signed_log_uniform, scale_cycle  # noqa: F401

# dgamma / dbeta of swv2_mlp_bwd: the fold's own order, read off the kernel's code.  mlp_bwd_kernel keeps a thread on 4 columns and sums its rows by fma, one per
# row pass (NPASS = 64 MT / RPP passes of RPP = 256 / LPR rows; LPR = 8, 16, 32, 32, 64, 64 lanes per row at C = 32 .. 256), stores the
# RPP row groups' sums to LDS and adds them in order (the first addition is onto 0: RPP - 1 roundings), writes one partial row per
# workgroup, and ln_partials_reduce adds ceil(workgroups / 64) partial rows in a thread (the first onto 0), six tree levels and the sum
# onto dgamma / dbeta.  Roundings of partial sums a row's contribution can pass through:
#   <32, 1>  2 + 31   <64, 1>  4 + 15   <96, 1> / <128, 1>  8 + 7    <192, 1> / <256, 1>  16 + 3      -> at most 33 (MT = 1)
#   <32, 2>  4 + 31   <64, 2>  8 + 15   <96, 2> / <128, 2>  16 + 7                                    -> at most 35 (MT = 2)
#   ln_partials_reduce: (ceil(workgroups / 64) - 1) + 6 + 1 <= 14 up to 512 workgroups (M <= 32 767 at MT = 1, M <= 65 536 at MT = 2)
# i.e. <= 35 + 14 = 49 additions, each rounding a partial sum of magnitude <= A = sum_rows |addend| by 2^-24, plus the roundings of the
# addend itself: d = s * dy (1) and xhat = (a2 - mean) * rstd (2); the product d * xhat enters by fma unrounded.  52 * 2^-24 * A to
# first order for M <= 65 536, and 2^-24 |base| for the baseline's share of the last addition.
C_FOLD_MLP = 52 * 2.0 ** -24

CS = (32, 64, 96, 128, 192, 256)
# hidden sizes: one chunk | odd chunk count (the tail store) | 128 | the recompute limit and <192, 1>'s bias-table limit | just past it |
# the maximum
HIDDENS = (32, 96, 128, 1024, 1056, 2048)
# rows: one | below a wave tile | one workgroup exactly | a workgroup + 13 | 2 workgroups + 48 (a whole wave of duplicates)
MS = (1, 13, 64, 77, 176)
M_BIG = 128 * 256 + 80          # MT = 2 (M >= 32 768): 256 workgroups of 128 rows + one of 80 (its third wave holds 16 rows, its fourth none)
# every C meets every hidden class; M cycles so that every M class meets every C
CASES = [(C, hid, MS[(i + j) % 5]) for i, C in enumerate(CS) for j, hid in enumerate(HIDDENS)] + [(192, 1056, 176)]
BIG_CASES = [(32, 64, M_BIG), (96, 64, M_BIG), (128, 64, M_BIG)]
NO_SCALE_CASES = [(C, 128, 176) for C in CS]
EXACT_CASES = [(32, 96, 77), (64, 128, 64), (96, 96, 176), (128, 1024, 77), (192, 1056, 77), (256, 2048, 13), (32, 64, M_BIG)]
RECOMP_MAX_HIDDEN = 1024


def case_id(p):
    return "C%d-hid%d-M%d" % tuple(p[:3])


def fwd_mt(C, hid, M):
    """row tiles per wave of the forward instantiation swv2_mlp_fwd launches"""
    if C == 192:
        return 2 if hid > 1024 else 1
    return 2 if (M >= 128 * 256 and C <= 128) else 1


def bwd_mt(C, M):
    return 2 if (M >= 128 * 256 and C <= 128) else 1


# ---------------------------------------------------------------------------------------------------------------
# GELU and GELU' : fp64, the fp32 formulas of csrc/gemm_common.h transcribed, the table range
# ---------------------------------------------------------------------------------------------------------------
def gelu64(x):
    """erf-GELU in fp64, through erfc so that the negative tail keeps its digits"""
    x = x.double()
    return 0.5 * x * torch.special.erfc(-x / math.sqrt(2.0))


def gelu_grad64(x):
    """GELU'(x) = Phi(x) + x phi(x) in fp64"""
    x = x.double()
    return 0.5 * torch.special.erfc(-x / math.sqrt(2.0)) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def bf16_bits_all(device="cpu"):
    """all 65 536 bf16 patterns, indexed by the pattern"""
    return torch.arange(65536, dtype=torch.int32, device=device).to(torch.int16).view(BF)


def bits_of(t):
    """bf16 tensor -> its patterns as int64 in 0 .. 65535"""
    return t.contiguous().view(torch.int16).long() & 0xFFFF


def lut_of(lut, pre_bf16):
    return lut[bits_of(pre_bf16)]


GT_LO, GT_HALF = (127 - 14) << 7, 18 * 128           # the table: bf16 patterns of 2^-14 <= |x| < 16


def in_table(t):
    a = bits_of(t) & 0x7FFF
    return (a >= GT_LO) & (a < GT_LO + GT_HALF)


def _fma(a, b, c):
    """fp32 fma: the product of two fp32 values is exact in fp64; one fp64 rounding of the sum before the fp32 one (a double rounding
    can differ from the fused result by one fp32 ulp in rare ties, far below what this emulation is used to measure)"""
    return (a.double() * b.double() + c.double()).float()


def erf_parts32(x):
    """erf_parts of gemm_common.h in fp32, with a correctly rounded reciprocal and exp (v_rcp_f32 and __expf are not) -> (erf, gauss)"""
    x = x.float()
    z = x.abs() * torch.tensor(0.70710678118654752, dtype=torch.float32)
    t = (1.0 / _fma(torch.tensor(0.3275911, dtype=torch.float32), z, torch.ones((), dtype=torch.float32)).double()).float()
    gauss = torch.exp(-(z * z).double()).float()
    c = [torch.tensor(v, dtype=torch.float32) for v in (1.061405429, -1.453152027, 1.421413741, -0.284496736, 0.254829592)]
    poly = t * _fma(t, _fma(t, _fma(t, _fma(t, c[0], c[1]), c[2]), c[3]), c[4])
    e = _fma(-poly, gauss, torch.ones((), dtype=torch.float32))
    return torch.copysign(e, x), gauss


def gelu32(x):
    e, _ = erf_parts32(x)
    return (0.5 * x.float()) * (1.0 + e)


def gelu_grad32(x):
    e, gs = erf_parts32(x)
    return _fma(x.float() * torch.tensor(0.3989422804014327, dtype=torch.float32), gs, 0.5 * (1.0 + e))


_CACHE = {}


def host_gelu_lut():
    """the host stand-in of the library's bf16(GELU(x)) for all 65 536 patterns (fp32, indexed by the pattern)"""
    if "lut" not in _CACHE:
        _CACHE["lut"] = gelu32(bf16_bits_all().float()).to(BF).float()
    return _CACHE["lut"]


def host_gelu_grad_lut():
    """fp32 GELU' (emulated gelu_grad_f) for all 65 536 patterns"""
    if "glut" not in _CACHE:
        _CACHE["glut"] = gelu_grad32(bf16_bits_all().float())
    return _CACHE["glut"]


def gelu_grad_emulation_error():
    """(worst |emulated fp32 gelu_grad_f - fp64| over every finite bf16 input, the input)"""
    if "gerr" not in _CACHE:
        x = bf16_bits_all().float()
        fin = torch.isfinite(x)
        err = (host_gelu_grad_lut().double() - gelu_grad64(x)).abs()
        err = torch.where(fin, err, torch.zeros_like(err))
        i = int(err.argmax())
        _CACHE["gerr"] = (float(err[i]), float(x[i]))
    return _CACHE["gerr"]


def gelu_grad_bar():
    """B': the absolute error bar of the fp32 gelu_grad_f.  4 x the worst error of its fp32 transcription (correctly rounded rcp and
    exp) against fp64 over every finite bf16 input: 4 x 2.28e-7 (at x = 0.0864), close to 2^-20.  The factor pays for v_rcp_f32
    (1 ulp) and __expf (a few ulp of a value <= 1), which enter through t -- poly has |d poly / d t| < 1.5 -- and through gauss
    (coefficient poly + |x| / sqrt(2 pi) < 1.3 where gauss matters), and for the half table's 1 - g (one rounding, 2^-25)."""
    return 4.0 * gelu_grad_emulation_error()[0]


def ref_gelu(x):
    """the forward GELU's bar as test_gelu_operand_on_every_bf16_input states it, for finite bf16 x -> (ref, bound): on [-3, 3] one
    bf16 ulp around bf16(fp64 GELU), the correctly rounded value (subnormal inputs: 2^-126 around fp64); outside [-3, 3]
    2^-8 |ref| + 2^-21 |x| around fp64 (1 + erf cancels in fp32 below -3)"""
    x = x.double()
    ref = gelu64(x)
    rq = ref.float().to(BF).double()
    ulp = torch.exp2(torch.floor(torch.log2(rq.abs().clamp_min(2.0 ** -126))) - 7)
    core, sub = x.abs() <= 3, x.abs() < 2.0 ** -126
    r = torch.where(core & ~sub, rq, ref)
    b = torch.where(core, torch.where(sub, torch.full_like(ulp, 2.0 ** -126), ulp), 2.0 ** -8 * ref.abs() + 2.0 ** -21 * x.abs())
    return r, b


# ---------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------
def _finish(c, g, with_scale, baseline):
    C, M = c.C, c.M
    c.rps = RPS
    c.scale = scale_cycle(M, RPS) if with_scale else None
    assert c.scale is None or float(c.scale[(M - 1) // RPS]) != 0            # the last row's sample is not dropped
    c.dy = torch.randn(M, C, generator=g)
    c.dy[M - 1] *= 64.0                  # a doubled or dropped last row moves dgamma / dbeta far beyond C_FOLD_MLP * A
    sgn = lambda: torch.randint(0, 2, (C,), generator=g).float() * 2 - 1          # noqa: E731
    if baseline:
        c.base_g, c.base_b = torch.randint(1, 4, (C,), generator=g).float() * sgn(), torch.randint(1, 4, (C,), generator=g).float() * sgn()
    else:
        c.base_g, c.base_b = torch.zeros(C), torch.zeros(C)
    return c


def make_case(C, hid, M, mode="random", with_scale=True, baseline=True, seed=0):
    """the operands of one fused-MLP case, on the CPU (case_to moves them); weights as the bf16 tensors the kernels read.
    "random": magnitudes log-uniform over three decades with random signs; pre-activations of order 1, fc2 outputs of order 2^-6 so
    that eps = 1e-5 is a visible share of every row's variance.
    "exact": operands for which no rounding can occur up to a2 and from the kernel's da2 to dh and dx (see test_exact_*): one-hot x
    rows, w1 + b1 in EXACT_PRE (bf16(GELU(p)) == p and GELU'(p) == 1, or p = -20 with both 0), w2 with one +-1 per column in its first
    4 C columns (|a2| <= 4 * 32 + 8), and a backward-only w1t with one +-1 per row."""
    g = torch.Generator().manual_seed(1000003 * seed + 7919 * C + 131 * hid + M)
    c = types.SimpleNamespace(C=C, hid=hid, M=M, mode=mode)
    if mode == "exact":
        col = torch.randint(0, C, (M,), generator=g)
        c.x = torch.zeros(M, C)
        c.x[torch.arange(M), col] = 1.0
        pre = torch.tensor(EXACT_PRE)[torch.randint(0, len(EXACT_PRE), (hid, C), generator=g)]
        c.b1 = torch.randint(-2, 3, (hid,), generator=g).float()
        c.w1 = (pre - c.b1.view(-1, 1)).to(BF)
        w2 = torch.zeros(C, hid)
        j = torch.arange(min(hid, 4 * C))
        w2[j % C, j] = torch.randint(0, 2, (j.numel(),), generator=g).float() * 2 - 1
        c.w2, c.b2 = w2.to(BF), torch.randint(-8, 9, (C,), generator=g).float()
        w1t = torch.zeros(C, hid)
        w1t[torch.arange(C), torch.randint(0, hid, (C,), generator=g)] = torch.randint(0, 2, (C,), generator=g).float() * 2 - 1
        c.w1t_exact = w1t.to(BF)
    else:
        c.x = signed_log_uniform(M * C, 4e-3, 4.0, g).view(M, C)
        c.w1 = (signed_log_uniform(hid * C, 2e-3, 2.0, g).view(hid, C) * (2.0 / math.sqrt(C))).to(BF)
        c.b1 = signed_log_uniform(hid, 1e-3, 1.0, g)
        c.w2 = (signed_log_uniform(C * hid, 2e-3, 2.0, g).view(C, hid) * (2.0 ** -5 / math.sqrt(hid))).to(BF)
        c.b2 = signed_log_uniform(C, 1e-3, 1.0, g) * 2.0 ** -6
    c.w1t, c.w2t = c.w1.T.contiguous(), c.w2.T.contiguous()
    c.gamma, c.beta = signed_log_uniform(C, 1e-3, 2.0, g), torch.randn(C, generator=g)
    return _finish(c, g, with_scale, baseline)


EXACT_PRE = [8.0, 9.0, 10.0, 11.0, 12.0, 13.0, 14.0, 15.0, 16.0, 24.0, 32.0, -20.0]


# ---- the two sweeps over every finite bf16 pattern --------------------------------------------------------------
# A wave of either kernel decides between the table and the formula for 16 rows x 16 hidden units at a time (`__any(bad)` over the
# lanes (row, 4 hidden units) of one accumulator tile), and 93 % of the finite patterns lie outside the table: patterns shuffled
# freely would send every tile to the formula.  The sweeps therefore lay the patterns out in aligned 16 x 16 tiles: per copy 18 tiles
# of table patterns only (the table path), 237 tiles of patterns outside it, and at least one mixed tile per layout: table patterns
# around +0, -0, the largest |x| < 2^-14, 16 and -16 and subnormals -- the formula path with table neighbours present.
def sweep_bits(rows, cols, g):
    """int64 [rows][cols] of bf16 patterns: floor(tiles / 255) copies of every finite pattern, the remaining tiles mixed; tiles at
    random places.  rows, cols multiples of 16."""
    assert rows % 16 == 0 and cols % 16 == 0
    tiles = (rows // 16) * (cols // 16)
    copies = tiles // 255
    assert copies >= 1 and tiles - 255 * copies >= 1, (rows, cols)
    bits = torch.arange(65536)
    fin = torch.isfinite(bf16_bits_all().float())
    tab = in_table(bf16_bits_all())
    t_in, t_out = bits[fin & tab], bits[fin & ~tab]
    assert t_in.numel() == 18 * 256 and t_out.numel() == 237 * 256
    parts = []
    for _ in range(copies):
        parts += [t_in[torch.randperm(t_in.numel(), generator=g)], t_out[torch.randperm(t_out.numel(), generator=g)]]
    special = torch.tensor([0x0000, 0x8000, GT_LO - 1, 0x8000 | (GT_LO - 1), GT_LO + GT_HALF, 0x8000 | (GT_LO + GT_HALF), 0x0001, 0x807F])
    for _ in range(tiles - 255 * copies):
        t = t_in[torch.randint(0, t_in.numel(), (256,), generator=g)]
        t[torch.randperm(256, generator=g)[:special.numel()]] = special
        parts.append(t)
    stream = torch.cat(parts).view(tiles, 16, 16)[torch.randperm(tiles, generator=g)]
    return stream.view(rows // 16, cols // 16, 16, 16).permute(0, 2, 1, 3).reshape(rows, cols).contiguous()


def from_bits(b):
    return b.to(torch.int32).to(torch.int16).view(BF)


def sweep_tiles(bits):
    """per 16 x 16 tile: (any pattern outside the table, any inside) -> the tile's class: 0 table only, 1 formula only, 2 mixed"""
    r, c = bits.shape
    t = in_table(from_bits(bits)).view(r // 16, 16, c // 16, 16)
    any_in, all_in = t.any(3).any(1), t.all(3).all(1)
    return torch.where(all_in, 0, torch.where(any_in, 2, 1))


def fwd_sweep_rows(C):
    """65 536 / C rows, rounded up to whole 16-row tiles that leave at least one tile beyond the 255 of one copy"""
    return 16 * -(-256 // (C // 16))


def hpre_matches(hpre, want_bits):
    """the sweeps' identity products: hpre is the pattern bit for bit; for zeros and subnormal patterns it may also be a signed zero
    (a sum that starts from a +0 bias turns -0 into +0, and the matrix cores may flush subnormal operands)"""
    got = bits_of(hpre)
    return (got == want_bits) | (((want_bits & 0x7F80) == 0) & ((got & 0x7FFF) == 0))


def make_fwd_sweep(C, rows, hid=None, seed=0):
    """forward GELU sweep: hidden = C, w1 = w2 = I, b1 = b2 = 0 (hid > C: w1[j][j % C] = 1, w2[n][n] = 1), x = the patterns as fp32"""
    g = torch.Generator().manual_seed(424243 * seed + 31 * C + rows)
    hid = hid or C
    c = types.SimpleNamespace(C=C, hid=hid, M=rows, mode="fwd_sweep", rps=RPS, scale=None)
    c.bits = sweep_bits(rows, C, g)
    c.x = from_bits(c.bits).float()
    w1 = torch.zeros(hid, C)
    w1[torch.arange(hid), torch.arange(hid) % C] = 1.0
    w2 = torch.zeros(C, hid)
    w2[torch.arange(C), torch.arange(C)] = 1.0
    c.w1, c.w2, c.b1, c.b2 = w1.to(BF), w2.to(BF), torch.zeros(hid), torch.zeros(C)
    c.gamma, c.beta = torch.ones(C), torch.zeros(C)
    return c


SWEEP_MIN_G = 2.0 ** -4            # every pattern must meet a |da2| of at least this


def make_bwd_sweep(C, M, hid, recompute=False, seed=0):
    """backward GELU' sweep: hpre = the patterns (recompute: hidden = C, w1 = I, b1 = 0, the patterns in x), w2t[j][j % C] = 1, so that
    G[m][j] is the kernel's own da2[m][j % C] exactly; a2 random bf16 with its true statistics, dy random, no drop-path."""
    g = torch.Generator().manual_seed(535357 * seed + 37 * C + M + hid + int(recompute))
    c = types.SimpleNamespace(C=C, hid=hid, M=M, mode="bwd_sweep", rps=RPS, scale=None, recompute=recompute)
    c.bits = sweep_bits(M, hid, g)
    c.hpre = from_bits(c.bits)
    w2t = torch.zeros(hid, C)
    w2t[torch.arange(hid), torch.arange(hid) % C] = 1.0
    c.w2t = w2t.to(BF)
    if recompute:
        assert hid == C
        c.x, c.w1, c.b1 = c.hpre.float(), torch.eye(C).to(BF), torch.zeros(hid)
    else:
        c.x = None
        c.w1 = (signed_log_uniform(hid * C, 2e-3, 2.0, g).view(hid, C) * (2.0 / math.sqrt(C))).to(BF)
        c.b1 = torch.zeros(hid)
    c.w1t = c.w1.T.contiguous()
    c.a2 = (torch.randn(M, C, generator=g) * 1.5 + 0.25 * torch.randn(M, 1, generator=g)).to(BF)
    af = c.a2.float()
    c.mean = af.mean(1)
    c.rstd = 1.0 / torch.sqrt(((af - c.mean.view(-1, 1)) ** 2).mean(1) + 1e-5)
    c.gamma = signed_log_uniform(C, 0.5, 2.0, g)
    c.dy = signed_log_uniform(M * C, 0.5, 4.0, g).view(M, C)
    c.base_g, c.base_b = torch.zeros(C), torch.zeros(C)
    return c


def sweep_coverage(bits, G):
    """bool [65536]: pattern p sits somewhere with |G| >= SWEEP_MIN_G (G shaped like bits)"""
    ok = torch.zeros(65536, dtype=torch.bool, device=bits.device)
    ok[bits[G.abs() >= SWEEP_MIN_G]] = True
    return ok


def finite_patterns(device="cpu"):
    return torch.isfinite(bf16_bits_all(device).float())


# ---------------------------------------------------------------------------------------------------------------
# references (fp64) with their bounds
# ---------------------------------------------------------------------------------------------------------------
def ref_linear(a, w, b, K):
    """v = a w^T + b in fp64 and 2^-8 |v| + K 2^-23 (|a| |w|^T + |b|): a bf16 result of K fp32 accumulations in any order"""
    a, w = a.double(), w.double()
    v = a @ w.T
    A = a.abs() @ w.abs().T
    if b is not None:
        v, A = v + b.double(), A + b.double().abs()
    return v, 2.0 ** -8 * v.abs() + K * 2.0 ** -23 * A


def ref_hpre(x, w1, b1):
    """-> (v, bound) from the fp32 x (rounded to bf16 as the kernels round it), the bf16 w1 [hid][C] and the fp32 bias"""
    return ref_linear(x.to(BF), w1, b1, w1.shape[1])


def ref_a2(hpre, lut, w2, b2):
    """-> (v, bound) from the KERNEL's hpre, the library's bf16(GELU) table, the bf16 w2 [C][hid]"""
    return ref_linear(lut_of(lut, hpre), w2, b2, w2.shape[1])


def ref_dh(da2, w2t, hpre, Bp):
    """dh = ((kernel's da2) w2) GELU'(kernel's / caller's hpre); w2t bf16 [hid][C].  -> (ref, bound, G)"""
    d, w = da2.double(), w2t.double()
    G = d @ w.T
    gp = gelu_grad64(hpre.float())
    ref = G * gp
    bound = 2.0 ** -8 * ref.abs() + da2.shape[1] * 2.0 ** -23 * (d.abs() @ w.abs().T) * gp.abs() + Bp * G.abs()
    return ref, bound, G


def ref_dx(dy, dh, w1t):
    """dx = dy + (kernel's dh) w1; w1t bf16 [C][hid].  -> (ref, bound)"""
    d, w = dh.double(), w1t.double()
    return dy.double() + d @ w.T, 2.0 ** -23 * dy.double().abs() + dh.shape[1] * 2.0 ** -23 * (d.abs() @ w.abs().T)


def fold_bound(A, base):
    """dgamma / dbeta: C_FOLD_MLP * A + 2^-24 |base| (nothing where A = 0: base + 0 is exact)"""
    return C_FOLD_MLP * A + 2.0 ** -24 * base.double().abs() * (A > 0)


# ---------------------------------------------------------------------------------------------------------------
# checkers
# ---------------------------------------------------------------------------------------------------------------
WORST = {}          # name -> worst |err| / bound seen so far (reported by the GPU tests)


def assert_within(name, got, ref, bound, what="", rnd=None):
    """proj_ln_reference.assert_within, filed in this module's WORST"""
    return P.assert_within(name, got, ref, bound, what, rnd, worst=WORST)


def check_fc1(name, c, hpre, what=""):
    v, vb = ref_hpre(c.x, c.w1, c.b1)
    return {"hpre": assert_within(name + " hpre", hpre, v, vb, what, rounding_share(v))}


def check_fc2(name, c, lut, hpre, a2, what=""):
    v, vb = ref_a2(hpre, lut, c.w2, c.b2)
    return {"a2": assert_within(name + " a2", a2, v, vb, what, rounding_share(v))}


def check_ln(name, c, a2, mean, rstd, y, what=""):
    """mean, rstd, y from the kernel's saved a2 (and y from its saved statistics); no row table, every row written"""
    mu, mub, rho, rhob = P.ref_stats(a2)
    r = {"mean": assert_within(name + " mean", mean, mu, mub, what), "rstd": assert_within(name + " rstd", rstd, rho, rhob, what)}
    yr, yb = P.ref_y(torch.full_like(c.x, SENT), a2, mean, rstd, c.gamma, c.beta, c.x, c.scale, None, c.rps)
    r["y"] = assert_within(name + " y", y, yr, yb, what)
    return r


def check_all_forward(name, c, lut, hpre, a2, mean, rstd, y, what="", hpre_for_a2=None):
    """every forward bound on one run's outputs -> {output: worst ratio}.  hpre = None: a run that kept none; its a2 is judged from
    hpre_for_a2, the pre-activation its twin saved"""
    r = check_fc1(name, c, hpre, what) if hpre is not None else {}
    r.update(check_fc2(name, c, lut, hpre if hpre is not None else hpre_for_a2, a2, what))
    r.update(check_ln(name, c, a2, mean, rstd, y, what))
    return r


def check_ln_backward(name, c, a2, mean, rstd, da2, dgamma, dbeta, what=""):
    rf = P.ref_ln_bwd(a2, mean, rstd, c.gamma, c.dy, c.scale, None, c.rps)
    r = {"da2": assert_within(name + " da2", da2, rf.da, rf.da_bound, what, rounding_share(rf.da))}
    # (the baseline is an integer: got - base is exact in fp64.  Its 2^-24 |base| is a rounding term like the 2^-8 of the bf16 outputs --
    # the last addition rounds to the baseline's grid, so a column with A << |base| reaches it by construction: what the fold itself
    # uses of C_FOLD_MLP * A is filed apart as "beyond rounding")
    r["dgamma"] = assert_within(name + " dgamma", dgamma.double() - c.base_g.double(), rf.dgamma, fold_bound(rf.A_g, c.base_g), what,
                                2.0 ** -24 * c.base_g.double().abs() * (rf.A_g > 0))
    r["dbeta"] = assert_within(name + " dbeta", dbeta.double() - c.base_b.double(), rf.dbeta, fold_bound(rf.A_b, c.base_b), what,
                               2.0 ** -24 * c.base_b.double().abs() * (rf.A_b > 0))
    return r


def check_dh(name, da2, w2t, hpre, dh, Bp, what=""):
    ref, bound, G = ref_dh(da2, w2t, hpre, Bp)
    return {"dh": assert_within(name + " dh", dh, ref, bound, what, rounding_share(ref))}


def check_dx(name, dy, dh, w1t, dx, what=""):
    ref, bound = ref_dx(dy, dh, w1t)
    return {"dx": assert_within(name + " dx", dx, ref, bound, what)}


def check_all_backward(name, c, a2, mean, rstd, hpre, da2, dh, dx, dgamma, dbeta, Bp, what="", w1t=None):
    r = check_ln_backward(name, c, a2, mean, rstd, da2, dgamma, dbeta, what)
    r.update(check_dh(name, da2, c.w2t, hpre, dh, Bp, what))
    r.update(check_dx(name, c.dy, dh, c.w1t if w1t is None else w1t, dx, what))
    return r


def gelu_grad_ratio(da2, w2t, hpre, dh):
    """the share of B' |G| that dh's error uses once the rounding of dh itself and G's accumulation are taken off:
    worst (|dh - ref| - 2^-8 |ref| - C 2^-23 (|da2| |w2|) |GELU'|) / (B' |G|) over the elements with G != 0, for B' = 1: i.e. an
    upper estimate of the fp32 GELU's absolute error, to be compared with gelu_grad_bar()"""
    ref, bound, G = ref_dh(da2, w2t, hpre, 0.0)
    ex = ((dh.double() - ref).abs() - bound).clamp_min(0) / G.abs().clamp_min(1e-300)
    return float(torch.where(G == 0, torch.zeros_like(ex), ex).max())


def check_guard_rows(buf, g):
    """buf: a flat buffer whose first and last g elements are guards prefilled with SENT"""
    return bool((buf[:g] == SENT).all() and (buf[buf.numel() - g:] == SENT).all())


# ---------------------------------------------------------------------------------------------------------------
# fp32 / bf16 emulation of both kernels from the oracle's rounding points (host tests; mutate = one of the mutants' twins)
# ---------------------------------------------------------------------------------------------------------------
GUARD = 128           # guard rows on either side of every emulated output


def _guarded(rows, cols, dtype):
    buf = torch.full(((rows + 2 * GUARD) * cols,), SENT, dtype=dtype)
    return buf, buf[GUARD * cols:(GUARD + rows) * cols].view(rows, cols) if cols > 1 else buf[GUARD:GUARD + rows]


def _chunked_matmul(a, w, step=32):
    """a [M][K] w[N][K]^T accumulated in fp32 in chunks of `step` along K, in order"""
    acc = torch.zeros(a.shape[0], w.shape[0])
    for k in range(0, a.shape[1], step):
        acc = acc + a[:, k:k + step] @ w[:, k:k + step].T
    return acc


def emulate(c, mutate=None, hpre_in=None):
    """forward and backward in fp32 torch with the kernels' rounding points: bf16 x, hpre, GELU (table), a2, da2, dh; fp32 sums over
    32 hidden units at a time.  Outputs sit between guard rows (namespace fields *_buf).  hpre_in: the backward reads this
    pre-activation (the sweeps).  mutate: "a" .. "i", the host twins of the kernel mutants in LABNOTES.md."""
    C, hid, M = c.C, c.hid, c.M
    lut, glut = host_gelu_lut().clone(), host_gelu_grad_lut().clone()
    allb = bf16_bits_all()
    tab = in_table(allb)
    if mutate == "b":            # arguments outside the table read the clamped entry: the last one of their sign's half
        idx = torch.arange(65536)
        clamp = (idx & 0x8000) | (GT_LO + GT_HALF - 1)
        lut[~tab], glut[~tab] = lut[clamp[~tab]], glut[clamp[~tab]]
    if mutate == "c":            # the table holds the next pattern's value
        idx = torch.arange(65536)
        lut[tab], glut[tab] = host_gelu_lut()[idx[tab] + 1], host_gelu_grad_lut()[idx[tab] + 1]
    e = types.SimpleNamespace()
    bufs = {}
    for k, cols, dt in (("y", C, torch.float32), ("hpre", hid, BF), ("a2", C, BF), ("mean", 1, torch.float32), ("rstd", 1, torch.float32),
                        ("da2", C, BF), ("dh", hid, BF), ("dx", C, torch.float32)):
        bufs[k], view = _guarded(M, cols, dt)
        setattr(e, k, view)
        setattr(e, k + "_buf", bufs[k])
    rows = torch.arange(M)
    s = torch.ones(M, 1) if c.scale is None else c.scale[rows // c.rps].view(-1, 1)
    if getattr(c, "x", None) is not None and getattr(c, "w2", None) is not None:          # forward
        b1 = c.b1
        if mutate == "d":        # the second 16 hidden units of every chunk take the first 16's bias
            j = torch.arange(hid)
            b1 = c.b1[j - 16 * ((j // 16) % 2)]
        hp = (c.x.to(BF).float() @ c.w1.float().T + b1).to(BF)
        e.hpre.copy_(hp)
        if mutate == "f" and (hid // 32) % 2 == 1:
            e.hpre[:, hid - 32:] = SENT
        af = (_chunked_matmul(lut_of(lut, hp), c.w2.float()) + c.b2).to(BF)
        e.a2.copy_(af)
        af = af.float()
        mean = af.mean(1)
        var = ((af - mean.view(-1, 1)) ** 2).mean(1)
        rstd = 1.0 / torch.sqrt(var + (0.0 if mutate == "h" else 1e-5))
        e.mean.copy_(mean)
        e.rstd.copy_(rstd)
        sf = s if mutate != "e" else (torch.ones(M, 1) if c.scale is None else c.scale[(rows % 16) // c.rps].view(-1, 1))
        e.y.copy_(c.x + sf * ((af - mean.view(-1, 1)) * rstd.view(-1, 1) * c.gamma + c.beta))
        if mutate == "g":        # rows past M of the last 64-row tile are stored where they fall: behind the tensor
            extra = min(-M % 64, GUARD)
            if extra:
                bufs["a2"][(GUARD + M) * C:(GUARD + M + extra) * C] = e.a2[M - 1].repeat(extra)
        a2, mean, rstd = e.a2, e.mean, e.rstd
    else:
        a2, mean, rstd = c.a2, c.mean, c.rstd
    if getattr(c, "dy", None) is None:
        e.guards = {k: check_guard_rows(bufs[k], GUARD * (1 if k in ("mean", "rstd") else (hid if k in ("hpre", "dh") else C))) for k in bufs}
        return e
    hp = hpre_in if hpre_in is not None else e.hpre
    af = a2.float()
    d = s * c.dy
    xh = (af - mean.view(-1, 1)) * rstd.view(-1, 1)
    gg = d * c.gamma
    da2 = (rstd.view(-1, 1) * (gg - gg.mean(1, keepdim=True) - xh * (gg * xh).mean(1, keepdim=True))).to(BF)
    e.da2.copy_(da2)
    G = da2.float() @ c.w2t.float().T
    gp = lut_of(glut, hp)
    if mutate == "a" and C == 192:      # half table: the sign of the NEIGHBOURING element of the pair selects 1 - g
        b = bits_of(hp)
        j = torch.arange(hid)
        nb = b[:, j ^ 1]
        pos = lut_of(glut, from_bits(b & 0x7FFF))
        gp = torch.where(in_table(hp) & in_table(from_bits(nb)), torch.where((nb & 0x8000) != 0, 1.0 - pos, pos), gp)
    dh = (G * gp).to(BF)
    e.dh.copy_(dh)
    w1t = c.w1t if getattr(c, "w1t_exact", None) is None else c.w1t_exact
    e.dx.copy_(c.dy + _chunked_matmul(dh.float(), w1t.float()))
    e.w1t_used = w1t
    e.dgamma, e.dbeta = c.base_g + (d * xh).sum(0), c.base_b + d.sum(0)
    if mutate == "i" and bwd_mt(C, M) == 2:       # cdiv(M, 64) partial rows folded where cdiv(M, 128) were written: the rest is prefill
        extra = -(-M // 64) - -(-M // 128)
        e.dgamma, e.dbeta = e.dgamma + extra * SENT, e.dbeta + extra * SENT
    e.guards = {k: check_guard_rows(bufs[k], GUARD * (1 if k in ("mean", "rstd") else (hid if k in ("hpre", "dh") else C))) for k in bufs}
    return e


# ---------------------------------------------------------------------------------------------------------------
# helpers of the GPU tests
# ---------------------------------------------------------------------------------------------------------------
GUARD_ROWS = 128                  # guard rows on either side of every output: a whole row tile of the largest kernel


class Guarded:
    """shape[0] rows between GUARD_ROWS guard rows, all prefilled with SENT; .t is the tensor the kernels get"""

    def __init__(self, shape, dtype, dev):
        n = 1
        for s in shape:
            n *= s
        self.g = GUARD_ROWS * (n // shape[0])
        self.buf = torch.full((n + 2 * self.g,), SENT, dtype=dtype, device=dev)
        self.t = self.buf[self.g:self.g + n].view(*shape)

    def intact(self):
        return bool((self.buf[:self.g] == SENT).all() and (self.buf[self.buf.numel() - self.g:] == SENT).all())

    def untouched(self):
        return bool((self.buf == SENT).all())


def library_gelu_lut(ops, L, dev):
    """the library's own bf16(GELU(x)) for all 65 536 bf16 patterns x, as fp32 [65536] indexed by the pattern: the identity
    product  linear(op_bf16(x, gelu=True), I, EPI_F32)  returns the GELU operand exactly (one non-zero term per output).
    Non-finite inputs get a row of their own with zeros elsewhere (0 * inf is NaN in the other columns)."""
    pats = bf16_bits_all(dev)
    bits = torch.arange(65536, device=dev)
    finite = torch.isfinite(pats.float())
    fin_bits, inf_bits = bits[finite], bits[~finite]
    assert fin_bits.numel() == 65280 and inf_bits.numel() == 256
    W = 256
    x = torch.zeros(255 + 256, W, dtype=BF, device=dev)
    x[:255] = pats[fin_bits].view(255, W)
    rows = torch.arange(256, device=dev)
    x[255 + rows, rows] = pats[inf_bits]                        # one non-finite input per row, in column (its index)
    out = torch.empty(x.shape[0], W, dtype=torch.float32, device=dev)
    ops.linear(ops.op_bf16(x, gelu=True), torch.eye(W, dtype=BF, device=dev), ops.epilogue(L.EPI_F32, out, ld=W), W)
    torch.cuda.synchronize()
    lut = torch.empty(65536, dtype=torch.float32, device=dev)
    lut[fin_bits] = out[:255].reshape(-1)
    lut[inf_bits] = out[255 + rows, rows]
    return lut
