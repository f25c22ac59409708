"""fp64 references, derived per-element bounds, host emulations and checkers for the continuous-position-bias kernels of
csrc/cpb.hip, shared by tests/test_cpb_exact_gpu.py (the kernels) and tests/test_cpb_exact_host.py (the references, bounds and
emulations themselves, no GPU).  Plain torch; everything runs on the device its inputs live on.

A case holds nblk blocks (the per-block entry points: nblk = 1, nchunk = 1).  Per block: w1 [Hd][2], b1 [Hd], w2 [heads][Hd],
b2 [heads] fp32; dtab [nchunk][heads][L^2] fp32; a random baseline [3 Hd + heads Hd + heads] = (dw1 | db1 | dw2 | db2) the
gradients are added onto.  Keep data: a bf16 mask [L^2][Hd] (any non-zero = keep) for the per-block kernels, int32 words
[L^2][Hd / 8] for the multi kernels (decode_keep_words: the formula of include/swv2.h).

Reference (fp64, from the fp32 inputs widened; reference()):
  R[p] = sign(delta) log1p(|delta|),  pre = R w1^T + b1,  hidden = relu(pre) keep s,  bias[h][p] = sum_j w2[h][j] hidden[p][j] + b2[h]
  d = sum_chunks dtab,  dh = d^T w2,  g = [pre > 0] keep s dh,  dw1 = g^T R,  db1 = sum_p g,  dw2 = d hidden,  db2 = sum_p d
written out by hand (no autograd): the gate is explicit and closed at pre == 0, as in torch.

Bounds (bounds(); u = 2^-24, first order in u; every constant has its count beside it below).  Which product bound an output carries:
every MFMA output (bias, dw1, db1, dw2 of the multi kernels) carries the WORST-CASE split bound 2^-13 sum |x| |y|, because one operand
of each of the three products is a device intermediate the test cannot read (hidden, the chunk sum d, hidden again).  The sharper bound
from the operands' actual low parts (split_residual()) needs both operands exactly; it is derived here and checked on the host against
the emulation where both operands ARE inputs (dh = d^T w2 at nchunk = 1), where it is 0.02 - 0.3 of the worst case.
  R      |R_dev - R| <= C_LOG1P |R| = 2 ulp: OCML log1p follows the OpenCL accuracy table (2 ulp); the library is built without
         fast-math.  delta -> float, copysign and the (delta != 0) factor are exact; R = 0 exactly on the diagonal.
  pre    P = |w1_0 R_0| + |w1_1 R_1| + |b1|, Pw = P - |b1|:  E_pre = u (2 P + 4 Pw): two fused roundings of sums <= P, and
         C_LOG1P = 4 u on each coordinate term.  Multi kernels: s w1_0, s w1_1, s b1 are rounded first, one rounding on each of the
         three terms of P: u (3 P + 4 Pw), in units of pre (the kernel holds s pre).
  hidden E_h = keep s E_pre + 2 u |hidden| (VALU: fl(1 / (1 - p)) and the product with it) or + 1 u |hidden| (MFMA: fl(s) is a common
         factor of the three scaled constants; relu(x (1 + e)) = (1 + e) relu(x)).  ReLU is 1-Lipschitz: no gate ambiguity forward.
  bias   A = sum_j |w2| |hidden| + |b2|.  VALU: sum_j |w2| E_h + (ceil(Hd / 4) + 4) u A: an fma chain of ceil(Hd / 4) terms per wave,
         three additions of the four LDS partials and one of b2.  MFMA: sum_j |w2| E_h + 2^-13 (A - |b2|) + (35.5 KS + 1) u A with
         KS = Hd / 32 k-steps of three MFMAs: the hi hi product adds 32 terms and the accumulator (33 roundings of <= A), each cross
         product rounds the accumulator once and adds 32 terms 2^-7 as large (2 (1 + 32 2^-7) = 2.5), and b2 is added last (1).
  split  hi = bf16 truncation (|x - hi| < 2^-7 |x|), lo = bf16_rne(x - hi) (|x - hi - lo| <= 2^-15 |x|): xy - (hi hi + lo hi + hi lo)
         = lo_x lo_y + e_x y + (hi_x + lo_x) e_y, at most (2^-14 + 2 2^-15) |xy| = 2^-13 |xy|.
  d      multi: (nchunk - 1) u sum_c |dtab| =: E_d (n terms in any tree pass through <= n - 1 rounded additions; 0 + x is exact)
  g      certain gates: E_g = keep s [pre > 0] (c_dh DH + sum_h E_d |w2|), DH = sum_h |d| |w2|; c_dh = (HEADS_MAX + 2) u for the
         VALU kernel (an fma chain over HEADS_MAX heads, fl(s), the product with it) and 2^-13 + 19.5 u for the MFMA kernel (K = 16:
         17 + 2 (1 + 16 2^-7) = 19.25 roundings, rounded up).  Ambiguous gates (0 < |pre| <= E_pre): the whole term T = keep s |dh| is
         added to the bound of the elements it feeds, not left out.  pre == 0 is not ambiguous: the gate is closed.
  sums   a pair's term passes through  VALU: 128 fmas of its workgroup's chain;  MFMA dw1 / db1: 32 fmas of its lane (four 32-pair
         steps of 8), 2 __shfl_xor levels and 2 roundings of the final * s (36);  MFMA dw2: four steps of 35.5 as in the forward (142);
         db2: a chain of 128 additions;  then the fold (C_FOLD_FIXED + ceil(rows / 8)): <= ceil(rows / 8) additions in a thread,
         2 for (a0 + a1) + (a2 + a3), 3 levels of the LDS tree and 1 onto the baseline, whose own share is 2^-24 |base|.
         Atomics: the rows' partial sums reach the output in any order: max(rows, fold count) additions, and the baseline is rounded
         in each of them (rows u |base|).
  dw1    sum_p (E_g + T) |R| + C_LOG1P sum_p G |R| + C u sum_p G |R| + u |base|,  G = |g| + T;  db1 alike without R
  dw2    sum_p |d| E_h + sum_p E_d |hidden| + [MFMA: 2^-13 sum_p |d| |hidden|] + C u sum_p |d| |hidden| + u |base|
  db2    sum_p E_d + C u sum_p |d| + u |base|
A second backward onto the first result: |out2 - (base + 2 c)| <= 2 bound + 2 u |c| (the same contribution again, one more rounded
addition of a sum of magnitude <= |base| + 2 |c|).
"""
import math
import types

import torch

from tests.proj_ln_reference import assert_within, within  # noqa: F401  (re-exported for the two test files)

BF = torch.bfloat16
F64 = torch.float64
U = 2.0 ** -24
C_LOG1P = 2 * 2.0 ** -23              # 2 ulp of log1pf (OpenCL accuracy table, followed by OCML); ulp(R) <= 2^-23 |R|
C_SPLIT = 2.0 ** -13                  # 2^-14 (lo lo dropped) + 2 * 2^-15 (the two representation terms)
C_MFMA_K32 = 35.5                     # per k-step of three 32-deep MFMAs: 33 + 2 (1 + 32 2^-7)
C_MFMA_K16 = 19.5                     # three 16-deep MFMAs: 17 + 2 (1 + 16 2^-7) = 19.25, rounded up
C_FOLD_FIXED = 6                      # (a0 + a1) + (a2 + a3): 2; LDS tree of 8: 3; onto the baseline: 1
C_VALU_CHAIN = 128                    # CPB_PPB pairs in one thread's fma chain
C_MFMA_LANE = 36                      # 32 fmas + 2 shuffle levels + 2 roundings of * s
C_MFMA_DW2 = 4 * C_MFMA_K32           # four 32-pair steps
PPB = 128                             # CPB_PPB: pairs per backward workgroup (= one partial row)
WORST = {}                            # name -> worst |err| / bound seen so far (printed by the GPU tests)

KEEP_BF16_BITS = (0x3F92, 0x3F80, 0x0001)          # 1.140625, 1.0, the smallest positive bf16: all "keep"

# (wh, ww, heads, hidden, train): per-block kernels.  Train: bf16 keep mask, drop_p 0.125.
BLOCK_CASES = [
    (1, 1, 1, 1, False),      # one pair, one unit, three idle forward waves (jq = 1: waves 1 - 3 have j0 >= Hd)
    (2, 2, 4, 2, True),       # jq = 1: two waves with one unit each; cpb_fwd_kernel<4>, scalar loop with mask
    (2, 2, 4, 32, True),      # fast path, jq = 8: exactly one 8-unit trip per wave (one 16-byte mask load)
    (3, 5, 5, 72, True),      # HEADS_MAX 8 with 5 heads (min(h, heads - 1) rows); Hd % 8 == 0 but jq = 18: scalar path with mask;
                              # L^2 = 225: last forward workgroup of 33 lanes, second backward workgroup of 97 pairs
    (4, 4, 8, 96, True),      # fast path (jq = 24: three trips); L^2 = 256: exact forward and backward workgroups
    (4, 4, 12, 130, True),    # odd hidden with mask (scalar path, jq = 33); 192 backward threads, 62 idle (act = false)
    (2, 9, 17, 64, True),     # smallest HEADS_MAX 32: cpb_fwd_kernel<32> / cpb_bwd_kernel<32> with 15 idle head rows
    (3, 3, 32, 512, True),    # both maxima: all 32 head rows, the 512-thread backward
    (7, 9, 16, 384, False),   # L^2 = 3969: 32 partial rows, the last backward workgroup holds ONE pair; the fold's unrolled loop, no tail
    (9, 18, 8, 384, True),    # production: 206 partial rows = six unrolled trips + a tail of 14 rows
]
# (wh, ww, heads, hidden, train, nchunk, nblk): multi kernels
MULTI_CASES = [
    (1, 1, 1, 64, True, 1, 1),      # one pair; heads 1 (15 zero head rows); JT 1, forward KI 2
    (2, 2, 16, 64, True, 8, 2),     # one 16-pair tile exactly; full head tile (no zero rows); VEC4 with one 8-wide chunk trip
    (3, 5, 3, 128, True, 13, 3),    # L^2 = 225 odd: scalar staging, three 4-wide chunk trips + 1; per-block pointers and bits
    (4, 4, 12, 256, False, 7, 2),   # VEC4, nchunk 7: the tail chunk loop only; no mask
    (2, 9, 5, 512, True, 32, 1),    # JT 8 / KS 16 (full LDS arrays, NIT 32); production chunk count (four 8-wide trips); L^2 = 324: the
                                    # third backward workgroup's last step holds 4 pairs
    (7, 9, 8, 384, True, 4, 2),     # L^2 = 3969 odd: scalar staging with one 4-wide trip exactly; one-pair last workgroup; 16 forward workgroups
    (3, 5, 16, 384, False, 1, 1),   # nchunk 1: a plain d bias table (both operands of dh are inputs)
    (9, 18, 8, 384, True, 32, 2),   # production
]
KEEP_WORD_VARIANTS = ("zero", "all", "top", "onebit")


def case_id(p):
    return "x".join(str(int(v)) for v in p)


def heads_max(heads):
    """the HEADS_MAX instantiation swv2_cpb_fwd / _bwd choose"""
    return 4 if heads <= 4 else 8 if heads <= 8 else 16 if heads <= 16 else 32


# ---------------------------------------------------------------------------------------------------------------
# case builders
# ---------------------------------------------------------------------------------------------------------------
def decode_keep_words(bits, hidden, natural=False):
    """[..., hidden / 8] int32 words -> bool [..., hidden] by the header's formula: unit j <-> bit (j & 7) of W | W >> 8 | W >> 16,
    W = word ((j >> 3) & 3) * (hidden / 32) + (j >> 5); kept iff set.  natural: word j >> 3 instead (the host twin of mutant 3)"""
    w = bits.to(torch.int64) & 0xFFFFFFFF
    dec = (w | (w >> 8) | (w >> 16)) & 0xFF
    j = torch.arange(hidden, device=bits.device)
    widx = (j >> 3) if natural else ((j >> 3) & 3) * (hidden // 32) + (j >> 5)
    return ((dec[..., widx] >> (j & 7)) & 1).bool()


def keep_words(variant, L2, hidden, g):
    nw = hidden // 8
    if variant == "random":
        return torch.randint(0, 2 ** 31 - 1, (L2, nw), generator=g, dtype=torch.int64).to(torch.int32)
    if variant == "zero":
        return torch.zeros(L2, nw, dtype=torch.int32)
    if variant == "all":
        return torch.full((L2, nw), 0x00FFFFFF, dtype=torch.int32)
    if variant == "top":                  # only bits 24 - 31: the top byte is not read, every unit dropped
        return torch.full((L2, nw), 0xFF000000 - 2 ** 32, dtype=torch.int32)
    assert variant == "onebit"            # one bit of byte 0, 1 or 2 per word, cycling through units and pairs
    k = torch.arange(L2).view(-1, 1) + 3 * torch.arange(nw).view(1, -1)
    return (torch.ones_like(k) << (8 * ((k // 8) % 3) + k % 8)).to(torch.int32)


def make_case(geom, kind, variant="random", keep="random", drop_p=0.125, train=None, seed=0):
    """kind 'block' (geom of BLOCK_CASES) or 'multi' (MULTI_CASES); variant 'random' (Part 2) or 'exact' (Part 1: w1 = 0, small
    integers); keep: 'random', one of KEEP_WORD_VARIANTS (multi) or 'values' (block: the three bf16 keep values mixed)"""
    if kind == "block":
        wh, ww, heads, hidden, tr = geom
        nchunk, nblk = 1, 1
    else:
        wh, ww, heads, hidden, tr, nchunk, nblk = geom
    train = tr if train is None else train
    L2 = (wh * ww) ** 2
    g = torch.Generator().manual_seed(1000 * seed + 7 * L2 + 131 * heads + hidden + (kind == "multi"))
    c = types.SimpleNamespace(kind=kind, wh=wh, ww=ww, heads=heads, hidden=hidden, train=bool(train), nchunk=nchunk, nblk=nblk, L2=L2,
                              drop_p=float(drop_p) if train else 0.0, variant=variant, n=3 * hidden + heads * hidden + heads,
                              w1=[], b1=[], w2=[], b2=[], dtab=[], base=[], keep_bf16=None, bits=None)
    c.drop_arg = float(drop_p)            # what the entry points are given (the multi ones insist on 0.125 in eval too)
    c.s = 1.0 / (1.0 - c.drop_p)
    c.rows = -(-L2 // PPB)
    for _ in range(nblk):
        if variant == "exact":
            ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).float()
            w1, b1, w2, b2 = torch.zeros(hidden, 2), ri(-3, 3, hidden), ri(-3, 3, heads, hidden), ri(-3, 3, heads)
            a = 1 if nchunk > 8 else 2
            dtab = ri(-a, a, nchunk, heads, L2)
            base = ri(-64, 64, c.n)
        else:
            us = 10.0 ** (torch.rand(hidden, generator=g) * 3 - 1.5)          # per-unit scale, three decades
            hs = 10.0 ** (torch.rand(heads, generator=g) * 2 - 1.0)           # per-head scale, two decades
            w1 = torch.randn(hidden, 2, generator=g) * 0.7 * us.view(-1, 1)
            b1 = torch.randn(hidden, generator=g) * 0.3 * us
            w2 = torch.randn(heads, hidden, generator=g) * 0.1 * hs.view(-1, 1)
            b2 = torch.randn(heads, generator=g) * 0.1 * hs
            dtab = torch.randn(nchunk, heads, L2, generator=g) * (10.0 ** (torch.rand(heads, generator=g) * 2 - 1.0)).view(1, -1, 1)
            base = torch.randn(c.n, generator=g)
            # pre == 0 exactly: b1 = 0 puts it on the diagonal pairs (R = 0), a zero w1 row with b1 = 0 on every pair of that unit
            if hidden >= 4:
                b1[[0, hidden // 2, hidden - 1]] = 0.0
                w1[hidden - 1] = 0.0
                w1[1] = 0.0                                                   # (b1[1] != 0: pre = b1[1] on every pair)
            elif hidden == 2:
                b1[0] = 0.0
                w1[1] = 0.0
            else:
                w1[0] = 0.0                                                   # one unit (L = 1 here: the only pair is diagonal, pre = b1)
        for lst, t in zip((c.w1, c.b1, c.w2, c.b2, c.dtab, c.base), (w1, b1, w2, b2, dtab, base)):
            lst.append(t.contiguous())
    if train:
        if kind == "block":
            if keep == "values":
                k = (torch.rand(L2, hidden, generator=g) >= drop_p)
                sel = (torch.arange(L2).view(-1, 1) + torch.arange(hidden).view(1, -1)) % 3
                bits = torch.tensor(KEEP_BF16_BITS, dtype=torch.int32)[sel] * k
                c.keep_bf16 = bits.to(torch.int16).view(BF)
            else:
                c.keep_bf16 = (torch.rand(L2, hidden, generator=g) >= drop_p).to(BF) * 1.140625
        else:
            c.bits = torch.stack([keep_words(keep, L2, hidden, g) for _ in range(nblk)])
    return c


def case_to(c, dev):
    d = types.SimpleNamespace(**vars(c))
    for k in ("w1", "b1", "w2", "b2", "dtab", "base"):
        setattr(d, k, [t.to(dev) for t in getattr(c, k)])
    d.keep_bf16 = None if c.keep_bf16 is None else c.keep_bf16.to(dev)
    d.bits = None if c.bits is None else c.bits.to(dev)
    return d


def keep_of(c, b, natural=False):
    """bool [L^2][Hd] or None (eval)"""
    if c.keep_bf16 is not None:
        return c.keep_bf16.view(torch.int16) != 0
    if c.bits is not None:
        return decode_keep_words(c.bits[b], c.hidden, natural)
    return None


def split_grads(v, c):
    """[n] (or [..., n]) -> dict of views dw1 [Hd][2], db1 [Hd], dw2 [heads][Hd], db2 [heads]"""
    Hd, h = c.hidden, c.heads
    return dict(dw1=v[..., :2 * Hd].reshape(*v.shape[:-1], Hd, 2), db1=v[..., 2 * Hd:3 * Hd],
                dw2=v[..., 3 * Hd:3 * Hd + h * Hd].reshape(*v.shape[:-1], h, Hd), db2=v[..., 3 * Hd + h * Hd:])


# ---------------------------------------------------------------------------------------------------------------
# reference and bounds
# ---------------------------------------------------------------------------------------------------------------
def rel_delta(wh, ww, dev):
    """integer (row, column) differences [L^2][2], p = t_q L + t_k, t = r ww + c"""
    t = torch.arange(wh * ww, device=dev)
    r, col = t // ww, t % ww
    return torch.stack([r.view(-1, 1) - r.view(1, -1), col.view(-1, 1) - col.view(1, -1)], -1).reshape(-1, 2)


def coords(wh, ww, dev, dtype=F64):
    d = rel_delta(wh, ww, dev).to(dtype)
    return torch.sign(d) * torch.log1p(d.abs())


def reference(c, b=0):
    dev = c.w1[b].device
    R = coords(c.wh, c.ww, dev)
    w1, b1, w2, b2 = (t.double() for t in (c.w1[b], c.b1[b], c.w2[b], c.b2[b]))
    pre = R @ w1.T + b1
    keep = keep_of(c, b)
    m = torch.full_like(pre, c.s) if keep is None else keep.double() * c.s
    hidden = torch.relu(pre) * m
    bias = (hidden @ w2.T + b2).T.contiguous()
    d = c.dtab[b].double().sum(0)
    dh = d.T @ w2
    g = (pre > 0) * m * dh
    con = torch.cat([(g.T @ R).reshape(-1), g.sum(0), (d @ hidden).reshape(-1), d.sum(1)])
    return types.SimpleNamespace(R=R, pre=pre, m=m, hidden=hidden, bias=bias, d=d, dh=dh, g=g, con=con,
                                 grads=c.base[b].double() + con)


def bounds(c, b, r, form):
    """form 'valu' (swv2_cpb_fwd, swv2_cpb_bwd_ws), 'atomics' (swv2_cpb_bwd) or 'mfma' (the multi kernels) -> namespace with
    bias [heads][L^2], grads [n] (incl. the baseline's share), con [n] (the contribution's own share), amb_share (fraction of the
    dw1 / db1 elements whose ambiguity term exceeds the rest of their bound), n_amb"""
    mfma = form == "mfma"
    Hd, heads = c.hidden, c.heads
    w1, b1, w2, b2 = (t.double().abs() for t in (c.w1[b], c.b1[b], c.w2[b], c.b2[b]))
    aR = r.R.abs()
    Pw = aR @ w1.T
    P = Pw + b1
    Epre = U * ((3 if mfma else 2) * P + 4 * Pw)
    ah = r.hidden.abs()
    Eh = r.m * Epre + (1 if mfma else 2) * U * ah
    A = ah @ w2.T + b2
    if mfma:
        bias = Eh @ w2.T + C_SPLIT * (A - b2) + (C_MFMA_K32 * (Hd // 32) + 1) * U * A
    else:
        bias = Eh @ w2.T + (-(-Hd // 4) + 4) * U * A
    ad = r.d.abs()
    Ed = (c.nchunk - 1) * U * c.dtab[b].double().abs().sum(0)
    DH = ad.T @ w2
    c_dh = (C_SPLIT + C_MFMA_K16 * U) if mfma else (heads_max(heads) + 2) * U
    amb = (r.pre.abs() <= Epre) & (r.pre != 0)
    T = amb * r.m * r.dh.abs()
    Eg = r.m * ((r.pre > 0) | amb) * (c_dh * DH + Ed.T @ w2)
    G = r.g.abs() + T
    fold = -(-c.rows // 8) + C_FOLD_FIXED
    tail = max(c.rows, fold) if form == "atomics" else fold
    c_g = (C_MFMA_LANE if mfma else C_VALU_CHAIN) + tail
    c_w2 = (C_MFMA_DW2 if mfma else C_VALU_CHAIN) + tail
    c_b2 = C_VALU_CHAIN + tail
    rest1 = (Eg.T @ aR) + (C_LOG1P + c_g * U) * (G.T @ aR)
    restb = Eg.sum(0) + c_g * U * G.sum(0)
    amb1, ambb = T.T @ aR, T.sum(0)
    dhid = ad @ ah
    dw2 = ad @ Eh + Ed @ ah + (C_SPLIT if mfma else 0.0) * dhid + c_w2 * U * dhid
    db2 = Ed.sum(1) + c_b2 * U * ad.sum(1)
    con = torch.cat([(rest1 + amb1).reshape(-1), restb + ambb, dw2.reshape(-1), db2])
    # the share of each bound that is the hi + lo representation term itself (MFMA kernels; reported apart as "beyond rounding")
    rep_bias, rep = None, None
    if mfma:
        rg = r.m * ((r.pre > 0) | amb) * (C_SPLIT * DH)
        rep_bias = (C_SPLIT * (A - b2)).T.contiguous()
        rep = torch.cat([(rg.T @ aR).reshape(-1), rg.sum(0), (C_SPLIT * dhid).reshape(-1), torch.zeros_like(db2)])
    nbase = c.rows if form == "atomics" else 1
    a_el = torch.cat([(amb1 > rest1).reshape(-1), ambb > restb])
    return types.SimpleNamespace(bias=bias.T.contiguous(), con=con, grads=con + nbase * U * c.base[b].double().abs(),
                                 amb_share=float(a_el.double().mean()), n_amb=int(amb.sum()), Epre=Epre, rep_bias=rep_bias, rep=rep)


def second_bound(bnd, r):
    """a second backward onto the first result against base + 2 contribution"""
    return 2 * bnd.grads + 2 * U * r.con.abs()


def bf16_split(x):
    """fp32 -> (hi, lo) as fp32: hi the bf16 truncation, lo = bf16_rne(x - hi)"""
    x = x.float().contiguous()
    hi = (x.view(torch.int32) & -65536).view(torch.float32)
    return hi, (x - hi).to(BF).float()


def split_residual(x, y):
    """the representation error of one split product from the operands' ACTUAL low parts, as a bound on
    |x y - (hi hi + lo hi + hi lo)| summed over the inner index: x [M][K], y [K][N] fp32 -> fp64 [M][N]"""
    xh, xl = (t.double() for t in bf16_split(x))
    yh, yl = (t.double() for t in bf16_split(y))
    ex, ey = x.double() - xh - xl, y.double() - yh - yl
    return xl.abs() @ yl.abs() + ex.abs() @ y.double().abs() + (xh + xl).abs() @ ey.abs()


# ---------------------------------------------------------------------------------------------------------------
# host emulations of the kernels' operation order (fp32; `mut` = the host twin of a kernel mutant)
# ---------------------------------------------------------------------------------------------------------------
def fma32(a, b, acc):
    """fmaf: the product of two fp32 is exact in fp64; one rounding to fp32 (the double rounding through fp64 moves a result by
    at most one more part in 2^29 of an ulp-tie: far inside every bound here)"""
    return (a.double() * b.double() + acc.double()).float()


def _scale32(c):
    return float(torch.tensor(1.0, dtype=torch.float32) / (torch.tensor(1.0, dtype=torch.float32) - torch.tensor(c.drop_p, dtype=torch.float32)))


def _coords32(c, dev, mut):
    R = coords(c.wh, c.ww, dev, torch.float32)
    return R[:, [1, 0]].contiguous() if mut == "coord" else R


def mfma_chain(A, B, kstep, drop=None, acc=None):
    """sum_k A[.., m, k] B[.., k, n] as the kernels form it: per k-step hi hi, then lo hi, then hi lo, each added to the fp32
    accumulator.  drop = 'alo': without the lo(A) hi(B) product"""
    Ah, Al = bf16_split(A)
    Bh, Bl = bf16_split(B)
    acc = torch.zeros(*A.shape[:-1], B.shape[-1], dtype=torch.float32, device=A.device) if acc is None else acc
    for k in range(0, A.shape[-1], kstep):
        sa, sb = (Ellipsis, slice(k, k + kstep)), (Ellipsis, slice(k, k + kstep), slice(None))
        acc = acc + Ah[sa] @ Bh[sb]
        if drop != "alo":
            acc = acc + Al[sa] @ Bh[sb]
        acc = acc + Ah[sa] @ Bl[sb]
    return acc


def emu_fwd_valu(c, b=0, mut=None):
    """cpb_fwd_kernel: four waves with ceil(Hd / 4) units each, one fma chain per (pair, head), the LDS sum, b2"""
    dev = c.w1[b].device
    R = _coords32(c, dev, mut)
    w1, b1, w2, b2 = c.w1[b], c.b1[b], c.w2[b], c.b2[b]
    pre = fma32(w1[:, 0].view(1, -1), R[:, 0:1], fma32(w1[:, 1].view(1, -1), R[:, 1:2], b1.view(1, -1)))
    hid = torch.relu(pre)
    keep = keep_of(c, b)
    if keep is not None:
        hid = torch.where(keep, hid * _scale32(c), torch.zeros_like(hid))
    jq = (c.hidden + 3) // 4
    red = []
    for wave in range(4):
        acc = torch.zeros(c.L2, c.heads, device=dev)
        for j in range(wave * jq, min(c.hidden, wave * jq + jq)):
            acc = fma32(w2[:, j].view(1, -1), hid[:, j:j + 1], acc)
        red.append(acc)
    return (red[0] + red[1] + red[2] + red[3] + b2.view(1, -1)).T.contiguous()


def _pre_scaled(c, b, R, s32):
    w1, b1 = c.w1[b], c.b1[b]
    return fma32((w1[:, 0] * s32).view(1, -1), R[:, 0:1], fma32((w1[:, 1] * s32).view(1, -1), R[:, 1:2], (b1 * s32).view(1, -1)))


def emu_fwd_mfma(c, b=0, mut=None):
    """cpb_fwd_mfma_kernel: first layer with the scaled constants, keep bit, KS k-steps of three MFMAs, b2"""
    dev = c.w1[b].device
    R = _coords32(c, dev, mut)
    s32 = _scale32(c) if c.bits is not None else 1.0
    x = torch.relu(_pre_scaled(c, b, R, s32))
    keep = keep_of(c, b, natural=(mut == "widx_fwd"))
    if keep is not None:
        x = x * keep
    acc = mfma_chain(x, c.w2[b].T.contiguous(), 32, drop="alo" if mut == "fwd_alo" else None)
    return (acc + c.b2[b].view(1, -1)).T.contiguous()


def emu_fold(part, base, mut=None):
    """cpb_fold_kernel / cpb_fold_multi_kernel: part [rows][n] fp32 added onto base [n] in the kernels' order"""
    rows = part.shape[0]
    red = []
    for rg in range(8):
        a = [torch.zeros_like(base) for _ in range(4)]
        r = rg
        while r + 24 < rows:
            for q in range(4):
                a[q] = a[q] + part[r + 8 * q]
            r += 32
        while r < rows and mut != "fold_tail":
            a[0] = a[0] + part[r]
            r += 8
        red.append((a[0] + a[1]) + (a[2] + a[3]))
    return base + (((red[0] + red[1]) + (red[2] + red[3])) + ((red[4] + red[5]) + (red[6] + red[7])))


def _padded(t, rows):
    """[L^2, ...] -> [rows][128][...], zeros behind L^2 (pairs past L^2 carry d = 0 in the kernels: no contribution)"""
    out = torch.zeros(rows * PPB, *t.shape[1:], dtype=t.dtype, device=t.device)
    out[:t.shape[0]] = t
    return out.view(rows, PPB, *t.shape[1:])


def emu_bwd_valu(c, b=0, mut=None):
    """cpb_bwd_kernel with a workspace: -> partial rows [rows][n] fp32 (thread = unit, an fma chain over the workgroup's 128 pairs)"""
    dev = c.w1[b].device
    Hd, heads, rows = c.hidden, c.heads, c.rows
    R = _padded(_coords32(c, dev, mut), rows)
    d = _padded(c.dtab[b][0].T.contiguous(), rows)                    # [rows][128][heads]
    keep = keep_of(c, b)
    s32 = _scale32(c)
    m = None if keep is None else _padded(keep.float() * s32, rows)
    w1, b1, w2 = c.w1[b], c.b1[b], c.w2[b]
    z = lambda *s: torch.zeros(*s, device=dev)
    ga, gb, gbias, g2, gb2 = z(rows, Hd), z(rows, Hd), z(rows, Hd), z(rows, heads, Hd), z(rows, heads)
    for pp in range(PPB):
        r0, r1 = R[:, pp, 0:1], R[:, pp, 1:2]
        pre = fma32(w1[:, 0].view(1, -1), r0, fma32(w1[:, 1].view(1, -1), r1, b1.view(1, -1)))
        mm = torch.ones_like(pre) if m is None else m[:, pp]
        hdn = torch.relu(pre) * mm
        g2 = fma32(d[:, pp, :, None], hdn[:, None, :], g2)
        dh = z(rows, Hd)
        for h in range(heads):
            dh = fma32(d[:, pp, h:h + 1], w2[h].view(1, -1), dh)
        gate = (pre >= 0) if mut == "gate" else (pre > 0)
        dh = torch.where(gate, dh * mm, torch.zeros_like(dh))
        ga, gb, gbias = fma32(dh, r0, ga), fma32(dh, r1, gb), gbias + dh
        gb2 = gb2 + d[:, pp]
    return torch.cat([torch.stack([ga, gb], -1).reshape(rows, -1), gbias, g2.reshape(rows, -1), gb2], 1)


def emu_chunk_sum(dtab, L2, mut=None):
    """the staging loops of cpb_bwd_mfma_kernel: [nchunk][heads][L^2] -> [heads][L^2] fp32"""
    n = dtab.shape[0]
    z = torch.zeros_like(dtab[0])
    if L2 % 4 == 0:
        s0, s1, ch = z, z.clone(), 0
        while ch + 7 < n:
            for e in range(0, 8, 2):
                s0 = s0 + dtab[ch + e]
                if not (mut == "chunk7" and e == 6):
                    s1 = s1 + dtab[ch + e + 1]
            ch += 8
        for k in range(ch, n):
            s0 = s0 + dtab[k]
        return s0 + s1
    s, ch = [z, z.clone(), z.clone(), z.clone()], 0
    while ch + 3 < n:
        for q in range(4):
            s[q] = s[q] + dtab[ch + q]
        ch += 4
    for k in range(ch, n):
        s[0] = s[0] + dtab[k]
    return (s[0] + s[1]) + (s[2] + s[3])


def emu_bwd_mfma(c, b=0, mut=None):
    """cpb_bwd_mfma_kernel: -> partial rows [rows][n] fp32"""
    dev = c.w1[b].device
    Hd, heads, rows = c.hidden, c.heads, c.rows
    s32 = _scale32(c) if c.bits is not None else 1.0
    Rf = _coords32(c, dev, mut)
    R = _padded(Rf, rows)
    d = _padded(emu_chunk_sum(c.dtab[b], c.L2, mut).T.contiguous(), rows)           # [rows][128][heads]
    pre = _padded(_pre_scaled(c, b, Rf, s32), rows)
    # (pairs past L^2: the kernel computes pre from a clamped pair, but d = 0 there makes every product with it 0)
    keep = keep_of(c, b)
    kf = torch.ones(rows, PPB, Hd, device=dev) if keep is None else _padded(keep.float(), rows)
    if mut == "keep_bwd" and keep is not None:          # second 16-pair tile of a step reads bit e instead of bit 12 + e
        q = torch.arange(PPB, device=dev)
        kf = kf[:, torch.where((q % 32) >= 16, (q // 32) * 32 + (q % 16) + 4, q)]
    dh = mfma_chain(d, c.w2[b], 16)                      # K = the 16 head rows (rows >= heads are zero)
    hdn = torch.relu(pre) * kf
    gate = (pre >= 0) if mut == "gate" else (pre > 0)
    dm = torch.where(gate, dh, torch.zeros_like(dh)) * kf
    # the lane's 32 pairs in issue order: steps st, then e = 0 .. 7 (pairs 32 st + 4 g + e, 32 st + 16 + 4 g + e - 4)
    order = torch.tensor([[32 * st + (4 * g + e if e < 4 else 16 + 4 * g + e - 4) for st in range(4) for e in range(8)] for g in range(4)], device=dev)
    z = lambda: torch.zeros(rows, 4, Hd, device=dev)
    ga, gb, gs = z(), z(), z()
    for k in range(32):
        p = order[:, k]
        dmk = dm[:, p]
        ga, gb, gs = fma32(dmk, R[:, p, 0:1], ga), fma32(dmk, R[:, p, 1:2], gb), gs + dmk
    tree = lambda t: (t[:, 0] + t[:, 1]) + (t[:, 2] + t[:, 3])
    ga, gb, gs = tree(ga) * s32, tree(gb) * s32, tree(gs) * (1.0 if mut == "db1_scale" else s32)
    g2 = torch.zeros(rows, heads, Hd, device=dev)
    dT = d.transpose(1, 2).contiguous()                                             # [rows][heads][128]
    g2 = mfma_chain(dT, hdn, 32, drop="alo" if mut == "bwd_adl" else None, acc=g2)
    gb2 = torch.zeros(rows, heads, device=dev)
    for pp in range(PPB):
        gb2 = gb2 + d[:, pp]
    return torch.cat([torch.stack([ga, gb], -1).reshape(rows, -1), gs, g2.reshape(rows, -1), gb2], 1)


# ---------------------------------------------------------------------------------------------------------------
# checkers
# ---------------------------------------------------------------------------------------------------------------
def check_bias(name, got, r, bnd, what="", exact=False):
    """bias [heads][L^2] finite and within its bound everywhere (exact: equal to fp64)"""
    assert bool(torch.isfinite(got).all()), f"{name} {what}: bias holds a non-finite value (an element the kernel did not write)"
    if exact:
        assert torch.equal(got.double(), r.bias), f"{name} {what}: bias differs from fp64 on an integer case"
    return assert_within(name + " bias", got, r.bias, bnd.bias, what, rnd=bnd.rep_bias, worst=WORST)


def check_grads(name, got, c, r, bnd, what="", exact=False, second=False):
    """the four gradients [n] against base + contribution (second: base + 2 contribution) within their bounds; exact: db1, dw2, db2
    equal to fp64 (dw1 keeps its bound: R is irrational)"""
    assert bool(torch.isfinite(got).all()), f"{name} {what}: a gradient is not finite (a partial-row entry read before it was written)"
    ref = r.grads + r.con if second else r.grads
    bound = second_bound(bnd, r) if second else bnd.grads
    gv, rv, bv = split_grads(got, c), split_grads(ref, c), split_grads(bound, c)
    pv = None if bnd.rep is None else split_grads((2 if second else 1) * bnd.rep, c)
    out = {}
    for k in ("dw1", "db1", "dw2", "db2"):
        if exact and k != "dw1":
            assert torch.equal(gv[k].double(), rv[k]), f"{name} {what}: {k} differs from fp64 on an integer case"
        out[k] = assert_within(f"{name} {k}" + (" x2" if second else ""), gv[k], rv[k], bv[k], what, rnd=None if pv is None or k == "db2" else pv[k], worst=WORST)
    return out
