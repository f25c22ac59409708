"""GPU (-m gpu): the fused MLP pair (swv2_mlp_fwd / swv2_mlp_bwd, csrc/mlp.hip) and the unfused fc1 / dh epilogues
(EPI_BF16_GELU, EPI_GELU_GRAD of swv2_linear), element by element against fp64.

The references, the bounds and their derivations are in tests/mlp_reference.py (checked without a GPU by
tests/test_mlp_exact_host.py, which also holds the host twins of the kernel mutants).  Every case checks every element of every
output, the guard rows around every output (still the sentinel) and bit-for-bit equality of a second run, dgamma / dbeta and the
workspace included.  Every output is judged against the kernel's own saved upstream tensor.

  random cases   log-uniform operands, rows_per_sample = 100, drop-path factors cycling through 0, 1.25, 1, dgamma / dbeta onto a
                 non-zero baseline: every C x every hidden class, M in 1, 13, 64, 77, 176; MT = 2 at M = 32 848 (C 32, 96, 128) with
                 257 partial rows folded; <192, 2> forward at hidden 1056; recompute mode wherever hidden <= 1024, under the same
                 checkers and bit-identical to the saved-hpre mode; scale = NULL once per C
  exact cases    operands for which no rounding can occur: hpre, a2, dh, dx bit for bit, one case per C and one at MT = 2
  GELU sweep     forward: hidden = C, w1 = w2 = I, x = every finite bf16 pattern in 16 x 16 tiles (table only / formula only /
                 mixed, see mlp_reference.sweep_bits): hpre == x, a2 == the library's bf16(GELU) table bit for bit, and within the
                 fp64 bar of test_gelu_operand_on_every_bf16_input
  GELU' sweep    backward: hpre = the patterns, w2t[j][j % C] = 1, so G is the kernel's own da2 element: dh against
                 G * GELU'_64(hpre) at the full table (C 128), the half table with 1 - g (C 192), the formula (C 256), MT = 2 (C 32)
                 and in recompute mode (C 128, C 192); every pattern must meet a |da2| >= 2^-4
  unfused        fc1 with EPI_BF16_GELU and dh with EPI_GELU_GRAD under the same checkers on TILE128, WIDE and WIDE_DMA (asked of
                 swv2_linear_kernel before each launch), both sweeps through these epilogues
  refusals       unsupported shapes and missing operands return non-zero and write nothing

Worst |err| / bound measured on an MI355X over every case of this file (the bounds are derived; none is fitted to these).
"beyond" is (|err| - rounding term) / (bound - rounding term): the bf16 outputs reach the 2^-8 |ref| of their bound by construction,
dgamma / dbeta the 2^-24 |baseline| where a column's sum is small against the baseline (M = 1, 13).  mt1 / mt2: C <= 128 at one /
two row tiles per wave; c192: <192, 1> / <192, 2> forward, half GELU' table; c256: GELU' by formula.
          hpre   beyond   a2     beyond   mean    rstd    y      da2    beyond   dh     beyond  dx     dgamma beyond  dbeta  beyond
  mt1     0.993  0.0056   0.989  0.0007   0.0039  0.013   0.151  0.987  0.0002   0.994  0.027   0.125  0.387  0.065   0.054  0.042
  mt2     0.994  0.0052   0.993  0.0030   0.0105  0.020   0.182  0.993  0.0023   0.994  0.095   0.074  0.0025 0.0025  0.0014 0.0014
  c192    0.983  0.0014   0.988  0.00003  0.0011  0.0034  0.174  0.971  0.0003   0.985  0.091   0.099  0.373  0.049   0.403  0.040
  c256    0.984  0.0002   0.983  0.0001   0.0002  0.0027  0.181  0.976  0        0.980  0.011   0.047  0.063  0.063   0.050  0.049
  unfused 0.982  0.0008                                                          0.979  0.042
Recompute mode: the same bits.  dx reaches 0.493 only in the recompute-mode GELU' sweeps, where w1 = I makes dx = dy + dh a single fp32
addition (2^-24 of the result against 2^-23 |dy|: 0.5 by construction).  Forward GELU against its fp64 bar: 0.648 (one table, one worst
input).  What dh's error leaves of B' |G| once its own rounding and G's accumulation are taken off, as a share of B': table 0.015,
formula 0.014, half table with 1 - g 0.093, recompute 0.095, epilogues 0.015.  Mutants and the rechecked ratios: LABNOTES.md ("The fused
MLP pair element by element").
"""
import ctypes

import pytest
import torch

from tests import mlp_reference as R

pytestmark = pytest.mark.gpu

BF = R.BF
Guarded = R.Guarded


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def K():
    from swin_v2_weather_amd import _lib as L, ops
    L.load()
    yield dict(L=L, ops=ops)
    # (shown with -s) the worst |err| / bound of every output over the cases that ran
    print("\n[mlp worst |err| / bound] " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(R.WORST.items())))
    print("[mlp worst GELU' error left after rounding and accumulation / B'] " + ", ".join(f"{k} {v / R.gelu_grad_bar():.3g}" for k, v in sorted(GRAD_ERR.items())))


@pytest.fixture(scope="module")
def gelu_lut(dev, K):
    return R.library_gelu_lut(K["ops"], K["L"], dev)


GRAD_ERR = {}            # family -> worst estimate of the fp32 GELU's absolute error (mlp_reference.gelu_grad_ratio)


def family(c):
    """the instantiation family a case's figures are filed under: C <= 128 at one / two row tiles per wave, C 192 (half GELU' table;
    <192, 2> forward past hidden 1024), C 256 (GELU' by formula)"""
    if c.C == 192:
        return "c192"
    if c.C == 256:
        return "c256"
    return "mt2" if c.M >= 128 * 256 else "mt1"


def _guards(outs, what):
    bad = [k for k, v in outs.items() if isinstance(v, Guarded) and not v.intact()]
    assert not bad, f"{what}: guard rows written around {bad}"


def _report(tag, what, ratios):
    print(f"\n[mlp {tag}] {what}: " + ", ".join(f"{k} {v:.3g}" for k, v in ratios.items()))


def _first_bad(got, ref, n=4):
    bad = (got.double() != ref.double()).nonzero()
    return int(bad.shape[0]), [(tuple(int(v) for v in ix), float(got[tuple(ix)]), float(ref[tuple(ix)])) for ix in bad[:n]]


def forward(K, c, dev, keep=True):
    o = dict(y=Guarded((c.M, c.C), torch.float32, dev), hpre=Guarded((c.M, c.hid), BF, dev) if keep else None,
             a2=Guarded((c.M, c.C), BF, dev), mean=Guarded((c.M,), torch.float32, dev), rstd=Guarded((c.M,), torch.float32, dev))
    K["ops"].mlp_fwd(c.x, c.w1, c.b1, c.w2, c.b2, c.gamma, c.beta, c.scale, c.rps,
                     out=(o["y"].t, o["hpre"].t if keep else None, o["a2"].t, o["mean"].t, o["rstd"].t))
    torch.cuda.synchronize()
    _guards(o, "swv2_mlp_fwd")
    return o


def backward(K, c, dev, a2, mean, rstd, hpre, w1t=None):
    """hpre = None: recompute mode (x, w1, b1 of the case)"""
    lib = K["L"].load()
    nws = lib.swv2_mlp_bwd_ws_floats(c.M, c.C)
    assert nws == -(-c.M // 64) * 2 * c.C
    o = dict(dx=Guarded((c.M, c.C), torch.float32, dev), da2=Guarded((c.M, c.C), BF, dev), dh=Guarded((c.M, c.hid), BF, dev),
             ws=Guarded((nws // (2 * c.C), 2 * c.C), torch.float32, dev), dgamma=c.base_g.clone(), dbeta=c.base_b.clone())
    rec = dict(x=c.x, w1=c.w1, b1=c.b1) if hpre is None else {}
    K["ops"].mlp_bwd(c.dy, a2, mean, rstd, c.gamma, c.scale, hpre, c.w2t, None if hpre is None else (c.w1t if w1t is None else w1t),
                     o["dgamma"], o["dbeta"], c.rps, out=(o["dx"].t, o["da2"].t, o["dh"].t), ws=o["ws"].t, **rec)
    torch.cuda.synchronize()
    _guards(o, "swv2_mlp_bwd")
    return o


def _same(a, b, keys, what):
    for k in keys:
        x, y = (a[k].buf, b[k].buf) if isinstance(a[k], Guarded) else (a[k], b[k])
        assert torch.equal(x, y), (what, "differs in", k, _first_bad(x, y))


def _grad_err(fam, da2, w2t, hpre, dh):
    GRAD_ERR[fam] = max(GRAD_ERR.get(fam, 0.0), R.gelu_grad_ratio(da2, w2t, hpre, dh))


# ---------------------------------------------------------------------------------------------------------------
# random operands, per-element bounds
# ---------------------------------------------------------------------------------------------------------------
def _random_case(K, dev, lut, geo, with_scale=True, baseline=True):
    c = R.case_to(R.make_case(*geo, with_scale=with_scale, baseline=baseline, seed=12), dev)
    fam = family(c)
    what = R.case_id(geo) + ("" if with_scale else " no scale")
    Bp = R.gelu_grad_bar()
    f = forward(K, c, dev)
    r = R.check_all_forward(fam, c, lut, f["hpre"].t, f["a2"].t, f["mean"].t, f["rstd"].t, f["y"].t, what)
    b = backward(K, c, dev, f["a2"].t, f["mean"].t, f["rstd"].t, f["hpre"].t)
    r.update(R.check_all_backward(fam, c, f["a2"].t, f["mean"].t, f["rstd"].t, f["hpre"].t, b["da2"].t, b["dh"].t, b["dx"].t, b["dgamma"],
                                  b["dbeta"], Bp, what))
    _grad_err(fam, b["da2"].t, c.w2t, f["hpre"].t, b["dh"].t)
    _report(fam, what, r)
    if c.scale is not None and c.M > c.rps:              # a dropped sample keeps y == x exactly
        drop = c.scale[torch.arange(c.M, device=dev) // c.rps] == 0
        assert int(drop.sum()) > 0 and torch.equal(f["y"].t[drop], c.x[drop]), (what, "y of dropped samples")
    # a second run agrees bit for bit, guards and workspace included
    f2 = forward(K, c, dev)
    b2 = backward(K, c, dev, f2["a2"].t, f2["mean"].t, f2["rstd"].t, f2["hpre"].t)
    _same(f2, f, ("y", "hpre", "a2", "mean", "rstd"), what + " second forward")
    _same(b2, b, ("dx", "da2", "dh", "ws", "dgamma", "dbeta"), what + " second backward")
    # recompute mode: under the same checkers against fp64 (the pre-activation it never stores is the one its twin saved), and
    # bit-identical to the saved-hpre mode
    if c.hid <= R.RECOMP_MAX_HIDDEN:
        assert K["L"].load().swv2_mlp_recompute_supported(c.C, c.hid) == 1
        fr = forward(K, c, dev, keep=False)
        rr = R.check_all_forward("recomp", c, lut, None, fr["a2"].t, fr["mean"].t, fr["rstd"].t, fr["y"].t, what, hpre_for_a2=f["hpre"].t)
        br = backward(K, c, dev, fr["a2"].t, fr["mean"].t, fr["rstd"].t, None)
        rr.update(R.check_all_backward("recomp", c, fr["a2"].t, fr["mean"].t, fr["rstd"].t, f["hpre"].t, br["da2"].t, br["dh"].t, br["dx"].t,
                                       br["dgamma"], br["dbeta"], Bp, what))
        _grad_err("recomp", br["da2"].t, c.w2t, f["hpre"].t, br["dh"].t)
        _report("recomp", what, rr)
        _same(fr, f, ("y", "a2", "mean", "rstd"), what + " recompute forward")
        _same(br, b, ("dx", "da2", "dh", "ws", "dgamma", "dbeta"), what + " recompute backward")
    else:
        assert K["L"].load().swv2_mlp_recompute_supported(c.C, c.hid) == 0


@pytest.mark.parametrize("geo", R.CASES, ids=R.case_id)
def test_random_per_element(dev, K, gelu_lut, geo):
    _random_case(K, dev, gelu_lut, geo)


@pytest.mark.parametrize("geo", R.BIG_CASES, ids=R.case_id)
def test_random_per_element_two_row_tiles(dev, K, gelu_lut, geo):
    """M = 32 848: the MT = 2 instantiations, 257 workgroups, the last with 80 rows; the backward folds cdiv(M, 128) partial rows"""
    assert geo[2] >= 128 * 256 and -(-geo[2] // 128) == 257
    _random_case(K, dev, gelu_lut, geo)


@pytest.mark.parametrize("geo", R.NO_SCALE_CASES, ids=R.case_id)
def test_random_per_element_without_scale(dev, K, gelu_lut, geo):
    """scale = NULL, dgamma / dbeta onto zeros"""
    _random_case(K, dev, gelu_lut, geo, with_scale=False, baseline=False)


# ---------------------------------------------------------------------------------------------------------------
# exact operands, bit for bit
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geo", R.EXACT_CASES, ids=R.case_id)
def test_exact_bit_for_bit(dev, K, gelu_lut, geo):
    """operands for which no rounding can occur (mlp_reference.make_case, "exact"): hpre and a2 equal fp64 on every element, dh is
    +-(the kernel's own da2 element its w2 column names) where the pre-activation is positive and 0 where it is -20, dx is the fp32
    sum of dy and the one dh element its w1t row names; the rest within the random cases' bounds"""
    c = R.case_to(R.make_case(*geo, mode="exact", seed=11), dev)
    what = R.case_id(geo)
    f = forward(K, c, dev)
    v, _ = R.ref_hpre(c.x, c.w1, c.b1)
    assert torch.equal(f["hpre"].t.double(), v), (what, "hpre", _first_bad(f["hpre"].t, v))
    v2, _ = R.ref_a2(f["hpre"].t, gelu_lut, c.w2, c.b2)
    assert float(v2.abs().max()) <= 136
    assert torch.equal(f["a2"].t.double(), v2), (what, "a2", _first_bad(f["a2"].t, v2))
    r = R.check_ln("exact", c, f["a2"].t, f["mean"].t, f["rstd"].t, f["y"].t, what)
    b = backward(K, c, dev, f["a2"].t, f["mean"].t, f["rstd"].t, f["hpre"].t, w1t=c.w1t_exact)
    r.update(R.check_ln_backward("exact", c, f["a2"].t, f["mean"].t, f["rstd"].t, b["da2"].t, b["dgamma"], b["dbeta"], what))
    _report("exact", what, r)
    G = R.ref_dh(b["da2"].t, c.w2t, f["hpre"].t, 0.0)[2]
    want = G * (v > 0)
    assert torch.equal(b["dh"].t.double(), want), (what, "dh", _first_bad(b["dh"].t, want))
    dxr = (c.dy.double() + b["dh"].t.double() @ c.w1t_exact.double().T).float()
    assert torch.equal(b["dx"].t, dxr), (what, "dx", _first_bad(b["dx"].t, dxr))
    f2 = forward(K, c, dev)
    b2 = backward(K, c, dev, f2["a2"].t, f2["mean"].t, f2["rstd"].t, f2["hpre"].t, w1t=c.w1t_exact)
    _same(f2, f, ("y", "hpre", "a2", "mean", "rstd"), what + " second forward")
    _same(b2, b, ("dx", "da2", "dh", "ws", "dgamma", "dbeta"), what + " second backward")
    if c.hid <= R.RECOMP_MAX_HIDDEN:
        fr = forward(K, c, dev, keep=False)
        _same(fr, f, ("y", "a2", "mean", "rstd"), what + " recompute forward")


# ---------------------------------------------------------------------------------------------------------------
# the forward's GELU on every finite bf16 input
# ---------------------------------------------------------------------------------------------------------------
def _judge_gelu(what, bits, hpre, act, lut, dev):
    """hpre [rows][n] against the patterns, act [rows][n] against the library's table and the fp64 bar"""
    ok = R.hpre_matches(hpre, bits)
    assert bool(ok.all()), (what, "hpre is not the pattern", int((~ok).sum()), [hex(int(v)) for v in bits[~ok][:4]])
    got = R.bits_of(hpre)
    sub = ((bits & 0x7F80) == 0) & ((bits & 0x7F) != 0)
    flushed = int((sub & (got != bits)).sum())
    assert torch.equal(act.float(), R.lut_of(lut, hpre)), (what, "GELU is not the library's table", _first_bad(act.float(), R.lut_of(lut, hpre)))
    ref, bound = R.ref_gelu(hpre.float())
    R.assert_within("gelu " + what, act, ref, bound, what)
    cls = R.sweep_tiles(got)
    print(f"\n[mlp gelu sweep] {what}: {int(sub.sum())} subnormal inputs, {flushed} stored as a signed zero; tiles by path: table "
          f"{int((cls == 0).sum())}, formula {int((cls == 1).sum())}, mixed {int((cls == 2).sum())}")
    assert int((cls == 0).sum()) >= 18 and int((cls == 2).sum()) >= 1
    present = torch.zeros(65536, dtype=torch.bool, device=dev)
    present[bits.reshape(-1)] = True
    assert bool(present[R.finite_patterns(dev)].all())


FWD_SWEEPS = [(C, R.fwd_sweep_rows(C), None) for C in R.CS] + [(32, 32768, None), (192, R.fwd_sweep_rows(192), 1056)]


@pytest.mark.parametrize("C,rows,hid", FWD_SWEEPS, ids=lambda v: str(v))
def test_forward_gelu_on_every_finite_bf16_input(dev, K, gelu_lut, C, rows, hid):
    """w1 = w2 = I: hpre must be x and a2 the library's bf16(GELU(x)), on the table path, the formula path and in mixed tiles.  y is
    not judged (its rows hold huge values); its guard rows are."""
    c = R.case_to(R.make_fwd_sweep(C, rows, hid), dev)
    f = forward(K, c, dev)
    bits = c.bits[:, torch.arange(c.hid, device=dev) % C]
    ok = R.hpre_matches(f["hpre"].t, bits)
    assert bool(ok.all()), ("hpre is not the pattern", int((~ok).sum()))
    _judge_gelu(f"C{C} rows {rows} hidden {c.hid}", c.bits, f["hpre"].t[:, :C], f["a2"].t, gelu_lut, dev)
    f2 = forward(K, c, dev)
    _same(f2, f, ("hpre", "a2"), "second forward")


# ---------------------------------------------------------------------------------------------------------------
# the backward's GELU' on every finite bf16 input
# ---------------------------------------------------------------------------------------------------------------
def _coverage(what, bits, G, dev):
    ok = R.sweep_coverage(bits, G)
    fin = R.finite_patterns(dev)
    assert bool(ok[fin].all()), (what, "patterns that met no |da2| >= 2^-4", int((~ok[fin]).sum()))


BWD_SWEEPS = [(128, 128, 2048, False, "mt1"), (192, 128, 2048, False, "c192"), (256, 128, 2048, False, "c256"), (32, 32768, 64, False, "mt2"),
              (128, 4096, 128, True, "recomp"), (192, 4096, 192, True, "recomp")]


@pytest.mark.parametrize("C,M,hid,recompute,fam", BWD_SWEEPS, ids=lambda v: str(v))
def test_backward_gelu_grad_on_every_finite_bf16_input(dev, K, C, M, hid, recompute, fam):
    """hpre = every finite pattern (table-only, formula-only and mixed 16 x 16 tiles), w2t[j][j % C] = 1: G is the kernel's own da2
    element exactly and dh = G * GELU'(hpre) is held to  2^-8 |ref| + C 2^-23 |G| |GELU'| + B' |G|  on every element; every finite
    pattern must meet a |da2| >= 2^-4.  C 128: the full table, C 192: the positive half with 1 - g, C 256: the formula."""
    c = R.case_to(R.make_bwd_sweep(C, M, hid, recompute), dev)
    what = f"C{C} M{M} hidden {hid}" + (" recompute" if recompute else "")
    b = backward(K, c, dev, c.a2, c.mean, c.rstd, None if recompute else c.hpre)
    G = R.ref_dh(b["da2"].t, c.w2t, c.hpre, 0.0)[2]
    assert torch.equal(G, b["da2"].t.double()[:, torch.arange(hid, device=dev) % C])
    _coverage(what, c.bits, G, dev)
    r = R.check_ln_backward(fam, c, c.a2, c.mean, c.rstd, b["da2"].t, b["dgamma"], b["dbeta"], what)
    r.update(R.check_dh("gelu' " + fam, b["da2"].t, c.w2t, c.hpre, b["dh"].t, R.gelu_grad_bar(), what))
    r.update(R.check_dx(fam, c.dy, b["dh"].t, c.w1t, b["dx"].t, what))
    _grad_err("sweep " + fam, b["da2"].t, c.w2t, c.hpre, b["dh"].t)
    r["GELU' error / B'"] = R.gelu_grad_ratio(b["da2"].t, c.w2t, c.hpre, b["dh"].t) / R.gelu_grad_bar()
    _report("gelu' sweep", what, r)
    b2 = backward(K, c, dev, c.a2, c.mean, c.rstd, None if recompute else c.hpre)
    _same(b2, b, ("dx", "da2", "dh", "ws", "dgamma", "dbeta"), what + " second backward")


# ---------------------------------------------------------------------------------------------------------------
# the unfused sequence (blocks with C >= 512 never take the fused kernels) under the same checkers
# ---------------------------------------------------------------------------------------------------------------
def _linear(K, a, w, e, N, kernel):
    L = K["L"]
    got = L.load().swv2_linear_kernel(ctypes.byref(a), ctypes.byref(e), N)
    assert got == getattr(L, "LINEAR_" + kernel), (kernel, got)
    K["ops"].linear(a, w, e, N)


def _fc1(K, dev, x, w1, b1, kernel):
    ops, L = K["ops"], K["L"]
    M, hid = x.shape[0], w1.shape[0]
    o = dict(pre=Guarded((M, hid), BF, dev), act=Guarded((M, hid), BF, dev))
    _linear(K, ops.op_f32(x), w1, ops.epilogue(L.EPI_BF16_GELU, o["pre"].t, ld=hid, bias=b1, aux_out=o["act"].t), hid, kernel)
    torch.cuda.synchronize()
    _guards(o, "swv2_linear EPI_BF16_GELU " + kernel)
    return o


def _dh(K, dev, da2, w2t, hpre, kernel):
    ops, L = K["ops"], K["L"]
    M, hid = da2.shape[0], w2t.shape[0]
    o = dict(dh=Guarded((M, hid), BF, dev))
    _linear(K, ops.op_bf16(da2), w2t, ops.epilogue(L.EPI_GELU_GRAD, o["dh"].t, ld=hid, aux=hpre), hid, kernel)
    torch.cuda.synchronize()
    _guards(o, "swv2_linear EPI_GELU_GRAD " + kernel)
    return o


@pytest.mark.parametrize("C,hid,M,k1,k2", [(128, 512, 176, "TILE128", "TILE128"), (512, 512, 4096 + 48, "WIDE", "WIDE_DMA")])
def test_unfused_fc1_and_dh_per_element(dev, K, gelu_lut, C, hid, M, k1, k2):
    """fc1 with EPI_BF16_GELU (hpre per element, the activation == the library's table of the stored hpre bit for bit) and dh with
    EPI_GELU_GRAD (from a bf16 da2), on the kernel the case names"""
    c = R.case_to(R.make_case(C, hid, M, seed=13) if C <= 256 else _wide_case(C, hid, M), dev)
    what = f"{R.case_id((C, hid, M))} {k1} / {k2}"
    o = _fc1(K, dev, c.x, c.w1, c.b1, k1)
    r = R.check_fc1("unfused", c, o["pre"].t, what)
    want = R.lut_of(gelu_lut, o["pre"].t)
    assert torch.equal(o["act"].t.float(), want), (what, "activation", _first_bad(o["act"].t.float(), want))
    g = torch.Generator().manual_seed(C + M)
    da2 = R.signed_log_uniform(M * C, 1e-3, 4.0, g).view(M, C).to(BF).to(dev)
    d = _dh(K, dev, da2, c.w2t, o["pre"].t, k2)
    r.update(R.check_dh("unfused", da2, c.w2t, o["pre"].t, d["dh"].t, R.gelu_grad_bar(), what))
    _grad_err("unfused", da2, c.w2t, o["pre"].t, d["dh"].t)
    _report("unfused", what, r)
    o2, d2 = _fc1(K, dev, c.x, c.w1, c.b1, k1), _dh(K, dev, da2, c.w2t, o["pre"].t, k2)
    _same(o2, o, ("pre", "act"), what + " second fc1")
    _same(d2, d, ("dh",), what + " second dh")


def _wide_case(C, hid, M):
    """operands as make_case's for widths the fused kernels do not take (only what fc1 and dh read)"""
    g = torch.Generator().manual_seed(7919 * C + 131 * hid + M)
    c = R.types.SimpleNamespace(C=C, hid=hid, M=M)
    c.x = R.signed_log_uniform(M * C, 4e-3, 4.0, g).view(M, C)
    c.w1 = (R.signed_log_uniform(hid * C, 2e-3, 2.0, g).view(hid, C) * (2.0 / C ** 0.5)).to(BF)
    c.b1 = R.signed_log_uniform(hid, 1e-3, 1.0, g)
    c.w2t = (R.signed_log_uniform(hid * C, 2e-3, 2.0, g).view(hid, C) * (2.0 / hid ** 0.5)).to(BF)
    return c


@pytest.mark.parametrize("C,rows,k1,k2", [(256, 256, "TILE128", "TILE128"), (512, 4096, "WIDE", "WIDE_DMA")])
def test_unfused_epilogues_on_every_finite_bf16_input(dev, K, gelu_lut, C, rows, k1, k2):
    """both sweeps through the epilogues: fc1 of the patterns by the identity, dh = da2 * GELU'(patterns) by the identity"""
    g = torch.Generator().manual_seed(C + rows)
    bits = R.sweep_bits(rows, C, g).to(dev)
    pat = R.from_bits(bits)
    eye = torch.eye(C, dtype=BF, device=dev)
    what = f"unfused C{C} rows {rows} {k1} / {k2}"
    o = _fc1(K, dev, pat.float(), eye, torch.zeros(C, device=dev), k1)
    _judge_gelu(what, bits, o["pre"].t, o["act"].t, gelu_lut, dev)
    da2 = R.signed_log_uniform(rows * C, 0.25, 4.0, g).view(rows, C).to(BF).to(dev)
    d = _dh(K, dev, da2, eye, pat, k2)
    _coverage(what, bits, da2.double(), dev)
    r = R.check_dh("gelu' unfused", da2, eye, pat, d["dh"].t, R.gelu_grad_bar(), what)
    _grad_err("sweep unfused", da2, eye, pat, d["dh"].t)
    r["GELU' error / B'"] = R.gelu_grad_ratio(da2, eye, pat, d["dh"].t) / R.gelu_grad_bar()
    _report("gelu' sweep", what, r)
    o2, d2 = _fc1(K, dev, pat.float(), eye, torch.zeros(C, device=dev), k1), _dh(K, dev, da2, eye, pat, k2)
    _same(o2, o, ("pre", "act"), what + " second fc1")
    _same(d2, d, ("dh",), what + " second dh")


# ---------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------
REFUSALS = ["hidden % 32", "hidden > 2048", "unsupported C", "no hpre at hidden 1056", "neither operand set", "M = 0", "rows_per_sample = 0"]


@pytest.mark.parametrize("how", REFUSALS)
def test_refusals_write_nothing(dev, K, how):
    """swv2_mlp_fwd / swv2_mlp_bwd return non-zero and leave every output, the workspace and dgamma / dbeta as they were"""
    L = K["L"]
    lib = L.load()
    M, Cc, hid, rps = 64, 128, 128, R.RPS
    if how == "hidden % 32":
        hid = 48
    elif how == "hidden > 2048":
        hid = 2080
    elif how == "unsupported C":
        Cc = 160
    elif how == "no hpre at hidden 1056":
        hid = 1056
    g = torch.Generator().manual_seed(len(how))
    rnd = lambda *s: torch.randn(*s, generator=g).to(dev)          # noqa: E731
    # (inputs sized for the largest shape named, so that a launch that is wrongly accepted still reads inside them)
    x, w1, w2, b1, vec = rnd(M, 256), rnd(2112, 256).to(BF), rnd(256, 2112).to(BF), rnd(2112), rnd(256)
    hpre_in, a2_in, stat = rnd(M, 2112).to(BF), rnd(M, 256).to(BF), rnd(M).abs() + 0.5
    scale = torch.ones(1, device=dev)
    outs = dict(y=Guarded((M, 256), torch.float32, dev), hpre=Guarded((M, 2112), BF, dev), a2=Guarded((M, 256), BF, dev),
                mean=Guarded((M,), torch.float32, dev), rstd=Guarded((M,), torch.float32, dev), dx=Guarded((M, 256), torch.float32, dev),
                da2=Guarded((M, 256), BF, dev), dh=Guarded((M, 2112), BF, dev), ws=Guarded((4, 512), torch.float32, dev))
    dg, db = torch.full((256,), 3.0, device=dev), torch.full((256,), -2.0, device=dev)
    a = L.MlpArgs()
    a.x, a.w1, a.b1, a.w2, a.b2, a.gamma, a.beta, a.scale = (t.data_ptr() for t in (x, w1, b1, w2, vec, vec, vec, scale))
    a.hpre, a.a2, a.mean, a.rstd, a.y = (outs[k].t.data_ptr() for k in ("hpre", "a2", "mean", "rstd", "y"))
    a.M, a.C, a.hidden, a.rows_per_sample, a.eps = M, Cc, hid, rps, 1e-5
    b = L.MlpBwdArgs()
    b.dy, b.a2, b.mean, b.rstd, b.gamma, b.scale, b.hpre, b.w2t, b.w1t = (t.data_ptr() for t in (x, a2_in, stat, stat, vec, scale, hpre_in, w1, w2))
    b.da2, b.dh, b.dx, b.ws = (outs[k].t.data_ptr() for k in ("da2", "dh", "dx", "ws"))
    b.dgamma, b.dbeta = dg.data_ptr(), db.data_ptr()
    b.M, b.C, b.hidden, b.rows_per_sample = M, Cc, hid, rps
    b.x, b.w1, b.b1 = None, None, None
    fwd = True
    if how == "no hpre at hidden 1056":
        fwd = False                                  # (the forward takes hidden 1056 with or without hpre)
        b.hpre, b.w1t = None, None
        b.x, b.w1, b.b1 = x.data_ptr(), w1.data_ptr(), b1.data_ptr()
        assert lib.swv2_mlp_supported(Cc, hid) == 1 and lib.swv2_mlp_recompute_supported(Cc, hid) == 0
    elif how == "neither operand set":
        fwd = False
        b.w1t = None                                 # hpre without w1t, and x without w1 / b1
        b.x = x.data_ptr()
    elif how == "M = 0":
        a.M = b.M = 0
    elif how == "rows_per_sample = 0":
        a.rows_per_sample = b.rows_per_sample = 0
    else:
        assert lib.swv2_mlp_supported(Cc, hid) == 0
    if fwd:
        assert lib.swv2_mlp_fwd(ctypes.byref(a), None) != 0, how
    assert lib.swv2_mlp_bwd(ctypes.byref(b), None) != 0, how
    torch.cuda.synchronize()
    touched = [k for k, o in outs.items() if not o.untouched()]
    assert not touched and bool((dg == 3.0).all() and (db == -2.0).all()), (how, touched)
    assert lib.swv2_mlp_bwd_ws_floats(0, 128) == 0 and lib.swv2_mlp_bwd_ws_floats(64, 0) == 0
