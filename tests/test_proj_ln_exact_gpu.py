"""GPU (-m gpu): the fused proj + LayerNorm1 pair (swv2_proj_ln_fwd / _bwd, csrc/proj_ln.hip) and the row-table LayerNorm
(swv2_ln_residual_fwd / _bwd, csrc/rowops.hip), element by element against fp64.

The references, the bounds and their derivations are in tests/proj_ln_reference.py (checked without a GPU by
tests/test_proj_ln_exact_host.py).  Every (C, heads) pair swv2_proj_ln_supported admits runs at one tile exactly, at ragged
last tiles and over several workgroups; four of them at 32 912 window rows, where the MT = 2 instantiations take over.  The row
table sends the valid rows of every window through a random permutation and marks the padded ones -1; rows_per_sample = 100
divides nothing, the drop-path factors cycle through 0, 1.25, 1.

Part A (exact): integer operands for which no rounding can occur; a1 equals fp64 bit for bit on every row, fused and unfused
(swv2_linear + swv2_ln_residual_fwd), mean is exact where C is a power of two, and a dropped sample leaves y[dst] = x[dst].
Part B (random operands): per-element bounds on a1, mean, rstd, y, da1, doh, dgamma, dbeta; past the projection the reference
is built from the kernel's own saved tensors.  The unfused kernels run on the same data under the same bounds.
Part C: swv2_ln_residual_fwd / _bwd alone, past their grid caps, with a row table, res_mod and res = NULL.
Every output sits between guard rows that no launch may touch, y is prefilled (rows no table entry names keep their value),
dgamma / dbeta accumulate onto a non-zero integer baseline.

Worst |err| / bound measured on an MI355X over every case of this file (the bounds are derived; none is fitted to these).
"beyond rounding" is (|err| - 2^-8 |ref|) / (bound - 2^-8 |ref|): the bf16 outputs reach the first term of their bound by
construction (2^-8 is the format's unit roundoff), the margin of the fp32 arithmetic is in the second.
                        a1      beyond    mean     rstd     y       da1     beyond    doh     beyond    dgamma   dbeta
  fused                 0.994   0.00097   0.0046   0.019    0.188   0.992   0.0033    0.994   0.0017    0.064    0.097
  unfused               0.994   0.00097   0.0046   0.020    0.188   0.992   0.0080    0.994   0.0017    0.053    0.045
  ln_residual (Part C)                    0.0033   0.0045   0.192   0.986   0.00025                     0.0040   0.0033
Every fp32 term is below a quarter of its bar (y, 2^-20: 0.19; the fold's 51 * 2^-24: 0.10).  Against the weight gradients'
2^-20, which dgamma / dbeta were first held to, the fused dbeta measured 0.31 and dgamma 0.20: see C_FOLD in proj_ln_reference.py.
"""
import ctypes

import pytest
import torch

from tests import proj_ln_reference as R

pytestmark = pytest.mark.gpu

BF = R.BF
GUARD_ROWS = 128                  # guard rows on either side of every output: a whole row tile of the largest kernel


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
    print("\n[proj_ln worst |err| / bound] " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(R.WORST.items())))


class Guarded:
    """n rows of `cols` elements between GUARD_ROWS guard rows, all prefilled with R.SENT; .t is the tensor the kernels get"""

    def __init__(self, shape, dtype, dev):
        n = 1
        for s in shape:
            n *= s
        self.g = GUARD_ROWS * (n // shape[0])
        self.buf = torch.full((n + 2 * self.g,), R.SENT, dtype=dtype, device=dev)
        self.t = self.buf[self.g:self.g + n].view(*shape)

    def intact(self):
        return bool((self.buf[:self.g] == R.SENT).all() and (self.buf[self.buf.numel() - self.g:] == R.SENT).all())

    def untouched(self):
        return bool((self.buf == R.SENT).all())


def _guards(outs, what):
    bad = [k for k, v in outs.items() if isinstance(v, Guarded) and not v.intact()]
    assert not bad, f"{what}: guard rows written around {bad}"


def fused_forward(K, c, dev):
    ops = K["ops"]
    o = dict(wpb=ops.prep_weight(c.wp, col_map=c.pmap, out_cols=c.K), y=Guarded((c.rows, c.C), torch.float32, dev),
             a1=Guarded((c.Mw, c.C), BF, dev), mean=Guarded((c.Mw,), torch.float32, dev), rstd=Guarded((c.Mw,), torch.float32, dev))
    ops.proj_ln_fwd(c.oh, o["wpb"], c.bp, c.gamma, c.beta, c.scale, c.rowidx, c.x, c.Bw, c.Lp, c.heads, c.rps,
                    out=(o["y"].t, o["a1"].t, o["mean"].t, o["rstd"].t))
    torch.cuda.synchronize()
    _guards(o, "swv2_proj_ln_fwd")
    return o


def unfused_forward(K, c, dev, wpb):
    """the launches swv2_proj_ln_fwd replaces: swv2_linear (head-major operand, bf16 + bias) and swv2_ln_residual_fwd"""
    ops, L = K["ops"], K["L"]
    o = dict(y=Guarded((c.rows, c.C), torch.float32, dev), a1=Guarded((c.Mw, c.C), BF, dev), mean=Guarded((c.Mw,), torch.float32, dev),
             rstd=Guarded((c.Mw,), torch.float32, dev))
    ops.linear(ops.op_heads(c.oh, c.Bw, c.heads, 1, c.Lp, c.HS), wpb, ops.epilogue(L.EPI_BF16, o["a1"].t, ld=c.C, bias=c.bp), c.C)
    ops.ln_residual_fwd(o["a1"].t, c.x, c.gamma, c.beta, c.scale, c.rowidx, o["y"].t, o["mean"].t, o["rstd"].t, c.Mw, c.C, 0, c.rps)
    torch.cuda.synchronize()
    _guards(o, "swv2_linear + swv2_ln_residual_fwd")
    return o


def fused_backward(K, c, dev, f):
    ops, lib = K["ops"], K["L"].load()
    wpt = ops.prep_weight(c.wp, transpose=True, row_map=c.pmap, out_rows=c.K)
    nws = lib.swv2_proj_ln_bwd_ws_floats(c.Mw, c.C)
    assert nws == -(-c.Mw // 64) * 2 * c.C
    o = dict(wpt=wpt, da1=Guarded((c.Mw, c.C), BF, dev), doh=Guarded((c.Bw, c.heads, c.Lp, c.HS), BF, dev),
             ws=Guarded((nws // (2 * c.C), 2 * c.C), torch.float32, dev), dgamma=c.base_g.clone(), dbeta=c.base_b.clone())
    ops.proj_ln_bwd(c.dy, f["a1"].t, f["mean"].t, f["rstd"].t, c.gamma, c.scale, c.rowidx, wpt, o["dgamma"], o["dbeta"], c.Bw, c.Lp,
                    c.heads, c.rps, out=(o["da1"].t, o["doh"].t), ws=o["ws"].t)
    torch.cuda.synchronize()
    _guards(o, "swv2_proj_ln_bwd")
    return o


def unfused_backward(K, c, dev, f, wpt):
    """swv2_ln_residual_bwd with the row table, then swv2_linear into the head-major split for d(oh)"""
    ops, L = K["ops"], K["L"]
    o = dict(da1=Guarded((c.Mw, c.C), BF, dev), doh=Guarded((c.Bw, c.heads, c.Lp, c.HS), BF, dev), dgamma=c.base_g.clone(), dbeta=c.base_b.clone())
    ops.ln_residual_bwd(f["a1"].t, c.dy, c.gamma, c.scale, c.rowidx, f["mean"].t, f["rstd"].t, o["da1"].t, o["dgamma"], o["dbeta"], c.Mw, c.C, c.rps)
    ops.linear(ops.op_bf16(o["da1"].t), wpt, ops.epilogue(L.EPI_HEADS, o["doh"].t, p=(c.heads, 0, c.Lp, c.HS, c.Lv if c.rowidx is not None else c.Lp)),
               c.K)
    torch.cuda.synchronize()
    _guards(o, "swv2_ln_residual_bwd + swv2_linear")
    return o


def _report(tag, what, ratios):
    print(f"\n[proj_ln {tag}] {what}: " + ", ".join(f"{k} {v:.3g}" for k, v in ratios.items()))


def _first_bad(got, ref, n=4):
    bad = (got.double() != ref).nonzero()
    return int(bad.shape[0]), [(tuple(int(v) for v in ix), float(got[tuple(ix)]), float(ref[tuple(ix)])) for ix in bad[:n]]


# ---------------------------------------------------------------------------------------------------------------
# Part A: exact forward projection
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geo", R.GEOMETRY, ids=R.geometry_id)
def test_exact_forward_bit_for_bit(dev, K, geo):
    """integer operands: a1 == fp64 on every element of every row (padded rows are computed like any other), fused and unfused;
    mean exact for C a power of two; a sample with drop-path factor 0 keeps y[dst] == x[dst]; the rest within the Part B bounds"""
    c = R.case_to(R.make_case(*geo, "exact", seed=11), dev)
    what = R.geometry_id(geo)
    f = fused_forward(K, c, dev)
    u = unfused_forward(K, c, dev, f["wpb"])
    v, _ = R.ref_proj(c.oh, f["wpb"], c.bp, c.Bw, c.heads, c.Lp)
    assert float(v.abs().max()) <= 136
    y0 = torch.full_like(c.x, R.SENT)
    live, dst = R.table_of(c.rowidx, c.Mw, dev)
    dropped = live & (R.sample_scale(c.scale, dst, c.rps) == 0)
    assert int(dropped.sum()) > 0 or c.rows <= c.rps
    for name, o in (("fused", f), ("unfused", u)):
        assert torch.equal(o["a1"].t.double(), v), (what, name, "a1", _first_bad(o["a1"].t, v))
        if c.C & (c.C - 1) == 0:
            mu = o["a1"].t.double().mean(1)
            assert torch.equal(o["mean"].t.double(), mu), (what, name, "mean", _first_bad(o["mean"].t, mu))
        assert torch.equal(o["y"].t[dst[dropped]], c.x[dst[dropped]]), (what, name, "y of dropped samples")
        _report("exact " + name, what, R.check_ln_forward(name, o["a1"].t, o["mean"].t, o["rstd"].t, o["y"].t, y0, c.gamma, c.beta, c.x,
                                                          c.scale, c.rowidx, c.rps, 0, what))


# ---------------------------------------------------------------------------------------------------------------
# Part B: random operands, per-element bounds, forward and backward, fused and unfused
# ---------------------------------------------------------------------------------------------------------------
def _random_case(K, dev, geo, table=True, with_scale=True):
    c = R.case_to(R.make_case(*geo, "random", table=table, with_scale=with_scale, seed=12), dev)
    what = R.geometry_id(geo) + ("" if table else " identity") + ("" if with_scale else " no scale")
    y0 = torch.full_like(c.x, R.SENT)
    f = fused_forward(K, c, dev)
    _report("fused fwd", what, R.check_forward("fused", c, f["wpb"], f["a1"].t, f["mean"].t, f["rstd"].t, f["y"].t, y0, what))
    u = unfused_forward(K, c, dev, f["wpb"])
    _report("unfused fwd", what, R.check_forward("unfused", c, f["wpb"], u["a1"].t, u["mean"].t, u["rstd"].t, u["y"].t, y0, what))
    # backward of both from the FUSED forward's saved tensors
    b = fused_backward(K, c, dev, f)
    r = R.check_ln_backward("fused", f["a1"].t, f["mean"].t, f["rstd"].t, c.gamma, c.dy, c.scale, c.rowidx, c.rps, b["da1"].t, b["dgamma"],
                            b["dbeta"], c.base_g, c.base_b, what)
    r.update(R.check_doh("fused", c, b["da1"].t, b["wpt"], b["doh"].t, what))
    _report("fused bwd", what, r)
    ub = unfused_backward(K, c, dev, f, b["wpt"])
    r = R.check_ln_backward("unfused", f["a1"].t, f["mean"].t, f["rstd"].t, c.gamma, c.dy, c.scale, c.rowidx, c.rps, ub["da1"].t, ub["dgamma"],
                            ub["dbeta"], c.base_g, c.base_b, what)
    r.update(R.check_doh("unfused", c, ub["da1"].t, b["wpt"], ub["doh"].t, what))
    _report("unfused bwd", what, r)
    # determinism: a second run of forward and backward agrees bit for bit (guards and workspace included)
    f2 = fused_forward(K, c, dev)
    b2 = fused_backward(K, c, dev, f2)
    for k in ("y", "a1", "mean", "rstd"):
        assert torch.equal(f2[k].buf, f[k].buf), (what, "second forward differs in", k)
    for k in ("da1", "doh", "ws"):
        assert torch.equal(b2[k].buf, b[k].buf), (what, "second backward differs in", k)
    assert torch.equal(b2["dgamma"], b["dgamma"]) and torch.equal(b2["dbeta"], b["dbeta"]), (what, "second backward differs in dgamma / dbeta")


@pytest.mark.parametrize("geo", R.GEOMETRY, ids=R.geometry_id)
def test_random_per_element(dev, K, geo):
    _random_case(K, dev, geo)


# rowidx = NULL (identity: every window row is a destination, the LAST row is live, so a clamped duplicate of it in a ragged last
# tile would be counted in dgamma / dbeta): every pair at 176 rows (MT = 1: 64-row tiles, 48 left; C 192: 128-row tiles, 48
# left) and the MT = 2 kernels at 32 912 rows (16 left)
IDENTITY = [(C, h, 1, 176) for C, h in R.PAIRS] + [(C, h) + R.BIG_CASE for C, h in R.BIG_PAIRS]


@pytest.mark.parametrize("geo", IDENTITY, ids=R.geometry_id)
def test_random_per_element_identity_rows(dev, K, geo):
    _random_case(K, dev, geo, table=False)


@pytest.mark.parametrize("geo,table", [((128, 8, 5, 176), True), ((192, 3, 1, 176), False)], ids=["C128-h8-table", "C192-h3-identity"])
def test_random_per_element_without_scale(dev, K, geo, table):
    _random_case(K, dev, geo, table=table, with_scale=False)


# ---------------------------------------------------------------------------------------------------------------
# Part C: swv2_ln_residual_fwd / _bwd beyond the fused shapes
# ---------------------------------------------------------------------------------------------------------------
def _ln_case(C, M, how, seed, dev):
    """how: "table" (7 of 8 rows valid, permuted; res in destination order), "res_mod" (the same table, res = [37][C] added at
    dst % 37: PatchEmbed's pos_embed add), "nores" (the same table, res = NULL)"""
    g = torch.Generator().manual_seed(seed)
    valid = torch.rand(M, generator=g) >= 0.125
    valid[M - 1] = True                                    # the last row of a ragged last workgroup is live
    rowidx, rows = R.row_table(M, valid, g)
    T = 37 if how == "res_mod" else 0
    c = R.types.SimpleNamespace(C=C, M=M, rows=rows, rowidx=rowidx, res_mod=T, rps=R.RPS)
    c.a = (torch.randn(M, C, generator=g) * 1.5 + 0.25 * torch.randn(M, 1, generator=g)).to(BF)
    c.res = None if how == "nores" else torch.randn(T if T else rows, C, generator=g)
    c.gamma, c.beta = R.signed_log_uniform(C, 1e-3, 2.0, g), torch.randn(C, generator=g)
    c.scale = R.scale_cycle(rows, R.RPS)
    c.dy = torch.randn(rows, C, generator=g)
    c.dy[R.last_live_dst(rowidx, M)] *= 64.0
    c.base_g = torch.randint(1, 4, (C,), generator=g).float()
    c.base_b = -torch.randint(1, 4, (C,), generator=g).float()
    return R.case_to(c, dev)


def _ln_forward(K, c, dev):
    o = dict(y=Guarded((c.rows, c.C), torch.float32, dev), mean=Guarded((c.M,), torch.float32, dev), rstd=Guarded((c.M,), torch.float32, dev))
    K["ops"].ln_residual_fwd(c.a, c.res, c.gamma, c.beta, c.scale, c.rowidx, o["y"].t, o["mean"].t, o["rstd"].t, c.M, c.C, c.res_mod, c.rps)
    torch.cuda.synchronize()
    _guards(o, "swv2_ln_residual_fwd")
    return o


# C 128: 16 rows per workgroup, 65 552 rows = 4097 workgroups' worth: past the 4096-workgroup cap (grid stride), ragged end
@pytest.mark.parametrize("C,M,how", [(128, 65552, "table"), (128, 65552, "nores"), (768, 300, "table"), (768, 300, "res_mod")])
def test_ln_residual_forward_row_table(dev, K, C, M, how):
    c = _ln_case(C, M, how, 21 + C + M, dev)
    o = _ln_forward(K, c, dev)
    y0 = torch.full((c.rows, c.C), R.SENT, device=dev)
    _report("ln fwd", f"C{C} M{M} {how}", R.check_ln_forward("ln_residual", c.a, o["mean"].t, o["rstd"].t, o["y"].t, y0, c.gamma, c.beta, c.res,
                                                             c.scale, c.rowidx, c.rps, c.res_mod, f"C{C} M{M} {how}"))


# C 128: 16 rows per workgroup, 8 200 rows > 512 x 16; C 384: 4 rows per workgroup, 4 104 rows > 512 x 8: past
# SWV2_LN_BWD_MAX_BLOCKS (grid stride, every workgroup's partial row folded)
@pytest.mark.parametrize("C,M", [(128, 8200), (384, 4104)])
def test_ln_residual_backward_row_table(dev, K, C, M):
    c = _ln_case(C, M, "table", 31 + C + M, dev)
    f = _ln_forward(K, c, dev)
    da, dg, db = Guarded((c.M, c.C), BF, dev), c.base_g.clone(), c.base_b.clone()
    K["ops"].ln_residual_bwd(c.a, c.dy, c.gamma, c.scale, c.rowidx, f["mean"].t, f["rstd"].t, da.t, dg, db, c.M, c.C, c.rps)
    torch.cuda.synchronize()
    assert da.intact(), "swv2_ln_residual_bwd: guard rows written around da"
    _report("ln bwd", f"C{C} M{M}", R.check_ln_backward("ln_residual", c.a, f["mean"].t, f["rstd"].t, c.gamma, c.dy, c.scale, c.rowidx, c.rps,
                                                        da.t, dg, db, c.base_g, c.base_b, f"C{C} M{M}"))


# ---------------------------------------------------------------------------------------------------------------
# Refusals
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,heads,Lp", [(128, 3, 64), (128, 10, 64), (160, 2, 64), (128, 8, 60)])
def test_unsupported_shapes_are_refused(dev, K, C, heads, Lp):
    """swv2_proj_ln_fwd / _bwd return non-zero for a head count, a width or a window pitch without an instantiation and write nothing"""
    ops, L = K["ops"], K["L"]
    Bw, HS = 2, 16
    Mw = Bw * Lp
    g = torch.Generator().manual_seed(C + heads + Lp)
    rnd = lambda *s: torch.randn(*s, generator=g).to(dev)          # noqa: E731
    oh, wpb, wpt = rnd(Bw, heads, Lp, HS).to(BF), rnd(C, heads * HS).to(BF), rnd(heads * HS, C).to(BF)
    vec, x = rnd(C), rnd(Mw, C)
    outs = dict(y=Guarded((Mw, C), torch.float32, dev), a1=Guarded((Mw, C), BF, dev), mean=Guarded((Mw,), torch.float32, dev),
                rstd=Guarded((Mw,), torch.float32, dev), da1=Guarded((Mw, C), BF, dev), doh=Guarded((Bw, heads, Lp, HS), BF, dev),
                ws=Guarded((-(-Mw // 64), 2 * C), torch.float32, dev))
    assert Lp % 16 or L.load().swv2_proj_ln_supported(C, heads, HS) == 0
    with pytest.raises(L.Swv2Error):
        ops.proj_ln_fwd(oh, wpb, vec, vec, vec, None, None, x, Bw, Lp, heads, R.RPS, out=(outs["y"].t, outs["a1"].t, outs["mean"].t, outs["rstd"].t))
    dg, db = torch.full((C,), 3.0, device=dev), torch.full((C,), -2.0, device=dev)
    a1, mean, rstd = rnd(Mw, C).to(BF), rnd(Mw), rnd(Mw).abs()
    with pytest.raises(L.Swv2Error):
        ops.proj_ln_bwd(x, a1, mean, rstd, vec, None, None, wpt, dg, db, Bw, Lp, heads, R.RPS, out=(outs["da1"].t, outs["doh"].t), ws=outs["ws"].t)
    torch.cuda.synchronize()
    assert all(o.untouched() for o in outs.values()) and bool((dg == 3.0).all() and (db == -2.0).all())
    # the raw entry points say so by their return value
    a = L.ProjLnArgs()
    a.oh, a.wp, a.bp, a.gamma, a.beta, a.x = (t.data_ptr() for t in (oh, wpb, vec, vec, vec, x))
    a.a1, a.mean, a.rstd, a.y = (outs[k].t.data_ptr() for k in ("a1", "mean", "rstd", "y"))
    a.Bw, a.Lp, a.heads, a.C, a.rows_per_sample, a.eps = Bw, Lp, heads, C, R.RPS, 1e-5
    assert L.load().swv2_proj_ln_fwd(ctypes.byref(a), None) != 0
