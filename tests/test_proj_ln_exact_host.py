"""No GPU: the fp64 references and per-element bounds of tests/proj_ln_reference.py, checked on their own.

  * the hand-written LayerNorm backward equals fp64 autograd of  x + s * layer_norm(a1)  scattered through the row table
  * an fp32 emulation of the same formulas (bf16 rounding at a1, da1 and doh) passes every checker at every geometry case of the
    GPU tests: the bounds admit the reference arithmetic itself, no element excluded
  * every checker fails when one element of its input is moved by four times its bound
"""
import pytest
import torch

from tests import proj_ln_reference as R

BF, F64 = R.BF, R.F64


def emulate(c):
    """proj + LN1 forward and backward in fp32 torch with the kernels' rounding points; -> namespace of what the kernels write"""
    wpb = R.prep_dense(c.wp, c.pmap)
    wpt = wpb.T.contiguous()
    a1 = (R.dense_rows(c.oh, c.Bw, c.heads, c.Lp, c.HS).float() @ wpb.float().T + c.bp).to(BF)
    af = a1.float()
    mean = af.mean(1)
    rstd = 1.0 / torch.sqrt(((af - mean.view(-1, 1)) ** 2).mean(1) + 1e-5)
    live, dst = R.table_of(c.rowidx, c.Mw, af.device)
    s = R.sample_scale(c.scale, dst, c.rps).float().view(-1, 1)
    xh = (af - mean.view(-1, 1)) * rstd.view(-1, 1)
    y0 = torch.full((c.rows, c.C), R.SENT)
    y = y0.clone()
    y[dst[live]] = (c.x[dst] + s * (xh * c.gamma + c.beta))[live]
    d = s * c.dy[dst] * live.float().view(-1, 1)
    g = d * c.gamma
    da1 = rstd.view(-1, 1) * (g - g.mean(1, keepdim=True) - xh * (g * xh).mean(1, keepdim=True))
    da1 = torch.where(live.view(-1, 1), da1, torch.zeros(())).to(BF)                  # +0 on padded rows, as the kernels write it
    doh = R.head_major((da1.float() @ wpt.float().T).to(BF), c.Bw, c.heads, c.Lp, c.HS)
    return R.types.SimpleNamespace(wpb=wpb, wpt=wpt, a1=a1, mean=mean, rstd=rstd, y=y, y0=y0, da1=da1, doh=doh,
                                   dgamma=c.base_g + (d * xh).sum(0), dbeta=c.base_b + d.sum(0))


def _variants():
    out = [(p, True, True) for p in R.GEOMETRY]
    out += [((128, 8, 5, 176), True, False), ((96, 4, 1, 176), False, True), ((192, 3, 1, 176), False, False)]
    return out


@pytest.mark.parametrize("geo,table,with_scale", _variants(), ids=lambda v: R.geometry_id(v) if isinstance(v, tuple) else str(int(v)))
def test_fp32_emulation_passes_every_checker(geo, table, with_scale):
    c = R.make_case(*geo, "random", table=table, with_scale=with_scale, seed=1)
    e = emulate(c)
    R.check_forward("emulation", c, e.wpb, e.a1, e.mean, e.rstd, e.y, e.y0)
    R.check_ln_backward("emulation", e.a1, e.mean, e.rstd, c.gamma, c.dy, c.scale, c.rowidx, c.rps, e.da1, e.dgamma, e.dbeta, c.base_g, c.base_b)
    R.check_doh("emulation", c, e.da1, e.wpt, e.doh)


@pytest.mark.parametrize("geo", [p for p in R.GEOMETRY if p[2:] == (1, 176) or p == (128, 8, 5, 176)], ids=R.geometry_id)
def test_exact_operands_are_exact(geo):
    """the premise of the bit-for-bit forward test: integer operands, |a1| <= 136, so fp32 arithmetic in any order, bf16 storage
    and fp64 agree exactly; at most four non-zero entries per oh row, none in a padded head column"""
    c = R.make_case(*geo, "exact", seed=2)
    wpb = R.prep_dense(c.wp, c.pmap)
    rows = R.dense_rows(c.oh, c.Bw, c.heads, c.Lp, c.HS).double()
    assert int((rows != 0).sum(1).max()) <= 4 and float(rows.abs().max()) <= 8 and bool((rows[:, c.pmap < 0] == 0).all())
    assert torch.equal(wpb.double()[:, c.pmap >= 0], c.wp.double()) and bool((wpb[:, c.pmap < 0] == 0).all())
    v, _ = R.ref_proj(c.oh, wpb, c.bp, c.Bw, c.heads, c.Lp)
    assert float(v.abs().max()) <= 136 and torch.equal(v, v.round()) and torch.equal(v.to(BF).double(), v)
    assert torch.equal((rows.float() @ wpb.float().T + c.bp).double(), v)


@pytest.mark.parametrize("geo,table,with_scale", [((32, 2, 1, 64), True, True), ((96, 6, 1, 176), True, True), ((128, 8, 5, 176), True, True),
                                                  ((192, 3, 5, 176), True, False), ((64, 4, 1, 176), False, True)],
                         ids=lambda v: R.geometry_id(v) if isinstance(v, tuple) else str(int(v)))
def test_reference_backward_equals_autograd(geo, table, with_scale):
    """ref_ln_bwd at the true statistics against fp64 autograd of y[dst] = x[dst] + s * layer_norm(a1) (eps as the kernels read it),
    rows with a negative table entry taking no part: d a1, d gamma, d beta to 1e-12 (of the largest entry where that exceeds 1)"""
    c = R.make_case(*geo, "random", table=table, with_scale=with_scale, seed=3)
    a1 = (torch.randn(c.Mw, c.C, dtype=F64, generator=torch.Generator().manual_seed(5)) * 1.5 + 0.3).requires_grad_(True)
    gm, bt = c.gamma.double().requires_grad_(True), c.beta.double().requires_grad_(True)
    live, dst = R.table_of(c.rowidx, c.Mw, a1.device)
    s = R.sample_scale(c.scale, dst, c.rps).view(-1, 1)
    ln = torch.nn.functional.layer_norm(a1, (c.C,), gm, bt, R.EPS32)
    y = c.x.double().clone()
    y = y.index_put((dst[live],), (c.x.double()[dst] + s * ln)[live])
    (y * c.dy.double()).sum().backward()
    mu, _, rho, _ = R.ref_stats(a1.detach())
    rf = R.ref_ln_bwd(a1.detach(), mu, rho, c.gamma, c.dy, c.scale, c.rowidx, c.rps)
    for got, ref in ((rf.da, a1.grad), (rf.dgamma, gm.grad), (rf.dbeta, bt.grad)):
        assert float((got - ref).abs().max()) <= 1e-12 * max(1.0, float(ref.abs().max()))
    assert bool((rf.da[~live] == 0).all()) and (table is False or int((~live).sum()) == c.Bw * (c.Lp - c.Lv))
    # the forward reference at the true statistics is the same function
    yr, _ = R.ref_y(torch.full_like(c.x, R.SENT), a1.detach(), mu, rho, c.gamma, c.beta, c.x, c.scale, c.rowidx, c.rps)
    assert float((yr - y.detach()).abs().max()) <= 1e-12 * max(1.0, float(y.detach().abs().max()))


def test_each_checker_fails_at_four_times_its_bound():
    """one element of each output moved by 4 x its bound (where the bound is 0: by the smallest step) fails that output's checker"""
    c = R.make_case(128, 8, 5, 176, "random", seed=4)
    e = emulate(c)
    v, vb = R.ref_proj(c.oh, e.wpb, c.bp, c.Bw, c.heads, c.Lp)
    mu, mub, rho, rhob = R.ref_stats(e.a1)
    yr, yb = R.ref_y(e.y0, e.a1, e.mean, e.rstd, c.gamma, c.beta, c.x, c.scale, c.rowidx, c.rps)
    rf = R.ref_ln_bwd(e.a1, e.mean, e.rstd, c.gamma, c.dy, c.scale, c.rowidx, c.rps)
    dr, db = R.ref_doh(e.da1, e.wpt, c.Bw, c.heads, c.Lp)
    live, dst = R.table_of(c.rowidx, c.Mw, e.a1.device)
    m_live, m_pad = int(live.nonzero()[7]), int((~live).nonzero()[3])
    # a live row whose sample is not dropped (scale != 0: its gradient bounds are positive)
    m_on = int((live & (R.sample_scale(c.scale, dst, c.rps) != 0)).nonzero()[11])
    tried = 0
    for name, got, ref, bound, idx in (("a1", e.a1, v, vb, (m_live, 5)), ("a1", e.a1, v, vb, (m_pad, 9)), ("mean", e.mean, mu, mub, (m_live,)),
                                       ("rstd", e.rstd, rho, rhob, (m_pad,)), ("y", e.y, yr, yb, (int(dst[m_live]), 17)),
                                       ("da1", e.da1, rf.da, rf.da_bound, (m_on, 3)), ("da1", e.da1, rf.da, rf.da_bound, (m_pad, 3)),
                                       ("doh", e.doh, dr, db, (m_on // c.Lp, 2, m_on % c.Lp, 1)),
                                       ("doh", e.doh, dr, db, (m_on // c.Lp, 2, m_on % c.Lp, c.HS - 1)),
                                       ("dgamma", e.dgamma.double() - c.base_g.double(), rf.dgamma, R.fold_bound(rf.A_g, c.base_g), (40,)),
                                       ("dbeta", e.dbeta.double() - c.base_b.double(), rf.dbeta, R.fold_bound(rf.A_b, c.base_b), (0,))):
        assert R.within(got, ref, bound)[0] == 0, name
        for sign in (1.0, -1.0):
            moved = got.double().clone()
            moved[idx] = ref[idx] + sign * (4.0 * float(bound[idx]) if float(bound[idx]) > 0 else 2.0 ** -140)
            nbad, ratio, where = R.within(moved, ref, bound)
            assert nbad == 1 and where == idx and ratio >= 4.0 * (1 - 1e-9), (name, idx, nbad, ratio, where)
            with pytest.raises(AssertionError):
                R.assert_within("perturbed " + name, moved, ref, bound)
            tried += 1
    assert tried == 22
    # an unnamed destination row of y (bound 0) and the exact-zero rows of da1 as a sign bit
    assert float(yb[dst[m_live]].min()) > 0 and float(db[m_on // c.Lp, 2, m_on % c.Lp, c.HS - 1]) == 0 and float(rf.da_bound[m_pad, 3]) == 0
    da_neg = e.da1.clone()
    da_neg[m_pad, 3] = -0.0
    with pytest.raises(AssertionError):
        R.check_ln_backward("sign bit", e.a1, e.mean, e.rstd, c.gamma, c.dy, c.scale, c.rowidx, c.rps, da_neg, e.dgamma, e.dbeta, c.base_g, c.base_b)
    # a doubled last valid row moves dgamma / dbeta out of their bound
    last = R.last_live_dst(c.rowidx, c.Mw)
    m_last = int((c.rowidx == last).nonzero())
    xh = (e.a1.double()[m_last] - e.mean.double()[m_last]) * e.rstd.double()[m_last]
    dlast = float(R.sample_scale(c.scale, dst, c.rps)[m_last]) * c.dy.double()[last]
    assert R.within(e.dgamma.double() - c.base_g.double() + dlast * xh, rf.dgamma, R.fold_bound(rf.A_g, c.base_g))[0] > c.C // 2
    assert R.within(e.dbeta.double() - c.base_b.double() + dlast, rf.dbeta, R.fold_bound(rf.A_b, c.base_b))[0] > c.C // 2
