"""No GPU: the fp64 references and per-element bounds of tests/mlp_reference.py, checked on their own.

  * the references equal fp64 autograd of the plain formula  x + s * layer_norm(gelu(x w1^T + b1) w2^T + b2)
  * B', the bar of the fp32 GELU', is 4 x the worst error of the transcribed fp32 formula over every finite bf16 input
  * an fp32 / bf16 emulation of both kernels (the oracle's rounding points, fp32 sums over 32 hidden units at a time) passes every
    checker on every case of the GPU tests' tables, the exact cases bit for bit, both sweeps on every finite pattern
  * the sweeps' generators: every finite pattern present, table-only / formula-only / mixed tiles present, every pattern meeting
    a |da2| >= 2^-4 in fp64
  * every checker fails when one element of its input is moved by four times its bound
  * the host twins of the kernel mutants (a) .. (i) of LABNOTES.md are each rejected by the checker the GPU test relies on
"""
import math

import pytest
import torch

from tests import mlp_reference as R
from tests import proj_ln_reference as P

BF, F64 = R.BF, R.F64
LUT = R.host_gelu_lut
BP = R.gelu_grad_bar


def _check_all(c, e, tag="emulation"):
    r = R.check_all_forward(tag, c, LUT(), e.hpre, e.a2, e.mean, e.rstd, e.y)
    r.update(R.check_all_backward(tag, c, e.a2, e.mean, e.rstd, e.hpre, e.da2, e.dh, e.dx, e.dgamma, e.dbeta, BP()))
    assert all(e.guards.values()), e.guards
    return r


def test_case_table_covers_what_it_claims():
    """every C meets every hidden class, every M class at least two C; the instantiations named in the issue are reached"""
    for C in R.CS:
        assert {h for c_, h, _ in R.CASES if c_ == C} == set(R.HIDDENS)
    for M in R.MS:
        assert len({c_ for c_, _, m in R.CASES if m == M}) >= 2
    assert all(R.fwd_mt(*p) == 2 and R.bwd_mt(p[0], p[2]) == 2 for p in R.BIG_CASES) and -(-R.M_BIG // 128) == 257 and R.M_BIG % 128 == 80
    assert R.fwd_mt(192, 1056, 77) == 2 and R.bwd_mt(192, 77) == 1 and (192, 1056, 77) in R.CASES and (192, 1056, 176) in R.CASES
    assert {C for C, _, _ in R.EXACT_CASES} == set(R.CS) and any(m == R.M_BIG for _, _, m in R.EXACT_CASES)


def test_gelu_grad_bar_is_four_times_the_emulated_formulas_worst_error():
    """B' = 4 x worst |fp32 gelu_grad_f (rcp and exp correctly rounded) - fp64| over the 65 280 finite bf16 inputs: 2.28e-7 at
    x = 0.0864 on a CPU, so the bar is 0.96 * 2^-20; the fp64 GELU' is the derivative of the fp64 GELU"""
    worst, at = R.gelu_grad_emulation_error()
    print(f"\n[mlp host] worst emulated GELU' error {worst:.4g} at x = {at:.4g}; B' = {R.gelu_grad_bar():.4g} = {R.gelu_grad_bar() * 2 ** 20:.3f} * 2^-20")
    assert 2.0e-7 < worst < 2.6e-7 and R.gelu_grad_bar() == 4.0 * worst
    x = torch.linspace(-9, 9, 4001, dtype=F64).requires_grad_(True)
    R.gelu64(x).sum().backward()
    assert float((x.grad - R.gelu_grad64(x.detach())).abs().max()) <= 1e-14
    # the emulated forward GELU meets the forward's bar on every finite input: the host's stand-in for the library's table is sound
    pats = R.bf16_bits_all()
    fin = R.finite_patterns()
    ref, bound = R.ref_gelu(pats[fin].float())
    assert R.within(LUT()[fin], ref, bound)[0] == 0
    # the premise of the exact cases
    p = torch.tensor(R.EXACT_PRE).to(BF)
    want = torch.tensor([v if v > 0 else 0.0 for v in R.EXACT_PRE])
    assert torch.equal(R.lut_of(LUT(), p), want) and torch.equal(R.gelu64(p.float()).float().to(BF).float(), want)
    assert torch.equal(R.lut_of(R.host_gelu_grad_lut(), p).abs(), (want > 0).float())


@pytest.mark.parametrize("C,hid,M,with_scale", [(32, 96, 77, True), (128, 128, 176, True), (192, 1056, 13, False)])
def test_references_equal_autograd(C, hid, M, with_scale):
    """every fp64 reference, chained at the true intermediate values, against fp64 autograd of the plain formula: to 1e-12 (of the
    largest entry where that exceeds 1)"""
    c = R.make_case(C, hid, M, with_scale=with_scale, seed=3)
    xb = c.x.to(BF).double().requires_grad_(True)              # the matrix products read bf16(x); the residual reads x
    gm, bt = c.gamma.double().requires_grad_(True), c.beta.double().requires_grad_(True)
    hp = xb @ c.w1.double().T + c.b1.double()
    hp.retain_grad()
    a2 = R.gelu64(hp) @ c.w2.double().T + c.b2.double()
    a2.retain_grad()
    s = P.sample_scale(c.scale, torch.arange(M), c.rps).view(-1, 1)
    y = c.x.double() + s * torch.nn.functional.layer_norm(a2, (C,), gm, bt, P.EPS32)
    (y * c.dy.double()).sum().backward()
    close = lambda got, ref: float((got - ref).abs().max()) <= 1e-12 * max(1.0, float(ref.abs().max()))      # noqa: E731
    v, _ = R.ref_hpre(c.x, c.w1, c.b1)
    assert close(v, hp.detach())
    # (fc2 from the fp64 GELU instead of the table: ref_linear is the function ref_a2 applies to the table's values)
    v2, _ = R.ref_linear(R.gelu64(hp.detach()), c.w2, c.b2, hid)
    assert close(v2, a2.detach())
    mu, _, rho, _ = P.ref_stats(a2.detach())
    yr, _ = P.ref_y(torch.full_like(c.x, R.SENT), a2.detach(), mu, rho, c.gamma, c.beta, c.x, c.scale, None, c.rps)
    assert close(yr, y.detach())
    rf = P.ref_ln_bwd(a2.detach(), mu, rho, c.gamma, c.dy, c.scale, None, c.rps)
    assert close(rf.da, a2.grad) and close(rf.dgamma, gm.grad) and close(rf.dbeta, bt.grad)
    G = a2.grad @ c.w2.double()
    dh = G * R.gelu_grad64(hp.detach())
    assert close(dh, hp.grad)
    assert close(c.dy.double() + hp.grad @ c.w1.double(), c.dy.double() + xb.grad)
    # ref_dh / ref_dx are these formulas on bf16 inputs
    d_b, h_b = a2.grad.to(BF), hp.detach().to(BF)
    ref, _, G2 = R.ref_dh(d_b, c.w2t, h_b, BP())
    assert torch.equal(G2, d_b.double() @ c.w2.double()) and torch.equal(ref, G2 * R.gelu_grad64(h_b.float()))
    dh_b = hp.grad.to(BF)
    assert torch.equal(R.ref_dx(c.dy, dh_b, c.w1t)[0], c.dy.double() + dh_b.double() @ c.w1.double())


def _variants():
    out = [(p, True, True) for p in R.CASES + R.BIG_CASES] + [(p, False, False) for p in R.NO_SCALE_CASES]
    return out


@pytest.mark.parametrize("geo,with_scale,baseline", _variants(), ids=lambda v: R.case_id(v) if isinstance(v, tuple) else str(int(v)))
def test_fp32_emulation_passes_every_checker(geo, with_scale, baseline):
    c = R.make_case(*geo, with_scale=with_scale, baseline=baseline, seed=1)
    r = _check_all(c, R.emulate(c))
    # the fp32 terms leave room: nothing but the bf16 roundings comes near its bar
    assert max(r[k] for k in ("mean", "rstd", "y", "dx", "dgamma", "dbeta")) < 0.5, r


@pytest.mark.parametrize("geo", R.EXACT_CASES, ids=R.case_id)
def test_exact_operands_are_exact(geo):
    """the premise of the bit-for-bit tests: hpre in EXACT_PRE, |a2| <= 136 an integer, and fp32 arithmetic in any order, bf16 storage
    and fp64 agree exactly; dh = +-(the da2 element its w2 column names) or 0, dx = fp32(dy + one dh element)"""
    c = R.make_case(*geo, mode="exact", seed=2)
    e = R.emulate(c)
    v, _ = R.ref_hpre(c.x, c.w1, c.b1)
    assert bool(torch.isin(v, torch.tensor(R.EXACT_PRE, dtype=F64)).all()) and torch.equal(e.hpre.double(), v)
    v2, _ = R.ref_a2(e.hpre, LUT(), c.w2, c.b2)
    assert float(v2.abs().max()) <= 136 and torch.equal(v2, v2.round()) and torch.equal(e.a2.double(), v2)
    assert int((c.w2 != 0).sum(0).max()) <= 1 and int((c.w2 != 0).sum(1).max()) <= 4 and int((c.w1t_exact != 0).sum(1).max()) == 1
    ref, _, G = R.ref_dh(e.da2, c.w2t, e.hpre, 0.0)
    want = G * (v > 0)
    assert torch.equal(e.dh.double(), want) and bool(((ref - want).abs() <= 2.0 ** -40 * G.abs()).all())      # (GELU'(8) = 1 - 5e-15)
    dxr = (c.dy.double() + e.dh.double() @ c.w1t_exact.double().T).float()
    assert torch.equal(e.dx, dxr)


SWEEPS_FWD = [(C, R.fwd_sweep_rows(C), None) for C in R.CS] + [(32, 32768, None), (192, R.fwd_sweep_rows(192), 1056)]
SWEEPS_BWD = [(128, 128, 2048, False), (192, 128, 2048, False), (256, 128, 2048, False), (32, 32768, 64, False), (128, 4096, 128, True),
              (192, 4096, 192, True)]


def _assert_layout(bits, copies):
    fin = R.finite_patterns()
    count = torch.bincount(bits.reshape(-1), minlength=65536)
    assert bool((count[fin] >= copies).all()) and int(count[~fin].sum()) == 0
    cls = R.sweep_tiles(bits)
    assert int((cls == 0).sum()) >= 18 * copies and int((cls == 1).sum()) >= 230 * copies and int((cls == 2).sum()) >= 1
    # a mixed tile holds table patterns and +0, -0, below and above the table
    r, ccol = [int(v) for v in (cls == 2).nonzero()[0]]
    tile = bits[16 * r:16 * r + 16, 16 * ccol:16 * ccol + 16].reshape(-1)
    assert all(int((tile == p).sum()) >= 1 for p in (0, 0x8000, R.GT_LO - 1, R.GT_LO + R.GT_HALF)) and int(R.in_table(R.from_bits(tile)).sum()) >= 200


@pytest.mark.parametrize("C,rows,hid", SWEEPS_FWD)
def test_forward_sweep_generator_and_emulation(C, rows, hid):
    c = R.make_fwd_sweep(C, rows, hid)
    _assert_layout(c.bits, (rows // 16) * (C // 16) // 255)
    if rows > 4096:
        return
    hp = (c.x.to(BF).float() @ c.w1.float().T).to(BF)
    assert bool(R.hpre_matches(hp, c.bits[:, torch.arange(c.hid) % C]).all())
    act = R.lut_of(LUT(), hp)
    a2 = (act @ c.w2.float().T).to(BF)
    assert torch.equal(a2.float(), act[:, :C])
    ref, bound = R.ref_gelu(hp[:, :C].float())
    assert R.within(a2, ref, bound)[0] == 0


@pytest.mark.parametrize("C,M,hid,recompute", SWEEPS_BWD)
def test_backward_sweep_generator_and_emulation(C, M, hid, recompute):
    """the layout; every finite pattern meets an fp64 |da2| >= 2^-4 * (1 + 2^-6) (the margin covers the kernel's bf16 rounding of da2);
    the emulation passes the dh checker on every element"""
    c = R.make_bwd_sweep(C, M, hid, recompute)
    _assert_layout(c.bits, (M // 16) * (hid // 16) // 255)
    rf = P.ref_ln_bwd(c.a2, c.mean, c.rstd, c.gamma, c.dy, None, None, c.rps)
    G = rf.da[:, torch.arange(hid) % C]
    ok = R.sweep_coverage(c.bits, G / (1 + 2.0 ** -6))
    assert bool(ok[R.finite_patterns()].all()), int((~ok[R.finite_patterns()]).sum())
    if M > 4096:
        return
    e = R.emulate(c, hpre_in=c.hpre)
    assert torch.equal(e.da2.double()[:, torch.arange(hid) % C], R.ref_dh(e.da2, c.w2t, c.hpre, 0.0)[2])
    R.check_dh("emulation", e.da2, c.w2t, c.hpre, e.dh, BP())
    assert R.gelu_grad_ratio(e.da2, c.w2t, c.hpre, e.dh) <= R.gelu_grad_emulation_error()[0] * (1 + 1e-6)


def test_each_checker_fails_at_four_times_its_bound():
    """one element of each output moved by 4 x its bound fails that output's checker, at the moved element and nowhere else"""
    c = R.make_case(128, 96, 176, seed=4)
    e = R.emulate(c)
    v, vb = R.ref_hpre(c.x, c.w1, c.b1)
    v2, v2b = R.ref_a2(e.hpre, LUT(), c.w2, c.b2)
    mu, mub, rho, rhob = P.ref_stats(e.a2)
    yr, yb = P.ref_y(torch.full_like(c.x, R.SENT), e.a2, e.mean, e.rstd, c.gamma, c.beta, c.x, c.scale, None, c.rps)
    rf = P.ref_ln_bwd(e.a2, e.mean, e.rstd, c.gamma, c.dy, c.scale, None, c.rps)
    dhr, dhb, _ = R.ref_dh(e.da2, c.w2t, e.hpre, BP())
    dxr, dxb = R.ref_dx(c.dy, e.dh, c.w1t)
    m_on = 130                                   # a row of the second sample (factor 1.25; the first is dropped)
    assert float(c.scale[m_on // c.rps]) != 0 and float(c.scale[0]) == 0
    tried = 0
    for name, got, ref, bound, idx in (("hpre", e.hpre, v, vb, (7, 5)), ("hpre", e.hpre, v, vb, (175, 95)), ("a2", e.a2, v2, v2b, (64, 127)),
                                       ("mean", e.mean, mu, mub, (3,)), ("rstd", e.rstd, rho, rhob, (175,)), ("y", e.y, yr, yb, (m_on, 17)),
                                       ("da2", e.da2, rf.da, rf.da_bound, (m_on, 3)), ("dh", e.dh, dhr, dhb, (m_on, 64)),
                                       ("dh", e.dh, dhr, dhb, (175, 95)), ("dx", e.dx, dxr, dxb, (m_on, 0)), ("dx", e.dx, dxr, dxb, (2, 9)),
                                       ("dgamma", e.dgamma.double() - c.base_g.double(), rf.dgamma, R.fold_bound(rf.A_g, c.base_g), (40,)),
                                       ("dbeta", e.dbeta.double() - c.base_b.double(), rf.dbeta, R.fold_bound(rf.A_b, c.base_b), (0,))):
        assert R.within(got, ref, bound)[0] == 0 and float(bound[idx]) > 0, name
        for sign in (1.0, -1.0):
            moved = got.double().clone()
            moved[idx] = ref[idx] + sign * 4.0 * float(bound[idx])
            nbad, ratio, where = R.within(moved, ref, bound)
            assert nbad == 1 and where == idx and ratio >= 4.0 * (1 - 1e-9), (name, idx, nbad, ratio, where)
            with pytest.raises(AssertionError):
                R.assert_within("perturbed " + name, moved, ref, bound)
            tried += 1
    assert tried == 26
    # the forward GELU's bar and B' alone: a table value one bf16 step off, a GELU' off by 4 B'
    pats = R.bf16_bits_all()
    x = pats[R.finite_patterns()].float()
    ref, bound = R.ref_gelu(x)
    lut = LUT()[R.finite_patterns()].double()
    i = int((x == 1.5).nonzero())
    lut[i] = lut[i] + 2 * 2.0 ** -7
    assert R.within(lut, ref, bound)[0] == 1
    dh = e.dh.double().clone()
    G = R.ref_dh(e.da2, c.w2t, e.hpre, 0.0)[2]
    j = (m_on, int(G[m_on].abs().argmax()))
    dh[j] = dhr[j] + 2.0 ** -8 * abs(float(dhr[j])) + 128 * 2.0 ** -23 * float((e.da2.double().abs() @ c.w2t.double().abs().T)[j]) + 4 * BP() * abs(float(G[j]))
    assert R.within(dh, dhr, dhb)[0] == 1
    # a doubled last row moves dgamma / dbeta out of their bound
    xh = (e.a2.double()[-1] - e.mean.double()[-1]) * e.rstd.double()[-1]
    dlast = float(c.scale[-1]) * c.dy.double()[-1]
    assert R.within(e.dgamma.double() - c.base_g.double() + dlast * xh, rf.dgamma, R.fold_bound(rf.A_g, c.base_g))[0] > c.C // 2
    assert R.within(e.dbeta.double() - c.base_b.double() + dlast, rf.dbeta, R.fold_bound(rf.A_b, c.base_b))[0] > c.C // 2


# ---------------------------------------------------------------------------------------------------------------
# host twins of the kernel mutants: each is rejected by the check the GPU tests rely on for it
# ---------------------------------------------------------------------------------------------------------------
def _rejected(fn):
    with pytest.raises(AssertionError):
        fn()


def test_mutant_a_half_table_sign_from_the_wrong_half_word():
    c = R.make_bwd_sweep(192, 128, 2048)
    e = R.emulate(c, mutate="a", hpre_in=c.hpre)
    _rejected(lambda: R.check_dh("a", e.da2, c.w2t, c.hpre, e.dh, BP()))
    # at C 128 (the full table) the twin changes nothing
    c = R.make_bwd_sweep(128, 128, 2048)
    e = R.emulate(c, mutate="a", hpre_in=c.hpre)
    R.check_dh("a", e.da2, c.w2t, c.hpre, e.dh, BP())


def test_mutant_b_clamped_offsets_without_the_fallback():
    c = R.make_fwd_sweep(64, 1024)
    e = R.emulate(c, mutate="b")
    assert bool(R.hpre_matches(e.hpre, c.bits).all()) and not torch.equal(e.a2.float(), R.lut_of(LUT(), e.hpre))
    ref, bound = R.ref_gelu(e.hpre.float())
    assert R.within(e.a2, ref, bound)[0] > 0
    c = R.make_bwd_sweep(128, 128, 2048)
    e = R.emulate(c, mutate="b", hpre_in=c.hpre)
    _rejected(lambda: R.check_dh("b", e.da2, c.w2t, c.hpre, e.dh, BP()))


def test_mutant_c_table_of_the_next_pattern():
    c = R.make_fwd_sweep(64, 1024)
    e = R.emulate(c, mutate="c")
    assert not torch.equal(e.a2.float(), R.lut_of(LUT(), e.hpre))
    c = R.make_bwd_sweep(128, 128, 2048)
    e = R.emulate(c, mutate="c", hpre_in=c.hpre)
    _rejected(lambda: R.check_dh("c", e.da2, c.w2t, c.hpre, e.dh, BP()))
    # the random cases notice as well: fc2 is judged from the library's own table
    c = R.make_case(96, 128, 77, seed=1)
    e = R.emulate(c, mutate="c")
    _rejected(lambda: R.check_fc2("c", c, LUT(), e.hpre, e.a2))


@pytest.mark.parametrize("geo", [(32, 32, 1), (128, 96, 176), (192, 1056, 77)], ids=R.case_id)
def test_mutant_d_bias_of_the_wrong_half_chunk(geo):
    c = R.make_case(*geo, seed=1)
    e = R.emulate(c, mutate="d")
    _rejected(lambda: R.check_fc1("d", c, e.hpre))


def test_mutant_e_drop_path_factor_of_the_tile_row():
    c = R.make_case(64, 128, 176, seed=1)
    e = R.emulate(c, mutate="e")
    _rejected(lambda: R.check_ln("e", c, e.a2, e.mean, e.rstd, e.y))
    # (a single sample cannot tell)
    c = R.make_case(64, 128, 77, seed=1)
    e = R.emulate(c, mutate="e")
    R.check_ln("e", c, e.a2, e.mean, e.rstd, e.y)


def test_mutant_f_tail_store_skipped():
    c = R.make_case(96, 96, 13, seed=1)
    e = R.emulate(c, mutate="f")
    _rejected(lambda: R.check_fc1("f", c, e.hpre))
    assert bool((e.hpre[:, 64:] == R.SENT).all())


def test_mutant_g_store_without_the_row_clamp():
    """(host twin only: the kernel mutant writes out of bounds)"""
    c = R.make_case(128, 128, 77, seed=1)
    e = R.emulate(c, mutate="g")
    assert not e.guards["a2"] and all(v for k, v in e.guards.items() if k != "a2")
    assert all(R.emulate(c).guards.values())
    # one workgroup exactly: nothing past M
    assert all(R.emulate(R.make_case(128, 128, 64, seed=1), mutate="g").guards.values())


@pytest.mark.parametrize("geo", [(32, 128, 13), (256, 2048, 176)], ids=R.case_id)
def test_mutant_h_rstd_without_eps(geo):
    """the random cases keep fc2's outputs near 2^-6, so that eps = 1e-5 is percents of a row's variance: far beyond C 2^-22"""
    c = R.make_case(*geo, seed=1)
    e = R.emulate(c, mutate="h")
    _rejected(lambda: R.check_ln("h", c, e.a2, e.mean, e.rstd, e.y))
    mu, mub, rho, rhob = P.ref_stats(e.a2)
    assert R.within(e.rstd, rho, rhob)[0] == c.M


def test_mutant_i_fold_count_of_the_small_tile():
    c = R.make_case(32, 64, R.M_BIG, seed=1)
    e = R.emulate(c, mutate="i")
    _rejected(lambda: R.check_ln_backward("i", c, e.a2, e.mean, e.rstd, e.da2, e.dgamma, e.dbeta))
    assert math.isfinite(float(e.dgamma.abs().max()))
