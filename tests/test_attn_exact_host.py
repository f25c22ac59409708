"""The fp64 attention references and per-element checkers of tests/attn_reference.py, checked without a GPU:
  * the references are the autograd of the plain softmax formula (1e-12);
  * an fp32 / bf16 emulation of the kernels' data flow (oracle._AttnCoreEmu's rounding points, restated here in fp32 with both softmax
    regimes, both lse sources and the operand-carried statistics of the backward) passes every checker on every input generator;
  * every checker fails when the error it bounds is 4 x the bound;
  * value mutants of the emulation -- the ones a kernel could have -- are each caught by a named checker.
"""
import pytest
import torch

from tests import attn_reference as R

F32 = torch.float32
bf = R.bf16


# ---------------------------------------------------------------------------------------------------------------
# fp32 / bf16 emulation (rounding points of oracle._AttnCoreEmu; log2 domain like the kernels)
# ---------------------------------------------------------------------------------------------------------------
def emu_mask(Bw, L, nwh, nww, thr, mut):
    m = torch.zeros(Bw, 1, L, L, dtype=F32)
    if thr > 0:
        reg = torch.arange(L) > thr if mut == "mask_gt" else torch.arange(L) >= thr
        cross = (reg[:, None] != reg[None, :]).float() * (R.MASK_VALUE * R.LOG2E)
        row = 0 if mut == "mask_row0" else nwh - 1
        m[((torch.arange(Bw) % (nwh * nww)) // nww) == row] = cross
    return m


def emu_bias2(bias):
    return None if bias is None else bf(bias.float() * R.LOG2E)


def emu_forward(x, bias, nwh, nww, thr, regime, mut=None, lse_rounded=None):
    """-> o (bf16 values), lse (fp32, log2 domain).  regime 0: row maximum, exact sum; 1: operand-folded logits, fixed maximum where
    2 sigma' + (table max - min) <= 80 in unmasked windows, sum of the rounded exponentials."""
    q, k, v = x.qn.float(), x.kn.float(), x.v.float()
    Bw, h, L, d = q.shape
    sc2 = (torch.exp(torch.clamp(x.tau.float(), max=R.LN100)) * R.LOG2E).view(1, h, 1, 1)
    b2 = emu_bias2(bias)
    m2 = emu_mask(Bw, L, nwh, nww, thr, mut)
    if regime == 1:
        xs = q * sc2
        hi = bf(xs)
        lo = torch.zeros_like(hi) if mut == "no_lo" else bf(xs - hi)
        S2 = torch.einsum("bhqd,bhkd->bhqk", hi + lo, k)
    else:
        S2 = torch.einsum("bhqd,bhkd->bhqk", q, k) * sc2
    if b2 is not None:
        S2 = S2 + b2.unsqueeze(0)
    S2 = S2 + m2
    ref = S2.amax(-1, keepdim=True)
    if regime == 1:
        bmax = b2.flatten(1).amax(1) if b2 is not None else torch.zeros(h)
        bmin = b2.flatten(1).amin(1) if b2 is not None else torch.zeros(h)
        fixed = (2 * sc2.view(h) + (bmax - bmin) <= 80.0).view(1, h, 1, 1) & ~(m2 != 0).flatten(1).any(1).view(Bw, 1, 1, 1)
        ref = torch.where(fixed, (sc2.view(h) + bmax).view(1, h, 1, 1).expand_as(ref), ref)
    E = torch.exp2(S2 - ref)
    Er = bf(E)
    extra = 0.0
    if mut == "pad_key_late":                  # key L (a zero K row, region 1) counted as a real key: weight exp2(0 + mask - ref)
        reg_q = (torch.arange(L) >= thr).view(1, 1, L, 1)
        mrow = (m2 != 0).flatten(1).any(1).view(Bw, 1, 1, 1)
        extra = torch.exp2(torch.where(mrow & ~reg_q, torch.tensor(R.MASK_VALUE * R.LOG2E), torch.tensor(0.0)) - ref)
    rounded = regime == 1
    ssum = (Er if rounded else E).sum(-1, keepdim=True) + extra
    o = bf(torch.einsum("bhqk,bhkd->bhqd", Er, v) / ssum)
    if lse_rounded is None:
        lse_rounded = rounded and mut != "lse_unrounded"
    lsum = (Er if lse_rounded else E).sum(-1, keepdim=True) + extra
    return o, (ref + torch.log2(lsum)).squeeze(-1)


def split3(x):
    a = bf(x)
    b = bf(x - a)
    return a, b, bf(x - a - b)


def emu_backward(x, bias, nwh, nww, thr, oh, lse, aug, mask_parts=2, mut=None):
    """the kernels' backward from the stored oh / lse / dO / rnorm; aug: statistics and mask as bf16 parts inside the product"""
    q, k, v, dO = x.qn.float(), x.kn.float(), x.v.float(), x.dO.float()
    Bw, h, L, d = q.shape
    tau = x.tau.float()
    sigma = torch.exp(torch.clamp(tau, max=R.LN100)).view(1, h, 1, 1)
    sc2 = sigma * R.LOG2E
    b2 = emu_bias2(bias)
    cos = torch.einsum("bhqd,bhkd->bhqk", q, k)
    oh, lse = oh.float(), lse.float()
    n_delta = d - 8 if mut == "delta_short" else d
    delta = (dO[..., :n_delta] * oh[..., :n_delta]).sum(-1, keepdim=True)
    dP = torch.einsum("bhqd,bhkd->bhqk", dO, v)
    if aug:
        l3 = sum(split3(lse.unsqueeze(-1) / sc2))
        c = (R.MASK_VALUE * R.LOG2E) / sc2
        chi = bf(c)
        c = chi + (bf(c - chi) if mask_parts == 2 else 0.0)
        cross = (emu_mask(Bw, L, nwh, nww, thr, None) != 0).float()
        Sx = (cos - l3 + cross * c) * sc2
        if b2 is not None:
            Sx = Sx + b2.unsqueeze(0)
        P = torch.exp2(Sx)
        dS = P * (dP - sum(split3(delta)))
    else:
        S2 = cos * sc2
        if b2 is not None:
            S2 = S2 + b2.unsqueeze(0)
        P = torch.exp2(S2 + emu_mask(Bw, L, nwh, nww, thr, None) - lse.unsqueeze(-1))
        dS = P * (dP - delta)
    dv = bf(torch.einsum("bhqk,bhqd->bhkd", bf(P), dO))
    dSr = bf(dS)
    gq = torch.einsum("bhqk,bhkd->bhqd", dSr, k)
    gk = torch.einsum("bhqk,bhqd->bhkd", dSr, q)
    rq, rk = (x.rk, x.rq) if mut == "rq_rk" else (x.rq, x.rk)
    dq = bf(rq.unsqueeze(-1) * sigma * (gq - q * (gq * q).sum(-1, keepdim=True)))
    dk = bf(rk.unsqueeze(-1) * sigma * (gk - k * (gk * k).sum(-1, keepdim=True)))
    dlogit = (tau <= R.LN100).float() * sigma.view(h) * (gk * k).sum((0, 2, 3))
    dbias = dS.sum(0) if bias is not None else None
    return dq, dk, dv, dlogit, dbias


# ---------------------------------------------------------------------------------------------------------------
# cases: (L, d, h, nwh, nww, thr, bias, regime)
# ---------------------------------------------------------------------------------------------------------------
CASES = {
    "L54_d16_bias_rowmax": (54, 16, 4, 2, 1, 27, True, 0),
    "L162_d16_folded": (162, 16, 3, 2, 1, 81, False, 1),
    "L162_d16_bias_folded": (162, 16, 3, 2, 1, 90, True, 1),
    "L65_d36_rowmax": (65, 36, 3, 2, 1, 13, False, 0),
}


def setup(case, gen):
    L, d, h, nwh, nww, thr, use_bias, regime = CASES[case]
    Bw = nwh * nww
    x = R.generate(gen, Bw, h, L, d, thr, seed=1)
    bias = R.make_bias(h, L) if use_bias else None
    ref = R.forward_reference(x.qn, x.kn, x.v, x.tau, bias, nwh, nww, thr)
    return x, bias, ref, (nwh, nww, thr), regime


def handed(ref):
    """what the GPU tests hand the backward: oh = bf16(o_ref), lse = fp32(lse_ref)"""
    return bf(ref.o.float()), ref.lse.float()


def test_references_equal_autograd():
    L, d, h, nwh, nww, thr = 20, 8, 3, 2, 1, 7
    x = R.generate("normal", 2, h, L, d, thr, seed=3)
    bias = R.make_bias(h, L)
    ref = R.forward_reference(x.qn, x.kn, x.v, x.tau, bias, nwh, nww, thr)
    q, k, v = (t.double().requires_grad_(True) for t in (x.qn, x.kn, x.v))
    tau = x.tau.double().requires_grad_(True)
    b = (R.bf16(bias.float() * R.LOG2E).double() / R.LOG2E).requires_grad_(True)
    S = torch.einsum("bhqd,bhkd->bhqk", q, k) * torch.exp(torch.clamp(tau, max=R.LN100)).view(1, h, 1, 1) + b + R.mask_table(2, L, nwh, nww, thr)
    o = torch.einsum("bhqk,bhkd->bhqd", torch.softmax(S, -1), v)
    assert float((o.detach() - ref.o).abs().max()) < 1e-12
    assert float((torch.logsumexp(S, -1).detach() * R.LOG2E - ref.lse).abs().max()) < 1e-12
    o.backward(x.dO.double())
    bw = R.backward_reference(ref, ref.o, ref.lse, x.dO, x.rq, x.rk, True)       # the exact oh and lse
    proj = lambda g, n, r: r.double().unsqueeze(-1) * (g - n * (g * n).sum(-1, keepdim=True))      # noqa: E731
    for got, want in ((bw.dv, v.grad), (bw.dq, proj(q.grad, x.qn.double(), x.rq)), (bw.dk, proj(k.grad, x.kn.double(), x.rk)),
                      (bw.dlogit, tau.grad), (bw.dbias, b.grad)):
        assert float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))
    assert float(bw.dlogit[-1]) == 0.0          # tau = 5 > ln 100


@pytest.mark.parametrize("gen", R.GENERATORS)
@pytest.mark.parametrize("case", list(CASES))
def test_emulation_passes_every_checker(case, gen):
    x, bias, ref, (nwh, nww, thr), regime = setup(case, gen)
    d = ref.d
    cS = R.CS_FOLDED if regime == 1 else R.CS_ROW_MAX(d)
    rep = {}
    for lse_rounded in ((True, False) if regime == 1 else (False,)):
        o, lse = emu_forward(x, bias, nwh, nww, thr, regime, lse_rounded=lse_rounded)
        R.check_forward(o, lse, ref, cS, regime == 1, rep)
    oh, lse = handed(ref)
    bw = R.backward_reference(ref, oh, lse, x.dO, x.rq, x.rk, bias is not None)
    for aug in (False, True):
        R.check_backward(*emu_backward(x, bias, nwh, nww, thr, oh, lse, aug), ref, bw, R.CS_ROW_MAX(d), R.MASK_EPS_AUG if aug else R.MASK_EPS_F32, rep, random_data=gen == "normal")
    # chained: the backward from the emulated forward's own outputs against the reference fed the same stored tensors
    o, lse = emu_forward(x, bias, nwh, nww, thr, regime)
    bw2 = R.backward_reference(ref, o, lse, x.dO, x.rq, x.rk, bias is not None)
    R.check_backward(*emu_backward(x, bias, nwh, nww, thr, o, lse, True), ref, bw2, R.CS_ROW_MAX(d), R.MASK_EPS_AUG, rep, random_data=gen == "normal")
    print(case, gen, {k: f"{v:.3f}" for k, v in rep.items()})
    # the derivation is not vacuous: no per-element bound is more than 100 x what this emulation needs (outputs that are exact aside).
    # d logit_scale is left out: one number summed over Bw L^2 pairs whose rounding errors have random signs, so a bound of absolute
    # values is ~sqrt(Bw L^2) above a typical error by construction (measured here: 0.002 - 0.2).
    assert all(v == 0.0 or v > 0.01 for k, v in rep.items() if k != "dlogit"), rep
    if gen == "normal":          # ... which is why random data gets the statistical bound as well: 6 deviations, so a typical error is ~1/6 of it
        assert 0.01 < rep["dlogit_stat"] <= 1.0 and bool((R.backward_bounds(ref, bw, R.CS_ROW_MAX(d), R.MASK_EPS_F32).dlogit_stat
                                                          <= R.backward_bounds(ref, bw, R.CS_ROW_MAX(d), R.MASK_EPS_F32).dlogit).all()), rep


def test_every_checker_fails_at_four_times_its_bound():
    x, bias, ref, (nwh, nww, thr), regime = setup("L54_d16_bias_rowmax", "normal")
    cS = R.CS_ROW_MAX(ref.d)
    fb = R.forward_bounds(ref, cS, False)
    oh, lse = handed(ref)
    bw = R.backward_reference(ref, oh, lse, x.dO, x.rq, x.rk, True)
    bb = R.backward_bounds(ref, bw, cS, R.MASK_EPS_F32)
    pairs = {"o": (ref.o, fb.o), "lse": (ref.lse, fb.lse), "dv": (bw.dv, bb.dv), "dq": (bw.dq, bb.dq), "dk": (bw.dk, bb.dk),
             "dlogit": (bw.dlogit, bb.dlogit), "dlogit_stat": (bw.dlogit, bb.dlogit_stat), "dbias": (bw.dbias, bb.dbias)}
    for name, (r, b) in pairs.items():
        assert bool((b >= 0).all())
        assert R.check(name, r + 0.99 * b, r, b) <= 1.0
        worst = torch.zeros_like(r)
        i = int(b.flatten().argmax())
        worst.view(-1)[i] = 4.0 * b.flatten()[i]            # ONE element off by 4 x its bound
        with pytest.raises(AssertionError, match=name):
            R.check(name, r + worst, r, b)
        with pytest.raises(AssertionError, match=name):
            R.check(name, torch.where(worst != 0, torch.full_like(r, float("nan")), r), r, b)
    assert float(bb.dlogit[-1]) == 0.0 and float(bw.dlogit[-1]) == 0.0
    with pytest.raises(AssertionError):                     # above the clamp the gradient is exactly 0: any value fails
        g = bw.dlogit.clone()
        g[-1] = 1e-30
        R.check("dlogit", g, bw.dlogit, bb.dlogit)


def _fwd_fails(case, gen, mut, names):
    x, bias, ref, (nwh, nww, thr), regime = setup(case, gen)
    cS = R.CS_FOLDED if regime == 1 else R.CS_ROW_MAX(ref.d)
    o, lse = emu_forward(x, bias, nwh, nww, thr, regime, mut=mut)
    b = R.forward_bounds(ref, cS, regime == 1)
    worst = {"o": float(R.ratio(o, ref.o, b.o).max()), "lse": float(R.ratio(lse, ref.lse, b.lse).max())}
    for n in names:
        assert worst[n] > 1.0, (mut, gen, worst)
    return worst


# mutants 1 - 3: the counting generator (uniform attention over a query's allowed keys) makes every key's membership visible
def test_mutant_mask_comparison_off_by_one():
    _fwd_fails("L54_d16_bias_rowmax", "counting", "mask_gt", ("o", "lse"))
    _fwd_fails("L162_d16_folded", "counting", "mask_gt", ("o", "lse"))
    _fwd_fails("L162_d16_folded", "adversarial", "mask_gt", ("o",))


def test_mutant_mask_in_first_window_row():
    _fwd_fails("L162_d16_folded", "counting", "mask_row0", ("o", "lse"))
    _fwd_fails("L162_d16_folded", "adversarial", "mask_row0", ("lse",))


def test_mutant_padded_key_one_late():
    # one leaking padded key moves a uniform row's normaliser by 1 / n: beyond the lse bound at every n <= 176, beyond the o bound for n <= 85
    _fwd_fails("L162_d16_folded", "counting", "pad_key_late", ("lse",))
    _fwd_fails("L65_d36_rowmax", "counting", "pad_key_late", ("o", "lse"))


def test_mutant_folded_operand_without_low_part():
    _fwd_fails("L162_d16_folded", "peaked", "no_lo", ("lse",))
    _fwd_fails("L162_d16_folded", "normal", "no_lo", ("lse",))


def _bwd_worst(case, gen, aug=False, mask_parts=2, mut=None):
    x, bias, ref, (nwh, nww, thr), regime = setup(case, gen)
    oh, lse = handed(ref)
    bw = R.backward_reference(ref, oh, lse, x.dO, x.rq, x.rk, bias is not None)
    b = R.backward_bounds(ref, bw, R.CS_ROW_MAX(ref.d), R.MASK_EPS_AUG if aug else R.MASK_EPS_F32)
    dq, dk, dv, dl, db = emu_backward(x, bias, nwh, nww, thr, oh, lse, aug, mask_parts, mut)
    w = {"dq": R.ratio(dq, bw.dq, b.dq).max(), "dk": R.ratio(dk, bw.dk, b.dk).max(), "dv": R.ratio(dv, bw.dv, b.dv).max(),
         "dlogit": R.ratio(dl, bw.dlogit, b.dlogit).max()}
    if db is not None:
        w["dbias"] = R.ratio(db, bw.dbias, b.dbias).max()
    return {k: float(v) for k, v in w.items()}


def test_mutant_delta_without_last_channel_chunk():
    w = _bwd_worst("L54_d16_bias_rowmax", "normal", mut="delta_short")
    assert w["dq"] > 1 and w["dk"] > 1 and w["dbias"] > 1 and w["dlogit"] > 1, w
    w = _bwd_worst("L65_d36_rowmax", "counting", mut="delta_short")
    assert w["dq"] > 1, w              # (q^ = 0: dk and d logit_scale are exactly 0 there)


def test_mutant_rq_rk_exchanged():
    for gen in ("normal", "peaked"):
        w = _bwd_worst("L162_d16_folded", gen, aug=True, mut="rq_rk")
        assert w["dq"] > 1 and w["dk"] > 1 and w["dv"] <= 1, w


def test_single_part_mask_term_fails_on_adversarial_data_only():
    """-100 / sigma as ONE bf16 value inside the operand (the backward kernels before the hi + lo parts): P of a masked pair is off by up
    to 100 * 2^-9 nat.  Invisible on ordinary data, where masked keys carry no weight; the adversarial generator puts the row's
    mass on them."""
    assert max(_bwd_worst("L162_d16_folded", "normal", aug=True, mask_parts=1).values()) <= 1
    w = _bwd_worst("L162_d16_folded", "adversarial", aug=True, mask_parts=1)
    assert w["dv"] > 1 and w["dq"] > 1 and w["dk"] > 1, w
    assert max(_bwd_worst("L162_d16_folded", "adversarial", aug=True, mask_parts=2).values()) <= 1


def test_lse_from_the_unrounded_sum_is_inside_the_bound():
    """Regime 1 divides by the sum of the ROUNDED exponentials and stores its log2.  A kernel that stored log2 of the unrounded sum would
    be NEARER the fp64 value (by up to log2 e * 2^-9), so no bound against fp64 that admits the shipped kernel can reject it: recorded
    here so that nobody expects the lse check to."""
    w = _fwd_fails("L162_d16_folded", "normal", "lse_unrounded", ())
    assert w["lse"] <= 1.0


def test_emulation_has_the_rounding_points_of_the_oracle():
    """The emulation above restates oracle._AttnCoreEmu (in fp32, log2 domain, with mutant switches) instead of calling it; this ties the two:
    same inputs, both regimes -> the same o, lse, dv, d bias up to bf16 ties (they exponentiate in different bases, so not bit for bit)."""
    from oracle import swin_oracle as O

    class Ctx:
        def save_for_backward(self, *t):
            self.saved_tensors = t

    for case, regime in (("L54_d16_bias_rowmax", 0), ("L162_d16_bias_folded", 1)):
        x, bias, ref, (nwh, nww, thr), _ = setup(case, "normal")
        q, k, v = x.qn.float(), x.kn.float(), x.v.float()
        Bw, h, L, d = q.shape
        sigma = torch.exp(torch.clamp(x.tau.float(), max=R.LN100))
        b = emu_bias2(bias) / R.LOG2E
        m = emu_mask(Bw, L, nwh, nww, thr, None) / R.LOG2E
        S = torch.einsum("bhqd,bhkd->bhqk", q, k) * sigma.view(1, h, 1, 1) + b + m
        rowmax = S.amax(-1, keepdim=True)
        if regime:       # the fixed reference sigma + table maximum of unmasked windows, as oracle.attention_core_normed hands it over
            bmax, bmin = b.flatten(1).amax(1), b.flatten(1).amin(1)
            fixed = (2 * sigma * R.LOG2E + (bmax - bmin) * R.LOG2E <= 80.0).view(1, h, 1, 1) & ~(m != 0).flatten(1).any(1).view(Bw, 1, 1, 1)
            rowmax = torch.where(fixed, (sigma + bmax).view(1, h, 1, 1).expand_as(rowmax), rowmax)
        O.set_rounding(O.bf16_round, softmax="operand_folded" if regime else "row_max")
        try:
            ctx = Ctx()
            o_or = O._AttnCoreEmu.forward(ctx, q, k, v, sigma, b, m, rowmax, bool(regime), bool(regime))
            lse_or = ctx.saved_tensors[-1].squeeze(-1) * R.LOG2E
            grads = O._AttnCoreEmu.backward(ctx, x.dO.float())
        finally:
            O.set_rounding(None)
        o, lse = emu_forward(x, bias, nwh, nww, thr, regime)
        rel = lambda x_, y_: float((x_ - y_).norm() / y_.norm())      # noqa: E731
        figures = (rel(o, o_or), float((lse - lse_or).abs().max()))
        dq, dk, dv, dl, db = emu_backward(x, bias, nwh, nww, thr, o_or, lse_or, False)
        figures += (rel(dv, bf(grads[2])), rel(db, grads[4]))      # (the oracle leaves the bf16 store of dv to its caller)
        print(case, ["%.2e" % f_ for f_ in figures])
        # a rounding point more or less on one side moves a tensor by ~2^-9 / sqrt(3) = 1.1e-3 in this norm; two implementations of the
        # same points differ only where exp and exp2 land on different sides of a bf16 tie
        assert figures[0] < 3e-4 and figures[2] < 3e-4 and figures[3] < 1e-4, figures
        assert figures[1] < (2.0 ** -7 if regime else 1e-4), figures
