"""No GPU: the fp64 reference, the derived bounds and the host emulations of tests/cpb_reference.py themselves.

  * the reference agrees with oracle.swin_oracle (cpb_bias, rel_coords_log) to fp32 noise and with torch autograd of the fp64 formula
    to fp64 noise;
  * an fp32 emulation of every kernel form (the VALU chain order, the hi + lo split summed as the three MFMAs, the chunk-summing loops,
    the fold order, the atomics in reverse row order) stays inside its own bounds for every case of both tables, and equals fp64 on the
    integer cases;
  * the gate-ambiguity condition holds for every case: the ambiguity term exceeds the rest of the bound in at most 1 % of the dw1 /
    db1 elements;
  * the keep-word decode agrees with test_gpu_parity._decode_keep_bits, and the structured words mean what their names say;
  * every checker fails at 4 x its bound, and the host twin of each kernel mutant (LABNOTES.md, "The CPB kernels element by element")
    fails the checker its GPU counterpart fails.
"""
import pytest
import torch

from oracle import swin_oracle as O
from tests import cpb_reference as R

BLOCK = [pytest.param(g, id=R.case_id(g)) for g in R.BLOCK_CASES]
MULTI = [pytest.param(g, id=R.case_id(g)) for g in R.MULTI_CASES]


def _small(cases, limit=1100):
    return [pytest.param(g, id=R.case_id(g)) for g in cases if (g[0] * g[1]) ** 2 <= limit]


@pytest.mark.parametrize("geom", _small(R.BLOCK_CASES))
def test_reference_agrees_with_the_oracle_and_with_autograd(geom):
    wh, ww, heads, hidden, train = geom
    c = R.make_case(geom, "block")
    r = R.reference(c)
    assert R.within(O.rel_coords_log(wh, ww), r.R, R.C_LOG1P * r.R.abs())[0] == 0
    # eval-mode table of the oracle (fp32 torch matmuls in an order of their own: hidden + 2 roundings of A per element, doubled)
    e = R.make_case(geom, "block", train=False)
    re_ = R.reference(e)
    p = {"a.meta_mlp.fc1.weight": e.w1[0], "a.meta_mlp.fc1.bias": e.b1[0], "a.meta_mlp.fc2.weight": e.w2[0], "a.meta_mlp.fc2.bias": e.b2[0]}
    A = (re_.hidden.abs() @ e.w2[0].double().abs().T + e.b2[0].double().abs()).T
    noise = R.bounds(e, 0, re_, "valu").bias + 2 * (hidden + 2) * R.U * A
    assert R.within(O.cpb_bias(p, "a.", wh, ww, heads, False).reshape(heads, -1), re_.bias, noise)[0] == 0
    # torch autograd of the fp64 formula, with the same keep mask
    ps = [t.double().requires_grad_(True) for t in (c.w1[0], c.b1[0], c.w2[0], c.b2[0])]
    hdn = torch.relu(r.R @ ps[0].T + ps[1]) * r.m
    bias = (hdn @ ps[2].T + ps[3]).T
    assert torch.allclose(bias, r.bias, rtol=1e-13, atol=1e-300)
    bias.backward(r.d)
    auto = torch.cat([t.grad.reshape(-1) for t in ps])
    mag = torch.cat([((r.g.abs().T @ r.R.abs())).reshape(-1), r.g.abs().sum(0), (r.d.abs() @ r.hidden.abs()).reshape(-1), r.d.abs().sum(1)])
    assert bool(((auto - r.con).abs() <= 1e-13 * mag).all())


def _check_emulated(c, forms, blocks):
    exact = c.variant == "exact"
    for b in blocks:
        r = R.reference(c, b)
        if exact:           # every sum an integer below 2^24, so that no order of fp32 additions rounds
            tot = torch.cat([(r.hidden.abs() @ c.w2[b].double().abs().T).reshape(-1), (r.m * (r.d.abs().T @ c.w2[b].double().abs())).sum(0),
                             (r.d.abs() @ r.hidden.abs()).reshape(-1), r.d.abs().sum(1)])
            assert float(tot.max()) + 64 < 2 ** 24
        mf = "mfma" in forms
        bnd = R.bounds(c, b, r, "mfma" if mf else "valu")
        assert bnd.amb_share <= 0.01, (bnd.amb_share, bnd.n_amb)
        wl = {}
        fwd = R.emu_fwd_mfma(c, b) if mf else R.emu_fwd_valu(c, b)
        R.assert_within("bias", fwd, r.bias, bnd.bias, worst=wl)
        part = R.emu_bwd_mfma(c, b) if mf else R.emu_bwd_valu(c, b)
        got = R.emu_fold(part, c.base[b])
        out = [got]
        if not mf:          # the atomics in one of their possible orders: last workgroup first
            acc = c.base[b].clone()
            for row in reversed(range(part.shape[0])):
                acc = acc + part[row]
            R.assert_within("atomics", acc, r.grads, R.bounds(c, b, r, "atomics").grads, worst=wl)
            out.append(acc)
        R.assert_within("grads", got, r.grads, bnd.grads, worst=wl)
        R.assert_within("grads x2", R.emu_fold(part, got), r.grads + r.con, R.second_bound(bnd, r), worst=wl)
        if exact:
            assert torch.equal(fwd.double(), r.bias)
            for o in out:
                gv, rv = R.split_grads(o, c), R.split_grads(r.grads, c)
                assert all(torch.equal(gv[k].double(), rv[k]) for k in ("db1", "dw2", "db2"))


@pytest.mark.parametrize("geom", BLOCK)
def test_valu_emulation_stays_inside_its_bounds(geom):
    _check_emulated(R.make_case(geom, "block"), ("valu",), (0,))
    _check_emulated(R.make_case(geom, "block", "exact", train=False), ("valu",), (0,))
    _check_emulated(R.make_case(geom, "block", "exact", train=True, drop_p=0.5), ("valu",), (0,))
    if geom[4] and (geom[0] * geom[1]) ** 2 <= 4000:
        _check_emulated(R.make_case(geom, "block", keep="values"), ("valu",), (0,))


@pytest.mark.parametrize("geom", MULTI)
def test_mfma_emulation_stays_inside_its_bounds(geom):
    big = (geom[0] * geom[1]) ** 2 > 4000
    c = R.make_case(geom, "multi")
    _check_emulated(c, ("mfma",), (0,) if big else range(c.nblk))
    _check_emulated(R.make_case(geom, "multi", "exact", train=False), ("mfma",), (0,))


@pytest.mark.parametrize("geom", [R.MULTI_CASES[1], R.MULTI_CASES[2]], ids=R.case_id)
@pytest.mark.parametrize("variant", R.KEEP_WORD_VARIANTS)
def test_structured_keep_words(geom, variant):
    from tests.test_gpu_parity import _decode_keep_bits
    hidden = geom[3]
    c = R.make_case(geom, "multi", keep=variant)
    for b in range(c.nblk):
        k = R.decode_keep_words(c.bits[b], hidden)
        assert torch.equal(k, _decode_keep_bits(c.bits[b], hidden))
        if variant in ("zero", "top"):
            assert not bool(k.any())
        elif variant == "all":
            assert bool(k.all())
        else:               # one unit of every word's eight, every unit position in use
            per_word = k.view(c.L2, hidden // 32, 4, 8)
            assert bool((per_word.sum(-1) == 1).all()) and bool(per_word.any(0).any(0).any(0).all())
    _check_emulated(c, ("mfma",), range(c.nblk))


def test_random_keep_words_agree_with_the_older_decode():
    from tests.test_gpu_parity import _decode_keep_bits
    for hidden in (64, 128, 256, 384, 512):
        bits = R.keep_words("random", 37, hidden, torch.Generator().manual_seed(hidden))
        k = R.decode_keep_words(bits, hidden)
        assert torch.equal(k, _decode_keep_bits(bits, hidden)) and 0.8 < float(k.float().mean()) < 0.95
        assert not torch.equal(k, R.decode_keep_words(bits, hidden, natural=True))


def test_actual_low_part_bound_is_sharper_and_holds():
    """dh = d^T w2 at nchunk = 1: both operands are inputs, so the bound from their actual low parts applies"""
    c = R.make_case(R.MULTI_CASES[6], "multi")
    d, w2 = c.dtab[0][0].T.contiguous(), c.w2[0]
    exact = d.double() @ w2.double()
    worst = R.C_SPLIT * (d.double().abs() @ w2.double().abs())
    sharp = R.split_residual(d, w2)
    assert bool((sharp <= worst).all()) and float((sharp / worst.clamp_min(1e-300)).max()) < 0.5
    acc = R.C_MFMA_K16 * R.U * (d.double().abs() @ w2.double().abs())
    assert R.within(R.mfma_chain(d, w2, 16), exact, sharp + acc)[0] == 0
    assert R.within(R.mfma_chain(d, w2, 16, drop="alo"), exact, sharp + acc)[0] > 0


def test_every_checker_fails_at_four_times_its_bound():
    for kind, geom, form in (("block", R.BLOCK_CASES[3], "valu"), ("block", R.BLOCK_CASES[3], "atomics"), ("multi", R.MULTI_CASES[2], "mfma")):
        c = R.make_case(geom, kind)
        r = R.reference(c)
        bnd = R.bounds(c, 0, r, form)
        wl = {}
        ok = r.bias.float()
        R.assert_within("bias", r.bias, r.bias, bnd.bias, worst=wl)
        i = int(bnd.bias.argmax())
        bad = r.bias.clone()
        bad.view(-1)[i] += 4 * bnd.bias.view(-1)[i]
        with pytest.raises(AssertionError):
            R.check_bias("x", bad, r, bnd)
        nan = ok.clone()
        nan.view(-1)[0] = float("nan")
        with pytest.raises(AssertionError):
            R.check_bias("x", nan, r, bnd)
        R.check_grads("x", r.grads, c, r, bnd)
        R.check_grads("x", r.grads + r.con, c, r, bnd, second=True)
        gb = R.split_grads(bnd.grads, c)
        for k in ("dw1", "db1", "dw2", "db2"):
            for second in (False, True):
                bound = R.second_bound(bnd, r) if second else bnd.grads
                ref = r.grads + r.con if second else r.grads
                pert = torch.zeros_like(ref)
                pv, bv = R.split_grads(pert, c)[k], R.split_grads(bound, c)[k]
                j = int(bv.reshape(-1).argmax())
                pv.reshape(-1)[j] = 4 * bv.reshape(-1)[j]
                assert float(pert.abs().max()) > 0 and gb[k].numel() > 0
                with pytest.raises(AssertionError):
                    R.check_grads("x", ref + pert, c, r, bnd, second=second)


# host twin of mutant n -> (table, case index, emulation argument, the outputs its GPU counterpart moves out of bound)
TWINS = {
    1: ("multi", 1, "fwd_alo", ("bias",)),
    2: ("multi", 1, "bwd_adl", ("dw2",)),
    3: ("multi", 1, "widx_fwd", ("bias",)),
    4: ("multi", 2, "keep_bwd", ("dw1", "db1", "dw2")),
    5: ("block", 3, "coord", ("bias", "dw1")),
    6: ("multi", 2, "db1_scale", ("db1",)),
    7: ("block", 3, "gate", ("db1",)),
    8: ("multi", 1, "chunk7", ("dw1", "db1", "dw2", "db2")),
    9: ("block", 3, "fold_tail", ("dw1", "db1", "dw2", "db2")),
}


@pytest.mark.parametrize("n", sorted(TWINS))
def test_host_twin_of_each_mutant_fails_its_checker(n):
    kind, idx, mut, outs = TWINS[n]
    c = R.make_case((R.BLOCK_CASES if kind == "block" else R.MULTI_CASES)[idx], kind)
    mf = kind == "multi"
    r = R.reference(c)
    bnd = R.bounds(c, 0, r, "mfma" if mf else "valu")
    fwd = (R.emu_fwd_mfma if mf else R.emu_fwd_valu)(c, 0, mut)
    part = (R.emu_bwd_mfma if mf else R.emu_bwd_valu)(c, 0, mut)
    got = R.emu_fold(part, c.base[0], mut)
    failed = set()
    if R.within(fwd, r.bias, bnd.bias)[0]:
        failed.add("bias")
    gv, rv, bv = R.split_grads(got, c), R.split_grads(r.grads, c), R.split_grads(bnd.grads, c)
    failed |= {k for k in gv if R.within(gv[k], rv[k], bv[k])[0]}
    assert set(outs) <= failed, (n, mut, failed)
    if n == 7:              # the gate mutant on the MFMA form as well (cpb_bwd_mfma_kernel carries the same comparison)
        c = R.make_case(R.MULTI_CASES[2], "multi")
        r = R.reference(c)
        bnd = R.bounds(c, 0, r, "mfma")
        got = R.split_grads(R.emu_fold(R.emu_bwd_mfma(c, 0, mut), c.base[0]), c)
        assert R.within(got["db1"], R.split_grads(r.grads, c)["db1"], R.split_grads(bnd.grads, c)["db1"])[0] > 0
