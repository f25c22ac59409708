"""GPU (-m gpu): the continuous-position-bias kernels of csrc/cpb.hip element by element against fp64: swv2_cpb_fwd, swv2_cpb_bwd (float
atomics), swv2_cpb_bwd_ws with cpb_fold_kernel, swv2_cpb_fwd_multi, swv2_cpb_bwd_multi with cpb_fold_multi_kernel.

The case tables (each row names the code path it exists for), the fp64 reference, the bounds and their derivations are in
tests/cpb_reference.py (checked without a GPU by tests/test_cpb_exact_host.py, which also holds the host twins of the kernel mutants).
For every case:
  * every output lies in a guarded buffer (mlp_reference.Guarded) whose guard rows must be intact; `bias` is prefilled with NaN and must
    come back finite everywhere; the gradients start from a random baseline; the workspace is the test's own, of exactly
    swv2_cpb_bwd_ws_bytes / swv2_cpb_bwd_multi_ws_bytes, guarded and prefilled with NaN (the C ABI is called directly, not through
    ops._scratch): a partial-row entry the fold reads before it is written surfaces as NaN in a gradient;
  * parameters, keep data and d bias tables are compared with copies after the launches;
  * each launch runs twice and the two runs agree bit for bit; the atomics backward is held to its bound on both runs instead;
  * a second backward onto the first result equals base + 2 x contribution within the bound.
Part 1 (exact): w1 = 0 and small integers, every sum an integer below 2^24: bias, db1, dw2, db2 equal fp64 (torch.equal; db2 is the sum
over pairs of the chunk sums, so it pins those), dw1 keeps its bound.  Per-block kernels in eval and in train at drop_p 0.5 (s = 2), multi
kernels in eval.  Part 2 (random): log-uniform per-head and per-unit scales, b1 = 0 on a few units and two zero w1 rows (pre == 0: the
closed gate), the derived bounds.  Keep data: structured keep words on the second and third multi row (0; 0x00FFFFFF; the top byte only;
one bit per word cycling through bytes, units and pairs), the three bf16 keep values 1.140625 / 1.0 / the smallest positive mixed.

Worst |err| / bound measured on an MI355X over every case of this file (the `[cpb worst |err| / bound]` line printed under -s; records,
not bars: every bound is derived in cpb_reference.py, none is fitted to these figures, and none was changed after the run).  The MFMA
bounds hold a representation term (2^-13 sum |x| |y|, the hi + lo split); "beyond rounding" is (|err| - that term) / (bound - that term),
0 where the error stays inside the representation term alone.  The VALU kernels' bounds have no such term.
  kernel              bias    dw1     db1     dw2     db2       second backward (dw1 db1 dw2 db2)      atomics (dw1 db1 dw2 db2)
  cpb_*_kernel<4>     0.144   0.247   0.069   0.244   0.0084    0.246  0.068  0.244  0.0083            0.247  0.069  0.244  0.0084
  cpb_*_kernel<8>     0.097   0.013   0.0089  0.139   0.0055    0.012  0.014  0.139  0.0056            0.014  0.0092 0.115  0.0055
  cpb_*_kernel<16>    0.063   0.011   0.011   0.128   0.0061    0.0092 0.0066 0.128  0.0065            0.011  0.011  0.111  0.0061
  cpb_*_kernel<32>    0.111   0.037   0.033   0.364   0.0087    0.040  0.034  0.364  0.0086            0.037  0.033  0.364  0.0087
  mfma, hidden 64     0.281   0.133   0.228   0.385   0.028     as the first                           beyond rounding: dw2 0.074, else 0
  mfma, hidden 128    0.291   0.256   0.150   0.229   0.0054    as the first                           beyond rounding: 0
  mfma, hidden 256    0.119   0.233   0.233   0.109   0.0051    as the first                           beyond rounding: 0
  mfma, hidden 384    0.101   0.035   0.029   0.085   0.0029    as the first                           beyond rounding: 0
  mfma, hidden 512    0.078   0.089   0.084   0.065   0.0004    as the first                           beyond rounding: 0
The host emulation of the same cases gives the same picture (dw2 0.23 at 3 x 3 x 32 x 512 and 2 x 2 x 4 x 32, the production window's
largest 0.029 (VALU) and 0.10 (MFMA), both on bias).  All 62 tests passed on the first run of the
library as it stands; no kernel changed.  The mutants these tests were run against: LABNOTES.md ("The CPB kernels element by element").
"""
import pytest
import torch

from tests import cpb_reference as R
from tests import mlp_reference as MR

pytestmark = pytest.mark.gpu

NAN = float("nan")
BLOCK = [pytest.param(g, id=R.case_id(g)) for g in R.BLOCK_CASES]
MULTI = [pytest.param(g, id=R.case_id(g)) for g in R.MULTI_CASES]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def K():
    from swin_v2_weather_amd import _lib as L
    lib = L.load()
    yield dict(L=L, lib=lib)
    # (shown with -s) the worst |err| / bound of every output per kernel family over the cases that ran
    print("\n[cpb worst |err| / bound] " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(R.WORST.items())))


def _p(t):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _guarded(shape, dev, fill):
    g = MR.Guarded(shape, torch.float32, dev)
    if torch.is_tensor(fill):
        g.t.copy_(fill)
    else:
        g.t.fill_(fill)
    return g


class _Inputs:
    """copies of every input of a case; same() after the launches"""

    def __init__(self, tensors):
        self.live = [t for t in tensors if t is not None]
        self.copies = [t.clone() for t in self.live]

    def same(self):
        return all(torch.equal(a.view(torch.uint8) if a.dtype == R.BF else a, b.view(torch.uint8) if b.dtype == R.BF else b)
                   for a, b in zip(self.live, self.copies))


def run_block(K, dev, c0):
    lib, c = K["lib"], R.case_to(c0, dev)
    wh, ww, heads, Hd = c.wh, c.ww, c.heads, c.hidden
    exact = c.variant == "exact"
    name = f"block<{R.heads_max(heads)}>"
    what = f"{R.case_id((wh, ww, heads, Hd))} {c.variant} {'train' if c.train else 'eval'}"
    r = R.reference(c)
    bv, ba = R.bounds(c, 0, r, "valu"), R.bounds(c, 0, r, "atomics")
    w1, b1, w2, b2, keep, dbias, base = c.w1[0], c.b1[0], c.w2[0], c.b2[0], c.keep_bf16, c.dtab[0][0].contiguous(), c.base[0]
    inp = _Inputs([w1, b1, w2, b2, keep, dbias])
    # forward, twice
    outs = []
    for _ in range(2):
        gb = _guarded((heads, c.L2), dev, NAN)
        assert lib.swv2_cpb_fwd(_p(w1), _p(b1), _p(w2), _p(b2), _p(keep), _p(gb.t), wh, ww, heads, Hd, c.drop_arg, _stream()) == 0
        torch.cuda.synchronize()
        assert gb.intact(), what
        outs.append(gb.t.clone())
    assert torch.equal(outs[0], outs[1]), what
    R.check_bias(name + " fwd", outs[0], r, bv, what, exact=exact)
    # backward with the test's own workspace, twice from the baseline and once more onto the result
    nb = lib.swv2_cpb_bwd_ws_bytes(wh, ww, heads, Hd)
    assert nb == c.rows * c.n * 4

    def bwd(gg, ws, nbytes):
        v = R.split_grads(gg.t, c)
        if ws is None:
            return lib.swv2_cpb_bwd(_p(dbias), _p(w1), _p(b1), _p(w2), _p(keep), _p(v["dw1"]), _p(v["db1"]), _p(v["dw2"]), _p(v["db2"]),
                                    wh, ww, heads, Hd, c.drop_arg, _stream())
        return lib.swv2_cpb_bwd_ws(_p(dbias), _p(w1), _p(b1), _p(w2), _p(keep), _p(v["dw1"]), _p(v["db1"]), _p(v["dw2"]), _p(v["db2"]),
                                   wh, ww, heads, Hd, c.drop_arg, _p(ws.t), nbytes, _stream())

    res = []
    for _ in range(2):
        gg, ws = _guarded((c.n,), dev, base), _guarded((nb // 4,), dev, NAN)
        assert bwd(gg, ws, nb) == 0
        torch.cuda.synchronize()
        assert gg.intact() and ws.intact(), what
        assert bool(torch.isfinite(ws.t).all()), f"{what}: a partial-row entry was never written"
        res.append(gg.t.clone())
    assert torch.equal(res[0], res[1]), what
    R.check_grads(name + " ws", res[0], c, r, bv, what, exact=exact)
    ws = _guarded((nb // 4,), dev, NAN)
    assert bwd(gg, ws, nb) == 0
    torch.cuda.synchronize()
    assert gg.intact() and ws.intact(), what
    R.check_grads(name + " ws", gg.t, c, r, bv, what, second=True)
    # a workspace one byte short: an error, nothing written
    gg, ws = _guarded((c.n,), dev, base), _guarded((nb // 4,), dev, NAN)
    assert bwd(gg, ws, nb - 1) != 0
    torch.cuda.synchronize()
    assert torch.equal(gg.t, base) and bool(torch.isnan(ws.t).all()) and gg.intact() and ws.intact(), what
    # float atomics: held to the bound on both runs
    for _ in range(2):
        gg = _guarded((c.n,), dev, base)
        assert bwd(gg, None, 0) == 0
        torch.cuda.synchronize()
        assert gg.intact(), what
        R.check_grads(name + " atomics", gg.t, c, r, ba, what, exact=exact)
    assert inp.same(), f"{what}: an input was written"


def run_multi(K, dev, c0):
    lib, c = K["lib"], R.case_to(c0, dev)
    wh, ww, heads, Hd, nblk, nchunk = c.wh, c.ww, c.heads, c.hidden, c.nblk, c.nchunk
    exact = c.variant == "exact"
    name = f"multi JT{Hd // 64}"
    what = f"{R.case_id((wh, ww, heads, Hd, nchunk, nblk))} {c.variant} {'train' if c.train else 'eval'}"
    params = [t for b in range(nblk) for t in (c.w1[b], c.b1[b], c.w2[b], c.b2[b])]
    ptab = torch.tensor([t.data_ptr() for t in params], dtype=torch.int64).to(dev)
    dtab = torch.stack(c.dtab).contiguous()
    base = torch.stack(c.base).contiguous()
    inp = _Inputs(params + [ptab, c.bits, dtab])
    refs = [R.reference(c, b) for b in range(nblk)]
    bnds = [R.bounds(c, b, refs[b], "mfma") for b in range(nblk)]
    outs = []
    for _ in range(2):
        gb = _guarded((nblk * heads, c.L2), dev, NAN)
        assert lib.swv2_cpb_fwd_multi(_p(ptab), nblk, _p(c.bits), _p(gb.t), wh, ww, heads, Hd, c.drop_arg, _stream()) == 0
        torch.cuda.synchronize()
        assert gb.intact(), what
        outs.append(gb.t.clone().view(nblk, heads, c.L2))
    assert torch.equal(outs[0], outs[1]), what
    for b in range(nblk):
        R.check_bias(name + " fwd", outs[0][b], refs[b], bnds[b], f"{what} block {b}", exact=exact)
    nb = lib.swv2_cpb_bwd_multi_ws_bytes(nblk, wh, ww, heads, Hd)
    assert nb == nblk * c.rows * c.n * 4

    def bwd(gg, ws):
        rc = lib.swv2_cpb_bwd_multi(_p(dtab), nchunk, _p(ptab), nblk, _p(c.bits), _p(gg.t), wh, ww, heads, Hd, c.drop_arg, _p(ws.t), nb, _stream())
        torch.cuda.synchronize()
        assert rc == 0 and gg.intact() and ws.intact(), what
        assert bool(torch.isfinite(ws.t).all()), f"{what}: a partial-row entry was never written"

    res = []
    for _ in range(2):
        gg = _guarded((nblk, c.n), dev, base)
        bwd(gg, _guarded((nb // 4,), dev, NAN))
        res.append(gg.t.clone())
    assert torch.equal(res[0], res[1]), what
    bwd(gg, _guarded((nb // 4,), dev, NAN))
    for b in range(nblk):
        R.check_grads(name + " bwd", res[0][b], c, refs[b], bnds[b], f"{what} block {b}", exact=exact)
        R.check_grads(name + " bwd", gg.t[b], c, refs[b], bnds[b], f"{what} block {b}", second=True)
    assert inp.same(), f"{what}: an input was written"


@pytest.mark.parametrize("geom", BLOCK)
def test_block_kernels_random(dev, K, geom):
    run_block(K, dev, R.make_case(geom, "block"))


@pytest.mark.parametrize("train", [False, True], ids=["eval", "train0.5"])
@pytest.mark.parametrize("geom", BLOCK)
def test_block_kernels_exact(dev, K, geom, train):
    run_block(K, dev, R.make_case(geom, "block", "exact", train=train, drop_p=0.5 if train else 0.125))


@pytest.mark.parametrize("geom", [g for g in BLOCK if g.values[0][4] and (g.values[0][0] * g.values[0][1]) ** 2 <= 4000])
def test_block_kernels_keep_values(dev, K, geom):
    """any non-zero bf16 = keep: 1.140625, 1.0 and the smallest positive bf16, mixed"""
    run_block(K, dev, R.make_case(geom, "block", keep="values", seed=1))


@pytest.mark.parametrize("geom", MULTI)
def test_multi_kernels_random(dev, K, geom):
    run_multi(K, dev, R.make_case(geom, "multi"))


@pytest.mark.parametrize("geom", MULTI)
def test_multi_kernels_exact(dev, K, geom):
    run_multi(K, dev, R.make_case(geom, "multi", "exact", train=False))


@pytest.mark.parametrize("variant", R.KEEP_WORD_VARIANTS)
@pytest.mark.parametrize("geom", [MULTI[1], MULTI[2]])
def test_multi_kernels_structured_keep_words(dev, K, geom, variant):
    """the forward table and all four gradients against the reference that decodes the same words by the header's formula"""
    run_multi(K, dev, R.make_case(geom, "multi", keep=variant))


def test_multi_entry_points_refuse_what_they_do_not_cover(dev, K):
    """hidden 96, heads 17 and drop_p 0.1 are errors of swv2_cpb_fwd_multi / _bwd_multi, and nothing is written"""
    lib = K["lib"]
    for heads, hidden, drop in ((4, 96, 0.125), (17, 64, 0.125), (4, 64, 0.1)):
        c = R.case_to(R.make_case((2, 2, heads, 128 if hidden == 96 else hidden, True, 1, 1), "multi"), dev)
        ptab = torch.tensor([t.data_ptr() for t in (c.w1[0], c.b1[0], c.w2[0], c.b2[0])], dtype=torch.int64).to(dev)
        gb = _guarded((heads, c.L2), dev, NAN)
        gg = _guarded((1, c.n), dev, c.base[0])
        ws = _guarded((c.rows * c.n,), dev, NAN)
        assert lib.swv2_cpb_fwd_multi(_p(ptab), 1, _p(c.bits), _p(gb.t), 2, 2, heads, hidden, drop, _stream()) != 0
        assert lib.swv2_cpb_bwd_multi(_p(c.dtab[0]), 1, _p(ptab), 1, _p(c.bits), _p(gg.t), 2, 2, heads, hidden, drop, _p(ws.t), c.rows * c.n * 4,
                                      _stream()) != 0
        torch.cuda.synchronize()
        assert bool(torch.isnan(gb.t).all()) and bool(torch.isnan(ws.t).all()) and torch.equal(gg.t[0], c.base[0])
        assert gb.intact() and gg.intact() and ws.intact()
