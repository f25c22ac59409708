"""GPU (-m gpu): swv2_batch_sum, swv2_merge_ln_bwd (csrc/rowops.hip) and swv2_loss_finalize (csrc/loss_l2.hip) through the C ABI, element by
element against the fp64 statements of tests/rows_reference.py, whose docstring derives every bound used here.  Every output sits between
guards (tests/plane_harness.py::Guarded), outputs that are written and not accumulated start as NaN, accumulated ones from a baseline, and
every launch is repeated: deterministic outputs must come back with the same bits, atomically accumulated ones within their bound again.
Each case prints its worst error / bound per output (-s); the figures are records of one MI355X run (LABNOTES, "Adam and the remaining row
kernels element by element"), asserted nowhere:
    swv2_merge_ln_bwd   dx 0.509  dgamma 0.332  dbeta 0.248  (largest over the six shapes and both runs; dgamma moves with the atomics' arrival order)
    swv2_loss_finalize  loss 0.104  coef 0.423             (largest over shapes, layers and the four variants)
Only 16-byte-aligned pointers are passed: swv2_batch_sum does not check alignment, and these tests do not probe that."""
import numpy as np
import pytest
import torch

from swin_v2_weather_amd import _lib as L
from tests import rows_reference as R
from tests.plane_harness import Guarded, dev, lib  # noqa: F401  (dev, lib: fixtures)

pytestmark = pytest.mark.gpu


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _bits(t):
    return t.cpu().numpy().view(np.int32)


# ---------------------------------------------------------------------------------------------------------------
# swv2_batch_sum
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,n", [(1, 4), (3, 4 * 257), (2, 6 * 10 * 24), (2, R.BATCH_SUM_CAP + 4 * 257)],
                         ids=["1x4", "3x1028", "2xgrid6x10xC24", "2xbeyond_the_grid_cap"])
def test_batch_sum_bit_for_bit(dev, lib, B, n):
    """fp32 additions in the order baseline, b = 0 .. B - 1: numpy's bits.  accumulate = 0 lands on a NaN-filled out and must not read it;
    accumulate = 1 lands on a random baseline.  The last case runs 4 * 257 elements past what one pass of the capped grid covers
    (67 MB in, 34 MB out)."""
    rng = np.random.default_rng(B * 31 + n % 1009)
    inp = rng.standard_normal((B, n), dtype=np.float32)
    base = rng.standard_normal(n, dtype=np.float32)
    for accumulate in (0, 1):
        want = R.batch_sum(inp, base if accumulate else None)
        runs = []
        for _ in range(2):
            g = Guarded(dev, inp=B * n, out=n)
            g["inp"].copy_(torch.from_numpy(inp.reshape(-1)))
            g["out"].copy_(torch.from_numpy(base)) if accumulate else g["out"].fill_(float("nan"))
            assert g["inp"].data_ptr() % 16 == 0 and g["out"].data_ptr() % 16 == 0
            L.check(lib.swv2_batch_sum(g["inp"].data_ptr(), g["out"].data_ptr(), B, n, accumulate, _stream()), "swv2_batch_sum")
            torch.cuda.synchronize()
            assert g.guards_intact(), "a guard was written"
            assert np.array_equal(_bits(g["inp"]), inp.reshape(-1).view(np.int32)), "the input was written"
            got = g["out"].cpu().numpy()
            assert not np.isnan(got).any(), "out was read (or left unwritten) with accumulate = 0" if not accumulate else "NaN"
            assert np.array_equal(got.view(np.int32), want.view(np.int32)), "not the fp32 sum in the order baseline, b = 0 .. B - 1"
            runs.append(got)
        assert np.array_equal(runs[0].view(np.int32), runs[1].view(np.int32))


def test_batch_sum_refuses_n_not_a_multiple_of_4(dev, lib):
    g = Guarded(dev, inp=16, out=8)
    before = g.raw.clone()
    for n in (1, 2, 3, 5, 6, 7):
        assert lib.swv2_batch_sum(g["inp"].data_ptr(), g["out"].data_ptr(), 2, n, 0, _stream()) == -1
        assert b"batch_sum: bad argument (n must be a multiple of 4)" in lib.swv2_last_error()
    torch.cuda.synchronize()
    assert torch.equal(g.raw, before), "a refused call wrote"


# ---------------------------------------------------------------------------------------------------------------
# swv2_merge_ln_bwd
# ---------------------------------------------------------------------------------------------------------------
def _merge_run(dev, lib, shape, c, stats):
    """one launch into fresh guarded outputs -> (Guarded, mean, rstd as numpy); stats: None = swv2_merge_stats on the same x (as the module
    does), else the caller's (mean, rstd)"""
    B, H, W, C = shape
    M, K = B * (H // 2) * (W // 2), 4 * C
    x, g = torch.from_numpy(c["x"]).to(dev), torch.from_numpy(c["gamma"]).to(dev)
    dn = torch.from_numpy(c["dn_bits"].view(np.int16)).to(dev)
    if stats is None:
        mean, rstd = torch.empty(M, device=dev), torch.empty(M, device=dev)
        L.check(lib.swv2_merge_stats(x.data_ptr(), mean.data_ptr(), rstd.data_ptr(), B, H, W, C, 1e-5, _stream()), "swv2_merge_stats")
    else:
        mean, rstd = (torch.from_numpy(s).to(dev) for s in stats)
    out = Guarded(dev, dx=B * H * W * C, dgamma=K, dbeta=K)
    out["dx"].fill_(float("nan"))
    out["dgamma"].copy_(torch.from_numpy(c["base_g"]))
    out["dbeta"].copy_(torch.from_numpy(c["base_b"]))
    L.check(lib.swv2_merge_ln_bwd(x.data_ptr(), dn.data_ptr(), g.data_ptr(), mean.data_ptr(), rstd.data_ptr(), out["dx"].data_ptr(),
                                  out["dgamma"].data_ptr(), out["dbeta"].data_ptr(), B, H, W, C, _stream()), "swv2_merge_ln_bwd")
    torch.cuda.synchronize()
    assert out.guards_intact(), "a guard was written"
    return out, mean.cpu().numpy(), rstd.cpu().numpy()


@pytest.mark.parametrize("shape", R.MERGE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_merge_ln_bwd_against_fp64(dev, lib, shape):
    """4 C = 32 leaves half the lanes idle and M = 15 is no multiple of the 4 rows of a workgroup; 4 C = 96 is ragged over the lanes;
    M = 16 512 runs 128 rows past what one pass of the capped grid covers.  dx starts as NaN and must be finite everywhere; dgamma /
    dbeta start from a baseline and must end at baseline + sum within the atomics' bound, on both runs; dx comes back with the same bits."""
    c = R.merge_inputs(shape)
    runs = [_merge_run(dev, lib, shape, c, None) for _ in range(2)]
    out, mean, rstd = runs[0]
    assert np.array_equal(mean.view(np.int32), runs[1][1].view(np.int32)) and np.array_equal(rstd.view(np.int32), runs[1][2].view(np.int32))
    ref, bnd = R.merge_ln_bwd(c["x"], c["dn"], c["gamma"], mean, rstd, c["base_g"], c["base_b"])
    worst = {}
    for o, _, _ in runs:
        dx = o["dx"].cpu().numpy().reshape(shape)
        assert np.isfinite(dx).all(), "%d elements of dx were not written" % int((~np.isfinite(dx)).sum())
        for k, got, r, e in zip(("dx", "dgamma", "dbeta"), (dx, o["dgamma"].cpu().numpy(), o["dbeta"].cpu().numpy()), ref, bnd):
            worst[k] = max(worst.get(k, 0.0), R.ratio(got - r, e))
    print("merge_ln_bwd worst error/bound  %-16s " % (shape,) + "  ".join("%s %.3f" % kv for kv in sorted(worst.items())))
    assert all(val <= 1.0 for val in worst.values()), worst
    assert np.array_equal(_bits(runs[0][0]["dx"]), _bits(runs[1][0]["dx"])), "dx differs between two runs"


def test_merge_ln_bwd_integer_case_is_exact(dev, lib):
    """C = 16, K = 64: x, dn, gamma small integers, the caller's mean = 0, rstd = 1.  x^ = x and gg = dn gamma are integers; each lane
    holds one term and the wave adds integers far below 2^24 (exact); / 64 is a power of two, so s1, s2 are multiples of 1/64; x s2 and the
    two subtractions stay multiples of 1/64 of a few bits, the product with rstd = 1 is exact; dgamma and dbeta are integer sums, exact in
    any arrival order.  Every output equals the fp64 statement."""
    shape = (2, 8, 12, 16)
    c = R.merge_inputs(shape, integer=True)
    M = c["dn"].shape[0]
    stats = (np.zeros(M, np.float32), np.ones(M, np.float32))
    out, _, _ = _merge_run(dev, lib, shape, c, stats)
    ref, _ = R.merge_ln_bwd(c["x"], c["dn"], c["gamma"], *stats, c["base_g"], c["base_b"])
    assert np.array_equal(out["dx"].cpu().numpy().reshape(shape).astype(np.float64), ref[0])
    assert np.array_equal(out["dgamma"].cpu().numpy().astype(np.float64), ref[1])
    assert np.array_equal(out["dbeta"].cpu().numpy().astype(np.float64), ref[2])
    assert np.abs(ref[0]).max() > 1 and not np.array_equal(ref[1], R.d(c["base_g"]))


# ---------------------------------------------------------------------------------------------------------------
# swv2_loss_finalize
# ---------------------------------------------------------------------------------------------------------------
def _finalize_run(dev, lib, sums, chw, absolute, squared):
    layers, BC, _ = sums.shape
    s, w = torch.from_numpy(sums).to(dev), torch.from_numpy(chw).to(dev)
    out = Guarded(dev, loss=1, coef=BC)
    L.check(lib.swv2_loss_finalize(s.data_ptr(), layers, w.data_ptr(), BC, chw.size, absolute, squared, out["loss"].data_ptr(),
                                   out["coef"].data_ptr(), _stream()), "swv2_loss_finalize")
    torch.cuda.synchronize()
    assert out.guards_intact(), "a guard was written"
    assert out.written("loss") and out.written("coef"), "an output slot was left unwritten"
    return out


@pytest.mark.parametrize("layers", [1, R.LOSS_PART_SLICES])
@pytest.mark.parametrize("shape", R.FINALIZE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_loss_finalize_against_fp64(dev, lib, shape, layers):
    """the loss and every coef[i] of the four (absolute, squared) variants; B C = 584 walks i % C across three trips of the 256 threads"""
    sums, chw = R.finalize_inputs(*shape, layers)
    for absolute, squared in R.VARIANTS:
        out = _finalize_run(dev, lib, sums, chw, absolute, squared)
        ref, bl, cref, bc = R.loss_finalize(sums, chw, absolute, squared)
        w = dict(loss=R.ratio(float(out["loss"].cpu()[0]) - ref, bl), coef=R.ratio(out["coef"].cpu().numpy() - cref, bc))
        print("loss_finalize worst error/bound  %-9s layers %d absolute %d squared %d  " % (shape, layers, absolute, squared) +
              "  ".join("%s %.3f" % kv for kv in sorted(w.items())))
        assert all(val <= 1.0 for val in w.values()), (shape, layers, absolute, squared, w)
        again = _finalize_run(dev, lib, sums, chw, absolute, squared)
        assert torch.equal(out.raw, again.raw), "a second run differs"


def test_loss_finalize_on_a_plane_without_error(dev, lib):
    """S0 = 0 on plane 80 of 2 x 73 (every layer).  Squared variants: coef finite, the plane adds 0.  sqrt variants: coef = +-inf with the
    sign of the channel weight -- the class (inf, not NaN) and sign autograd gives for the plain-torch l2 statement of utils/losses.py on
    prd == tar, where d sqrt(r) / d r at r = 0 is inf; the loss stays finite and every other plane within its bound."""
    sums, chw = R.finalize_inputs(2, 73, R.LOSS_PART_SLICES, zero_plane=80)
    for absolute, squared in R.VARIANTS:
        out = _finalize_run(dev, lib, sums, chw, absolute, squared)
        loss, coef = float(out["loss"].cpu()[0]), out["coef"].cpu().numpy()
        ref, bl, cref, bc = R.loss_finalize(sums, chw, absolute, squared)
        auto = R.torch_l2_coef(sums, chw, absolute, squared)
        ok = np.isfinite(cref)
        assert np.isfinite(loss) and R.ratio(loss - ref, bl) <= 1.0 and R.ratio(coef[ok] - cref[ok], bc[ok]) <= 1.0
        if squared:
            assert ok.all() and np.isfinite(coef[80]) and np.isfinite(auto[80])
        else:
            assert ok.sum() == 2 * 73 - 1 and np.isinf(coef[80]) and np.isinf(auto[80])
            assert np.sign(coef[80]) == np.sign(auto[80]) == np.sign(chw[80 % 73])
        assert torch.equal(out.raw, _finalize_run(dev, lib, sums, chw, absolute, squared).raw)
