"""CPU: fp32 numpy twins of swv2_batch_sum, swv2_merge_ln_bwd and swv2_loss_finalize inside the bounds of tests/rows_reference.py on the GPU
test's own inputs, seven defective twins outside them, the argument tuples ops.batch_sum / ops.merge_ln_bwd / ops.loss_finalize hand to the
C ABI, and the refusals that need no GPU -- no GPU call."""
import numpy as np
import pytest
import torch

from swin_v2_weather_amd import _lib as L
from tests import rows_reference as R

F = np.float32


def fma(a, b, c):
    return (R.d(a) * R.d(b) + R.d(c)).astype(np.float32)


def wave_sum(v):
    """common.h: v += __shfl_xor(v, o) for o = 32 .. 1 over the last axis of 64 lanes -> every lane's total"""
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[..., lanes ^ o]
    assert v.dtype == np.float32
    return v


def lane_chunks(a, width):
    """[M][K] -> [n][M][width]: element k sits in trip k // width of lane k % width; zeros where a lane has no term"""
    M, K = a.shape
    n = -(-K // width)
    pad = np.zeros((M, n * width), np.float32)
    pad[:, :K] = a
    return pad.reshape(M, n, width).transpose(1, 0, 2)


# ---------------------------------------------------------------------------------------------------------------
# the twins
# ---------------------------------------------------------------------------------------------------------------
def twin_batch_sum(inp, out, accumulate, defect=None):
    start = out.copy() if (accumulate or defect == "reads_out_when_not_accumulating") else np.zeros_like(out)
    for b in range(inp.shape[0]):
        start = start + inp[b]
    return start


def twin_stats(x, eps=F(1e-5)):
    """fp32 mean / rstd per merged row (any fp32 values would do: the statement takes them as stored)"""
    xr = R.rows_of(x)
    K = F(xr.shape[1])
    mu = xr.sum(1, dtype=np.float32) / K
    var = np.maximum((xr * xr).sum(1, dtype=np.float32) / K - mu * mu, F(0))
    return mu, (F(1) / np.sqrt(var + eps)).astype(np.float32)


SWAPPED = ((0, 0), (0, 1), (1, 0), (1, 1))          # the hp / wp bits of a block exchanged


def twin_merge_ln_bwd(x, dn, g, mean, rstd, base_g, base_b, defect=None):
    order = SWAPPED if defect == "gather_bits_swapped" else R.MERGE_ORDER
    xr = R.rows_of(x, order)
    M, K = xr.shape
    mu, rs = mean.reshape(-1, 1), rstd.reshape(-1, 1)
    xh = (xr - mu) * rs
    gg = dn * g
    s1, s2 = np.zeros((M, 64), np.float32), np.zeros((M, 64), np.float32)
    for a, b in zip(lane_chunks(gg, 64), lane_chunks(xh, 64)):
        s1 = s1 + a
        s2 = fma(a, b, s2)
    s1 = wave_sum(s1)[:, :1] / F(K)
    s2 = wave_sum(s2)[:, :1] / F(K // 4 if defect == "s2_over_C" else K)
    dx = rs * (gg - s1 - xh * s2)
    zero = np.zeros((1, K), np.float32)
    first = zero if defect == "dgamma_overwritten" else base_g.reshape(1, K)
    dg = np.cumsum(np.concatenate([first, dn * xh]), axis=0, dtype=np.float32)[-1]        # arrival order m = 0 .. M - 1, one of many
    db = np.cumsum(np.concatenate([base_b.reshape(1, K), dn]), axis=0, dtype=np.float32)[-1]
    assert dx.dtype == dg.dtype == db.dtype == np.float32
    return R.scatter_rows(dx, x.shape, order), dg, db


def twin_loss_finalize(sums, chw, absolute, squared, defect=None):
    layers, BC, _ = sums.shape
    s0, s1 = np.zeros(BC, np.float32), np.zeros(BC, np.float32)
    for l in range(layers):
        s0 = s0 + sums[l, :, 0]
        if l == 0 or defect != "layers_for_S0_only":
            s1 = s1 + sums[l, :, 1]
    if defect == "chw_without_modulo":              # chw[i]: whatever follows the C weights (here: zeros)
        w = np.concatenate([chw, np.zeros(max(BC - chw.size, 0), np.float32)])[:BC]
    else:
        w = chw[np.arange(BC) % chw.size]
    den = np.ones(BC, np.float32) if absolute else s1
    with np.errstate(divide="ignore", invalid="ignore"):
        r = s0 / den
        f, df = (r, np.ones(BC, np.float32)) if squared else (np.sqrt(r), F(0.5) / np.sqrt(r))
        coef = (F(1) if defect == "coef_without_2" else F(2)) * w * df / den
    acc = np.zeros((1, 256), np.float32)
    for t in lane_chunks((w * f).reshape(1, BC), 256):
        acc = acc + t
    red = wave_sum(acc.reshape(4, 64))[:, 0]
    loss = (red[0] + red[1]) + (red[2] + red[3])
    assert coef.dtype == np.float32 and loss.dtype == np.float32
    return loss, coef


# ---------------------------------------------------------------------------------------------------------------
# batch sum
# ---------------------------------------------------------------------------------------------------------------
def test_batch_sum_statement_and_the_twin_that_reads_out():
    rng = np.random.default_rng(0)
    for B, n in ((1, 4), (3, 4 * 257), (2, 6 * 10 * 24)):
        inp = rng.standard_normal((B, n)).astype(np.float32)
        base = rng.standard_normal(n).astype(np.float32)
        nan = np.full(n, np.nan, np.float32)
        for acc, out in ((0, nan), (1, base)):
            want = R.batch_sum(inp, base if acc else None)
            assert np.array_equal(twin_batch_sum(inp, out, acc).view(np.int32), want.view(np.int32))
            exact = R.d(inp).sum(0) + (R.d(base) if acc else 0.0)
            assert np.all(np.abs(want - exact) <= R.gamma(B) * (np.abs(R.d(inp)).sum(0) + np.abs(R.d(base)) * acc))
        bad = twin_batch_sum(inp, nan, 0, "reads_out_when_not_accumulating")
        assert np.all(np.isnan(bad)) and not np.array_equal(bad.view(np.int32), R.batch_sum(inp).view(np.int32))


# ---------------------------------------------------------------------------------------------------------------
# merge backward
# ---------------------------------------------------------------------------------------------------------------
def _merge_ratios(shape, defect=None, integer=False):
    c = R.merge_inputs(shape, integer)
    M = c["dn"].shape[0]
    mean, rstd = (np.zeros(M, np.float32), np.ones(M, np.float32)) if integer else twin_stats(c["x"])
    args = (c["x"], c["dn"], c["gamma"], mean, rstd, c["base_g"], c["base_b"])
    got = twin_merge_ln_bwd(*args, defect=defect)
    ref, bnd = R.merge_ln_bwd(*args)
    return {k: R.ratio(a - b, e) for k, a, b, e in zip(("dx", "dgamma", "dbeta"), got, ref, bnd)}, got, ref


@pytest.mark.parametrize("shape", R.MERGE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_merge_ln_bwd_twin_inside_the_bounds(shape):
    w, _, _ = _merge_ratios(shape)
    print("merge_ln_bwd twin worst error/bound  %-16s " % (shape,) + "  ".join("%s %.3f" % kv for kv in sorted(w.items())))
    assert all(val <= 1.0 for val in w.values()), w


@pytest.mark.parametrize("defect,output", [("gather_bits_swapped", "dx"), ("s2_over_C", "dx"), ("dgamma_overwritten", "dgamma")])
@pytest.mark.parametrize("shape", R.MERGE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_merge_ln_bwd_defective_twins_outside_the_bounds(shape, defect, output):
    w, _, _ = _merge_ratios(shape, defect)
    print("merge_ln_bwd defective twin  %-20s %-16s " % (defect, shape) + "  ".join("%s %.3g" % kv for kv in sorted(w.items())))
    assert w[output] > 1.0, (defect, shape, w)


def test_merge_ln_bwd_integer_case_is_exact():
    """C = 16, K = 64: x, dn, gamma small integers, mean 0, rstd 1.  x^ = x and gg = dn gamma are integers; each lane holds one term and the
    wave adds integers below 2^24 (exact); / 64 is a power of two, so s1, s2 are multiples of 1/64; x s2 and the two subtractions stay
    multiples of 1/64 of a few bits; dgamma, dbeta are integer sums in any order."""
    w, got, ref = _merge_ratios((2, 8, 12, 16), integer=True)
    for a, b in zip(got, ref):
        assert np.array_equal(R.d(a), b)


# ---------------------------------------------------------------------------------------------------------------
# finalize
# ---------------------------------------------------------------------------------------------------------------
def _finalize_ratios(B, C, layers, absolute, squared, defect=None, zero_plane=None):
    sums, chw = R.finalize_inputs(B, C, layers, zero_plane)
    loss, coef = twin_loss_finalize(sums, chw, absolute, squared, defect)
    ref, bl, cref, bc = R.loss_finalize(sums, chw, absolute, squared)
    ok = np.isfinite(cref)
    return dict(loss=R.ratio(float(loss) - ref, bl), coef=R.ratio(coef[ok] - cref[ok], bc[ok])), coef, cref


@pytest.mark.parametrize("layers", [1, R.LOSS_PART_SLICES])
@pytest.mark.parametrize("shape", R.FINALIZE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_loss_finalize_twin_inside_the_bounds(shape, layers):
    for absolute, squared in R.VARIANTS:
        w, _, _ = _finalize_ratios(*shape, layers, absolute, squared)
        print("loss_finalize twin worst error/bound  %-9s layers %d absolute %d squared %d  " % (shape, layers, absolute, squared) +
              "  ".join("%s %.3f" % kv for kv in sorted(w.items())))
        assert all(val <= 1.0 for val in w.values()), (shape, layers, absolute, squared, w)


@pytest.mark.parametrize("defect,output,cases", [
    ("chw_without_modulo", "coef", [((8, 73), 1), ((2, 3), 8)]),                        # needs BC > C
    ("coef_without_2", "coef", [(s, l) for s in R.FINALIZE_SHAPES for l in (1, 8)]),
    ("layers_for_S0_only", "coef", [(s, 8) for s in R.FINALIZE_SHAPES])])              # needs layers > 1; absolute variants never read S1
def test_loss_finalize_defective_twins_outside_the_bounds(defect, output, cases):
    for shape, layers in cases:
        for absolute, squared in R.VARIANTS:
            if defect == "layers_for_S0_only" and absolute:
                continue
            w, _, _ = _finalize_ratios(*shape, layers, absolute, squared, defect)
            assert w[output] > 1.0, (defect, shape, layers, absolute, squared, w)
            if defect != "coef_without_2":
                assert w["loss"] > 1.0, (defect, shape, layers, absolute, squared, w)


def test_a_plane_without_error_has_autograds_class_of_coefficient():
    """S0 = 0 on one plane: the squared variants keep a finite coef and the plane adds 0; the sqrt variants have coef = +-inf with the sign
    of the channel weight -- the class and sign autograd gives for the plain-torch statement (sqrt'(0) = inf)."""
    for absolute, squared in R.VARIANTS:
        sums, chw = R.finalize_inputs(2, 73, 8, zero_plane=80)
        w, coef, cref = _finalize_ratios(2, 73, 8, absolute, squared, zero_plane=80)
        auto = R.torch_l2_coef(sums, chw, absolute, squared)
        assert all(val <= 1.0 for val in w.values())
        if squared:
            assert np.isfinite(coef[80]) and np.isfinite(auto[80]) and np.isfinite(cref[80])
        else:
            assert np.isinf(coef[80]) and np.isinf(auto[80]) and np.isinf(cref[80])
            assert np.sign(coef[80]) == np.sign(auto[80]) == np.sign(cref[80]) == np.sign(chw[80 % 73])
        ok = np.isfinite(cref)
        assert ok.sum() == 2 * 73 - (0 if squared else 1) and np.allclose(auto[ok], cref[ok], rtol=1e-12, atol=0)


# ---------------------------------------------------------------------------------------------------------------
# the Python wrappers and the refusals
# ---------------------------------------------------------------------------------------------------------------
class _Recorder:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args))
            return 0
        return fn


def test_ops_wrappers_pass_the_shapes_the_c_abi_documents(monkeypatch):
    from swin_v2_weather_amd import ops
    rec = _Recorder()
    monkeypatch.setattr(L, "load", lambda: rec)
    monkeypatch.setattr(ops, "_stream", lambda: 1234)
    p = lambda t: t.data_ptr()
    inp, out = torch.zeros(3, 6, 10, 24), torch.zeros(6, 10, 24)
    ops.batch_sum(inp, out, accumulate=True)
    ops.batch_sum(inp, out)
    B, H, W, C = 2, 6, 10, 24
    M = B * (H // 2) * (W // 2)
    x, dn, g = torch.zeros(B, H, W, C), torch.zeros(M, 4 * C, dtype=torch.bfloat16), torch.zeros(4 * C)
    mean, rstd, dx, dg, db = torch.zeros(M), torch.zeros(M), torch.zeros(B, H, W, C), torch.zeros(4 * C), torch.zeros(4 * C)
    ops.merge_ln_bwd(x, dn, g, mean, rstd, dx, dg, db)
    chw, loss, coef = torch.zeros(73), torch.zeros(1), torch.zeros(8, 73)
    s8, s1 = torch.zeros(R.LOSS_PART_SLICES, 8, 73, 2), torch.zeros(8, 73, 2)
    ops.loss_finalize(s8, chw, False, True, loss, coef)
    ops.loss_finalize(s1, chw, True, False, loss, coef)
    want = [("swv2_batch_sum", (p(inp), p(out), 3, 6 * 10 * 24, 1, 1234)),
            ("swv2_batch_sum", (p(inp), p(out), 3, 6 * 10 * 24, 0, 1234)),
            ("swv2_merge_ln_bwd", (p(x), p(dn), p(g), p(mean), p(rstd), p(dx), p(dg), p(db), B, H, W, C, 1234)),
            ("swv2_loss_finalize", (p(s8), 8, p(chw), 8 * 73, 73, 0, 1, p(loss), p(coef), 1234)),
            ("swv2_loss_finalize", (p(s1), 1, p(chw), 8 * 73, 73, 1, 0, p(loss), p(coef), 1234))]
    assert rec.calls == want
    for name, args in rec.calls:
        assert len(args) == len(L.SYMBOLS[name][1]) and all(type(a) is int for a in args)


def test_refusals_return_invalid_with_a_message_and_without_a_gpu():
    lib = L.load()
    P = 4096                                         # any non-null value: never dereferenced by a refused call
    for n in (1, 2, 3, 5, 4 * 257 + 2):
        assert lib.swv2_batch_sum(P, P, 2, n, 0, None) == -1
        assert b"batch_sum" in lib.swv2_last_error() and b"multiple of 4" in lib.swv2_last_error()
    for call, word in ((lambda: lib.swv2_batch_sum(None, P, 2, 4, 0, None), b"batch_sum"), (lambda: lib.swv2_batch_sum(P, None, 2, 4, 0, None), b"batch_sum"),
                       (lambda: lib.swv2_batch_sum(P, P, 0, 4, 0, None), b"batch_sum"), (lambda: lib.swv2_batch_sum(P, P, 2, 0, 0, None), b"batch_sum"),
                       (lambda: lib.swv2_merge_ln_bwd(P, P, P, P, P, None, P, P, 1, 4, 4, 8, None), b"merge_ln_bwd"),
                       (lambda: lib.swv2_merge_ln_bwd(None, P, P, P, P, P, P, P, 1, 4, 4, 8, None), b"merge_ln_bwd"),
                       (lambda: lib.swv2_loss_finalize(P, 0, P, 6, 3, 0, 0, P, P, None), b"loss_finalize"),
                       (lambda: lib.swv2_loss_finalize(P, 1, P, 7, 3, 0, 0, P, P, None), b"loss_finalize"),
                       (lambda: lib.swv2_loss_finalize(P, 1, P, 6, 3, 0, 0, P, None, None), b"loss_finalize"),
                       (lambda: lib.swv2_loss_finalize(P, 1, P, 6, 3, 0, 0, None, P, None), b"loss_finalize")):
        assert call() == -1
        assert word in lib.swv2_last_error(), lib.swv2_last_error()
    with pytest.raises(L.Swv2Error, match="multiple of 4"):
        L.check(lib.swv2_batch_sum(P, P, 2, 6, 0, None), "swv2_batch_sum")
