"""GPU (-m gpu): the forward GEMM engine behind swv2_linear (csrc/gemm.hip, csrc/gemm_wide.hip, csrc/gemm_rw.hip, csrc/gemm_epilogue.h, csrc/gemm_common.h) element by element against fp64:
every loader and epilogue that the earlier exact suites leave to a relative l2 norm, on every kernel linear_kernel_for can choose.

The case builders, the references, the bounds and their derivations are in tests/linear_reference.py (checked without a GPU by
tests/test_linear_exact_host.py, which also holds the host twins of the kernel mutants).  For every case:
  * the weight is what swv2_prep_weight returns (row_map / col_map / transpose / zero padding), compared with torch.equal against a host
    construction;
  * swv2_linear_kernel is asked with the launch's own descriptors and must name the kernel the case is named after;
  * every output sits between guard rows (mlp_reference.Guarded) that must be intact, and is prefilled with NaN (the accumulate
    epilogue: with its baseline; the squared norms of the wide heads: with the zeros their contract asks for); every element the contract
    says is written must be finite and within its bound, every other element must still be the prefill: scatter rows with index -1,
    pitch columns >= N, the residual's pad columns, the other channels of a sliced destination, slot 1 of loss groups that end no sample;
  * the launch runs twice and the two runs agree bit for bit.  The one exception: EPI_QKV_HEADS at DP 96 adds up to six squared-norm
    pieces per row with float atomics in no fixed order: `ss`, and behind swv2_qk_normalize `rnorm` and `qkvh`, are held to their bounds
    on both runs instead (ATOMIC_OUTPUTS).  At DP 128 there are two addends per row: order-independent, bit-equal.
Part 1 (exact): operands from small integers, every accumulator an integer below 2^24: fp32 outputs equal fp64, bf16 outputs equal its
round-to-nearest-even bf16, q / k / rnorm keep only their rounding terms.  Part 2 (random): log-uniform column / row scales, the
derived bounds of linear_reference.py.

Worst |err| / bound measured on an MI355X over every case of this file (the `[linear worst |err| / bound]` line printed under -s;
records, not bars: the bounds are derived in linear_reference.py, none is fitted to these).  "beyond" is (|err| - rounding term) /
(bound - rounding term): a bf16 output reaches the 2^-8 |ref| of its bound by construction.
  kernel             qkvh   beyond   rnorm   raw    beyond   ss       out (fp32)  out (bf16)  beyond   y      part    sums    resid  beyond
  RESIDENT_QKV128    0.996  0.0024   0.496
  RESIDENT_QKV192X3  0.996  0.0012   0.498
  RESIDENT_DX128                                                      0.0077
  WIDE_DMA                                                            0.0038
  WIDE               0.996  0.0006   0.496   0.971  0.0005   0.0006
  TILE64             0.996  0.0013   0.498                            0.0090                           0.336  0.0084  0.040   0.996  0
  TILE128            0.996  0.0016   0.496   0.971  0.0005   0.0006   0.389 (y)   0.992       0.00002  0.389
swv2_merge_stats: mean 0.0046, rstd 0.013.  swv2_loss_resid_to_image: 0.998 (one fp32 product held to 2^-24 of itself: a rounding term).
Ratios near 0.5 that are one rounding held to a bound of two: rnorm 0.494 (random) .. 0.498 (exact, where the bound is 3 2^-24 and sqrtf
and the division use up to 1.5 of them); EPI_F32_ACC 0.487 (one addition onto a baseline that is large against the product); the
un-patchify skip 0.389; OP_BF16_CSCALE 0.504 where one product dominates an output (the operand's own bf16 rounding: beyond it 0.0002).
By case family, random operands: OP_BF16 gathered -> EPI_F32 0.117, OP_BF16_GELU -> EPI_F32 0.119, PatchEmbed 0.985 (bf16), PatchMerging
0.355, dx 0.009.  No test failed on the library as it stands; the mutants that these
tests were run against are listed in LABNOTES.md ("The forward GEMM engine element by element").
"""
import ctypes
import os

import pytest
import torch

from tests import linear_reference as R
from tests import mlp_reference as MR

pytestmark = pytest.mark.gpu

BF = R.BF
SPECS = R.all_specs()
ATOMIC_OUTPUTS = ("ss", "rnorm", "qkvh")          # of EPI_QKV_HEADS at DP 96 only


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def K():
    from swin_v2_weather_amd import _lib as L, ops
    L.load()
    assert (R.Q128, R.Q192, R.DX128, R.DMA, R.WIDE, R.T64, R.T128) == (
        L.LINEAR_RESIDENT_QKV128, L.LINEAR_RESIDENT_QKV192X3, L.LINEAR_RESIDENT_DX128, L.LINEAR_WIDE_DMA, L.LINEAR_WIDE, L.LINEAR_TILE64,
        L.LINEAR_TILE128)
    assert (R.GROUP, R.SLICES, R.DUMP_BYTES) == (L.LOSS_GROUP_ROWS, L.LOSS_PART_SLICES, L.LOSS_DUMP_BYTES)
    yield dict(L=L, ops=ops)
    # (shown with -s) the worst |err| / bound of every output per kernel over the cases that ran
    print("\n[linear worst |err| / bound] " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(R.WORST.items())))


@pytest.fixture(scope="module")
def gelu_lut(dev, K):
    return MR.library_gelu_lut(K["ops"], K["L"], dev)


class _Env:
    """SWV2_GEMM_WIDE for the duration of one case (the library reads it per call)"""

    def __init__(self, value):
        self.value = value

    def __enter__(self):
        self.old = os.environ.get("SWV2_GEMM_WIDE")
        if self.value is None:
            os.environ.pop("SWV2_GEMM_WIDE", None)
        else:
            os.environ["SWV2_GEMM_WIDE"] = self.value

    def __exit__(self, *a):
        if self.old is None:
            os.environ.pop("SWV2_GEMM_WIDE", None)
        else:
            os.environ["SWV2_GEMM_WIDE"] = self.old


def _guarded(shape, dtype, dev, prefill, dump=False):
    """-> (Guarded, tensor of `shape` inside it): guard rows of the last dimension's width on either side; dump: SWV2_LOSS_DUMP_BYTES of
    scratch between the tensor and the guard behind it, where the loss epilogue's masked lanes store"""
    last, rows = shape[-1], 1
    for s in shape[:-1]:
        rows *= s
    extra = -(-R.DUMP_BYTES // (last * torch.empty((), dtype=dtype).element_size())) if dump else 0
    g = MR.Guarded((rows + extra, last), dtype, dev)
    t = g.t[:rows].view(*shape)
    if torch.is_tensor(prefill):
        t.copy_(prefill)
    else:
        t.fill_(prefill)
    return g, t


def prepared_weight(K, c):
    """the bf16 weight swv2_prep_weight returns for the case, checked against the host construction"""
    ops = K["ops"]
    kw = {k: v for k, v in (c.prep or {}).items()}
    wb = ops.prep_weight(c.w_src, **kw)
    torch.cuda.synchronize()
    assert torch.equal(wb, c.w), f"{c.name}: swv2_prep_weight differs from the host construction in {int((wb != c.w).sum())} elements"
    assert torch.equal(wb, R.host_prep_weight(c.w_src, **kw))
    return wb


def launch(K, c, dev, wb):
    """one run of the case -> {output: tensor} (guards checked)"""
    L, ops = K["L"], K["ops"]
    lib = L.load()
    loss = c.epk == "loss"
    guards, outs = {}, {}
    for name, (shape, dtype, prefill) in R.output_specs(c).items():
        guards[name], outs[name] = _guarded(shape, dtype, dev, prefill, dump=loss and name in ("y", "y2", "resid"))
    if loss:
        guards["sums"], outs["sums"] = _guarded((R.SLICES, c.B, c.Ctar, 2), torch.float32, dev, R.SENT)
    with _Env(c.wide_env):
        a, e, N = R.descriptors(c, ops, L, outs)
        kern = lib.swv2_linear_kernel(ctypes.byref(a), ctypes.byref(e), N)
        assert kern == c.kernel, f"{c.name}: swv2_linear_kernel names {R.KERNEL_NAMES[kern] if kern >= 0 else kern}, the case {R.KERNEL_NAMES[c.kernel]}"
        ops.linear(a, wb, e, N)
    if c.epk == "qkv" and R.wide_heads(c):
        torch.cuda.synchronize()
        outs["qkvh_raw"], outs["ss"] = outs["qkvh"].clone(), outs["rnorm"].clone()
        L.check(lib.swv2_qk_normalize(outs["qkvh"].data_ptr(), outs["rnorm"].data_ptr(), c.Bw, c.h, c.Lp, c.L, c.DP, ops._stream()), "swv2_qk_normalize")
    if loss:
        ops.loss_part_reduce(outs["part"], c.M, c.T, c.B, c.Cout, c.coff, outs["sums"])
    torch.cuda.synchronize()
    bad = [k for k, g in guards.items() if not g.intact()]
    assert not bad, f"{c.name}: guard rows written around {bad}"
    return outs


def run_case(K, dev, spec, exact, lut):
    L, ops = K["L"], K["ops"]
    c = R.case_to(R.build(spec, exact), dev)
    wb = prepared_weight(K, c)
    if c.opk == "merge" and not exact:
        # the library's own statistics, each row against fp64; the GEMM is then judged from them
        gm, mean = _guarded((c.M,), torch.float32, dev, R.NAN)
        gr, rstd = _guarded((c.M,), torch.float32, dev, R.NAN)
        ops.merge_stats(c.x, mean, rstd)
        torch.cuda.synchronize()
        assert gm.intact() and gr.intact()
        mu, mub, rho, rhob = R.ref_merge_stats(c.x)
        R.P.assert_within("merge_stats mean", mean, mu, mub, c.name, worst=R.WORST)
        R.P.assert_within("merge_stats rstd", rstd, rho, rhob, c.name, worst=R.WORST)
        c.mean, c.rstd = mean, rstd
    o1 = launch(K, c, dev, wb)
    r = R.check_case(c, o1, lut)
    o2 = launch(K, c, dev, wb)
    atomic = c.epk == "qkv" and c.DP == 96
    for name in o1:
        if atomic and name in ATOMIC_OUTPUTS:
            continue
        same = R.same_bits(o1[name], o2[name])
        assert bool(same.all()), f"{c.name}: {name} differs between two runs in {int((~same).sum())} elements"
    if atomic:
        R.check_case(c, o2, lut)
    if c.C2:            # the second destination holds the same values as the first
        assert torch.equal(o1["y"][:, c.c0:c.c0 + c.Cout], o1["y2"][:, :c.Cout]), f"{c.name}: the two destinations differ"
    print(f"\n[linear {R.KERNEL_NAMES[c.kernel]}] {c.name}: " + ", ".join(f"{k} {v:.3g}" for k, v in r.items()))
    return c, o1


@pytest.mark.parametrize("spec", SPECS, ids=R.spec_id)
def test_exact_operands_bit_for_bit(dev, K, gelu_lut, spec):
    """Part 1: integer operands, every accumulator exact: equality where the arithmetic allows it, the rounding-only bounds elsewhere"""
    c, o = run_case(K, dev, spec, True, gelu_lut)
    if c.epk == "qkv":
        q = o["qkvh"]
        pad_rows = torch.arange(c.Lp, device=dev) >= c.L
        assert bool((q[:, :, :, pad_rows].contiguous().view(torch.int16) == 0).all()), f"{c.name}: padded window rows are not exactly +0"
        assert bool((o["rnorm"][:, :, :, pad_rows] == 0).all()), f"{c.name}: rnorm of padded window rows is not exactly 0"
        cols = c.pad_cols.view(3, c.h, c.DP).permute(1, 0, 2)                      # [h][3][DP]
        assert bool((q.permute(0, 3, 1, 2, 4)[:, :, cols] == 0).all()), f"{c.name}: padded head columns are not exactly 0"


@pytest.mark.parametrize("spec", SPECS, ids=R.spec_id)
def test_random_operands_within_the_derived_bounds(dev, K, gelu_lut, spec):
    """Part 2: log-uniform scales, every element within its derived bound"""
    c, o = run_case(K, dev, spec, False, gelu_lut)
    if c.rowidx_out is not None and c.epk in ("f32", "bf16"):
        # the scatter names distinct rows: each is written once (check_case: finite and within its bound), every row that only a -1 entry
        # could have named is still NaN
        named = torch.zeros(c.rows_out, dtype=torch.bool, device=dev)
        named[c.rowidx_out[c.rowidx_out >= 0].long()] = True
        assert int(named.sum()) == int((c.rowidx_out >= 0).sum()) and (c.M == 1 or int(named.sum()) < c.rows_out)
        assert bool(torch.isnan(o["out"][~named].float()).all()) and bool(torch.isfinite(o["out"][named][:, :c.N].float()).all())


@pytest.mark.parametrize("spec", R.head_specs(True), ids=R.spec_id)
def test_loss_epilogue_predicts_what_the_plain_epilogue_predicts(dev, K, spec):
    """EPI_UNPATCH_LOSS and EPI_UNPATCH write the same prediction bit for bit (both destinations)"""
    c = R.case_to(R.build(spec, False), dev)
    wb = prepared_weight(K, c)
    o_loss = launch(K, c, dev, wb)
    c.epk, c.kernel = "unpatch", R.T128
    o_plain = launch(K, c, dev, wb)
    for name in o_plain:
        same = R.same_bits(o_plain[name], o_loss[name])
        assert bool(same.all()), f"{c.name}: {name} differs between the two epilogues in {int((~same).sum())} elements"


@pytest.mark.parametrize("Cout,gh,gw,add", [(5, 4, 8, False), (9, 12, 18, True), (73, 8, 8, True)])
def test_loss_resid_to_image(dev, K, Cout, gh, gw, add):
    """swv2_loss_resid_to_image (the rollout's skip gradient): out[:, :Cout] = coef[b][c] * un-patchify(resid) (+ add[:, :Cout]) per element
    against fp64: one fp32 product (2^-24 of it) and, with `add`, one addition (2^-24 of the result); the other channels of `out` and
    the pad columns of the residual's pitch are not touched / not read (they hold NaN)."""
    ops = K["ops"]
    g = R._gen(8, Cout, gh, gw, add)
    B, H, W = 3, 4 * gh, 4 * gw
    M, Nn = B * gh * gw, Cout * 16
    resid = torch.full((M, R.resid_pitch(Nn)), R.NAN, dtype=BF)
    resid[:, :Nn] = R._scaled(M, Nn, g).to(BF)
    coef = R.signed_log_uniform(B * Cout, 1e-2, 2.0, g).view(B, Cout)
    addt = torch.full((B, Cout + 1, H, W), R.NAN)
    addt[:, :Cout] = torch.randn(B, Cout, H, W, generator=g)
    resid, coef, addt = resid.to(dev), coef.to(dev), addt.to(dev)
    prod = coef.double().view(B, Cout, 1, 1) * R.unpatch_image(resid[:, :Nn].double(), B, Cout, H, W)
    ref = prod + addt[:, :Cout].double() if add else prod
    bound = R.U24 * prod.abs() + (R.U24 * ref.abs() if add else 0)
    runs = []
    for _ in range(2):
        go, out = _guarded((B, Cout + 2, H, W), torch.float32, dev, R.NAN)
        ops.loss_resid_to_image(resid, coef, out, Cout, add=addt if add else None)
        torch.cuda.synchronize()
        assert go.intact() and bool(torch.isnan(out[:, Cout:]).all())
        R.P.assert_within("loss_resid_to_image", out[:, :Cout], ref, bound, f"Cout {Cout} {H}x{W} add {add}", worst=R.WORST)
        runs.append(out)
    assert torch.equal(runs[0][:, :Cout], runs[1][:, :Cout])
