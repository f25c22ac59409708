"""No GPU: the case builders, fp64 references and per-element bounds of tests/linear_reference.py, checked on their own.

  * for every case of the GPU file that names a kernel, swv2_linear_kernel (a pure host function) names that kernel for the case's own
    descriptors, under the case's SWV2_GEMM_WIDE: a shape that silently stopped selecting its kernel is caught before the GPU run; every
    kernel of the selector is named by at least one case
  * Part 1's premise: the largest |accumulator| (|a| |w|^T + |bias|) and the largest squared norm of every exact case is below 2^24
  * an fp32 torch emulation with the kernels' rounding points (bf16 operands, fp32 accumulation over 64 columns at a time) passes every
    checker: the exact cases bit for bit, the random cases under HALF of every bound (bf16 outputs: of what the bound leaves beyond the
    rounding of the result itself) -- a bound the honest emulation nearly fills would not survive a second summation order
  * the host twins of eight plausible kernel defects are each rejected on a case the GPU file runs
  * the host construction of swv2_prep_weight's output; the 2 x 2 gather's column order against the reference fixture
"""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import linear_reference as R
from tests import mlp_reference as MR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPECS = R.all_specs()
# the emulation runs every builder; the cases of more than 12 000 rows (the resident kernels, TILE64 of the block products, the DMA kernel's
# partial column tile) repeat the arithmetic of their small twins and are left to the selection and premise checks
HOST_ROWS = 12000


def _small(spec):
    fn, args = spec
    return not (fn in (R.qkv_case, R.dx_case) and args[5] * args[6] > HOST_ROWS)


HOST_SPECS = [s for s in SPECS if _small(s)]


def _host_outs(c):
    outs = {}
    for n, (sh, dt, pf) in R.output_specs(c).items():
        numel = 1
        for s_ in sh:
            numel *= s_
        outs[n] = torch.empty(numel + R.DUMP_BYTES, dtype=dt)[:numel].view(*sh)
    return outs


def test_every_case_selects_the_kernel_it_is_named_after(monkeypatch):
    from swin_v2_weather_amd import _lib as L, ops
    lib = L.load()
    assert (R.Q128, R.Q192, R.DX128, R.DMA, R.WIDE, R.T64, R.T128) == (
        L.LINEAR_RESIDENT_QKV128, L.LINEAR_RESIDENT_QKV192X3, L.LINEAR_RESIDENT_DX128, L.LINEAR_WIDE_DMA, L.LINEAR_WIDE, L.LINEAR_TILE64,
        L.LINEAR_TILE128)
    assert (R.GROUP, R.SLICES, R.DUMP_BYTES) == (L.LOSS_GROUP_ROWS, L.LOSS_PART_SLICES, L.LOSS_DUMP_BYTES)
    assert all(R.resid_pitch(n) == L.loss_resid_pitch(n) for n in (80, 144, 1168)) and [R.resid_pitch(n) for n in (80, 144, 1168)] == [128, 192, 1216]
    named = {}
    for spec in SPECS:
        c = R.build(spec, False)
        if c.wide_env is None:
            monkeypatch.delenv("SWV2_GEMM_WIDE", raising=False)
        else:
            monkeypatch.setenv("SWV2_GEMM_WIDE", c.wide_env)
        a, e, N = R.descriptors(c, ops, L, _host_outs(c))
        kern = lib.swv2_linear_kernel(ctypes.byref(a), ctypes.byref(e), N)
        assert kern == c.kernel, (c.name, kern, lib.swv2_last_error())
        named.setdefault(kern, []).append((c.opk, c.epk))
    assert set(named) == set(range(7))
    # the (loader, epilogue) pairs the issue lists, each on every kernel it lists for them
    assert {k for k, v in named.items() if ("f32", "qkv") in v} == {R.Q128, R.Q192, R.WIDE, R.T64, R.T128}
    assert {k for k, v in named.items() if ("heads", "f32") in v} == {R.DX128, R.DMA, R.T64, R.T128}
    assert ("f32", "loss") in named[R.T64] and {("patch", "bf16"), ("merge", "f32"), ("cscale", "f32"), ("f32", "unpatch"), ("gelu", "f32"),
                                                ("bf16", "f32"), ("f32", "acc"), ("f32", "bf16")} <= set(named[R.T128])


def test_case_tables_cover_what_they_claim():
    plain = [a for _, a in R.plain_specs()]
    for vi, variant in enumerate(R.PLAIN_VARIANTS):
        mine = [a for a in plain if a[0] == variant]
        assert {a[1] for a in mine} == set(R.PLAIN_MS) and {a[2] for a in mine} == set(R.PLAIN_NS) and {a[3] for a in mine} == set(R.PLAIN_KS)
    heads = [a for _, a in R.head_specs(True)]
    for Cout in (5, 9, 73):
        assert {(a[1], a[2]) for a in heads if a[0] == Cout} >= set(R.HEAD_GRIDS)
    for pick in (5, 6, 7):                  # skip, second destination, sliced destination: each with every T
        assert {a[1] * a[2] for a in heads if a[pick]} >= {32, 64, 216}
    assert any(a[1] * a[2] > 12 * 8 * 32 for a in heads)          # more than 96 groups per sample: the reduce kernel's unrolled loop
    assert [R.resid_pitch(16 * c) for c in (5, 9, 73)] == [128, 192, 1216]
    assert {a[0] for _, a in R.patch_specs()} == {1, 7, 73} and {(a[1], a[2]) for _, a in R.patch_specs()} == {(8, 12), (24, 40)}
    for pick in (4, 5):                     # second source, planes inside a larger tensor: present and absent
        assert {a[pick] for _, a in R.patch_specs()} == {False, True}
    # the two row counts of each persistent kernel: a ragged and a full last tile
    assert 2053 * 16 == 128 * 256 + 80 and 2048 * 16 == 128 * 256 and 1027 * 16 == 64 * 256 + 48 and 1024 * 16 == 64 * 256
    assert R.M_WIDE_BW * R.LP >= 16 * 256 and (R.M_WIDE_BW * R.LP) % 256 != 0 and 94 * R.LP >= 64 * 256


@pytest.mark.parametrize("spec", SPECS, ids=R.spec_id)
def test_exact_cases_keep_every_accumulator_below_2_to_the_24(spec):
    c = R.build(spec, True)
    lut = MR.host_gelu_lut()
    assert R.max_accumulator(c, lut) < 2 ** 24, c.name
    assert R.dense_operand(c, lut)[1] is None, (c.name, "an exact case's operand must be exact")
    if c.epk == "qkv":
        v, E = R.product(c, lut)
        assert float(E.abs().max()) == 0 and float((R._split_heads(v, c)[:, :, :2] ** 2).sum(-1).max()) < 2 ** 24, c.name


def _half(worst, what):
    for k, v in worst.items():
        if k.endswith(" beyond rounding") or (k + " beyond rounding") in worst:
            continue
        assert v < 0.5, (what, k, v)
    for k, v in worst.items():
        if k.endswith(" beyond rounding"):
            assert v < 0.5, (what, k, v)


@pytest.mark.parametrize("spec", HOST_SPECS, ids=R.spec_id)
def test_emulation_passes_exact_and_stays_under_half_of_every_random_bound(spec):
    lut = MR.host_gelu_lut()
    for exact in (True, False):
        c = R.build(spec, exact)
        worst = {}
        R.check_case(c, R.emulate(c, lut), lut, worst=worst)
        if not exact:                   # (the exact cases' bounds are zero, or the rounding of the result alone, which it reaches by construction)
            _half(worst, c.name)


def _rejected(spec, exact, mutate):
    c = R.build(spec, exact)
    lut = MR.host_gelu_lut()
    try:
        R.check_case(c, R.emulate(c, lut, mutate=mutate), lut, worst={})
    except AssertionError as e:
        return str(e)
    return None


# defect -> cases of the GPU file's tables on which it must break a bound (random) or equality (exact)
TWIN_CASES = {
    "gather_next_row": [((R.qkv_case, (R.T128, 128, 8, 12, 16, 27, R.LP, R.LV)), e) for e in (True, False)] +
                       [((R.plain_case, ("bf16_gather-f32", 257, 96, 1168)), False)],
    "k_tail": [((R.plain_case, ("f32-acc", 64, 200, 72)), True), ((R.plain_case, ("gelu-f32_bias", 63, 128, 1168)), False),
               ((R.patch_case, (73, 8, 12, 96, False, True)), False)],
    "bias_slot": [((R.qkv_case, (R.T128, 192, 8, 24, 32, 2, R.LP, R.LV)), e) for e in (True, False)] + [((R.patch_case, (7, 8, 12, 96, True, False)), False)],
    "rnorm_padded": [((R.qkv_case, (R.T128, 128, 8, 12, 16, 1, R.LP, R.LV)), e) for e in (True, False)] +
                    [((R.qkv_case, (R.WIDE, 768, 8, 96, 96, R.M_WIDE_BW, R.LP, R.LV)), False)],
    "q_with_k_norm": [((R.qkv_case, (R.T128, 192, 8, 24, 32, 2, R.LP, R.LV)), e) for e in (True, False)],
    "loss_slot_fold": [((R.head_case, (5, 12, 18, 128, True, True, False, True)), e) for e in (True, False)],
    "unpatch_pq": [((R.head_case, (5, 4, 8, 96, False, False, False, False)), True), ((R.head_case, (73, 8, 8, 72, True, False, False, False)), False)],
    "skip_next_channel": [((R.head_case, (9, 4, 8, 96, False, True, True, False)), True), ((R.head_case, (5, 12, 18, 128, True, True, False, True)), False)],
}


@pytest.mark.parametrize("mutate", R.MUTANTS)
def test_host_twins_of_kernel_defects_are_rejected(mutate):
    ids = {R.spec_id(s) for s in SPECS}
    for spec, exact in TWIN_CASES[mutate]:
        assert R.spec_id(spec) in ids, (mutate, R.spec_id(spec), "is not a case of the GPU file")
        assert _rejected(spec, exact, None) is None
        msg = _rejected(spec, exact, mutate)
        assert msg is not None, (mutate, R.spec_id(spec), exact, "passes every check")
        print(f"\n[linear host twin] {mutate} on {R.spec_id(spec)}{' exact' if exact else ''}: {msg[:160]}")


def test_host_prep_weight_is_the_builders_weight():
    """the builders' weights (what the references use) are the host construction of swv2_prep_weight's output for their recorded arguments"""
    n = 0
    for spec in HOST_SPECS:
        c = R.build(spec, False)
        if c.prep:
            assert torch.equal(R.host_prep_weight(c.w_src, **c.prep), c.w), c.name
            n += 1
        else:
            assert torch.equal(c.w_src.to(R.BF), c.w), c.name
    assert n >= 20
    # padded rows / columns are exact zeros; a row map past its source is refused by nothing, so it must not occur
    c = R.build((R.qkv_case, (R.T128, 192, 8, 24, 32, 2, R.LP, R.LV)), False)
    assert int(c.pad_cols.sum()) == 3 * 8 * 8 and float(c.w[c.pad_cols].abs().max()) == 0 and float(c.bias[c.pad_cols].abs().max()) == 0
    assert int(c.hmap.max()) == c.w_src.shape[0] - 1


def test_merge_column_order_is_the_reference_fixtures():
    """the 2 x 2 gather's column order (MERGE_ORDER) reproduces the reference module's output stored in tests/golden/patch_merging.npz;
    the order with the two middle blocks swapped does not"""
    fx = np.load(os.path.join(ROOT, "tests", "golden", "patch_merging.npz"))
    x = torch.from_numpy(fx["x"]).double()
    g, b, w = (torch.from_numpy(fx[k]).double() for k in ("p:norm.weight", "p:norm.bias", "p:reduction.weight"))
    want = torch.from_numpy(fx["y"]).double().reshape(-1, w.shape[0])

    def run(order):
        rows = R.merge_rows(x, order)
        return torch.nn.functional.layer_norm(rows, (rows.shape[1],), g, b, 1e-5) @ w.T

    def rel(a):
        return float((a - want).norm() / want.norm())
    assert rel(run(R.MERGE_ORDER)) < 1e-5
    assert rel(run((R.MERGE_ORDER[0], R.MERGE_ORDER[2], R.MERGE_ORDER[1], R.MERGE_ORDER[3]))) > 1e-2
    # the fp64 statistics of the builder's rows are the layer norm's
    mu, _, rho, _ = R.ref_merge_stats(x.float())
    rows = R.merge_rows(x.float().double(), R.MERGE_ORDER)
    assert torch.allclose(mu, rows.mean(1)) and torch.allclose(rho, 1.0 / torch.sqrt(rows.var(1, unbiased=False) + R.P.EPS32))
