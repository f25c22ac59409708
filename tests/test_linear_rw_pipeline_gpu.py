"""GPU (-m gpu): the two resident row GEMMs of a block at C = 128 (swv2_linear: RESIDENT_QKV128 and RESIDENT_DX128) at the real window
geometry (Lp 176, L 162, 8 heads of 12 in 16-wide slots), at the row counts where a staged row pipeline can go wrong.  The d(qkv) -> dx
product runs csrc/gemm_rw.hip: rows by LDS-DMA in stages of 32, three stage slots, two stages in flight, counted waits.  The qkv product
runs the weight-in-LDS body of the same file; its two cases are kept so that a later move of qkv to the streaming body finds its tests here.

Every case goes through the machinery of tests/test_linear_exact_gpu.py (run_case: swv2_linear_kernel names the resident kernel, every
element against fp64 within the bounds of tests/linear_reference.py, guard rows, untouched elements still NaN, two runs bit-equal), once
with exact integer operands and once with random ones.  Then the same operands go through the tile kernels, window range by window range
(each range below the resident kernels' row thresholds; swv2_linear_kernel must name TILE64 / TILE128 for it), and every output must
agree with the resident kernel's bit for bit: the k order per output element is the same, so this is a condition, not a tolerance.

  product  Bw   rows     32-row stages over 256 workgroups
  qkv      187  32 912   (first body: 128-row tiles, ragged last tile of 16 rows)
  qkv      400  70 400   (first body: one benchmark sample)
  dx        94  16 544   517 stages: workgroups with 2 and 3 stages -- never more stages than stage slots, fill and drain only
  dx        95  16 720   522.5 stages: the last stage is ragged (rows 16 704 .. 16 719 of 32); 2 and 3 stages per workgroup
  dx       400  70 400   2 200 stages: 8 and 9 per workgroup, steady state, uneven counts
In every dx case a stage straddles windows (176 is no multiple of 32), the 14 padded rows of a window carry scatter entries of -1 next to
the about 1 / 8 of the real rows that scatter_table drops, so stores with every lane masked occur in most stages (the store count of
the counted waits), and the residual rows are fetched through the same table.
"""
import copy
import ctypes

import pytest
import torch

from tests import linear_reference as R
from tests.test_linear_exact_gpu import K, dev, gelu_lut, _Env, _guarded, prepared_weight, run_case  # noqa: F401  (fixtures + machinery)

pytestmark = pytest.mark.gpu

LP, LV = R.LP, R.LV
SPECS = [(R.qkv_case, (R.Q128, 128, 8, 12, 16, 187, LP, LV)),
         (R.qkv_case, (R.Q128, 128, 8, 12, 16, 400, LP, LV)),
         (R.dx_case, (R.DX128, 128, 8, 12, 16, 94, LP, LV)),
         (R.dx_case, (R.DX128, 128, 8, 12, 16, 95, LP, LV)),
         (R.dx_case, (R.DX128, 128, 8, 12, 16, 400, LP, LV))]
CHUNK_BW = 64                      # 64 * 176 = 11 264 rows: below both resident thresholds (16 384 / 32 768)


def tile_kernel_outputs(K, c, dev, wb):
    """the case's outputs from the tile kernels: one launch per range of CHUNK_BW windows into the same (prefilled) outputs"""
    L, ops = K["L"], K["ops"]
    lib = L.load()
    outs = {}
    for name, (shape, dtype, prefill) in R.output_specs(c).items():
        _, outs[name] = _guarded(shape, dtype, dev, prefill)
    for b0 in range(0, c.Bw, CHUNK_BW):
        b1 = min(b0 + CHUNK_BW, c.Bw)
        part = copy.copy(c)
        part.Bw, part.M = b1 - b0, (b1 - b0) * c.Lp
        if c.epk == "qkv":
            part.rowidx_in = c.rowidx_in[b0 * c.Lp:b1 * c.Lp].contiguous()
            o = {k: v[b0:b1] for k, v in outs.items()}
        else:
            part.x = c.x[b0:b1]
            part.rowidx_out = c.rowidx_out[b0 * c.Lp:b1 * c.Lp].contiguous()
            o = outs
        with _Env(None):
            a, e, N = R.descriptors(part, ops, L, o)
            kern = lib.swv2_linear_kernel(ctypes.byref(a), ctypes.byref(e), N)
            assert kern in L.LINEAR_TILE_KERNELS, f"{c.name}: windows {b0}..{b1} run {R.KERNEL_NAMES[kern] if kern >= 0 else kern}, not a tile kernel"
            ops.linear(a, wb, e, N)
    torch.cuda.synchronize()
    return outs


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "random"])
@pytest.mark.parametrize("spec", SPECS, ids=R.spec_id)
def test_resident_row_gemm_at_pipeline_edges(dev, K, gelu_lut, spec, exact):
    c, o = run_case(K, dev, spec, exact, gelu_lut)
    assert c.kernel in (R.Q128, R.DX128)                       # (run_case has asserted that swv2_linear_kernel names it)
    wb = prepared_weight(K, c)
    t = tile_kernel_outputs(K, c, dev, wb)
    for name in t:
        same = R.same_bits(o[name], t[name])
        assert bool(same.all()), f"{c.name}: {name} differs from the tile kernels' in {int((~same).sum())} elements"
