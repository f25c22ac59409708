"""CPU: the plan of a block's four weight gradients, asked from the library (swv2_block_wgrad_plan: the function swv2_block_wgrad
switches on, planning for a given CU count -- host arithmetic, no GPU).

The slab kernel (gemm_tn_slab.hip) runs one workgroup per CU; its planner splits them over the four products in proportion to their
bytes and hands the rounding remainder out slice by slice.  Whatever the CU count and the row counts, a plan must
  * launch at most `cus` workgroups (one per CU: a second round would double the time),
  * give every product 1 <= S <= ceil(rows / SR) row slices (no product without a workgroup, no slice without a stage),
  * fit the workspace the caller sized with swv2_block_wgrad_ws_bytes, which knows neither the rows nor the device.
Swept over both shape sets, every CU count from 16 to 320 (the bound the workspace is sized for) and the row counts of the GPU test
plus three extremes; the plans the GPU test's comments document at 256 CUs are pinned."""
import ctypes

import pytest

from swin_v2_weather_amd import _lib as L
from tests.test_wgrad_exact_gpu import CASES, LP, SETS, shape_items, slab_plan

ROWS = CASES + [(1, 1), (1000000, 1), (1, 5000)]          # (token rows M, windows Bw)


@pytest.mark.parametrize("tag", ["c128", "c192"])
def test_every_slab_plan_fits_the_device_the_rows_and_the_workspace(tag):
    sd = SETS[tag]
    n = 0
    for M, Bw in ROWS:
        rows = [M, M, Bw * LP, Bw * LP]
        for cus in range(16, 321):
            p, nb = slab_plan(L, sd, M, Bw, cus)
            assert p.kernel == L.BLOCK_WGRAD_SLAB, (M, Bw, cus)
            assert sum(p.wgs) <= cus, (M, Bw, cus, list(p.wgs))
            assert all(1 <= p.S[i] <= -(-rows[i] // p.SR[i]) for i in range(4)), (M, Bw, cus, list(p.S), list(p.SR))
            assert all(p.wgs[i] % p.S[i] == 0 for i in range(4)), (M, Bw, cus, list(p.wgs), list(p.S))     # whole slices
            assert 0 < p.bytes <= nb, (M, Bw, cus, p.bytes, nb)
            n += 1
    assert n == len(ROWS) * 305


# slices of fc2, fc1, proj, qkv at 256 CUs (tests/test_wgrad_exact_gpu.py, the comment above CASES)
PINNED = [("c128", 162, 1, [6, 6, 3, 6]), ("c192", 162, 1, [6, 6, 6, 6]),
          ("c128", 4383, 27, [91, 70, 25, 70]), ("c192", 4383, 27, [41, 35, 20, 42]),
          ("c192", 4374, 27, [40, 35, 22, 42]),
          ("c128", 4374, 1, [137, 112, 2, 5]), ("c192", 4374, 1, [67, 58, 2, 2])]


@pytest.mark.parametrize("tag,M,Bw,S", PINNED)
def test_documented_plans_at_256_cus(tag, M, Bw, S):
    p, _ = slab_plan(L, SETS[tag], M, Bw, 256)
    assert p.kernel == L.BLOCK_WGRAD_SLAB and list(p.S) == S
    assert list(p.SR) == ([32, 32, 64, 32] if tag == "c128" else [32, 32, 32, 32])


def test_plan_query_and_kernel_query_are_one_function():
    """swv2_block_wgrad_kernel is the plan's `kernel` (no GPU here: cus = 0 is the library's 256-CU fallback); an explicit slice count,
    a block shape without a slab set and a workspace below the plan's bytes get the grouped tile kernel's plan: its slices for every
    product, 128-row steps, tiles x slices workgroups, the partial tiles' bytes"""
    lib = L.load()
    sd = SETS["c128"]
    items = shape_items(L, sd, 4374, 27)
    p, nb = slab_plan(L, sd, 4374, 27, 0)
    q, _ = slab_plan(L, sd, 4374, 27, 256)
    assert lib.swv2_block_wgrad_kernel(items, 0, nb) == p.kernel == L.BLOCK_WGRAD_SLAB
    assert (list(p.S), list(p.wgs), p.bytes) == (list(q.S), list(q.wgs), q.bytes)
    g = L.BlockWgradPlan()
    for slices, ws, it, tiles, want_s in ((8, nb, items, [4, 4, 1, 3], 8), (0, p.bytes - 1, items, [4, 4, 1, 3], 40),
                                          (0, 1 << 30, shape_items(L, SETS["c512"], 8192, 48), [32, 32, 16, 48], 8)):
        assert lib.swv2_block_wgrad_plan(it, slices, ws, 0, ctypes.byref(g)) == 0
        assert g.kernel == lib.swv2_block_wgrad_kernel(it, slices, ws) == L.BLOCK_WGRAD_GROUPED
        assert list(g.S) == [want_s] * 4 and list(g.SR) == [128] * 4 and list(g.wgs) == [t * want_s for t in tiles]
        assert g.bytes == want_s * sum(tiles) * 128 * 128 * 4
    assert lib.swv2_block_wgrad_plan(None, 0, 0, 0, ctypes.byref(g)) == -1 and lib.swv2_block_wgrad_plan(items, 0, nb, -1, ctypes.byref(g)) == -1
