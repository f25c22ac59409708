"""GPU (-m gpu): swv2_loss_sums / swv2_loss_grad (csrc/loss_l2.hip) through the C ABI.  The sums are judged element by element against the
fp64 statement of tests/score_reference.py with its chain-length bound (no arrival-order term: the kernel has no atomics), bit for bit
against S_dd and S_tt of swv2_score_sums, and for what a plane-streaming kernel promises: every slot written, nothing else touched, the
same bits on a second run, a NaN confined to its plane.  The gradient is judged bit for bit against its fp32 statement."""
import numpy as np
import pytest
import torch

from tests import score_reference as R
from tests.plane_harness import Guarded, dev, lib  # noqa: F401  (dev, lib: fixtures)
from tests.test_score_gpu import SHAPES, _fields, _launch as _score_launch

pytestmark = pytest.mark.gpu


def _launch(lib, dev, prd, tar, w):
    """contiguous device tensors [B, C, H, W] -> (Guarded with ws / sums, both pre-filled with the sentinel, slices)"""
    from swin_v2_weather_amd import _lib as L
    B, C, H, W = prd.shape
    slices = lib.swv2_score_slices(B * C, H, W)
    wsb = lib.swv2_loss_ws_bytes(B * C, H, W)
    assert wsb == B * C * slices * 8
    g = Guarded(dev, ws=wsb // 4, sums=B * C * 2)
    L.check(lib.swv2_loss_sums(prd.data_ptr(), tar.data_ptr(), w.data_ptr(), g["sums"].data_ptr(), B * C, H, W, g["ws"].data_ptr(), wsb,
                               torch.cuda.current_stream().cuda_stream), "swv2_loss_sums")
    torch.cuda.synchronize()
    return g, slices


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_sums_against_fp64_against_the_score_sums_and_on_a_second_run(dev, lib, shape):
    B, C, H, W = shape
    prd, tar, _, w = _fields(*shape)
    d = [torch.tensor(a).to(dev) for a in (prd, tar, w)]
    g, slices = _launch(lib, dev, *d)
    assert g.guards_intact(), "a kernel wrote outside its outputs"
    assert g.written("ws") and g.written("sums"), "slots the plan names were left unwritten"
    # (a) element by element against fp64: S0 = S_dd, S1 = S_tt of the score statement, the chain of plane_stream.h
    got = g["sums"].cpu().numpy().reshape(B, C, 2)
    S, A = R.sums(prd, tar, w)
    n = R.chain_length(H, W, slices)
    dS = R.sum_bounds(A, n)
    rs = R.worst(np.abs(got.astype(np.float64) - S[..., [0, 3]]), dS[..., [0, 3]])
    print(f"{shape} n = {n}: worst error / bound  sums {rs:.3f}")
    assert rs <= 1.0
    # (b) bit for bit against swv2_score_sums without a climatology + swv2_score_finalize: the same fma chains over the same plan
    gs, _ = _score_launch(lib, dev, d[0], d[1], d[2], None)
    score = gs["sums"].cpu().numpy().reshape(B, C, 4)[..., [0, 3]]
    assert np.array_equal(got.view(np.int32), score.view(np.int32)), "S0 / S1 are not the bits of the score kernel's S_dd / S_tt"
    # (c) a second run into sentinel-filled buffers of its own: the same bits in the workspace and the sums
    g2, _ = _launch(lib, dev, *d)
    assert g2.guards_intact() and g2.written("ws") and g2.written("sums") and torch.equal(g.raw, g2.raw)


def test_nan_in_one_plane_reaches_that_planes_two_sums_only(dev, lib):
    B, C, H, W = 3, 4, 16, 32
    prd, tar0, _, w = _fields(B, C, H, W)
    tar = tar0.copy()
    tar[1, 2, 7, 9] = np.nan
    d = [torch.tensor(a).to(dev) for a in (prd, tar0, tar, w)]
    clean, _ = _launch(lib, dev, d[0], d[1], d[3])
    g, _ = _launch(lib, dev, d[0], d[2], d[3])
    assert g.guards_intact()
    s, s0 = g["sums"].view(B, C, 2), clean["sums"].view(B, C, 2)
    assert bool(torch.isnan(s[1, 2]).all()) and bool(torch.isfinite(s0).all())
    keep = torch.ones(B, C, dtype=torch.bool, device=dev)
    keep[1, 2] = False
    assert torch.equal(s[keep].view(torch.int32), s0[keep].view(torch.int32))


@pytest.mark.parametrize("shape", [(2, 3, 5, 8), (3, 73, 16, 32), (2, 73, 240, 480)], ids=lambda s: "x".join(map(str, s)))
def test_gradient_bit_for_bit_against_its_fp32_statement(dev, lib, shape):
    """dprd = fp32(fp32(coef q[h]) fp32(p - t)), with planted elements and one whole plane where prd == tar, and coefficients of both signs"""
    from swin_v2_weather_amd import _lib as L
    B, C, H, W = shape
    prd0, tar, _, w = _fields(*shape)
    prd = prd0.copy()
    prd[B - 1, C - 1] = tar[B - 1, C - 1]
    prd[0, 0, H // 2, ::3] = tar[0, 0, H // 2, ::3]
    prd[0, 1, :, 1] = tar[0, 1, :, 1]
    coef = np.random.default_rng(B * C).standard_normal((B, C)).astype(np.float32)
    d = [torch.tensor(a).to(dev) for a in (prd, tar, w, coef)]
    runs = []
    for _ in range(2):
        g = Guarded(dev, dprd=B * C * H * W)
        L.check(lib.swv2_loss_grad(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), g["dprd"].data_ptr(), B * C, H, W,
                                   torch.cuda.current_stream().cuda_stream), "swv2_loss_grad")
        torch.cuda.synchronize()
        assert g.guards_intact() and g.written("dprd")
        runs.append(g)
    c = (coef[:, :, None] * w.astype(np.float32)[None, None, :])[..., None]          # one fp32 product
    want = (c * (prd - tar)).astype(np.float32)                                         # fp32 difference, fp32 product
    assert c.dtype == np.float32 and (prd - tar).dtype == np.float32
    have = runs[0]["dprd"].cpu().numpy().reshape(B, C, H, W)
    assert np.array_equal(have.view(np.int32), want.view(np.int32)), "dprd is not fp32(fp32(coef q[row]) fp32(p - t))"
    assert np.all(have[B - 1, C - 1] == 0) and np.all(have[0, 0, H // 2, ::3] == 0) and np.all(have[0, 1, :, 1] == 0)
    assert torch.equal(runs[0].raw, runs[1].raw)
