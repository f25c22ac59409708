"""Host side of the forecast extremes metric (no GPU): the CPU path against the reference's recorded outputs
(tests/golden/quantiles.npz) and the sort statement of tests/quantile_reference.py, the rank builder, NaN planes, the RolloutScores
field, the lead-time table and the host half of the C ABI (workspace size, refusals)."""
import os

import numpy as np
import pytest
import torch

from swin_v2_weather_amd import _lib as L
from swin_v2_weather_amd.utils import weighted_acc_rmse as M
from tests import quantile_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "quantiles.npz"))


def test_levels_equal_the_recorded_ones_bit_for_bit():
    q = M.quantile_levels()
    assert q.dtype == torch.float32 and q.shape == (100,)
    assert np.array_equal(q.numpy(), GOLD["levels"]) and np.array_equal(R.levels().numpy(), GOLD["levels"])
    assert abs(float(q[0]) - 0.999) < 1e-6 and abs(float(q[-1]) - 0.2057) < 1e-4
    q5 = M.quantile_levels(qlim=5, qs=7)
    assert q5.shape == (7,) and abs(float(q5[0]) - (1 - 1e-5)) < 1e-6


def test_cpu_path_equals_the_recorded_reference_outputs_bit_for_bit():
    pred, target = torch.tensor(GOLD["pred"]), torch.tensor(GOLD["target"])
    got = M.top_quantiles_error_torch(pred, target)
    assert got.shape == (2, 3) and got.dtype == torch.float32
    assert np.array_equal(got.numpy(), GOLD["top_quantiles_error_torch"])
    assert np.all(GOLD["top_quantiles_error_torch"] < 0)                      # the damped prediction misses the upper tail
    # and the sort statement equals torch.quantile bit for bit on the CPU, also on clustered and mostly-zero planes
    q = M.quantile_levels()
    g = torch.Generator().manual_seed(5)
    zeros = torch.rand(1, 2, 12, 20, generator=g)
    zeros[zeros < 0.98] = 0.0
    for x in (pred, target, 1.0 + 1e-6 * torch.randn(1, 2, 33, 64, generator=g), zeros, torch.randint(-2, 3, (2, 2, 7, 12), generator=g).float()):
        ref, _ = R.quantiles(x, q)
        assert np.array_equal(M.plane_quantiles(x, q).numpy(), ref)
    ref, bound = R.top_quantiles_error(pred, target)
    assert np.all(np.abs(got.numpy() - ref) <= bound)


def test_numpy_form_against_the_recorded_reference_output():
    got = M.top_quantiles_error(GOLD["pred"][0], GOLD["target"][0])
    assert got.shape == (3,) and got.dtype == np.float64
    assert np.allclose(got, GOLD["top_quantiles_error"], rtol=0, atol=1e-12)
    one = M.top_quantiles_error(GOLD["pred"][0, 1], GOLD["target"][0, 1])      # [h, w]: one plane
    assert one.shape == (1,) and abs(one[0] - GOLD["top_quantiles_error"][1]) <= 1e-12


@pytest.mark.parametrize("hw, n_ranks", [((721, 1440), 196), ((8, 16), 67)])
def test_rank_builder_uses_fp32_arithmetic(hw, n_ranks):
    n = hw[0] * hw[1]
    q = M.quantile_levels()
    ranks, i_lo, i_hi, w = M.quantile_ranks(n, q)
    assert ranks.dtype == torch.int32 and ranks.numel() == n_ranks and w.dtype == torch.float32
    r = ranks.long()
    assert bool((r[1:] > r[:-1]).all()) and int(r[0]) >= 0 and int(r[-1]) < n
    lo, hi, w_ref = R.rank_arithmetic(n, q)
    assert torch.equal(r[i_lo], lo) and torch.equal(r[i_hi], hi) and torch.equal(w, w_ref)
    lo64 = torch.floor(q.double() * (n - 1)).long()
    if hw == (721, 1440):
        assert int((lo64 != lo).sum()) == 3                                    # fp32, not fp64: three floors differ at this size
    with pytest.raises(ValueError):
        M.quantile_ranks(n, torch.tensor([0.5, 1.5]))


def test_nan_plane_is_nan_in_that_plane_only():
    x = torch.tensor(GOLD["pred"]).clone()
    x[1, 2, 4, 5] = float("nan")
    q = M.quantile_levels()
    got = M.plane_quantiles(x, q)
    nan = torch.isnan(got)
    assert bool(nan[:, 1, 2].all()) and int(nan.sum()) == q.numel()
    e = M.top_quantiles_error_torch(x, torch.tensor(GOLD["target"]))
    assert bool(torch.isnan(e[1, 2])) and int(torch.isnan(e).sum()) == 1
    keep = torch.ones(2, 3, dtype=torch.bool)
    keep[1, 2] = False
    assert np.array_equal(e[keep].numpy(), GOLD["top_quantiles_error_torch"][keep.numpy()])


def test_forecast_scorer_quantile_error_on_the_cpu_equals_the_function():
    pred, target = torch.tensor(GOLD["pred"]), torch.tensor(GOLD["target"])
    wide_p, wide_t = torch.zeros(2, 6, 9, 16), torch.zeros(2, 7, 9, 16)
    wide_p[:, 2:5], wide_t[:, 4:7] = pred, target
    sc = M.ForecastScorer(9, 16, 3, "cpu")
    got = sc.quantile_error(wide_p, wide_t, coff_prd=2, coff_tar=4)
    assert np.array_equal(got.numpy(), GOLD["top_quantiles_error_torch"]) and sc._ws == {}
    with pytest.raises(ValueError):
        sc.quantile_error(wide_p, wide_t, coff_prd=5)
    assert M.Scores._fields == ("rmse", "acc", "rmse_mean", "acc_mean", "sums")


def test_rollout_scores_keeps_its_five_argument_form_and_the_table_its_columns():
    from swin_v2_weather_amd import inference
    five = inference.RolloutScores(torch.tensor([[1.0, 2.0], [3.0, 4.0]]), None, None, None, None)
    assert five.tqe is None and inference.RolloutScores._fields[-1] == "tqe" and len(inference.RolloutScores._fields) == 6
    names = [("u10m", 0), ("v10m", 1)]
    plain = inference.lead_time_table(five, names)
    assert plain.splitlines()[0].split() == ["lead_h", "rmse_u10m", "rmse_v10m"]
    six = five._replace(tqe=torch.tensor([[[0.5, -1.0], [1.5, -3.0]], [[0.0, 0.0], [0.25, 0.25]]]))      # [steps, B, C]
    lines = inference.lead_time_table(six, names).splitlines()
    assert lines[0].split() == ["lead_h", "rmse_u10m", "rmse_v10m", "tqe_u10m", "tqe_v10m"]
    assert [float(v) for v in lines[1].split()] == [6.0, 1.0, 2.0, 1.0, -2.0]                          # the batch means
    assert [float(v) for v in lines[2].split()] == [12.0, 3.0, 4.0, 0.125, 0.125]
    a = inference.build_parser().parse_args(["--registry", "R", "--truth", "t.npy", "--extremes"])
    assert a.extremes and not inference.build_parser().parse_args(["--registry", "R"]).extremes
    import inspect
    assert inspect.signature(inference.score_rollout).parameters["extremes"].default is False


def test_workspace_size_and_every_refusal_without_a_gpu():
    """swv2_quantile_ws_bytes is host arithmetic; swv2_plane_order_stats checks its arguments before anything is launched, so the
    pointers only have to be non-null here: a refused call touches nothing."""
    lib = L.load()
    for bad in ((0, 8, 16, 10), (4, 0, 16, 10), (4, 8, -1, 10), (4, 8, 16, 0), (-3, 8, 16, 10)):
        assert lib.swv2_quantile_ws_bytes(*bad) == 0
    ok = lib.swv2_quantile_ws_bytes(6, 8, 16, 67)
    assert ok == 6 * 35856 and ok % 16 == 0 and lib.swv2_quantile_ws_bytes(146, 720, 1440, 196) == 146 * 35856
    P = 4096
    B, C, H, W = 2, 3, 8, 16

    def call(x=P, bs=C * H * W, B=B, C=C, H=H, W=W, ranks=P, K=67, out=P, nc=P, ws=P, wb=ok):
        return lib.swv2_plane_order_stats(x, bs, B, C, H, W, ranks, K, out, nc, ws, wb, None)
    for f, word in ((lambda: call(x=None), b"null"), (lambda: call(ranks=None), b"null"), (lambda: call(out=None), b"null"),
                    (lambda: call(nc=None), b"null"), (lambda: call(ws=None), b"null"), (lambda: call(H=3, W=5), b"H * W % 4"),
                    (lambda: call(x=P + 4), b"aligned"), (lambda: call(ws=P + 8), b"aligned"), (lambda: call(out=P + 2), b"aligned"),
                    (lambda: call(bs=C * H * W + 2), b"stride"), (lambda: call(bs=H * W), b"stride"), (lambda: call(K=0), b"K outside"),
                    (lambda: call(K=257), b"K outside"), (lambda: call(H=1 << 15, W=1 << 15), b"shape"), (lambda: call(B=0), b"shape"),
                    (lambda: call(B=1 << 12, C=1 << 8), b"shape"), (lambda: call(wb=ok - 1), b"workspace"), (lambda: call(wb=0), b"workspace")):
        assert f() == -1
        assert word in lib.swv2_last_error(), lib.swv2_last_error()
    with pytest.raises(L.Swv2Error):
        L.check(call(K=257), "swv2_plane_order_stats")
    from swin_v2_weather_amd import ops
    x = torch.zeros(1, 2, 4, 8)
    assert not ops.quantile_planes_ok(x) and ops.QUANTILE_MAX_RANKS == 256     # a CPU tensor
    with pytest.raises(L.Swv2Error):
        ops.plane_order_stats(x, torch.zeros(3, dtype=torch.int32))
