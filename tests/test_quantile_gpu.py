"""GPU (-m gpu): swv2_plane_order_stats through the C ABI against the sorted planes of tests/quantile_reference.py (exact), then the
Python layer on top of it: plane_quantiles / top_quantiles_error_torch on CUDA, ForecastScorer.quantile_error,
inference.score_rollout(extremes=True) and the CLI's --extremes.  Every bound is derived in tests/quantile_reference.py."""
import functools
import json
import os

import numpy as np
import pytest
import torch

from tests import quantile_reference as R
from tests.plane_harness import SENTINEL, Guarded, dev, lib  # noqa: F401  (dev, lib: fixtures)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "quantiles.npz"))


def _case(name):
    """(field [B, C, H, W] fp32 numpy, why): the smallest shapes at which each path of the select can go wrong"""
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == "2x3x9x16":                            # a plane smaller than one workgroup sweep: most of the 341 slices are empty
        x = rng.standard_normal((2, 3, 9, 16))
    elif name == "clustered":                         # every key shares its top 20 bits: the last digits decide
        x = 1.0 + 1e-6 * rng.standard_normal((1, 2, 33, 64))
    elif name == "2x73x60x120":                       # the production slice count of 14, uneven slice bounds, scales 1e-3 .. 1e5, mixed signs
        scale = np.logspace(-3, 5, 73)[None, :, None, None] * np.where(np.arange(73) % 3 == 0, -1.0, 1.0)[None, :, None, None]
        x = rng.standard_normal((2, 73, 60, 120)) * scale
        x[:, 1::3] = np.abs(x[:, 1::3])
    elif name == "512x1024":                          # one plane, 2048 slices of 256 elements; more than 65 535 elements in one bin
        x = rng.standard_normal((1, 1, 512, 1024))
    elif name == "512x1024-constant":                 # every element in one bin at every level
        x = np.full((1, 1, 512, 1024), -3.25)
    elif name == "integers":                          # five distinct values (both zeros among them): heavy ties
        x = rng.integers(-2, 3, (2, 2, 40, 64)).astype(np.float64)
        x[0, 0][x[0, 0] == 0] = -0.0
    elif name == "mostly-zero":                       # 98 % exact zeros, the rest positive: precipitation
        x = rng.random((1, 3, 64, 96))
        x = np.where(x < 0.98, 0.0, 50.0 * (x - 0.98))
    elif name == "inf-and-denormal":                  # the ends of the key range
        x = rng.standard_normal((1, 2, 16, 32))
        x[0, 0, 0, :4] = [np.inf, -np.inf, 1e-42, -1e-42]
        x[0, 1, 3, :3] = [3.4e38, -3.4e38, 0.0]
    else:
        raise KeyError(name)
    x = x.astype(np.float32)
    x.setflags(write=False)
    return x


CASES = ["2x3x9x16", "clustered", "2x73x60x120", "512x1024", "512x1024-constant", "integers", "mostly-zero", "inf-and-denormal"]


@functools.lru_cache(maxsize=None)
def _field_and_sorted(name):
    x = _case(name)
    return x, R.sorted_planes(x)                      # sorted once per case, shared, never modified


def _ranks_for(n):
    """the metric's own ranks at this plane size plus both ends and their neighbours"""
    from swin_v2_weather_amd.utils.weighted_acc_rmse import quantile_levels, quantile_ranks
    r = set(quantile_ranks(n, quantile_levels())[0].tolist()) | {0, 1, n // 2, n - 2, n - 1}
    return np.array(sorted(r), np.int32)


def _launch(lib, dev, x, ranks, ws_fill=SENTINEL):
    """x: device tensor or channel-block view [B, C, H, W]; ranks: numpy int32 -> (values [K, B, C] numpy, nan_count [B, C] numpy, Guarded)"""
    from swin_v2_weather_amd import _lib as L
    B, C, H, W = x.shape
    K = len(ranks)
    wsb = lib.swv2_quantile_ws_bytes(B * C, H, W, K)
    assert wsb == B * C * 35856
    g = Guarded(dev, dtype=torch.int32, ws=wsb // 4, out=K * B * C, nan_count=B * C)
    if ws_fill != SENTINEL:
        g["ws"].fill_(ws_fill)
    d_ranks = torch.tensor(ranks, dtype=torch.int32).to(dev)
    L.check(lib.swv2_plane_order_stats(x.data_ptr(), x.stride(0) if B > 1 else C * H * W, B, C, H, W, d_ranks.data_ptr(), K, g["out"].data_ptr(),
                                       g["nan_count"].data_ptr(), g["ws"].data_ptr(), wsb, torch.cuda.current_stream().cuda_stream),
            "swv2_plane_order_stats")
    torch.cuda.synchronize()
    assert g.guards_intact(), "a kernel wrote outside its outputs"
    assert bool((g["out"] != SENTINEL).all()) and bool((g["nan_count"] != SENTINEL).all()), "outputs left unwritten"
    return g["out"].view(torch.float32).view(K, B, C).cpu().numpy(), g["nan_count"].view(B, C).cpu().numpy(), g


def _same_floats(a, b):
    """equal as floats (so -0.0 == +0.0), NaN where NaN"""
    return np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)])


@pytest.mark.parametrize("name", CASES)
def test_order_statistics_equal_the_sorted_planes(dev, lib, name):
    x, srt = _field_and_sorted(name)
    n = x.shape[2] * x.shape[3]
    ranks = _ranks_for(n)
    assert ranks[0] == 0 and ranks[-1] == n - 1 and len(ranks) <= 256
    got, nan_count, _ = _launch(lib, dev, torch.tensor(x).to(dev), ranks)
    want = srt[..., torch.tensor(ranks, dtype=torch.long)].permute(2, 0, 1).numpy()
    bad = int((got != want).sum())
    print(f"{name}: {len(ranks)} ranks x {x.shape[0] * x.shape[1]} planes of {n}, {bad} values differ from the sorted planes")
    assert np.array_equal(got, want)                  # exact: no tolerance
    assert not nan_count.any()


def test_all_256_ranks_and_a_single_rank(dev, lib):
    x, srt = _field_and_sorted("2x73x60x120")
    n = 60 * 120
    dx = torch.tensor(x).to(dev)
    many = np.unique(np.concatenate([np.linspace(0, n - 1, 250).astype(np.int32), np.arange(n - 7, n, dtype=np.int32)]))
    assert len(many) == 256
    for ranks in (many, np.array([n // 3], np.int32)):
        got, _, _ = _launch(lib, dev, dx, ranks)
        assert np.array_equal(got, srt[..., torch.tensor(ranks, dtype=torch.long)].permute(2, 0, 1).numpy())


def test_channel_block_of_a_wider_tensor_is_read_in_place(dev, lib):
    x, srt = _field_and_sorted("2x73x60x120")
    dx = torch.tensor(x).to(dev)
    blk = dx[:, 20:25]
    assert blk.stride(0) == 73 * 7200 and blk.data_ptr() % 16 == 0 and not blk.is_contiguous()
    ranks = _ranks_for(7200)
    in_place, _, _ = _launch(lib, dev, blk, ranks)
    copied, _, _ = _launch(lib, dev, blk.contiguous(), ranks)
    assert np.array_equal(in_place.view(np.int32), copied.view(np.int32))                       # the same bits
    assert np.array_equal(in_place, srt[:, 20:25][..., torch.tensor(ranks, dtype=torch.long)].permute(2, 0, 1).numpy())


def test_two_runs_and_a_dirty_workspace_give_the_same_bits(dev, lib):
    for name in ("2x73x60x120", "mostly-zero"):
        x, _ = _field_and_sorted(name)
        dx = torch.tensor(x).to(dev)
        ranks = _ranks_for(x.shape[2] * x.shape[3])
        runs = [_launch(lib, dev, dx, ranks, fill) for fill in (SENTINEL, SENTINEL, -1, 0)]       # -1: every byte 0xFF
        for o, c, g in runs[1:]:
            assert np.array_equal(o.view(np.int32), runs[0][0].view(np.int32)) and np.array_equal(c, runs[0][1])
            assert torch.equal(g["ws"], runs[0][2]["ws"])                                        # the workspace ends in the same state, too


def test_nan_in_one_plane(dev, lib):
    from swin_v2_weather_amd.utils import weighted_acc_rmse as M
    x = _case("2x3x9x16").copy()
    x[1, 0, 2, 3] = np.nan
    x[1, 0, 7, 15] = -np.nan
    x[1, 0, 0, 0] = np.float32(np.frombuffer(np.uint32(0xFFFFFFFF).tobytes(), np.float32)[0])    # a third NaN, another payload
    ranks = _ranks_for(144)
    got, nan_count, _ = _launch(lib, dev, torch.tensor(x).to(dev), ranks)
    want = R.order_stats(x, ranks).numpy()                                                       # torch.sort: NaNs last
    assert nan_count[1, 0] == 3 and nan_count.sum() == 3
    assert _same_floats(got, want) and np.isnan(want[-2:, 1, 0]).all() and not np.isnan(np.delete(want.reshape(len(ranks), 6), 3, axis=1)).any()
    q = M.quantile_levels()
    pq = M.plane_quantiles(torch.tensor(x).to(dev), q).cpu().numpy()
    ref, bound = R.quantiles(x, q)
    assert np.isnan(pq[:, 1, 0]).all() and np.isnan(pq).sum() == q.numel() and np.array_equal(np.isnan(pq), np.isnan(ref))
    ok = ~np.isnan(ref)
    assert np.all(np.abs(pq[ok].astype(np.float64) - ref[ok]) <= bound[ok])


@pytest.mark.parametrize("name", ["2x3x9x16", "2x73x60x120", "mostly-zero", "512x1024"])
def test_plane_quantiles_on_cuda_within_the_derived_bound(dev, lib, name):
    from swin_v2_weather_amd.utils import weighted_acc_rmse as M
    x, srt = _field_and_sorted(name)
    q = M.quantile_levels()
    dx = torch.tensor(x).to(dev)
    assert M._quantiles_on_kernels(dx)
    got = M.plane_quantiles(dx, q)
    assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == (100,) + x.shape[:2]
    ref, bound = R.quantiles(x, q, srt)
    r = R.worst(np.abs(got.cpu().numpy().astype(np.float64) - ref), bound)
    print(f"{name}: plane_quantiles worst error / bound {r:.3f}")
    assert r <= 1.0
    # what the kernel cannot take runs torch.quantile on the device and still agrees
    if name == "2x3x9x16":
        odd = dx[..., :15]                                                                       # H * W = 135
        assert not M._quantiles_on_kernels(odd)
        ref_o, bound_o = R.quantiles(x[..., :15], q)
        assert R.worst(np.abs(M.plane_quantiles(odd, q).cpu().numpy().astype(np.float64) - ref_o), bound_o) <= 1.0
        # more levels than one call's 256 ranks can serve: the levels go in chunks, 0 and 1 among them
        many = torch.linspace(0, 1, 300)
        ref_m, bound_m = R.quantiles(x, many, srt)
        got_m = M.plane_quantiles(dx, many)
        assert tuple(got_m.shape) == (300, 2, 3) and R.worst(np.abs(got_m.cpu().numpy().astype(np.float64) - ref_m), bound_m) <= 1.0


def test_top_quantiles_error_on_cuda_against_the_statement_and_the_recorded_reference(dev, lib):
    from swin_v2_weather_amd.utils import weighted_acc_rmse as M
    pred, target = GOLD["pred"], GOLD["target"]
    got = M.top_quantiles_error_torch(torch.tensor(pred).to(dev), torch.tensor(target).to(dev))
    assert got.is_cuda and tuple(got.shape) == (2, 3)
    ref, bound = R.top_quantiles_error(pred, target)
    g = got.cpu().numpy().astype(np.float64)
    print(f"top_quantiles_error_torch worst error / bound: statement {R.worst(np.abs(g - ref), bound):.3f}, "
          f"recorded reference {R.worst(np.abs(g - GOLD['top_quantiles_error_torch']), 2 * bound):.3f}")
    assert np.all(np.abs(g - ref) <= bound)
    # the recorded output is the reference's own fp32 result: it carries the same bound against the statement
    assert np.all(np.abs(g - GOLD["top_quantiles_error_torch"].astype(np.float64)) <= 2 * bound)
    x, _ = _field_and_sorted("2x73x60x120")
    y = (0.7 * x).astype(np.float32)
    got = M.top_quantiles_error_torch(torch.tensor(y).to(dev), torch.tensor(x).to(dev)).cpu().numpy().astype(np.float64)
    ref, bound = R.top_quantiles_error(y, x)
    assert R.worst(np.abs(got - ref), bound) <= 1.0


def test_forecast_scorer_quantile_error_with_offsets_reuses_its_workspace(dev, lib):
    from swin_v2_weather_amd.utils import weighted_acc_rmse as M
    x, _ = _field_and_sorted("2x73x60x120")
    dp = torch.tensor(x).to(dev)
    dt = torch.tensor(np.ascontiguousarray(x[:, ::-1][:, :40])).to(dev)
    sc = M.ForecastScorer(60, 120, 5, dev)
    got = sc.quantile_error(dp, dt, coff_prd=20, coff_tar=7)
    want = M.top_quantiles_error_torch(dp[:, 20:25].contiguous(), dt[:, 7:12].contiguous())
    assert torch.equal(got, want) and tuple(got.shape) == (2, 5)
    ws, ranks = sc._ws[("quantile", 2)], sc._qplan.ranks
    again = sc.quantile_error(dp, dt, coff_prd=20, coff_tar=7)
    assert torch.equal(again, got) and again.data_ptr() != got.data_ptr()
    assert len(sc._ws) == 1 and sc._ws[("quantile", 2)] is ws and sc._qplan.ranks is ranks
    one = sc.quantile_error(dp[:1], dt[:1], coff_prd=20, coff_tar=7)
    assert torch.equal(one, M.top_quantiles_error_torch(dp[:1, 20:25].contiguous(), dt[:1, 7:12].contiguous())) and set(sc._ws) == {("quantile", 1), ("quantile", 2)}
    r = sc.score(dp, dt, coff_prd=20, coff_tar=7)                                                # Scores and score() are what they were
    assert type(r)._fields == ("rmse", "acc", "rmse_mean", "acc_mean", "sums")


def test_refusals_are_made_on_the_host_before_any_launch(dev, lib):
    x = torch.zeros(2, 3, 8, 16, device=dev)
    K = 67
    ranks = torch.arange(K, dtype=torch.int32, device=dev)
    wsb = lib.swv2_quantile_ws_bytes(6, 8, 16, K)
    g = Guarded(dev, dtype=torch.int32, ws=wsb // 4, out=256 * 6, nan_count=6)
    st = torch.cuda.current_stream().cuda_stream

    def call(xp=x.data_ptr(), H=8, W=16, K=K, ws=g["ws"].data_ptr(), wb=wsb):
        return lib.swv2_plane_order_stats(xp, 3 * 8 * 16, 2, 3, H, W, ranks.data_ptr(), K, g["out"].data_ptr(), g["nan_count"].data_ptr(), ws, wb, st)
    before = g.raw.clone()
    for f, word in ((lambda: call(H=9, W=15), b"H * W % 4"), (lambda: call(K=257), b"K outside"), (lambda: call(wb=wsb - 4), b"workspace"),
                    (lambda: call(xp=x.data_ptr() + 4), b"aligned"), (lambda: call(ws=g["ws"].data_ptr() + 8), b"aligned")):
        assert f() == -1
        assert word in lib.swv2_last_error(), lib.swv2_last_error()
    torch.cuda.synchronize()
    assert torch.equal(g.raw, before)                                                            # nothing was launched: nothing was touched
    assert call() == 0
    torch.cuda.synchronize()
    assert g.guards_intact()


def test_score_rollout_with_extremes(dev, lib, tmp_path):
    from swin_v2_weather_amd import inference
    from swin_v2_weather_amd.utils.weighted_acc_rmse import ForecastScorer, _quantiles_on_kernels
    from tests.test_score_gpu import _registry_model
    model = _registry_model(dev, tmp_path)
    B, Cout, H, W, steps = 2, 5, 48, 72, 3
    g = torch.Generator(device=dev).manual_seed(3)
    x0 = torch.randn(B, 9, H, W, device=dev, generator=g)
    cz = torch.rand(B, steps - 1, H, W, device=dev, generator=g) * 2 - 1
    truth = torch.randn(B, steps, Cout, H, W, device=dev, generator=g)
    scorer = ForecastScorer(H, W, Cout, dev, climatology=0.3 * torch.randn(Cout, H, W, device=dev, generator=g))
    plain = inference.score_rollout(model, x0, truth, steps, cz, n_invar=3, scorer=scorer, keep_forecast=True)
    ext = inference.score_rollout(model, x0, truth, steps, cz, n_invar=3, scorer=scorer, keep_forecast=True, extremes=True)
    assert plain.tqe is None and tuple(ext.tqe.shape) == (steps, B, Cout)
    for a, b in zip(plain[:5], ext[:5]):                                                         # rmse, acc, the samples, the forecast
        assert torch.equal(a, b)
    assert torch.equal(ext.forecast, inference.rollout(model, x0, steps, cz, n_invar=3))
    for s in range(steps):
        assert _quantiles_on_kernels(ext.forecast[:, s]) and _quantiles_on_kernels(truth[:, s])
        assert torch.equal(ext.tqe[s], scorer.quantile_error(ext.forecast[:, s], truth[:, s]))
    ring = inference.score_rollout(model, x0, lambda s: truth[:, s].clone(), steps, cz, n_invar=3, scorer=scorer, extremes=True)
    assert ring.forecast is None and torch.equal(ring.tqe, ext.tqe) and torch.equal(ring.rmse, ext.rmse)
    ref, bound = R.top_quantiles_error(ext.forecast[:, 1].cpu().numpy(), truth[:, 1].cpu().numpy())
    assert np.all(np.abs(ext.tqe[1].cpu().numpy().astype(np.float64) - ref) <= bound)


def test_cli_extremes_adds_columns_and_a_key(dev, lib, tmp_path, capsys):
    from swin_v2_weather_amd import inference
    from tests.test_score_gpu import _registry_model
    _registry_model(dev, tmp_path)
    reg = tmp_path / "swin_test_registry"
    rng = np.random.default_rng(11)
    B, Cout, H, W, steps = 2, 5, 48, 72, 2
    np.save(tmp_path / "x0.npy", rng.standard_normal((B, 9, H, W)).astype(np.float32))
    np.save(tmp_path / "truth.npy", rng.standard_normal((B, steps, Cout, H, W)).astype(np.float32))
    base = ["--registry", str(reg), "--steps", str(steps), "--init", str(tmp_path / "x0.npy"), "--truth", str(tmp_path / "truth.npy")]
    inference.main(base + ["--scores-out", str(tmp_path / "plain.json")])
    plain = capsys.readouterr().out.splitlines()
    inference.main(base + ["--scores-out", str(tmp_path / "ext.json"), "--extremes"])
    ext = capsys.readouterr().out.splitlines()
    jp, je = json.load(open(tmp_path / "plain.json")), json.load(open(tmp_path / "ext.json"))
    assert set(jp) == {"lead_hours", "rmse", "acc", "tracked"} and set(je) == set(jp) | {"tqe"}
    assert all(je[k] == jp[k] for k in jp)
    assert plain[1].split() == ["lead_h", "rmse_u10m", "rmse_v10m"] and ext[1].split() == plain[1].split() + ["tqe_u10m", "tqe_v10m"]
    assert plain[0] == ext[0] and len(ext) == len(plain) == 2 + steps
    for s in range(steps):
        assert ext[2 + s].split()[:3] == plain[2 + s].split() and len(ext[2 + s].split()) == 5
        assert float(ext[2 + s].split()[3]) == pytest.approx(je["tqe"][s][0], abs=1e-5)
    assert np.asarray(je["tqe"]).shape == (steps, Cout) and np.isfinite(je["tqe"]).all()
