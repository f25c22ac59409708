"""GPU (-m gpu): swv2_score_sums / swv2_score_finalize through the C ABI, judged element by element against the fp64 statement of
tests/score_reference.py (every bound is derived there), then the Python layer on top of them: the CUDA dispatch of the
utils/weighted_acc_rmse names, ForecastScorer, inference.score_rollout and the Trainer's valid_acc_<var>."""
import functools
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import score_reference as R
from tests.plane_harness import Guarded, _weights, dev, lib  # noqa: F401  (dev, lib: fixtures)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (B, C, H, W): the smallest shapes that reach each branch of the plan (slices: tests/test_score_host.py::PLAN)
SHAPES = [(1, 1, 1, 4),            # a single vector: 2047 empty slices
          (2, 3, 5, 8),            # slices that cut rows
          (1, 2, 33, 132),         # 4356 elements over 1024 slices: most of them empty or a single vector
          (3, 73, 16, 32),         # B * C = 219: 9 slices per plane, a row count the slice boundaries do not divide
          (1, 2100, 2, 4),         # B * C above the slice threshold: one slice per plane
          (1, 2, 720, 1440),       # the real plane size (index width); 1024 slices of ~1012 elements: one vector per thread, tail loop only
          # the 4 x unrolled main loop (a slice of more than 3072 elements), which the production shape B * C = 146 at 720 x 1440 lives in:
          (1, 2048, 64, 64),       # one slice of exactly 4096 elements: one unrolled group per thread, no tail
          (2, 73, 240, 480)]       # B * C = 146, 14 slices of ~8228 elements that cut rows: two unrolled groups (u = 0 .. 3 on different
                                   # rows, 1024 elements = 2.13 rows apart) + a tail for threads 0 .. 8, and the batch stride inside the loop


@functools.lru_cache(maxsize=None)
def _fields(B, C, H, W, seed=0):
    """N(0, 1) fields on a smooth climatology, as numpy fp32 (generated once per shape, never modified)"""
    rng = np.random.default_rng(1000 * seed + B * 7 + C * 3 + H + W)
    y, x = np.linspace(0, np.pi, H)[:, None], np.linspace(0, 2 * np.pi, W)[None, :]
    clim = ((1.0 + np.arange(C)[:, None, None] % 5) * np.sin(y + 0.3 * np.arange(C)[:, None, None]) * np.cos(2 * x)).astype(np.float32)
    prd = (clim[None] + rng.standard_normal((B, C, H, W))).astype(np.float32)
    tar = (clim[None] + rng.standard_normal((B, C, H, W))).astype(np.float32)
    for a in (clim, prd, tar):
        a.setflags(write=False)
    return prd, tar, clim, _weights(H)


def _launch(lib, dev, prd, tar, w, clim, scale=None):
    """prd, tar: device tensors or channel-block views [B, C, H, W]; -> (Guarded with ws / sums / rmse / acc / rmse_mean / acc_mean, slices)"""
    from swin_v2_weather_amd import _lib as L
    B, C, H, W = prd.shape
    slices = lib.swv2_score_slices(B * C, H, W)
    wsb = lib.swv2_score_ws_bytes(B * C, H, W)
    assert wsb == B * C * slices * 16
    g = Guarded(dev, ws=wsb // 4, sums=B * C * 4, rmse=B * C, acc=B * C, rmse_mean=C, acc_mean=C)
    st = torch.cuda.current_stream().cuda_stream
    ps, ts = (prd.stride(0), tar.stride(0)) if B > 1 else (C * H * W, C * H * W)
    L.check(lib.swv2_score_sums(prd.data_ptr(), ps, tar.data_ptr(), ts, None if clim is None else clim.data_ptr(), w.data_ptr(), B, C, H, W,
                                g["ws"].data_ptr(), wsb, st), "swv2_score_sums")
    L.check(lib.swv2_score_finalize(g["ws"].data_ptr(), wsb, B, C, H, W, None if scale is None else scale.data_ptr(), g["sums"].data_ptr(),
                                    g["rmse"].data_ptr(), g["acc"].data_ptr(), g["rmse_mean"].data_ptr(), g["acc_mean"].data_ptr(), st),
            "swv2_score_finalize")
    torch.cuda.synchronize()
    return g, slices


def _verdict(g, slices, prd, tar, w, clim, scale=None, tag=""):
    """the element-by-element judgement of one launch pair (numpy inputs); asserts every bound, the guards and the written slots"""
    B, C, H, W = prd.shape
    assert g.guards_intact(), "a kernel wrote outside its outputs"
    for k in g.sizes:
        assert g.written(k), f"{k}: slots the plan names were left unwritten"
    n = R.chain_length(H, W, slices)
    got = {k: g[k].cpu().numpy() for k in g.sizes}
    rs, rr, ra = R.judge(got["sums"].reshape(B, C, 4), got["rmse"].reshape(B, C), got["acc"].reshape(B, C), prd, tar, w, clim, n, tag)
    assert rs <= 1.0 and rr <= 1.0 and ra <= 1.0
    m_ref, m_b = R.batch_mean(got["rmse"].reshape(B, C), scale)
    a_ref, a_b = R.batch_mean(got["acc"].reshape(B, C))
    nan = np.isnan(a_ref)
    assert np.array_equal(np.isnan(got["acc_mean"]), nan)
    rm, am = R.worst(np.abs(got["rmse_mean"] - m_ref), m_b), R.worst(np.abs(got["acc_mean"] - a_ref)[~nan], a_b[~nan])
    print(f"{tag} batch means: worst error / bound  rmse_mean {rm:.3f}  acc_mean {am:.3f}")
    assert rm <= 1.0 and am <= 1.0
    return got


@pytest.mark.parametrize("with_clim", [False, True], ids=["noclim", "clim"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernels_element_by_element_against_fp64(dev, lib, shape, with_clim):
    prd, tar, clim, w = _fields(*shape)
    d = [torch.tensor(a).to(dev) for a in (prd, tar, clim, w)]
    g, slices = _launch(lib, dev, d[0], d[1], d[3], d[2] if with_clim else None)
    _verdict(g, slices, prd, tar, w, clim if with_clim else None, tag=f"{shape} clim={with_clim}")


def test_channel_block_of_wider_tensors_with_different_strides(dev, lib):
    """channels 5:10 of a 15-channel prediction against channels 5:10 of an 18-channel truth, scored in place"""
    B, C, H, W = 2, 5, 9, 12
    prd_w, _, _, w = _fields(B, 15, H, W)
    tar_w = _fields(B, 18, H, W, seed=1)[1]
    clim = _fields(B, 15, H, W)[2][5:10]
    dp, dt = torch.tensor(prd_w).to(dev), torch.tensor(tar_w).to(dev)
    vp, vt = dp[:, 5:10], dt[:, 5:10]
    assert vp.stride(0) == 15 * H * W and vt.stride(0) == 18 * H * W and vp.data_ptr() % 16 == 0
    g, slices = _launch(lib, dev, vp, vt, torch.tensor(w).to(dev), torch.tensor(np.ascontiguousarray(clim)).to(dev))
    assert slices == 204
    _verdict(g, slices, prd_w[:, 5:10], tar_w[:, 5:10], w, clim, tag="block 5:10")


def test_nan_in_one_plane_only_bit_identical_reruns_and_scale(dev, lib):
    """prd == clim in one plane: 0 / 0 = NaN ACC there (and in that channel's batch mean), every other value judged as usual; a second
    launch pair gives the same bits; the scale vector reaches rmse_mean only"""
    B, C, H, W = 3, 4, 16, 32
    prd, tar, clim, w = _fields(B, C, H, W)
    prd = prd.copy()
    prd[1, 2] = clim[2]
    scale = np.array([2.0, 0.5, 3.0, 7.25], np.float32)
    d = [torch.tensor(a).to(dev) for a in (prd, tar, clim, w, scale)]
    g1, slices = _launch(lib, dev, d[0], d[1], d[3], d[2], d[4])
    got = _verdict(g1, slices, prd, tar, w, clim, scale, tag="nan plane")
    nan = np.isnan(got["acc"].reshape(B, C))
    assert nan[1, 2] and nan.sum() == 1 and np.isnan(got["acc_mean"][2]) and np.isnan(got["acc_mean"]).sum() == 1
    assert np.all(np.isfinite(got["rmse"])) and np.all(np.isfinite(got["rmse_mean"]))
    g2, _ = _launch(lib, dev, d[0], d[1], d[3], d[2], d[4])
    assert torch.equal(g1.raw, g2.raw)                        # workspace, sums, scores and means, bit for bit (NaN compared as bits)
    g3, _ = _launch(lib, dev, d[0], d[1], d[3], d[2], None)
    for k in ("ws", "sums", "rmse", "acc", "acc_mean"):
        assert torch.equal(g3[k].view(torch.int32), g1[k].view(torch.int32)), k
    assert not torch.equal(g3["rmse_mean"], g1["rmse_mean"])
    # RMSE does not depend on the climatology: the same S_dd bits without it
    g4, _ = _launch(lib, dev, d[0], d[1], d[3], None, None)
    assert torch.equal(g4["sums"].view(B, C, 4)[..., 0], g3["sums"].view(B, C, 4)[..., 0]) and torch.equal(g4["rmse"], g3["rmse"])


# ---- the Python layer ------------------------------------------------------------------------------------------------------
def _judge_names(M, pred, target, n, tag):
    """the five reference names on device tensors against fp64 with chain length n"""
    p, t = pred.cpu().numpy(), target.cpu().numpy()
    B, C, H, W = p.shape
    for weighted in (True, False):
        w = _weights(H) if weighted else np.ones(H, np.float32)
        S, A = R.sums(p, t, w)
        dS = R.sum_bounds(A, n)
        (r_ref, r_b), (a_ref, a_b) = R.rmse(S, dS, H, W), R.acc(S, dS)
        pre = "weighted" if weighted else "unweighted"
        a = getattr(M, pre + "_acc_torch_channels")(pred, target)
        am = getattr(M, pre + "_acc_torch")(pred, target)
        assert a.is_cuda and a.dtype == torch.float32 and tuple(a.shape) == (B, C) and tuple(am.shape) == (C,)
        ra = R.worst(np.abs(a.cpu().numpy() - a_ref), a_b)
        m_ref, m_b = R.batch_mean(a.cpu().numpy())
        rm = R.worst(np.abs(am.cpu().numpy() - m_ref), m_b)
        print(f"{tag} {pre}: worst error / bound  acc {ra:.3f}  acc mean {rm:.3f}")
        assert ra <= 1.0 and rm <= 1.0
        if weighted:
            r = M.weighted_rmse_torch_channels(pred, target)
            rr = R.worst(np.abs(r.cpu().numpy() - r_ref), r_b)
            print(f"{tag}: worst error / bound  rmse {rr:.3f}")
            assert rr <= 1.0 and tuple(r.shape) == (B, C)


def test_cuda_dispatch_of_the_reference_names_against_fp64(dev, lib):
    from swin_v2_weather_amd import ops
    from swin_v2_weather_amd.utils import weighted_acc_rmse as M
    B, C, H, W = 2, 3, 33, 132
    prd, tar, _, _ = _fields(B, C, H, W)
    dp, dt = torch.tensor(prd).to(dev), torch.tensor(tar).to(dev)
    assert M._on_kernels(dp, dt)
    _judge_names(M, dp, dt, R.chain_length(H, W, ops.score_slices(B * C, H, W)), "kernels")
    # a channel block is scored in place; anything the kernels cannot take runs plain torch (any order of H W terms) and still agrees
    wide = torch.randn(B, C + 4, H, W, device=dev)
    assert M._on_kernels(wide[:, 2:2 + C], dt)
    _judge_names(M, wide[:, 2:2 + C], dt, R.chain_length(H, W, ops.score_slices(B * C, H, W)), "kernels, channel block")
    nc = torch.randn(B, C, W, H, device=dev).transpose(2, 3)                     # planes not contiguous
    assert not M._on_kernels(nc, dt) and nc.shape == dt.shape
    _judge_names(M, nc, dt, H * W, "torch, non-contiguous")
    odd_p, odd_t = torch.randn(B, C, H, 130, device=dev), torch.randn(B, C, H, 130, device=dev)      # W % 4 != 0
    assert not M._on_kernels(odd_p, odd_t)
    _judge_names(M, odd_p, odd_t, H * 130, "torch, W % 4 != 0")
    # the weights on the device are the CPU's, bit for bit
    assert torch.equal(M.latitude_weights(H, dev).cpu(), M.latitude_weights(H)) and M.latitude_weights(H, dev) is M.latitude_weights(H, dev)


def test_forecast_scorer_against_fp64(dev, lib):
    from swin_v2_weather_amd import ops
    from swin_v2_weather_amd.utils.weighted_acc_rmse import ForecastScorer
    B, C, H, W = 2, 5, 9, 12
    prd_w, _, clim_w, w = _fields(B, 15, H, W)
    tar_w = _fields(B, 18, H, W, seed=1)[1]
    clim = np.ascontiguousarray(clim_w[5:10])
    stds = np.array([1.5, 2.0, 0.25, 9.0, 4.0], np.float32)
    dp, dt = torch.tensor(prd_w).to(dev), torch.tensor(tar_w).to(dev)
    n = R.chain_length(H, W, ops.score_slices(B * C, H, W))
    for cl in (clim, None):
        sc = ForecastScorer(H, W, C, dev, climatology=cl, stds=stds)
        r = sc.score(dp, dt, coff_prd=5, coff_tar=7)
        p, t = prd_w[:, 5:10], tar_w[:, 7:12]
        # (without a climatology the scorer hands out no ACC: the uncentred ratio of its sums stands in, three fp32 operations as in the kernel)
        acc = r.acc.cpu().numpy() if cl is not None else (r.sums[..., 1] / torch.sqrt(r.sums[..., 2] * r.sums[..., 3])).cpu().numpy()
        rs, rr, ra = R.judge(r.sums.cpu().numpy(), r.rmse.cpu().numpy(), acc, p, t, w, cl, n, f"ForecastScorer clim={cl is not None}")
        assert rs <= 1.0 and rr <= 1.0 and ra <= 1.0
        m_ref, m_b = R.batch_mean(r.rmse.cpu().numpy(), stds)
        assert np.all(np.abs(r.rmse_mean.cpu().numpy() - m_ref) <= m_b)
        if cl is None:
            assert r.acc is None and r.acc_mean is None
        else:
            a_ref, a_b = R.batch_mean(r.acc.cpu().numpy())
            assert np.all(np.abs(r.acc_mean.cpu().numpy() - a_ref) <= a_b)
        if cl is not None:
            sc_clim_sums = r.sums
        r2 = sc.score(dp, dt, coff_prd=5, coff_tar=7)                            # the workspace is reused; results are fresh tensors
        assert torch.equal(r2.rmse, r.rmse) and r2.rmse.data_ptr() != r.rmse.data_ptr() and len(sc._ws) == 1
    # a device given without an index is the current device: the kernel path all the same, the same bits
    named = ForecastScorer(H, W, C, "cuda", climatology=clim, stds=stds)
    assert named.device == dp.device and len(named._ws) == 0
    assert torch.equal(named.score(dp, dt, 5, 7).sums, sc_clim_sums) and len(named._ws) == 1
    # odd width: the torch path on the device, judged as a sum in any order
    Wo = 10
    po, to_ = np.ascontiguousarray(prd_w[..., :Wo]), np.ascontiguousarray(tar_w[..., :Wo])
    co = np.ascontiguousarray(clim[..., :Wo])
    r = ForecastScorer(H, Wo, C, dev, climatology=co).score(torch.tensor(po).to(dev), torch.tensor(to_).to(dev), 5, 7)
    rs, rr, ra = R.judge(r.sums.cpu().numpy(), r.rmse.cpu().numpy(), r.acc.cpu().numpy(), po[:, 5:10], to_[:, 7:12], w, co, H * Wo, "ForecastScorer torch path")
    assert rs <= 1.0 and rr <= 1.0 and ra <= 1.0


def _registry_model(dev, tmp_path):
    """the tiny registry folder of tests/test_gpu_parity.py::test_registry_checkpoint_and_inference_rollout (same construction)"""
    import yaml
    from swin_v2_weather_amd import inference
    from swin_v2_weather_amd.networks import helpers
    hp = dict(nettype="swin", img_size=[48, 72], patch_size=4, depth=2, num_heads=2, embed_dim=24, window_ratio=8,
              drop_path_rate=0.1, full_pos_embed=True, rel_pos=True, mlp_ratio=4, activation_ckpt=False, residual=True,
              in_channels=list(range(5)), out_channels=list(range(5)), add_zenith=True, add_orography=True, add_landmask=True,
              n_in_channels=9, n_out_channels=5, n_future=2, lr="1E-3")
    reg = tmp_path / "swin_test_registry"
    reg.mkdir()
    yaml.safe_dump(hp, open(reg / "hyperparams.yaml", "w"))
    torch.manual_seed(31)
    ms = helpers.get_model(SimpleNamespace(**hp))
    with torch.no_grad():
        for n_, p_ in ms.named_parameters():
            if n_.endswith("norm1.weight") or n_.endswith("norm2.weight"):
                p_.uniform_(0.5, 1.5)
    torch.save({"iters": 7, "epoch": 1, "model_state": {"module." + k: v for k, v in ms.state_dict().items()},
                "optimizer_state_dict": {}}, reg / "weights.tar")
    np.save(reg / "global_means.npy", np.zeros((1, 73, 1, 1), np.float32))
    np.save(reg / "global_stds.npy", np.full((1, 73, 1, 1), 2.0, np.float32))
    model, p, _ = inference.load_registry_model(str(reg), dev)
    return model


def test_score_rollout_equals_rollout_and_the_scorer_on_the_stored_forecast(dev, lib, tmp_path):
    from swin_v2_weather_amd import inference
    from swin_v2_weather_amd.utils.weighted_acc_rmse import ForecastScorer
    model = _registry_model(dev, tmp_path)
    B, Cout, H, W, steps = 2, 5, 48, 72, 3
    g = torch.Generator(device=dev).manual_seed(3)
    x0 = torch.randn(B, 9, H, W, device=dev, generator=g)
    cz = torch.rand(B, steps - 1, H, W, device=dev, generator=g) * 2 - 1
    truth = torch.randn(B, steps, Cout, H, W, device=dev, generator=g)
    clim = 0.3 * torch.randn(Cout, H, W, device=dev, generator=g)
    stds = torch.tensor([1.0, 2.0, 3.0, 4.0, 5.0], device=dev)
    scorer = ForecastScorer(H, W, Cout, dev, climatology=clim, stds=stds)
    y = inference.rollout(model, x0, steps, cz, n_invar=3)
    kept = inference.score_rollout(model, x0, truth, steps, cz, n_invar=3, scorer=scorer, keep_forecast=True)
    assert torch.equal(kept.forecast, y)                                         # the predictions are rollout's, bit for bit
    assert kept.rmse.shape == (steps, Cout) and kept.acc.shape == (steps, Cout) and kept.rmse_samples.shape == (steps, B, Cout)
    from swin_v2_weather_amd.utils.weighted_acc_rmse import _on_kernels
    ring_buf = torch.empty(B, 2 * Cout, H, W, device=dev)
    for s in range(steps):                                                       # scores = the scorer on the stored forecast, bit for bit
        # what score_rollout hands the scorer is what the HIP kernels take in place: a slot of the ring / of the kept forecast, truth[:, s]
        assert _on_kernels(ring_buf[:, (s % 2) * Cout:(s % 2 + 1) * Cout], truth[:, s]) and _on_kernels(kept.forecast[:, s], truth[:, s])
        r = scorer.score(y[:, s], truth[:, s])
        assert torch.equal(kept.rmse[s], r.rmse_mean) and torch.equal(kept.acc[s], r.acc_mean)
        assert torch.equal(kept.rmse_samples[s], r.rmse) and torch.equal(kept.acc_samples[s], r.acc)
    ring = inference.score_rollout(model, x0, truth, steps, cz, n_invar=3, scorer=scorer)
    assert ring.forecast is None
    fn = inference.score_rollout(model, x0, lambda s: truth[:, s].clone(), steps, cz, n_invar=3, scorer=scorer)
    for other in (ring, fn):                                                     # the two-slot ring and a callable truth change nothing
        for a, b in zip(other[:4], kept[:4]):
            assert torch.equal(a, b)
    plain = inference.score_rollout(model, x0, truth, steps, cz, n_invar=3)      # default scorer: no climatology, normalised units
    assert plain.acc is None and plain.acc_samples is None and torch.equal(plain.rmse_samples, kept.rmse_samples)
    assert torch.equal(plain.rmse[1], ForecastScorer(H, W, Cout, dev).score(y[:, 1], truth[:, 1]).rmse_mean)


def test_cli_scores_a_truth_file_per_lead_time(dev, lib, tmp_path, capsys):
    """python -m swin_v2_weather_amd.inference --truth ...: the table and the JSON hold score_rollout's numbers with the registry's
    climatology (time_means.npy, normalised with its global means / stds) and physical units (global_stds.npy)"""
    import json
    from swin_v2_weather_amd import inference
    from swin_v2_weather_amd.utils.data_loader_era5 import cos_zenith
    from swin_v2_weather_amd.utils.weighted_acc_rmse import ForecastScorer
    model = _registry_model(dev, tmp_path)
    reg = tmp_path / "swin_test_registry"
    rng = np.random.default_rng(11)
    B, Cout, H, W, steps = 2, 5, 48, 72, 3
    tm = rng.standard_normal((1, 73, 49, 80)).astype(np.float32)
    x0, truth = rng.standard_normal((B, 9, H, W)).astype(np.float32), rng.standard_normal((B, steps + 1, Cout, H, W)).astype(np.float32)
    np.save(reg / "time_means.npy", tm); np.save(tmp_path / "x0.npy", x0); np.save(tmp_path / "truth.npy", truth)
    inference.main(["--registry", str(reg), "--steps", str(steps), "--init", str(tmp_path / "x0.npy"), "--truth", str(tmp_path / "truth.npy"),
                    "--scores-out", str(tmp_path / "scores.json")])
    out = capsys.readouterr().out.splitlines()
    js = json.load(open(tmp_path / "scores.json"))
    scorer = ForecastScorer(H, W, Cout, dev, climatology=tm[0, :Cout, :H, :W] / 2.0, stds=np.full(Cout, 2.0, np.float32))
    cz = torch.stack([cos_zenith(2018, 6.0 * (s + 1), H, W) for s in range(steps - 1)], 0).unsqueeze(0).expand(B, -1, -1, -1).to(dev)
    want = inference.score_rollout(model, torch.tensor(x0).to(dev), torch.tensor(truth).to(dev), steps, cz, 3, scorer)
    assert js["lead_hours"] == [6.0, 12.0, 18.0] and js["tracked"] == {"u10m": 0, "v10m": 1}
    assert js["rmse"] == want.rmse.cpu().tolist() and js["acc"] == want.acc.cpu().tolist()
    assert "physical units" in out[0] and "with ACC" in out[0] and out[1].split() == ["lead_h", "rmse_u10m", "rmse_v10m", "acc_u10m", "acc_v10m"]
    assert len(out) == 2 + steps and float(out[3].split()[1]) == pytest.approx(js["rmse"][1][0], abs=1e-5)


def test_trainer_logs_valid_acc_when_time_means_is_a_file(dev, lib, tmp_path):
    """the construction of tests/test_gpu_parity.py::test_trainer_end_to_end_with_checkpoint_resume plus a temporary time_means.npy:
    validation logs valid_acc_<var> = a by-hand ForecastScorer pass, and everything it logged before keeps its value"""
    from swin_v2_weather_amd.train import Trainer
    from swin_v2_weather_amd.utils.YParams import YParams
    from swin_v2_weather_amd.utils.weighted_acc_rmse import ForecastScorer, _on_kernels, load_climatology
    p = YParams(os.path.join(ROOT, "swin_v2_weather_amd", "config", "swin.yaml"), "bench_tiny")
    p["img_size"] = [96, 144]
    p["window_ratio"] = 16
    p["embed_dim"], p["num_heads"], p["depth"] = 32, 2, 2
    p["in_channels"], p["out_channels"] = list(range(6)), list(range(6))
    p["channel_names"] = p["channel_names"][:6]
    p["track_channels"] = ["u10m", "t2m"]
    p["batch_size"], p["max_epochs"] = 2, 1
    p["synthetic_device_pool"], p["synthetic_steps_per_epoch"] = 2, 3
    p["exp_dir"], p["save_checkpoint"], p["log_to_screen"] = str(tmp_path), False, False
    p["loss"], p["drop_path_rate"], p["rel_pos"] = "squared geometric l2", 0.1, True
    t = Trainer(p, SimpleNamespace(sweep_id=None, config="bench_tiny", run_num="00", enable_amp=True))
    t.build()
    assert not os.path.isfile(str(p["time_means_path"]) if "time_means_path" in p else "")
    _, before = t.validate_one_epoch()
    assert set(before) == {"valid_loss", "valid_rmse_u10m", "valid_rmse_t2m"} and t._scorer is None
    tm = 0.5 * np.random.default_rng(0).standard_normal((1, 8, 97, 150)).astype(np.float32)
    np.save(tmp_path / "time_means.npy", tm)
    t.params["time_means_path"] = str(tmp_path / "time_means.npy")
    del t._scorer
    _, after = t.validate_one_epoch()
    assert set(after) == set(before) | {"valid_acc_u10m", "valid_acc_t2m"}
    # computed as before.  valid_rmse_* come from torch reductions of a deterministic forward, valid_loss from swv2_loss_sums, whose order
    # of additions the plan alone fixes (no atomics), and the deterministic swv2_loss_finalize: the same bits
    for k in ("valid_loss", "valid_rmse_u10m", "valid_rmse_t2m"):
        assert np.array_equal(np.asarray(before[k]), np.asarray(after[k])), k
    # by hand: the same batches through the same model and a scorer of one's own
    clim = load_climatology(t.params)
    assert clim.shape == (6, 96, 144) and np.array_equal(clim, tm[0, :6, :96, :144])
    sc = ForecastScorer(96, 144, 6, dev, climatology=clim)
    vals = []
    with torch.no_grad():
        for data in t.valid_data_loader:
            inp, tar, coszen = t.preprocessor(data)
            gen = t.model(inp, coszen=coszen).float()
            assert _on_kernels(gen[:, -6:], tar[:, -6:]) and t._scorer.device == gen.device      # the Trainer's scorer ran the HIP kernels
            vals.append(sc.score(gen[:, -6:], tar[:, -6:]).acc_mean.cpu().numpy())
    ref, b = R.batch_mean(np.stack(vals))                                        # the trainer adds the steps in fp32, then divides
    idx = {"u10m": t.params.channel_names.index("u10m"), "t2m": t.params.channel_names.index("t2m")}
    for var, i in idx.items():
        e = abs(float(after[f"valid_acc_{var}"]) - ref[i])
        print(f"valid_acc_{var} = {after[f'valid_acc_{var}']:.6f}: error / bound {e / b[i] if e else 0.0:.3f}")
        assert e <= b[i] and abs(ref[i]) <= 1.0
