"""CPU: the forecast-scoring names of utils/weighted_acc_rmse.py on their plain-torch path against the reference's recorded outputs
(tests/golden/metrics.npz) and the fp64 statement (tests/score_reference.py), the climatology loader, and the host half of the
swv2_score_* entry points (plan, workspace arithmetic, refusals) -- no GPU call."""
import os

import numpy as np
import pytest
import torch

from swin_v2_weather_amd import _lib as L
from swin_v2_weather_amd.utils import weighted_acc_rmse as M
from tests import score_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "metrics.npz"))

# the shapes of tests/test_score_gpu.py: (B, C, H, W) -> slices of the plan
PLAN = {(1, 1, 1, 4): 2048, (2, 3, 5, 8): 341, (1, 2, 33, 132): 1024, (3, 73, 16, 32): 9, (1, 2100, 2, 4): 1, (1, 2, 720, 1440): 1024,
        (2, 5, 9, 12): 204, (1, 2048, 64, 64): 1, (2, 73, 240, 480): 14}


def _gold_inputs():
    return torch.from_numpy(GOLD["pred"]), torch.from_numpy(GOLD["target"])


def _reference(prd, tar, weighted):
    """fp64 values and torch-path bounds (n = H W: any order) of the channel functions for numpy fp32 inputs"""
    B, C, H, W = prd.shape
    w = M.latitude_weights(H).numpy() if weighted else np.ones(H, np.float32)
    S, A = R.sums(prd, tar, w)
    dS = R.sum_bounds(A, H * W)
    return R.rmse(S, dS, H, W), R.acc(S, dS)


def test_latitude_weights_equal_the_formula_bit_for_bit():
    for n in (2, 9, 33, 720, 721):
        j = torch.arange(0, n)
        coslat = torch.cos(3.1416 / 180.0 * (90.0 - j * 180.0 / float(n - 1)))
        want = n * coslat / coslat.sum()
        got = M.latitude_weights(n)
        assert got.dtype == torch.float32 and got.device.type == "cpu" and torch.equal(got, want)
        assert M.latitude_weights(n) is got and M.latitude_weights(n, "cpu") is got              # cached per device
    assert np.array_equal(M.latitude_weights(9).numpy(), GOLD["weights"])                       # the reference's own, as recorded
    # both pole rows are NEGATIVE in fp32 (cos(3.1416 / 180 * 90) < 0): why the bounds of score_reference use |w|
    for n in (9, 720):
        w = M.latitude_weights(n)
        assert w[0] < 0 and w[-1] < 0 and bool((w[1:-1] > 0).all())
        assert -1e-5 < float(w[0]) < -1e-6


@pytest.mark.parametrize("name", ["weighted_rmse_torch_channels", "weighted_acc_torch_channels", "weighted_acc_torch",
                                  "unweighted_acc_torch_channels", "unweighted_acc_torch"])
def test_torch_path_against_the_recorded_reference_outputs_and_fp64(name):
    """each new name on CPU tensors: within the reordered-sum bound of the fp64 value, and within twice that bound of what the
    reference's own function returned for the same inputs (both are fp32 sums of the same H W terms in an order of their own)"""
    pred, target = _gold_inputs()
    got = getattr(M, name)(pred, target)
    gold = GOLD[name]
    assert got.dtype == torch.float32 and tuple(got.shape) == gold.shape
    (r_ref, r_b), (a_ref, a_b) = _reference(GOLD["pred"], GOLD["target"], not name.startswith("unweighted"))
    ref, b = (r_ref, r_b) if "rmse" in name else (a_ref, a_b)
    if not name.endswith("_channels"):
        B = ref.shape[0]
        ref, b = ref.mean(axis=0), b.mean(axis=0) + R.gamma(B + 1) * np.abs(ref).mean(axis=0)
    e64, eg = np.abs(got.numpy().astype(np.float64) - ref), np.abs(got.numpy().astype(np.float64) - gold.astype(np.float64))
    print(f"{name}: worst error / bound vs fp64 {R.worst(e64, b):.3f}, vs the recorded reference {R.worst(eg, 2 * b):.3f}")
    assert np.all(e64 <= b) and np.all(eg <= 2 * b)
    assert np.all(np.abs(gold.astype(np.float64) - ref) <= b)                                 # the fixture itself sits inside the bound


def test_existing_weighted_rmse_torch_is_unchanged_and_matches_the_fixture():
    pred, target = _gold_inputs()
    got = M.weighted_rmse_torch(pred, target)
    (r_ref, r_b), _ = _reference(GOLD["pred"], GOLD["target"], True)
    b = r_b.mean(axis=0) + R.gamma(3) * np.abs(r_ref).mean(axis=0)
    assert np.all(np.abs(got.numpy().astype(np.float64) - GOLD["weighted_rmse_torch"]) <= 2 * b)
    assert torch.equal(got, M.weighted_rmse_torch_channels(pred, target).mean(dim=0))


@pytest.mark.parametrize("with_clim", [False, True])
def test_forecast_scorer_torch_path_against_fp64(with_clim):
    rng = np.random.default_rng(5)
    B, C, H, W = 2, 3, 9, 10                                  # W % 4 != 0 too: the path any device takes for odd widths
    clim = (np.sin(np.linspace(0, 3, H))[None, :, None] * np.cos(np.linspace(0, 6, W))[None, None, :] * np.arange(1, C + 1)[:, None, None]).astype(np.float32)
    prd = (clim[None] + rng.standard_normal((B, C + 2, H, W))[:, 1:C + 1]).astype(np.float32)
    wide = rng.standard_normal((B, C + 2, H, W)).astype(np.float32)
    wide[:, 2:] = clim[None] + rng.standard_normal((B, C, H, W))
    stds = np.array([2.0, 0.5, 7.0], np.float32)
    sc = M.ForecastScorer(H, W, C, "cpu", climatology=clim if with_clim else None, stds=stds)
    r = sc.score(torch.from_numpy(prd), torch.from_numpy(wide), coff_tar=2)
    tar = wide[:, 2:]
    w = M.latitude_weights(H).numpy()
    n = H * W
    if not with_clim:
        assert r.acc is None and r.acc_mean is None
    S, A = R.sums(prd, tar, w, clim if with_clim else None)
    dS = R.sum_bounds(A, n)
    assert np.all(np.abs(r.sums.numpy().astype(np.float64) - S) <= dS)
    r_ref, r_b = R.rmse(S, dS, H, W)
    assert np.all(np.abs(r.rmse.numpy().astype(np.float64) - r_ref) <= r_b)
    m_ref, m_b = R.batch_mean(r.rmse.numpy(), stds)
    assert np.all(np.abs(r.rmse_mean.numpy().astype(np.float64) - m_ref) <= m_b)
    if with_clim:
        a_ref, a_b = R.acc(S, dS)
        assert np.all(np.abs(r.acc.numpy().astype(np.float64) - a_ref) <= a_b)
        m_ref, m_b = R.batch_mean(r.acc.numpy())
        assert np.all(np.abs(r.acc_mean.numpy().astype(np.float64) - m_ref) <= m_b)
        # RMSE does not depend on the climatology
        assert torch.equal(r.rmse, M.ForecastScorer(H, W, C, "cpu").score(torch.from_numpy(prd), torch.from_numpy(wide), coff_tar=2).rmse)
    with pytest.raises(ValueError):
        sc.score(torch.from_numpy(prd), torch.from_numpy(wide), coff_tar=3)                   # only two channels are left from there
    with pytest.raises(ValueError):
        M.ForecastScorer(H, W, C, "cpu", climatology=clim[:2])


def test_load_climatology_crops_selects_channels_and_normalises(tmp_path):
    rng = np.random.default_rng(1)
    tm = rng.standard_normal((1, 7, 11, 20)).astype(np.float32)
    means, stds = rng.standard_normal((1, 7, 1, 1)).astype(np.float32), (1 + rng.random((1, 7, 1, 1))).astype(np.float32)
    np.save(tmp_path / "tm.npy", tm); np.save(tmp_path / "gm.npy", means); np.save(tmp_path / "gs.npy", stds)
    chans = [4, 0, 5]
    p = dict(time_means_path=str(tmp_path / "tm.npy"), global_means_path=str(tmp_path / "gm.npy"), global_stds_path=str(tmp_path / "gs.npy"),
             img_size=[10, 16], out_channels=np.array(chans))
    c = M.load_climatology(p)
    assert c.shape == (3, 10, 16) and c.dtype == np.float32 and c.flags["C_CONTIGUOUS"]
    assert np.array_equal(c, ((tm[:, chans, :10, :16] - means[:, chans]) / stds[:, chans])[0])
    # statistics given by the caller (a registry's global_means.npy / global_stds.npy) replace the params' files
    c2 = M.load_climatology(p, means=np.zeros_like(means), stds=np.ones_like(stds))
    assert np.array_equal(c2, tm[0, chans, :10, :16])
    # no stats files: unit stds, zero means
    assert np.array_equal(M.load_climatology(dict(p, global_means_path=None, global_stds_path=str(tmp_path / "absent.npy"))), tm[0, chans, :10, :16])
    # time_means_path not a file (every shipped config on a machine without the data), or absent: None
    assert M.load_climatology(dict(p, time_means_path=str(tmp_path / "absent.npy"))) is None
    assert M.load_climatology({k: v for k, v in p.items() if k != "time_means_path"}) is None
    from swin_v2_weather_amd.utils.YParams import YParams
    y = YParams(os.path.join(ROOT, "swin_v2_weather_amd", "config", "swin.yaml"), "bench_tiny")
    assert M.load_climatology(y) is None


def test_abi_version_plan_and_workspace_arithmetic():
    assert L.ABI_VERSION == 113
    lib = L.load()
    assert lib.swv2_version() == 113
    for (B, C, H, W), slices in PLAN.items():
        assert lib.swv2_score_slices(B * C, H, W) == slices == R.plan_slices(B * C), (B, C, H, W)
        assert lib.swv2_score_ws_bytes(B * C, H, W) == B * C * slices * 16
        b = R.slice_bounds(H * W, slices)
        assert b[0][0] == 0 and b[-1][1] == H * W and all(lo % 4 == 0 and lo <= hi for lo, hi in b) and all(x[1] == y[0] for x, y in zip(b, b[1:]))
    assert lib.swv2_score_slices(2047, 4, 4) == 1 and lib.swv2_score_slices(2048, 4, 4) == 1 and lib.swv2_score_slices(1024, 4, 4) == 2
    assert lib.swv2_score_slices(146, 720, 1440) == 14
    for bad in ((0, 4, 4), (4, 0, 4), (4, 4, 0), (-1, 4, 4)):
        assert lib.swv2_score_slices(*bad) == 0 and lib.swv2_score_ws_bytes(*bad) == 0
    # chain lengths of the plan at the sizes the GPU tests use (thread + 6 + 2 + fold + 6)
    assert R.chain_length(1, 4, 2048) == 4 + 14 + 32 and R.chain_length(720, 1440, 1024) == 4 + 14 + 16
    assert R.chain_length(720, 1440, 14) == 4 * 73 + 14 + 1 and R.chain_length(2, 4, 1) == 4 + 14 + 1
    # the two shapes that reach the unrolled main loop (a slice of more than 3072 elements): 4 and 9 vectors per thread
    assert R.chain_length(64, 64, 1) == 4 * 4 + 14 + 1 and R.chain_length(240, 480, 14) == 4 * 9 + 14 + 1
    assert max(hi - lo for lo, hi in R.slice_bounds(240 * 480, 14)) == 8232 and any(lo % 480 for lo, _ in R.slice_bounds(240 * 480, 14))


def test_every_refusal_returns_invalid_with_a_message_and_without_a_gpu():
    """Arguments are checked before anything is launched, so the pointers only have to be non-null here: a refused call touches nothing."""
    lib = L.load()
    P = 4096                                          # any non-null, 16-byte aligned value: never dereferenced by a refused call
    B, C, H, W = 2, 3, 8, 16
    ok = lib.swv2_score_ws_bytes(B * C, H, W)

    def sums(prd=P, ps=C * H * W, tar=P, ts=C * H * W, clim=P, w=P, B=B, C=C, H=H, W=W, ws=P, wb=ok):
        return lib.swv2_score_sums(prd, ps, tar, ts, clim, w, B, C, H, W, ws, wb, None)

    def fin(ws=P, wb=ok, B=B, C=C, H=H, W=W, scale=None, s=P, r=P, a=P, rm=P, am=P):
        return lib.swv2_score_finalize(ws, wb, B, C, H, W, scale, s, r, a, rm, am, None)
    for call, word in ((lambda: sums(prd=None), b"null"), (lambda: sums(tar=None), b"null"), (lambda: sums(w=None), b"null"),
                       (lambda: sums(ws=None), b"null"), (lambda: sums(W=18), b"W % 4"), (lambda: sums(W=0), b"shape"),
                       (lambda: sums(B=0), b"shape"), (lambda: sums(prd=P + 4), b"aligned"), (lambda: sums(tar=P + 8), b"aligned"),
                       (lambda: sums(clim=P + 4), b"aligned"), (lambda: sums(ws=P + 4), b"aligned"), (lambda: sums(ps=C * H * W + 2), b"stride"),
                       (lambda: sums(ts=C * H * W + 1), b"stride"), (lambda: sums(ps=H * W), b"stride"), (lambda: sums(wb=ok - 1), b"workspace"),
                       (lambda: sums(wb=0), b"workspace"), (lambda: sums(B=1 << 12, C=1 << 8), b"shape"),
                       (lambda: fin(ws=None), b"null"), (lambda: fin(s=None), b"null"), (lambda: fin(r=None), b"null"),
                       (lambda: fin(a=None), b"null"), (lambda: fin(rm=None), b"null"), (lambda: fin(am=None), b"null"),
                       (lambda: fin(wb=ok - 16), b"workspace"), (lambda: fin(s=P + 4), b"aligned"), (lambda: fin(C=0), b"shape")):
        assert call() == -1
        assert word in lib.swv2_last_error(), lib.swv2_last_error()
    with pytest.raises(L.Swv2Error):
        L.check(sums(W=18), "swv2_score_sums")


def test_ops_wrappers_refuse_what_the_kernel_cannot_take():
    from swin_v2_weather_amd import ops
    x = torch.zeros(1, 2, 4, 8)
    assert not ops.score_planes_ok(x)                         # a CPU tensor
    with pytest.raises(L.Swv2Error):
        ops.score_sums(x, x, torch.ones(4), torch.zeros(64))


def test_inference_parser_accepts_the_scoring_flags():
    from swin_v2_weather_amd import inference
    a = inference.build_parser().parse_args(["--registry", "R", "--steps", "3", "--truth", "t.npy", "--climatology", "c.npy", "--scores-out", "s.json"])
    assert (a.truth, a.climatology, a.scores_out, a.steps, a.out) == ("t.npy", "c.npy", "s.json", 3, None)
    b = inference.build_parser().parse_args(["--registry", "R"])
    assert (b.truth, b.climatology, b.scores_out, b.steps) == (None, None, None, 4)          # without --truth nothing changes
    sc = inference.RolloutScores(torch.tensor([[1.0, 2.0], [3.0, 4.0]]), torch.tensor([[0.9, 0.8], [0.7, 0.6]]), None, None, None)
    table = inference.lead_time_table(sc, [("u10m", 0), ("v10m", 1)]).splitlines()
    assert table[0].split() == ["lead_h", "rmse_u10m", "rmse_v10m", "acc_u10m", "acc_v10m"]
    assert [float(v) for v in table[2].split()] == pytest.approx([12.0, 3.0, 4.0, 0.7, 0.6])
