"""GPU (-m gpu): swv2_fss_ens_rows through the C ABI into sentinel-guarded buffers, EQUAL to the independent numpy statement of
tests/efss_reference.py (the kernels deliver integers: there is no tolerance), then the Python layer on top of it:
ForecastScorer.ensemble_neighbourhood_score, RegriddedScorer, ensemble_rollout(..., ensemble_neighbourhoods=) and the command line."""
import ctypes
import json

import numpy as np
import pytest
import torch

from tests import efss_reference as ER
from tests import fss_reference as R
from tests.plane_harness import Guarded, dev, lib  # noqa: F401  (dev, lib: fixtures)
from tests.test_efss_host import CASE_IDS, CASES, bit_planes, reference, refusals
from tests.test_fss_host import fields, thresholds

pytestmark = pytest.mark.gpu


def _d(dev, *arrays):
    return [None if a is None else torch.tensor(np.asarray(a)).to(dev) for a in arrays]


def _launch(lib, dev, ens, tar, thr, scales, base=None, below=False, ws_fill=None):
    """ens [M, B, C, H, W], tar [B, C, H, W] device tensors or views with contiguous planes, thr numpy -> the Guarded with ws / rows / ninv"""
    from swin_v2_weather_amd import _lib as L
    M, B, C, H, W = ens.shape
    t = torch.tensor(np.ascontiguousarray(R.thresholds_3d(thr, B, C))).to(dev)
    K, S = t.shape[2], len(scales)
    tbs = C * K if t.shape[0] == B and B > 1 else 0
    wsb = lib.swv2_fss_ens_ws_bytes(B * C, H, W, M, K, S)
    assert wsb == 4 * B * C * ((bit_planes(M) + 1) * K * H * ((W + 31) // 32) + lib.swv2_score_slices(B * C, H, W))
    g = Guarded(dev, ws=(wsb // 4, torch.int32), rows=(B * C * K * S * H * 3, torch.float64), ninv=(B * C, torch.int32))      # (rows: 8-byte slots)
    if ws_fill is not None:
        g.ints("ws").fill_(ws_fill)
    span = C * H * W
    L.check(lib.swv2_fss_ens_rows(ens.data_ptr(), ens.stride(0), ens.stride(1) if B > 1 else span, tar.data_ptr(), tar.stride(0) if B > 1 else span,
                                  None if base is None else base.data_ptr(), t.data_ptr(), tbs, (ctypes.c_int * S)(*scales), M, K, S, int(below), B, C,
                                  H, W, g["ws"].data_ptr(), wsb, g["rows"].data_ptr(), g["ninv"].data_ptr(), torch.cuda.current_stream().cuda_stream),
            "swv2_fss_ens_rows")
    torch.cuda.synchronize()
    return g


def _got(g, B, C, K, S, H):
    assert g.guards_intact(), "a kernel wrote outside its outputs"
    for k in g.sizes:
        assert g.written(k), f"{k}: slots the plan names were left unwritten"
    return g["rows"].view(torch.int64).cpu().numpy().reshape(B, C, K, S, H, 3), g["ninv"].cpu().numpy().reshape(B, C)


def _check(lib, dev, ens, tar, thr, scales, want, ninv, base=None, below=False, tag="", views=None):
    M, B, C, H, W = ens.shape
    de, dt, db = _d(dev, ens, tar, base) if views is None else views
    g = _launch(lib, dev, de, dt, thr, scales, db, below)
    rows, ni = _got(g, B, C, R.thresholds_3d(thr, B, C).shape[2], len(scales), H)
    assert np.array_equal(ni, ninv), tag
    bad = np.argwhere(rows != want)
    assert bad.size == 0, f"{tag}: {len(bad)} of {rows.size} sums differ, the first at [b, c, k, s, h, j] = {bad[0].tolist()}: {rows[tuple(bad[0])]} != {want[tuple(bad[0])]}"
    return g


@pytest.mark.parametrize("shape,K,scales,M", CASES, ids=CASE_IDS)
def test_rows_equal_the_reference(dev, lib, shape, K, scales, M):
    ens, tar, _, thr, want, ninv = reference(*shape, K, scales, M)
    _check(lib, dev, ens, tar, thr, scales, want, ninv, tag=f"{shape} K = {K} {scales} M = {M}")


@pytest.mark.parametrize("mirror", [False, True], ids=["all-members", "analysis-only"])
def test_saturation_in_closed_form(dev, lib, mirror):
    """M = 64, r = 32: every member an event everywhere and the analysis nowhere gives N_f = 64 N_box(h), rows = (W (64 N_box)^2, the same, 0),
    up to 7e12 per row -- the 64-bit path at its maximum; the mirror image gives (64^2 W N_box^2, 0, W N_box^2)"""
    B, C, H, W, M, scales = 1, 1, 33, 96, 64, (0, 32)
    ens = torch.full((M, B, C, H, W), -10.0 if mirror else 10.0, device=dev)
    tar = torch.full((B, C, H, W), 10.0 if mirror else -10.0, device=dev)
    g = _launch(lib, dev, ens, tar, np.zeros(1, np.float32), scales)
    rows, ni = _got(g, B, C, 1, 2, H)
    nbox = R.box_sizes(H, scales)                             # [S, H]
    full = W * (M * nbox) ** 2
    assert int(full.max()) == 96 * (64 * 33 * 65) ** 2 > 1 << 40 and not ni.any()
    want = np.stack((full, np.zeros_like(full), W * nbox ** 2) if mirror else (full, full, np.zeros_like(full)), axis=-1)
    assert np.array_equal(rows[0, 0, 0], want)


@pytest.mark.parametrize("planes,bands", [(2, 4), (12, 1)], ids=["2-planes-4-bands", "12-planes-1-band"])
def test_row_bands_follow_the_plan(dev, lib, planes, bands):
    """70 x 1440 with r = 32 and M = 16 (5 bit planes: 512-column tiles, three of 480): two planes are cut into several bands, twelve get
    one band each"""
    H, W, M, scales = 70, 1440, 16, (0, 2, 32)
    band = lib.swv2_fss_ens_band_rows(planes, H, M, 1, 32)
    assert -(-H // band) == bands and band == (18 if planes == 2 else 70)
    ens, tar, _, thr, want, ninv = reference(1, planes, H, W, 1, scales, M, two_pass=True)
    _check(lib, dev, ens, tar, thr, scales, want, ninv, tag=f"{planes} planes")


@pytest.mark.parametrize("below", [False, True], ids=["above", "below"])
@pytest.mark.parametrize("use_base", [False, True], ids=["plain", "base"])
def test_base_field_direction_and_per_sample_thresholds(dev, lib, use_base, below):
    shape, K, scales, M = (3, 2, 12, 36), 2, (0, 1, 5, 17), 5
    ens, tar, base, thr, want, ninv = reference(*shape, K, scales, M, use_base, below, True)
    assert thr.shape == (3, 2, 2)
    _check(lib, dev, ens, tar, thr, scales, want, ninv, base, below, tag=f"base {use_base} below {below}")


def test_a_ring_slot_and_a_channel_block_in_place(dev, lib):
    """the members as channels 5:8 of slot 1 of a ring [M B, 2 Cout, H, W], the truth as channels 7:10 of an 18-channel tensor: nothing is copied"""
    M, B, C, Cout, H, W, scales = 3, 2, 3, 5, 9, 240, (0, 1, 5, 17)
    ring = np.ascontiguousarray(ER.members(M, B, 2 * Cout, H, W).reshape(M * B, 2 * Cout, H, W))
    tar_w, base_w = fields(B, 18, H, W, seed=1)[1:]
    thr = thresholds(2)
    dr, dt = _d(dev, ring, tar_w)
    ve, vt = dr.unflatten(0, (M, B))[:, :, 5:8], dt[:, 7:10]
    assert ve.stride(0) == B * 2 * Cout * H * W and ve.stride(1) == 2 * Cout * H * W and vt.stride(0) == 18 * H * W and ve.data_ptr() != dr.data_ptr()
    ens = ring.reshape(M, B, 2 * Cout, H, W)[:, :, 5:8]
    base = np.ascontiguousarray(base_w[7:10])
    want, ninv = ER.rows(ens, tar_w[:, 7:10], thr, scales, base)
    assert R.populated(want, H, W, scales)
    _check(lib, dev, ens, tar_w[:, 7:10], thr, scales, want, ninv, base, tag="ring slot 5:8 / 7:10", views=(ve, vt, _d(dev, base)[0]))


def test_nan_in_one_member_inf_ties_and_a_threshold_nobody_exceeds(dev, lib):
    B, C, H, W, M, scales = 2, 2, 12, 36, 5, (0, 1, 5, 17)
    _, tar, base = (a.copy() for a in fields(B, C, H, W, quantum=0.25))
    ens = (np.round(ER.members(M, B, C, H, W) / 0.25) * 0.25).astype(np.float32)
    thr = np.array([-0.25, 0.5, 1.0e6], np.float32)           # on the lattice: values equal to theta; the last one nobody exceeds
    assert (ens[:, :, :, None] == (base[None, None, :, None] + thr[None, None, None, :, None, None])).mean() > 0.02
    ens[3, 0, 0, 0, 0] = np.nan                               # ONE member only: the point is invalid in all, and counted once
    tar[0, 0, H - 1, W - 1] = np.nan
    ens[1, 0, 1, 5, W - 1] = tar[0, 1, 5, W - 1] = np.nan     # both at once: one point
    ens[4, 0, 1, 2, 2] = ens[0, 0, 1, 2, 2] = np.nan          # two members at one point: one point
    tar[1, 0, 0, W - 1] = np.inf                              # +-inf are values
    ens[2, 1, 0, H - 1, 0] = -np.inf
    base[1, 6, 0] = np.nan                                    # the base: that point leaves channel 1 of every sample
    for below in (False, True):
        want, ninv = ER.rows(ens, tar, thr, scales, base, below)
        assert ninv.tolist() == [[2, 3], [0, 1]]
        g = _check(lib, dev, ens, tar, thr, scales, want, ninv, base, below, tag=f"nan / inf / ties, below = {below}")
        rows = _got(g, B, C, 3, 4, H)[0]
        if not below:
            # nothing exceeds 1e6 but the +inf of the truth of plane (1, 0): everywhere else every sum is 0, and written as 0
            assert not rows[0, :, 2].any() and not rows[1, 1, 2].any() and rows[:, :, :2].sum(axis=(3, 4)).min() > 0
            assert not rows[1, 0, 2, :, :, 1].any() and int(rows[1, 0, 2, 0, :, 2].sum()) == 1


def test_reruns_and_a_dirty_workspace_give_the_same_bits(dev, lib):
    shape, K, scales, M = (2, 2, 12, 36), 3, (0, 1, 5, 17), 7
    ens, tar, _, thr, want, _ = reference(*shape, K, scales, M)
    de, dt = _d(dev, ens, tar)
    g1 = _launch(lib, dev, de, dt, thr, scales)               # (the workspace starts as the sentinel: nothing is accumulated into)
    g2 = _launch(lib, dev, de, dt, thr, scales)
    g3 = _launch(lib, dev, de, dt, thr, scales, ws_fill=-1)
    assert torch.equal(g1.raw, g2.raw) and torch.equal(g1.raw, g3.raw)                            # workspace, rows and counts, bit for bit
    assert np.array_equal(_got(g3, *shape[:2], K, len(scales), shape[2])[0], want)


def test_copies_of_one_forecast_equal_the_deterministic_kernel(dev, lib):
    """M copies of one forecast through swv2_fss_ens_rows = swv2_fss_rows x (M^2, M^2, 1), both on the GPU"""
    from swin_v2_weather_amd import ops
    B, C, H, W, scales = 2, 2, 12, 36, (0, 1, 5, 17)
    prd, tar, base = fields(B, C, H, W)
    dp, dt, db = _d(dev, prd, tar, base)
    thr = torch.tensor(R.thresholds_3d(thresholds(3), B, C)).to(dev).contiguous()
    det, dni = ops.fss_rows(dp, dt, thr, scales, ops.fss_workspace(B * C, H, W, 3, 4, dev), db)
    for M in (2, 5, 64):
        ens = dp.unsqueeze(0).repeat(M, 1, 1, 1, 1)
        rows, ni = ops.fss_ens_rows(ens, dt, thr, scales, ops.fss_ens_workspace(B * C, H, W, M, 3, 4, dev), db)
        assert torch.equal(rows, det * torch.tensor([M * M, M * M, 1], device=dev)) and torch.equal(ni, dni), M
    assert int(det.sum()) > 0


def test_every_refusal_on_the_gpu_machine(dev, lib):
    assert refusals(lib) == 37


# ---- the Python layer ------------------------------------------------------------------------------------------------------
def test_ensemble_neighbourhood_score_on_the_gpu_equals_the_cpu(dev, lib):
    from swin_v2_weather_amd.utils import events as E
    from swin_v2_weather_amd.utils.weighted_acc_rmse import ForecastScorer
    M, B, C, Cout, H, W = 3, 2, 3, 5, 9, 240
    ring = np.ascontiguousarray(ER.members(M, B, 2 * Cout, H, W).reshape(M * B, 2 * Cout, H, W))
    tar_w, clim_w = fields(B, 18, H, W, seed=1)[1:]
    clim = np.array(clim_w[7:10])                             # (a writable copy)
    thr = np.linspace(-1.0, 1.0, 11).astype(np.float32)      # K = 11: chunks of 8 and 3
    scales = (1, 2, 3, 4, 5, 8, 12, 17)                       # with the scale 0 put in front: 9 scales, chunks of 8 and 1
    gs, cs = ForecastScorer(H, W, C, dev, climatology=clim), ForecastScorer(H, W, C, "cpu", climatology=clim)
    dr, dt = _d(dev, ring, tar_w)
    g = gs.ensemble_neighbourhood_score(dr, dt, M, thr, scales, anomaly=True, coff_ens=5, coff_tar=7, members=True)
    c = cs.ensemble_neighbourhood_score(torch.tensor(ring), torch.tensor(tar_w), M, thr, scales, anomaly=True, coff_ens=5, coff_tar=7, members=True)
    want_ws = {("fss_ens", M, B, 8, 8), ("fss_ens", M, B, 8, 3), ("fss_ens", M, B, 1, 8), ("fss_ens", M, B, 1, 3)}
    assert want_ws <= set(gs._ws) and set(gs._ws) - want_ws == {("fss", B, 8, 8), ("fss", B, 8, 3), ("fss", B, 1, 8), ("fss", B, 1, 3)} and len(cs._ws) == 0
    assert g.rows.dtype == torch.int64 and tuple(g.rows.shape) == (B, C, 11, 8, H, 3) and g.rows.is_cuda
    assert torch.equal(g.rows.cpu(), c.rows) and torch.equal(g.n_invalid.cpu(), c.n_invalid)
    assert torch.equal(g.member_rows.cpu(), c.member_rows) and torch.equal(g.dispersion_rows.cpu(), c.dispersion_rows)
    ens = ring.reshape(M, B, 2 * Cout, H, W)[:, :, 5:8]
    want = ER.rows(ens, tar_w[:, 7:10], thr, (0,) + scales, clim, two_pass=True)[0]
    assert np.array_equal(g.rows.cpu().numpy(), want[:, :, :, 1:])
    for k in ("pfss", "fbs", "fss_uniform", "base_rate"):     # fp64 dot products over H: rounding only
        assert torch.allclose(g.scores[k].cpu(), c.scores[k], rtol=1e-12, atol=1e-12) and torch.allclose(g.pooled[k].cpu(), c.pooled[k], rtol=1e-12, atol=1e-12), k
    assert torch.equal(g.pooled["useful_scale"].cpu(), c.pooled["useful_scale"])
    assert torch.allclose(g.member_scores["fss"].cpu(), c.member_scores["fss"], rtol=1e-12, atol=1e-12)
    assert torch.allclose(g.dispersion_scores["fss"].cpu(), c.dispersion_scores["fss"], rtol=1e-12, atol=1e-12)
    det = sum(E.fss_rows_torch(torch.tensor(ens[m]), torch.tensor(tar_w[:, 7:10]), torch.tensor(thr), (0,) + scales, torch.tensor(clim))[0] for m in range(M))
    assert torch.equal(g.member_rows.cpu(), det[:, :, :, 1:])
    below = gs.ensemble_neighbourhood_score(dr, dt, M, thr[:2], (0, 4), base=clim, below=True, coff_ens=5, coff_tar=7)
    assert np.array_equal(below.rows.cpu().numpy(), ER.rows(ens, tar_w[:, 7:10], thr[:2], (0, 4), clim, True)[0]) and below.member_rows is None


def test_float64_and_odd_widths_take_the_statement(dev, lib):
    from swin_v2_weather_amd.utils.weighted_acc_rmse import ForecastScorer
    shape, K, scales, M = (2, 2, 12, 36), 3, (0, 1, 5, 17), 7
    ens, tar, _, thr, want, _ = reference(*shape, K, scales, M)
    B, C, H, W = shape
    s64 = ForecastScorer(H, W, C, dev)
    r = s64.ensemble_neighbourhood_score(torch.tensor(ens).double().to(dev), torch.tensor(tar).double().to(dev), M, thr, scales)
    assert len(s64._ws) == 0 and r.rows.is_cuda and np.array_equal(r.rows.cpu().numpy(), want)
    so = ForecastScorer(H, 34, C, dev)                        # W % 4 != 0
    de, dt = _d(dev, np.ascontiguousarray(ens[..., :34]), np.ascontiguousarray(tar[..., :34]))
    ro = so.ensemble_neighbourhood_score(de, dt, M, thr, (0, 1, 5))
    assert len(so._ws) == 0 and np.array_equal(ro.rows.cpu().numpy(), ER.rows(ens[..., :34], tar[..., :34], thr, (0, 1, 5))[0])


def test_regridded_scorer_takes_the_neighbourhoods_on_the_coarse_grid(dev, lib):
    from swin_v2_weather_amd.utils import regrid as G
    from swin_v2_weather_amd.utils.weighted_acc_rmse import ForecastScorer, RegriddedScorer
    M, B, C, H, W = 3, 2, 2, 48, 72
    _, tar, clim = fields(B, C, H, W)
    de, dt, dc = _d(dev, ER.members(M, B, C, H, W), tar, clim)
    rg = G.Regridder(G.model_grid(H, W), G.grid_for_degrees(15.0), dev)
    rs = RegriddedScorer(rg, C, climatology=dc)
    thr = np.array([-0.2, 0.3], np.float32)
    r = rs.ensemble_neighbourhood_score(de, dt, M, thr, (0, 1, 4), anomaly=True, members=True)
    inner = ForecastScorer(13, 24, C, dev, climatology=rg(dc), weights=rg.area_weights)
    want = inner.ensemble_neighbourhood_score(rg(de), rg(dt), M, thr, (0, 1, 4), anomaly=True, members=True)
    assert torch.equal(r.rows, want.rows) and tuple(r.rows.shape) == (B, C, 2, 3, 13, 3) and int(r.rows.sum()) > 0
    assert torch.equal(r.pooled["pfss"], want.pooled["pfss"]) and torch.equal(r.member_rows, want.member_rows)
    st = ER.rows(rg(de).cpu().numpy(), rg(dt).cpu().numpy(), thr, (0, 1, 4), rg(dc).cpu().numpy())[0]
    assert np.array_equal(r.rows.cpu().numpy(), st)


def test_rollout_with_ensemble_neighbourhoods_leaves_every_other_score_bit_identical(dev, lib, tmp_path):
    from tests.test_score_gpu import _registry_model
    from swin_v2_weather_amd import inference
    from swin_v2_weather_amd.utils.weighted_acc_rmse import EventSpec, ForecastScorer
    model = _registry_model(dev, tmp_path)
    B, Cout, H, W, steps, M = 2, 5, 48, 72, 2, 3
    g = torch.Generator(device=dev).manual_seed(3)
    x0 = torch.randn(B, 9, H, W, device=dev, generator=g)
    cz = torch.rand(B, steps - 1, H, W, device=dev, generator=g) * 2 - 1
    truth = torch.randn(B, steps, Cout, H, W, device=dev, generator=g)
    scorer = ForecastScorer(H, W, Cout, dev, climatology=0.3 * torch.randn(Cout, H, W, device=dev, generator=g))
    spec = EventSpec("quantile", (0.5, 0.9), False)
    kw = dict(scorer=scorer, keep_forecast=True, events=spec, score_control=True)
    ev = inference.ensemble_rollout(model, x0, truth, steps, M, 0.05, 1, cz, 3, **kw)
    got = inference.ensemble_rollout(model, x0, truth, steps, M, 0.05, 1, cz, 3, ensemble_neighbourhoods=(1, 4, 16), member_neighbourhoods=True, **kw)
    ring = inference.ensemble_rollout(model, x0, truth, steps, M, 0.05, 1, cz, 3, scorer=scorer, events=spec, ensemble_neighbourhoods=(1, 4, 16))
    assert ev.neighbourhoods is None and all(torch.equal(a, b) for a, b in zip(ev[:10], got[:10]))
    assert all(torch.equal(getattr(ev.events, k), getattr(got.events, k)) for k in ("sums", "wv", "hist", "n_invalid"))
    assert all(torch.equal(a, b) for a, b in zip(ev.control[:4], got.control[:4])) and torch.equal(ev.control.events.table, got.control.events.table)
    nb = got.neighbourhoods
    assert tuple(nb.rows.shape) == (steps, B, Cout, 2, 3, H, 3) and tuple(nb.scores["pfss"].shape) == (steps, Cout, 2, 3)
    assert torch.equal(ring.neighbourhoods.rows, nb.rows)     # the two-slot ring, read in place
    for s in range(steps):
        thr = scorer.event_thresholds(spec, truth[:, s])
        r = scorer.ensemble_neighbourhood_score(got.forecast[:, s], truth[:, s], M, thr, (1, 4, 16), members=True)
        assert torch.equal(nb.rows[s], r.rows) and torch.equal(nb.scores["pfss"][s], r.pooled["pfss"])
        assert torch.equal(nb.member_rows[s], r.member_rows) and torch.equal(nb.dispersion_scores["fss"][s], r.dispersion_scores["fss"])
        st = ER.rows(got.forecast[:, s].reshape(M, B, Cout, H, W).cpu().numpy(), truth[:, s].cpu().numpy(), thr.cpu().numpy(), (1, 4, 16), two_pass=True)[0]
        assert np.array_equal(nb.rows[s].cpu().numpy(), st)
    assert float(nb.scores["base_rate"][:, :, 1].mean()) == pytest.approx(0.1, abs=0.01)
    with pytest.raises(ValueError, match="ensemble_neighbourhoods"):
        inference.ensemble_rollout(model, x0, truth, steps, M, 0.05, 1, cz, 3, scorer, events=spec, neighbourhoods=(1,))


def test_cli_prints_the_pfss_columns_and_writes_the_pfss_key(dev, lib, tmp_path, capsys):
    from tests.test_score_gpu import _registry_model
    from swin_v2_weather_amd import inference
    _registry_model(dev, tmp_path)
    reg = tmp_path / "swin_test_registry"
    rng = np.random.default_rng(11)
    B, Cout, H, W, steps, M = 2, 5, 48, 72, 2, 3
    tm = rng.standard_normal((1, 73, 49, 80)).astype(np.float32)
    x0, truth = rng.standard_normal((B, 9, H, W)).astype(np.float32), rng.standard_normal((B, steps, Cout, H, W)).astype(np.float32)
    np.save(reg / "time_means.npy", tm); np.save(tmp_path / "x0.npy", x0); np.save(tmp_path / "truth.npy", truth)
    base = ["--registry", str(reg), "--steps", str(steps), "--init", str(tmp_path / "x0.npy"), "--truth", str(tmp_path / "truth.npy"),
            "--ensemble", str(M), "--perturbation", "0.1", "--event-anomaly", "1", "2"]
    inference.main(base + ["--scores-out", str(tmp_path / "ev.json")])
    ev_out = capsys.readouterr().out.splitlines()
    inference.main(base + ["--scores-out", str(tmp_path / "pfss.json"), "--ensemble-scales", "1", "4", "16"])
    out = capsys.readouterr().out.splitlines()
    ev, doc = json.load(open(tmp_path / "ev.json")), json.load(open(tmp_path / "pfss.json"))
    assert "pfss" not in ev and doc["events"] == ev["events"] and doc["rmse"] == ev["rmse"] and doc["ensemble"] == ev["ensemble"]
    f = doc["pfss"]
    assert sorted(f) == ["fss_uniform", "pfss", "scales", "useful_scale"] and f["scales"] == [1, 4, 16]
    assert np.asarray(f["pfss"]).shape == (steps, Cout, 2, 3) and np.asarray(f["fss_uniform"]).shape == (steps, Cout, 2)
    assert np.asarray(f["useful_scale"]).shape == (steps, Cout, 2) and set(np.asarray(f["useful_scale"]).ravel().tolist()) <= {-1, 1, 4, 16}
    assert out[1].startswith(ev_out[1]) and out[1].split()[-12:] == [f"pfss{k}_r{r}_{n}" for k in (0, 1) for r in (1, 4, 16) for n in ("u10m", "v10m")]
    assert float(out[2].split()[-12]) == pytest.approx(f["pfss"][0][0][0][0], abs=1e-5) and float(out[3].split()[-1]) == pytest.approx(f["pfss"][1][1][1][2], abs=1e-5)
    inference.main(base[:-3] + ["--event-quantile", "0.8", "--scores-out", str(tmp_path / "coarse.json"), "--ensemble-scales", "0", "2", "--ensemble-member-scores",
                                "--score-grid", "15"])
    out = capsys.readouterr().out.splitlines()
    fc = json.load(open(tmp_path / "coarse.json"))["pfss"]
    assert fc["scales"] == [0, 2] and all(np.asarray(fc[k]).shape == (steps, Cout, 1, 2) for k in ("pfss", "efss", "dfss"))
    assert out[2].split()[-12:] == [f"{k}0_r{r}_{n}" for k in ("pfss", "efss", "dfss") for r in (0, 2) for n in ("u10m", "v10m")]
