"""GPU (-m gpu): swv2_fss_rows through the C ABI into sentinel-guarded buffers, EQUAL to the independent numpy statement of
tests/fss_reference.py (the kernels deliver integers: there is no tolerance), then the Python layer on top of it:
ForecastScorer.neighbourhood_score, RegriddedScorer, score_rollout(..., neighbourhoods=) and the command line."""
import functools
import json

import numpy as np
import pytest
import torch

from tests import fss_reference as R
from tests.plane_harness import Guarded, dev, lib  # noqa: F401  (dev, lib: fixtures)
from tests.test_fss_host import fields, refusals, thresholds

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _reference(B, C, H, W, K, scales, use_base=False, below=False, per_sample=False):
    """the fields of a case, its thresholds and the reference's rows and n_invalid: computed once, shared, never modified"""
    prd, tar, base = fields(B, C, H, W)
    thr = thresholds(K)
    if per_sample:
        thr = thr[None, None] + 0.05 * np.arange(C, dtype=np.float32)[None, :, None] - 0.03 * np.arange(B, dtype=np.float32)[:, None, None]
    base = base if use_base else None
    want, ninv = R.rows(prd, tar, thr, scales, base, below)
    assert R.populated(want, H, W, scales), "the case is degenerate in the reference itself"
    want.setflags(write=False)
    return prd, tar, base, thr, want, ninv


def _d(dev, *arrays):
    return [None if a is None else torch.tensor(np.asarray(a)).to(dev) for a in arrays]


def _launch(lib, dev, prd, tar, thr, scales, base=None, below=False, ws_fill=None):
    """prd, tar [B, C, H, W] device tensors or channel-block views, thr numpy -> the Guarded with ws / rows / ninv"""
    from swin_v2_weather_amd import _lib as L
    import ctypes
    B, C, H, W = prd.shape
    t = torch.tensor(np.ascontiguousarray(R.thresholds_3d(thr, B, C))).to(dev)
    K, S = t.shape[2], len(scales)
    tbs = C * K if t.shape[0] == B and B > 1 else 0
    wsb = lib.swv2_fss_ws_bytes(B * C, H, W, K, S)
    assert wsb == 4 * B * C * (2 * K * H * ((W + 31) // 32) + lib.swv2_score_slices(B * C, H, W))
    g = Guarded(dev, ws=(wsb // 4, torch.int32), rows=(B * C * K * S * H * 3, torch.float64), ninv=(B * C, torch.int32))      # (rows: 8-byte slots)
    if ws_fill is not None:
        g.ints("ws").fill_(ws_fill)
    span = C * H * W
    L.check(lib.swv2_fss_rows(prd.data_ptr(), prd.stride(0) if B > 1 else span, tar.data_ptr(), tar.stride(0) if B > 1 else span,
                              None if base is None else base.data_ptr(), t.data_ptr(), tbs, (ctypes.c_int * S)(*scales), K, S, int(below), B, C, H, W,
                              g["ws"].data_ptr(), wsb, g["rows"].data_ptr(), g["ninv"].data_ptr(), torch.cuda.current_stream().cuda_stream),
            "swv2_fss_rows")
    torch.cuda.synchronize()
    return g


def _got(g, B, C, K, S, H):
    assert g.guards_intact(), "a kernel wrote outside its outputs"
    for k in g.sizes:
        assert g.written(k), f"{k}: slots the plan names were left unwritten"
    return g["rows"].view(torch.int64).cpu().numpy().reshape(B, C, K, S, H, 3), g["ninv"].cpu().numpy().reshape(B, C)


def _check(lib, dev, prd, tar, thr, scales, want, ninv, base=None, below=False, tag="", views=None):
    B, C, H, W = prd.shape
    dp, dt, db = _d(dev, prd, tar, base) if views is None else views
    g = _launch(lib, dev, dp, dt, thr, scales, db, below)
    rows, ni = _got(g, B, C, R.thresholds_3d(thr, B, C).shape[2], len(scales), H)
    assert np.array_equal(ni, ninv), tag
    bad = np.argwhere(rows != want)
    assert bad.size == 0, f"{tag}: {len(bad)} of {rows.size} sums differ, the first at [b, c, k, s, h, j] = {bad[0].tolist()}: {rows[tuple(bad[0])]} != {want[tuple(bad[0])]}"
    return g


# (B, C, H, W), K, scales: the smallest shapes at which the kernels can go wrong
CASES = [((2, 3, 5, 8), 2, (0, 1, 2, 3)),            # the box clips at both poles at once (r >= H / 2), 2 r + 1 = W - 1, less than one word
         ((2, 2, 12, 36), 3, (0, 1, 5, 17)),         # W % 32 != 0: the wrap crosses a word boundary; 2 r + 1 = W - 1
         ((1, 2, 9, 240), 2, (0, 1, 5, 17)),         # the 1.5 degree width: 7.5 words
         ((1, 2, 33, 96), 1, (0, 16, 32)),           # three words; r = 32 at H = 33: 65 bits, and rows beyond both poles in one box
         ((2, 2, 12, 36), 8, (0, 1, 2, 3, 4, 6, 9, 17)),      # K = 8 with S = 8
         ((1, 1, 3, 2052), 1, (0, 7, 32))]           # three column tiles of 684 columns


@pytest.mark.parametrize("shape,K,scales", CASES, ids=lambda s: "x".join(map(str, s)) if isinstance(s, tuple) else f"K{s}")
def test_rows_equal_the_reference(dev, lib, shape, K, scales):
    prd, tar, _, thr, want, ninv = _reference(*shape, K, scales)
    _check(lib, dev, prd, tar, thr, scales, want, ninv, tag=f"{shape} K = {K} {scales}")


@pytest.mark.parametrize("planes,bands", [(2, 4), (12, 1)], ids=["2-planes-4-bands", "12-planes-1-band"])
def test_row_bands_follow_the_plan(dev, lib, planes, bands):
    """70 x 1440 with r = 32: two planes are cut into several bands (a call of fewer than 8 workgroups), twelve get one band each; two
    column tiles of 720 either way"""
    H, W, scales = 70, 1440, (0, 2, 32)
    band = lib.swv2_fss_band_rows(planes, H, 1, 32)
    assert -(-H // band) == bands and band == (18 if planes == 2 else 70)
    prd, tar, _, thr, want, ninv = _reference(1, planes, H, W, 1, scales)
    _check(lib, dev, prd, tar, thr, scales, want, ninv, tag=f"{planes} planes")


@pytest.mark.parametrize("below", [False, True], ids=["above", "below"])
@pytest.mark.parametrize("use_base", [False, True], ids=["plain", "base"])
def test_base_field_direction_and_per_sample_thresholds(dev, lib, use_base, below):
    shape, K, scales = (3, 2, 12, 36), 2, (0, 1, 5, 17)
    prd, tar, base, thr, want, ninv = _reference(*shape, K, scales, use_base, below, True)
    assert thr.shape == (3, 2, 2)
    _check(lib, dev, prd, tar, thr, scales, want, ninv, base, below, tag=f"base {use_base} below {below}")


def test_channel_blocks_of_wider_tensors_in_place(dev, lib):
    """channels 5:8 of a 15-channel forecast against channels 7:10 of an 18-channel truth: nothing is copied"""
    B, C, H, W, scales = 2, 3, 9, 240, (0, 1, 5, 17)
    prd_w = fields(B, 15, H, W)[0]
    tar_w, base_w = fields(B, 18, H, W, seed=1)[1:]
    thr = thresholds(2)
    dp, dt = _d(dev, prd_w, tar_w)
    vp, vt = dp[:, 5:8], dt[:, 7:10]
    assert vp.stride(0) == 15 * H * W and vt.stride(0) == 18 * H * W and not vp.is_contiguous()
    base = np.ascontiguousarray(base_w[7:10])
    want, ninv = R.rows(prd_w[:, 5:8], tar_w[:, 7:10], thr, scales, base)
    assert R.populated(want, H, W, scales)
    _check(lib, dev, prd_w[:, 5:8], tar_w[:, 7:10], thr, scales, want, ninv, base, tag="block 5:8 / 7:10", views=(vp, vt, _d(dev, base)[0]))


def test_nan_inf_ties_and_a_plane_without_events(dev, lib):
    B, C, H, W, scales = 2, 2, 12, 36, (0, 1, 5, 17)
    prd, tar, base = (a.copy() for a in fields(B, C, H, W, quantum=0.25))
    thr = np.array([-0.25, 0.5, 1.0e6], np.float32)           # on the lattice: values equal to theta; the last one nobody exceeds
    assert (tar[:, :, None] == (base[None, :, None] + thr[None, None, :, None, None])).mean() > 0.02
    prd[0, 0, 0, 0] = np.nan                                  # the first row and column, in the prediction
    tar[0, 0, H - 1, W - 1] = np.nan                          # the last row and column, in the truth
    prd[0, 1, 5, W - 1] = tar[0, 1, 5, W - 1] = np.nan        # both at once: one point
    tar[1, 0, 0, W - 1] = np.inf                              # +-inf are values
    prd[1, 0, H - 1, 0] = -np.inf
    base[1, 6, 0] = np.nan                                    # the base: that point leaves channel 1 of every sample
    for below in (False, True):
        want, ninv = R.rows(prd, tar, thr, scales, base, below)
        assert ninv.tolist() == [[2, 2], [0, 1]]
        g = _check(lib, dev, prd, tar, thr, scales, want, ninv, base, below, tag=f"nan / inf / ties, below = {below}")
        rows = _got(g, B, C, 3, 4, H)[0]
        if not below:
            # nothing exceeds 1e6 but the +inf of the truth of plane (1, 0): everywhere else every sum is 0, and written as 0
            assert not rows[0, :, 2].any() and not rows[1, 1, 2].any() and rows[:, :, :2].sum(axis=(3, 4)).min() > 0
            assert not rows[1, 0, 2, :, :, 1].any() and int(rows[1, 0, 2, 0, :, 2].sum()) == 1


def test_reruns_and_a_dirty_workspace_give_the_same_bits(dev, lib):
    shape, K, scales = (2, 2, 12, 36), 3, (0, 1, 5, 17)
    prd, tar, base, thr, want, ninv = _reference(*shape, K, scales, True)
    dp, dt, db = _d(dev, prd, tar, base)
    g1 = _launch(lib, dev, dp, dt, thr, scales, db)           # (the workspace starts as the sentinel: nothing is accumulated into)
    g2 = _launch(lib, dev, dp, dt, thr, scales, db)
    g3 = _launch(lib, dev, dp, dt, thr, scales, db, ws_fill=-1)
    assert torch.equal(g1.raw, g2.raw) and torch.equal(g1.raw, g3.raw)                            # workspace, rows and counts, bit for bit
    assert np.array_equal(_got(g3, *shape[:2], K, len(scales), shape[2])[0], want)


def test_every_refusal_on_the_gpu_machine(dev, lib):
    assert refusals(lib) == 33


# ---- the Python layer ------------------------------------------------------------------------------------------------------
def test_neighbourhood_score_on_the_gpu_equals_the_cpu(dev, lib):
    from swin_v2_weather_amd.utils.weighted_acc_rmse import ForecastScorer
    B, C, H, W = 2, 3, 9, 240
    prd_w = fields(B, 15, H, W)[0]
    tar_w, clim_w = fields(B, 18, H, W, seed=1)[1:]
    clim = np.array(clim_w[7:10])                             # (a writable copy)
    thr = np.linspace(-1.0, 1.0, 11).astype(np.float32)      # K = 11: chunks of 8 and 3
    scales = (1, 2, 3, 4, 5, 8, 12, 17)                       # with the scale 0 put in front: 9 scales, chunks of 8 and 1
    gs, cs = ForecastScorer(H, W, C, dev, climatology=clim), ForecastScorer(H, W, C, "cpu", climatology=clim)
    dp, dt = _d(dev, prd_w, tar_w)
    g = gs.neighbourhood_score(dp, dt, thr, scales, anomaly=True, coff_prd=5, coff_tar=7)
    c = cs.neighbourhood_score(torch.tensor(prd_w), torch.tensor(tar_w), thr, scales, anomaly=True, coff_prd=5, coff_tar=7)
    assert set(gs._ws) == {("fss", B, 8, 8), ("fss", B, 8, 3), ("fss", B, 1, 8), ("fss", B, 1, 3)} and len(cs._ws) == 0
    assert g.rows.dtype == torch.int64 and tuple(g.rows.shape) == (B, C, 11, 8, H, 3) and g.rows.is_cuda
    assert torch.equal(g.rows.cpu(), c.rows) and torch.equal(g.n_invalid.cpu(), c.n_invalid)
    want = R.rows(prd_w[:, 5:8], tar_w[:, 7:10], thr, (0,) + scales, clim)[0]
    assert np.array_equal(g.rows.cpu().numpy(), want[:, :, :, 1:])
    for k in ("fss", "fbs", "fss_uniform", "base_rate"):      # fp64 dot products over H: rounding only
        assert torch.allclose(g.scores[k].cpu(), c.scores[k], rtol=1e-12, atol=1e-12) and torch.allclose(g.pooled[k].cpu(), c.pooled[k], rtol=1e-12, atol=1e-12), k
    assert torch.equal(g.pooled["useful_scale"].cpu(), c.pooled["useful_scale"])
    below = gs.neighbourhood_score(dp, dt, thr[:2], (0, 4), base=clim, below=True, coff_prd=5, coff_tar=7)
    assert np.array_equal(below.rows.cpu().numpy(), R.rows(prd_w[:, 5:8], tar_w[:, 7:10], thr[:2], (0, 4), clim, True)[0])


def test_float64_and_odd_widths_take_the_statement(dev, lib):
    from swin_v2_weather_amd.utils.weighted_acc_rmse import ForecastScorer
    B, C, H, W = 2, 2, 12, 36
    prd, tar, _ = fields(B, C, H, W)
    thr, scales = thresholds(2), (0, 1, 5)
    s64 = ForecastScorer(H, W, C, dev)
    r = s64.neighbourhood_score(torch.tensor(prd).double().to(dev), torch.tensor(tar).double().to(dev), thr, scales)
    assert len(s64._ws) == 0 and r.rows.is_cuda and np.array_equal(r.rows.cpu().numpy(), R.rows(prd, tar, thr, scales)[0])
    so = ForecastScorer(H, 34, C, dev)                        # W % 4 != 0
    dp, dt = _d(dev, np.ascontiguousarray(prd[..., :34]), np.ascontiguousarray(tar[..., :34]))
    ro = so.neighbourhood_score(dp, dt, thr, scales)
    assert len(so._ws) == 0 and np.array_equal(ro.rows.cpu().numpy(), R.rows(prd[..., :34], tar[..., :34], thr, scales)[0])


def test_regridded_scorer_takes_the_neighbourhoods_on_the_coarse_grid(dev, lib):
    from swin_v2_weather_amd.utils import regrid as G
    from swin_v2_weather_amd.utils.weighted_acc_rmse import ForecastScorer, RegriddedScorer
    B, C, H, W = 2, 2, 48, 72
    prd, tar, clim = fields(B, C, H, W)
    dp, dt, dc = _d(dev, prd, tar, clim)
    rg = G.Regridder(G.model_grid(H, W), G.grid_for_degrees(15.0), dev)
    rs = RegriddedScorer(rg, C, climatology=dc)
    thr = np.array([-0.2, 0.3], np.float32)
    r = rs.neighbourhood_score(dp, dt, thr, (0, 1, 4), anomaly=True)
    inner = ForecastScorer(13, 24, C, dev, climatology=rg(dc), weights=rg.area_weights)
    want = inner.neighbourhood_score(rg(dp), rg(dt), thr, (0, 1, 4), anomaly=True)
    assert torch.equal(r.rows, want.rows) and tuple(r.rows.shape) == (B, C, 2, 3, 13, 3) and int(r.rows.sum()) > 0
    assert torch.equal(r.pooled["fss"], want.pooled["fss"])
    st = R.rows(rg(dp).cpu().numpy(), rg(dt).cpu().numpy(), thr, (0, 1, 4), rg(dc).cpu().numpy())[0]
    assert np.array_equal(r.rows.cpu().numpy(), st)


def test_rollout_with_neighbourhoods_leaves_every_other_score_bit_identical(dev, lib, tmp_path):
    from tests.test_score_gpu import _registry_model
    from swin_v2_weather_amd import inference
    from swin_v2_weather_amd.utils.weighted_acc_rmse import EventSpec, ForecastScorer
    model = _registry_model(dev, tmp_path)
    B, Cout, H, W, steps = 2, 5, 48, 72, 2
    g = torch.Generator(device=dev).manual_seed(3)
    x0 = torch.randn(B, 9, H, W, device=dev, generator=g)
    cz = torch.rand(B, steps - 1, H, W, device=dev, generator=g) * 2 - 1
    truth = torch.randn(B, steps, Cout, H, W, device=dev, generator=g)
    scorer = ForecastScorer(H, W, Cout, dev, climatology=0.3 * torch.randn(Cout, H, W, device=dev, generator=g))
    spec = EventSpec("quantile", (0.5, 0.9), False)
    ev = inference.score_rollout(model, x0, truth, steps, cz, n_invar=3, scorer=scorer, keep_forecast=True, events=spec)
    got = inference.score_rollout(model, x0, truth, steps, cz, n_invar=3, scorer=scorer, keep_forecast=True, events=spec, neighbourhoods=(1, 4, 16))
    assert ev.neighbourhoods is None and all(torch.equal(a, b) for a, b in zip(ev[:5], got[:5])) and torch.equal(ev.events.table, got.events.table)
    nb = got.neighbourhoods
    assert tuple(nb.rows.shape) == (steps, B, Cout, 2, 3, H, 3) and tuple(nb.scores["fss"].shape) == (steps, Cout, 2, 3)
    for s in range(steps):
        thr = scorer.event_thresholds(spec, truth[:, s])
        r = scorer.neighbourhood_score(got.forecast[:, s], truth[:, s], thr, (1, 4, 16))
        assert torch.equal(nb.rows[s], r.rows) and torch.equal(nb.scores["fss"][s], r.pooled["fss"])
        st = R.rows(got.forecast[:, s].cpu().numpy(), truth[:, s].cpu().numpy(), thr.cpu().numpy(), (1, 4, 16))[0]
        assert np.array_equal(nb.rows[s].cpu().numpy(), st)
    assert float(nb.scores["base_rate"][:, :, 1].mean()) == pytest.approx(0.1, abs=0.01)
    with pytest.raises(ValueError, match="ensemble"):
        inference.ensemble_rollout(model, x0, truth, steps, 3, 0.05, 1, cz, 3, scorer, events=spec, neighbourhoods=(1,))


def test_cli_prints_the_fss_columns_and_writes_the_fss_key(dev, lib, tmp_path, capsys):
    from tests.test_score_gpu import _registry_model
    from swin_v2_weather_amd import inference
    _registry_model(dev, tmp_path)
    reg = tmp_path / "swin_test_registry"
    rng = np.random.default_rng(11)
    B, Cout, H, W, steps = 2, 5, 48, 72, 2
    tm = rng.standard_normal((1, 73, 49, 80)).astype(np.float32)
    x0, truth = rng.standard_normal((B, 9, H, W)).astype(np.float32), rng.standard_normal((B, steps, Cout, H, W)).astype(np.float32)
    np.save(reg / "time_means.npy", tm); np.save(tmp_path / "x0.npy", x0); np.save(tmp_path / "truth.npy", truth)
    base = ["--registry", str(reg), "--steps", str(steps), "--init", str(tmp_path / "x0.npy"), "--truth", str(tmp_path / "truth.npy")]
    inference.main(base + ["--scores-out", str(tmp_path / "ev.json"), "--event-anomaly", "1", "2"])
    ev_out = capsys.readouterr().out.splitlines()
    inference.main(base + ["--scores-out", str(tmp_path / "fss.json"), "--event-anomaly", "1", "2", "--event-scales", "1", "4", "16"])
    out = capsys.readouterr().out.splitlines()
    ev, doc = json.load(open(tmp_path / "ev.json")), json.load(open(tmp_path / "fss.json"))
    assert "fss" not in ev and doc["events"] == ev["events"] and doc["rmse"] == ev["rmse"]
    f = doc["fss"]
    assert sorted(f) == ["fss", "fss_uniform", "scales", "useful_scale"] and f["scales"] == [1, 4, 16]
    assert np.asarray(f["fss"]).shape == (steps, Cout, 2, 3) and np.asarray(f["fss_uniform"]).shape == (steps, Cout, 2)
    assert np.asarray(f["useful_scale"]).shape == (steps, Cout, 2) and set(np.asarray(f["useful_scale"]).ravel().tolist()) <= {-1, 1, 4, 16}
    assert out[1].startswith(ev_out[1]) and out[1].split()[-12:] == [f"fss{k}_r{r}_{n}" for k in (0, 1) for r in (1, 4, 16) for n in ("u10m", "v10m")]
    assert float(out[2].split()[-12]) == pytest.approx(f["fss"][0][0][0][0], abs=1e-5) and float(out[3].split()[-1]) == pytest.approx(f["fss"][1][1][1][2], abs=1e-5)
    inference.main(base + ["--scores-out", str(tmp_path / "coarse.json"), "--event-quantile", "0.8", "--event-scales", "0", "2", "--score-grid", "15"])
    capsys.readouterr()
    fc = json.load(open(tmp_path / "coarse.json"))["fss"]
    assert fc["scales"] == [0, 2] and np.asarray(fc["fss"]).shape == (steps, Cout, 1, 2)
