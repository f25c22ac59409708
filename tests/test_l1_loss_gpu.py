"""GPU (-m gpu): swv2_l1_sums / swv2_l1_finalize / swv2_l1_grad through the C ABI, judged element by element against the fp64
statement of tests/l1_reference.py (every bound is derived there), then the Python layer on top of them: LossHandler's l1 strings
against the reference's own numbers (tests/golden/loss_l1_*), the Gauss-Legendre rows, fused_with, ForecastScorer.mae and the Trainer."""
import json
import math
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import l1_reference as R
from tests import score_reference as RS
from tests.plane_harness import Guarded, _weights, dev, lib  # noqa: F401  (dev, lib: fixtures)
from tests.test_l1_loss_host import NAMES, golden, golden_fields, handler, relmax
from tests.test_score_gpu import SHAPES, _fields           # the eight shapes that reach each branch of the plan, and their cached fields

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _chw(C):
    return (0.25 + np.random.default_rng(C).random(C)).astype(np.float32) / C


def _launch(lib, dev, prd, tar, w, chw=None, absolute=False):
    """prd, tar: device tensors or channel-block views [B, C, H, W]; -> (Guarded with ws / sums (/ loss / coef with chw), slices)"""
    from swin_v2_weather_amd import _lib as L
    B, C, H, W = prd.shape
    slices = lib.swv2_score_slices(B * C, H, W)
    wsb = lib.swv2_l1_ws_bytes(B * C, H, W)
    assert wsb == B * C * slices * 8
    sizes = dict(ws=wsb // 4, sums=B * C * 2)
    if chw is not None:
        sizes.update(loss=1, coef=B * C)
    g = Guarded(dev, **sizes)
    st = torch.cuda.current_stream().cuda_stream
    ps, ts = (prd.stride(0), tar.stride(0)) if B > 1 else (C * H * W, C * H * W)
    L.check(lib.swv2_l1_sums(prd.data_ptr(), ps, tar.data_ptr(), ts, w.data_ptr(), B, C, H, W, g["ws"].data_ptr(), wsb, st), "swv2_l1_sums")
    L.check(lib.swv2_l1_finalize(g["ws"].data_ptr(), wsb, B, C, H, W, None if chw is None else chw.data_ptr(), int(absolute), g["sums"].data_ptr(),
                                 None if chw is None else g["loss"].data_ptr(), None if chw is None else g["coef"].data_ptr(), st),
            "swv2_l1_finalize")
    torch.cuda.synchronize()
    return g, slices


def _grad(lib, dev, prd, tar, w, coef):
    """contiguous device tensors, coef a device tensor [B C] -> Guarded with dprd"""
    from swin_v2_weather_amd import _lib as L
    B, C, H, W = prd.shape
    g = Guarded(dev, dprd=B * C * H * W)
    L.check(lib.swv2_l1_grad(prd.data_ptr(), tar.data_ptr(), w.data_ptr(), coef.data_ptr(), g["dprd"].data_ptr(), B * C, H, W,
                             torch.cuda.current_stream().cuda_stream), "swv2_l1_grad")
    torch.cuda.synchronize()
    return g


def _verdict(g, slices, prd, tar, w, chw, absolute, tag=""):
    """the element-by-element judgement of one launch pair (numpy inputs); asserts every bound, the guards and the written slots"""
    B, C, H, W = prd.shape
    assert g.guards_intact(), "a kernel wrote outside its outputs"
    for k in g.sizes:
        assert g.written(k), f"{k}: slots the plan names were left unwritten"
    n = R.chain_length(H, W, slices)
    got = {k: g[k].cpu().numpy() for k in g.sizes}
    S, A = R.sums(prd, tar, w)
    dS = R.sum_bounds(A, n)
    rs = R.worst(np.abs(got["sums"].reshape(B, C, 2).astype(np.float64) - S), dS)
    print(f"{tag} n = {n}: worst error / bound  sums {rs:.3f}")
    assert rs <= 1.0
    if chw is not None:
        l_ref, l_b, c_ref, c_b = R.loss(S, dS, chw, absolute)
        rl = R.worst(abs(float(got["loss"][0]) - l_ref), l_b)
        rc = R.worst(np.abs(got["coef"].reshape(B, C).astype(np.float64) - c_ref), c_b)
        print(f"{tag} absolute={absolute}: loss {got['loss'][0]:.7g} (fp64 {l_ref:.9g})  worst error / bound  loss {rl:.3f}  coef {rc:.3f}")
        assert rl <= 1.0 and rc <= 1.0
    return got


@pytest.mark.parametrize("absolute", [False, True], ids=["relative", "absolute"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_sums_and_finalize_element_by_element_against_fp64(dev, lib, shape, absolute):
    prd, tar, _, w = _fields(*shape)
    chw = _chw(shape[1])
    d = [torch.tensor(a).to(dev) for a in (prd, tar, w, chw)]
    g, slices = _launch(lib, dev, d[0], d[1], d[2], d[3], absolute)
    _verdict(g, slices, prd, tar, w, chw, absolute, tag=f"{shape}")


def test_channel_block_of_wider_tensors_with_different_strides(dev, lib):
    """channels 5:10 of a 15-channel prediction against channels 5:10 of an 18-channel target, read in place; without chw only the sums"""
    B, C, H, W = 2, 5, 9, 12
    prd_w, _, _, w = _fields(B, 15, H, W)
    tar_w = _fields(B, 18, H, W, seed=1)[1]
    dp, dt = torch.tensor(prd_w).to(dev), torch.tensor(tar_w).to(dev)
    vp, vt = dp[:, 5:10], dt[:, 5:10]
    assert vp.stride(0) == 15 * H * W and vt.stride(0) == 18 * H * W and vp.data_ptr() % 16 == 0
    chw = _chw(C)
    g, slices = _launch(lib, dev, vp, vt, torch.tensor(w).to(dev), torch.tensor(chw).to(dev), False)
    assert slices == 204
    _verdict(g, slices, prd_w[:, 5:10], tar_w[:, 5:10], w, chw, False, tag="block 5:10")
    g0, _ = _launch(lib, dev, vp, vt, torch.tensor(w).to(dev))
    _verdict(g0, slices, prd_w[:, 5:10], tar_w[:, 5:10], w, None, False, tag="block 5:10, no chw")
    assert torch.equal(g0["sums"].view(torch.int32), g["sums"].view(torch.int32))


@pytest.mark.parametrize("shape", [(2, 3, 5, 8), (3, 73, 16, 32), (2, 73, 240, 480)], ids=lambda s: "x".join(map(str, s)))
def test_gradient_bit_for_bit_and_coef_against_fp64(dev, lib, shape):
    """planted elements with prd == tar and one plane with prd == tar throughout; the scorer's rows (negative at the poles) and the
    loss's own rows; a second run of all three kernels gives the same bits"""
    from swin_v2_weather_amd.utils.grids import naive_quadrature_weights
    B, C, H, W = shape
    prd0, tar, _, w_lat = _fields(*shape)
    prd = prd0.copy()
    prd[B - 1, C - 1] = tar[B - 1, C - 1]
    prd[0, 0, H // 2, ::3] = tar[0, 0, H // 2, ::3]
    prd[0, 1, :, 1] = tar[0, 1, :, 1]
    chw = _chw(C)
    for w, absolute in ((w_lat, False), (naive_quadrature_weights(H, W, True).numpy(), True)):
        d = [torch.tensor(a).to(dev) for a in (prd, tar, w, chw)]
        g, slices = _launch(lib, dev, d[0], d[1], d[2], d[3], absolute)
        got = _verdict(g, slices, prd, tar, w, chw, absolute, tag=f"{shape} grad")
        assert got["sums"].reshape(B, C, 2)[B - 1, C - 1, 0] == 0.0
        gd = _grad(lib, dev, d[0], d[1], d[2], g["coef"])
        assert gd.guards_intact() and gd.written("dprd")
        want = R.grad_bits(prd, tar, w, got["coef"].reshape(B, C))
        have = gd["dprd"].cpu().numpy().reshape(B, C, H, W)
        assert np.array_equal(have.view(np.int32), want.view(np.int32)), "dprd is not +-fp32(coef q[row]) / 0 by the exact sign"
        assert np.all(have[B - 1, C - 1] == 0) and np.all(have[0, 0, H // 2, ::3] == 0) and np.all(have[0, 1, :, 1] == 0)
        g2, _ = _launch(lib, dev, d[0], d[1], d[2], d[3], absolute)
        gd2 = _grad(lib, dev, d[0], d[1], d[2], g2["coef"])
        assert torch.equal(g.raw, g2.raw) and torch.equal(gd.raw, gd2.raw)        # workspace, sums, loss, coef and gradient, bit for bit


def test_nan_in_one_plane_reaches_that_plane_and_the_loss_only(dev, lib):
    B, C, H, W = 3, 4, 16, 32
    prd, tar0, _, w = _fields(B, C, H, W)
    chw = _chw(C)
    tar = tar0.copy()
    tar[1, 2, 7, 9] = np.nan
    d = [torch.tensor(a).to(dev) for a in (prd, tar0, tar, w, chw)]
    clean, _ = _launch(lib, dev, d[0], d[1], d[3], d[4], False)
    g, _ = _launch(lib, dev, d[0], d[2], d[3], d[4], False)
    assert g.guards_intact()
    s, s0 = g["sums"].view(B, C, 2), clean["sums"].view(B, C, 2)
    assert bool(torch.isnan(s[1, 2]).all()) and bool(torch.isnan(g["loss"]).all()) and bool(torch.isfinite(clean["loss"]).all())
    keep = torch.ones(B, C, dtype=torch.bool, device=dev)
    keep[1, 2] = False
    assert torch.equal(s[keep].view(torch.int32), s0[keep].view(torch.int32))
    assert torch.equal(g["coef"].view(B, C)[keep], clean["coef"].view(B, C)[keep]) and bool(torch.isnan(g["coef"].view(B, C)[1, 2]))
    # the gradient of the NaN element is 0 (both comparisons are false), its plane's other elements carry the NaN coef
    gd = _grad(lib, dev, d[0], d[2], d[3], clean["coef"])
    assert float(gd["dprd"].view(B, C, H, W)[1, 2, 7, 9]) == 0.0 and bool(torch.isfinite(gd["dprd"]).all())


def test_loss_handler_on_the_device_against_reference_values_and_the_torch_statement(dev, lib, tmp_path):
    """the bars of the l2 strings: value within 2e-5 relative, gradient subsample within 1e-5 of its maximum"""
    from swin_v2_weather_amd.utils.losses import geometric_l1_torch
    meta, aux = golden()
    H, W, C = meta["H"], meta["W"], meta["C"]
    for key, case in meta["cases"].items():
        lh = handler(case["loss"], case["n_future"], tmp_path, aux).to(dev)
        lh.train(case["mode"] == "train")
        prd, tar = golden_fields(case, C, H, W)
        pd, td = prd.to(dev).requires_grad_(True), tar.to(dev)
        if case.get("raises"):
            with pytest.raises(RuntimeError):
                lh(pd, td, None)
            continue
        val = lh(pd, td, None)
        assert type(val.grad_fn).__name__ == "_GeoL1Backward" and len(lh._l1_ws) == 1            # the HIP kernels ran
        val.backward()
        ev = abs(float(val.detach()) - case["value"]) / abs(case["value"])
        eg = relmax(pd.grad[:, ::9, ::5, ::7].cpu(), torch.from_numpy(aux[f"gprd_{key}"]))
        p2 = prd.to(dev).requires_grad_(True)
        chw = lh._chw_now()
        v2 = geometric_l1_torch(p2, td, lh.quad_rows, chw, lh.absolute)
        v2.backward()
        ev2, eg2 = abs(float(val.detach()) - float(v2.detach())) / abs(float(v2.detach())), relmax(pd.grad, p2.grad)
        print(f"{key} '{case['loss']}': value {float(val.detach()):.7f}  rel err vs reference {ev:.2e} / torch statement {ev2:.2e}  "
              f"gradient {eg:.2e} / {eg2:.2e}")
        assert ev <= 2e-5 and eg < 1e-5 and ev2 <= 2e-5 and eg2 < 1e-5, key
        assert int((pd.grad == 0).sum()) == case["grad_zeros"]
        lh(pd, td, None)
        assert len(lh._l1_ws) == 1                                                               # the workspace is reused
    # what the kernels cannot take runs the statement: fp64, W % 4 != 0, a target that requires grad
    lh = handler("geometric l1", 0, tmp_path, aux).to(dev).train()
    prd, tar = golden_fields({"seed": 1, "n_future": 0}, C, H, W)
    for p, t in ((prd.double().to(dev), tar.double().to(dev)), (prd.to(dev), tar.to(dev).requires_grad_(True))):
        v = lh(p.requires_grad_(True), t, None)
        assert type(v.grad_fn).__name__ != "_GeoL1Backward" and abs(float(v.detach()) - 2.8246057) <= 2e-5 * 2.8246057
    odd = handler("geometric l1", 0, tmp_path, aux, W=46).to(dev)
    v = odd(prd[..., :46].to(dev).requires_grad_(True), tar[..., :46].to(dev), None)
    assert type(v.grad_fn).__name__ != "_GeoL1Backward" and bool(torch.isfinite(v))


def test_legendre_gauss_grid_for_l1_and_l2_against_fp64(dev, lib, tmp_path):
    from swin_v2_weather_amd.utils.grids import legendre_gauss_quadrature_weights
    _, aux = golden()
    B, C, H, W = 2, 73, 24, 48
    prd, tar = golden_fields({"seed": 4, "n_future": 0}, C, H, W)
    q = legendre_gauss_quadrature_weights(H, W, True)
    slices = RS.plan_slices(B * C)
    # l1: the bound of tests/l1_reference.py
    lh = handler("geometric l1", 0, tmp_path, aux, grid="legendre_gauss").to(dev).train()
    assert torch.equal(lh.quad_rows.cpu(), q)
    v = lh(prd.to(dev).requires_grad_(True), tar.to(dev), None)
    assert type(v.grad_fn).__name__ == "_GeoL1Backward"
    S, A = R.sums(prd.numpy(), tar.numpy(), q.numpy())
    ref, bound, _, _ = R.loss(S, R.sum_bounds(A, R.chain_length(H, W, slices)), lh.channel_weights.reshape(-1).cpu().numpy(), False)
    print(f"legendre_gauss 'geometric l1': {float(v.detach()):.7f}, fp64 {ref:.9f}, error / bound {abs(float(v.detach()) - ref) / bound:.3f}")
    assert abs(float(v.detach()) - ref) <= bound
    # l2: sum_bc chw S_dd / S_tt.  swv2_loss_sums: the chain of score.hip's sums (tests/score_reference.py::chain_length), 4 roundings per
    # term; swv2_loss_finalize: the division, the product with chw and ceil(B C / 256) + 6 + 3 additions
    lh2 = handler("squared geometric l2", 0, tmp_path, aux, grid="legendre_gauss").to(dev).train()
    assert torch.equal(lh2.quad_rows.cpu(), q) and lh2.squared
    v2 = lh2(prd.to(dev).requires_grad_(True), tar.to(dev), None)
    S2, A2 = RS.sums(prd.numpy(), tar.numpy(), q.numpy())
    d2 = RS.sum_bounds(A2, RS.chain_length(H, W, slices))
    cw = lh2.channel_weights.reshape(1, -1).cpu().numpy().astype(np.float64)
    ratio = S2[..., 0] / S2[..., 3]
    dratio = (S2[..., 0] + d2[..., 0]) * (1 + R.U) / (S2[..., 3] - d2[..., 3]) - ratio
    k = math.ceil(B * C / 256) + 6 + 3 + 1
    ref2, bound2 = float((cw * ratio).sum()), float((1 + RS.gamma(k)) * (cw * dratio).sum() + RS.gamma(k) * (cw * ratio).sum())
    print(f"legendre_gauss 'squared geometric l2': {float(v2.detach()):.7f}, fp64 {ref2:.9f}, error / bound {abs(float(v2.detach()) - ref2) / bound2:.3f}")
    assert abs(float(v2.detach()) - ref2) <= bound2


def test_fused_with_is_a_no_op_for_l1_through_a_tiny_model(dev, lib):
    from swin_v2_weather_amd.networks import swinv2_global as N
    from swin_v2_weather_amd.utils.losses import LossHandler, geometric_l1_torch
    torch.manual_seed(5)
    H, W, Cio = 48, 72, 6
    names = ["u10m", "t2m", "z500", "q850", "tp", "v100"]
    m = N.SwinTransformerV2Cr(img_size=(H, W), patch_size=4, depths=(2,), num_heads=(2,), in_chans=Cio, out_chans=Cio, embed_dim=24,
                              img_window_ratio=8, drop_path_rate=0.0, full_pos_embed=True, rel_pos=False, mlp_ratio=4, residual=True).to(dev)
    with torch.no_grad():
        for n, p_ in m.named_parameters():
            if n.endswith("norm1.weight") or n.endswith("norm2.weight"):
                p_.fill_(0.7)
    lh = LossHandler(SimpleNamespace(n_future=0, img_shape_x=H, img_shape_y=W, loss="weighted relative temp-std geometric l1", channel_weights="auto",
                                     n_out_channels=Cio, channel_names=names, out_channels=np.arange(Cio), dt=1,
                                     model_grid_type="equiangular")).to(dev)
    m.train(); lh.train()
    x, tar = torch.randn(3, Cio, H, W, device=dev), torch.randn(3, Cio, H, W, device=dev)
    with lh.fused_with(m, tar):
        assert m._loss_ctx is None and lh._fused is None          # the head is handed no l2 context
        gen = m(x)
    gen.retain_grad()
    val = lh(gen, tar, x)
    assert type(val.grad_fn).__name__ == "_GeoL1Backward"
    val.backward()
    out = gen.detach().clone().requires_grad_(True)
    ref = geometric_l1_torch(out, tar, lh.quad_rows, lh._chw_now(), lh.absolute)
    ref.backward()
    ev, eg = abs(float(val.detach()) - float(ref.detach())) / abs(float(ref.detach())), relmax(gen.grad, out.grad)
    print(f"fused_with, l1: loss {float(val.detach()):.7f} vs torch statement {float(ref.detach()):.7f} ({ev:.2e}), d loss / d output {eg:.2e}")
    assert ev <= 2e-5 and eg < 1e-5
    grads = [p_.grad for p_ in m.parameters() if p_.grad is not None]
    assert grads and all(bool(torch.isfinite(g_).all()) for g_ in grads) and any(float(g_.abs().max()) > 0 for g_ in grads)


def test_forecast_scorer_mae_against_fp64_in_place_at_a_channel_offset(dev, lib):
    from swin_v2_weather_amd import ops
    from swin_v2_weather_amd.utils.weighted_acc_rmse import ForecastScorer
    B, C, H, W = 2, 5, 9, 12
    prd_w, _, _, w = _fields(B, 15, H, W)
    tar_w = _fields(B, 18, H, W, seed=1)[1]
    stds = np.array([1.5, 2.0, 0.25, 9.0, 4.0], np.float32)
    dp, dt = torch.tensor(prd_w).to(dev), torch.tensor(tar_w).to(dev)
    sc = ForecastScorer(H, W, C, dev, stds=stds)
    r = sc.mae(dp, dt, coff_prd=5, coff_tar=7)
    assert r.mae.is_cuda and ("l1", B) in sc._ws
    p, t = prd_w[:, 5:10], tar_w[:, 7:12]
    S, A = R.sums(p, t, w)
    dS = R.sum_bounds(A, R.chain_length(H, W, ops.score_slices(B * C, H, W)))
    rs = R.worst(np.abs(r.sums.cpu().numpy() - S), dS)
    m_ref, m_b = R.mae(S, dS, H, W)
    rm = R.worst(np.abs(r.mae.cpu().numpy() - m_ref), m_b)
    mm_ref, mm_b = R.batch_mean(r.mae.cpu().numpy(), stds)
    rmm = R.worst(np.abs(r.mae_mean.cpu().numpy() - mm_ref), mm_b)
    print(f"ForecastScorer.mae: worst error / bound  sums {rs:.3f}  mae {rm:.3f}  mae_mean {rmm:.3f}")
    assert rs <= 1.0 and rm <= 1.0 and rmm <= 1.0
    r2 = sc.mae(dp, dt, 5, 7)
    assert torch.equal(r2.mae, r.mae) and r2.mae.data_ptr() != r.mae.data_ptr() and len(sc._ws) == 1
    # odd width: the torch path on the device, judged as a sum in any order
    Wo = 10
    po, to_ = np.ascontiguousarray(prd_w[..., :Wo]), np.ascontiguousarray(tar_w[..., :Wo])
    ro = ForecastScorer(H, Wo, C, dev).mae(torch.tensor(po).to(dev), torch.tensor(to_).to(dev), 5, 7)
    So, Ao = R.sums(po[:, 5:10], to_[:, 7:12], w)
    assert R.worst(np.abs(ro.sums.cpu().numpy() - So), R.sum_bounds(Ao, H * Wo)) <= 1.0


def test_trainer_trains_and_validates_with_an_l1_loss(dev, lib, tmp_path):
    """the construction of tests/test_score_gpu.py::test_trainer_logs_valid_acc_when_time_means_is_a_file with an l1 loss string: one epoch
    with a finite train loss, and valid_loss = a by-hand pass of the same batches through the torch statement"""
    from swin_v2_weather_amd.train import Trainer
    from swin_v2_weather_amd.utils.YParams import YParams
    from swin_v2_weather_amd.utils.losses import geometric_l1_torch
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
    p["loss"], p["drop_path_rate"], p["rel_pos"] = "weighted absolute temp-std geometric l1", 0.1, True
    p["channel_weights"] = "auto"                                                # (the config's 'none' goes with its unweighted l2)
    t = Trainer(p, SimpleNamespace(sweep_id=None, config="bench_tiny", run_num="00", enable_amp=True))
    t.build()
    assert t.loss_obj.p == 1
    _, _, train_logs = t.train_one_epoch()
    assert math.isfinite(float(train_logs["loss"])) and float(train_logs["loss"]) > 0 and len(t.loss_obj._l1_ws) == 1
    _, logs = t.validate_one_epoch()
    lh = t.loss_obj
    vals, bounds = [], []
    with torch.no_grad():
        for data in t.valid_data_loader:
            inp, tar, coszen = t.preprocessor(data)
            gen = t.model(inp, coszen=coszen).float()
            vals.append(float(geometric_l1_torch(gen, tar, lh.quad_rows, lh._chw_now(), lh.absolute)))
            B, C, H, W = gen.shape
            S, A = R.sums(gen.cpu().numpy(), tar.cpu().numpy(), lh.quad_rows.cpu().numpy())
            cw = lh._chw_now().reshape(-1).cpu().numpy()
            # the kernels and the statement each stand within their own bound of the fp64 value
            bounds.append(R.loss(S, R.sum_bounds(A, R.chain_length(H, W, RS.plan_slices(B * C))), cw, True)[1] +
                          R.loss(S, R.sum_bounds(A, H * W), cw, True, k=B * C + 1)[1])
    ref = sum(vals) / len(vals)
    bound = sum(bounds) / len(bounds) + 2 * RS.gamma(len(vals) + 1) * abs(ref)        # the trainer adds the steps in fp32, then divides
    e = abs(float(logs["valid_loss"]) - ref)
    print(f"valid_loss {float(logs['valid_loss']):.7f} vs by hand {ref:.7f}: error / bound {e / bound:.3f}")
    assert e <= bound
