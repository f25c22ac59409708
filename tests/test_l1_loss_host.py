"""Host (no GPU): the l1 loss family through its plain-torch statement against the reference's own numbers (tests/golden/loss_l1_*,
made by tests/golden/make_golden_l1.py from the real reference), the string quirks, the Gauss-Legendre rows against what defines the
rule, the host half of the swv2_l1_* entry points, and ForecastScorer.mae on CPU tensors against the fp64 statement of
tests/l1_reference.py."""
import ctypes
import json
import math
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from swin_v2_weather_amd import _lib as L
from tests import l1_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
NAMES = (["u10m", "v10m", "u100m", "v100m", "t2m", "sp", "msl", "tcwv"] +
         [f"{v}{l}" for v in "uvztq" for l in (50, 100, 150, 200, 250, 300, 400, 500, 600, 700, 850, 925, 1000)])


def golden():
    meta = json.load(open(os.path.join(GOLD, "loss_l1_values.json")))
    return meta, np.load(os.path.join(GOLD, "loss_l1_aux.npz"))


def handler(loss, n_future, tmp_path, aux, H=24, W=48, C=73, grid="equiangular", names=NAMES):
    from swin_v2_weather_amd.utils.losses import LossHandler
    gs, td = str(tmp_path / "gs.npy"), str(tmp_path / "td.npy")
    np.save(gs, aux["global_stds"]); np.save(td, aux["time_diff_stds"])
    return LossHandler(SimpleNamespace(n_future=n_future, img_shape_x=H, img_shape_y=W, loss=loss, channel_weights="auto", n_out_channels=C,
                                       channel_names=names, out_channels=np.arange(C), global_stds_path=gs, time_diff_stds_path=td, dt=1,
                                       model_grid_type=grid))


def golden_fields(case, C, H, W):
    torch.manual_seed(case["seed"])
    n = C * (case["n_future"] + 1)
    return torch.randn(2, n, H, W), torch.randn(2, n, H, W)


def relmax(a, b):
    return float((a - b).abs().max() / b.abs().max())


def test_torch_statement_against_every_reference_value_and_gradient(tmp_path):
    """the bars of the l2 strings (tests/test_gpu_parity.py::test_loss_handler_against_reference_values): value within 2e-5 relative,
    gradient subsample within 1e-5 of its maximum; where the reference itself raises (eval with n_future = 1) so does the statement"""
    meta, aux = golden()
    H, W, C = meta["H"], meta["W"], meta["C"]
    assert len(meta["cases"]) == 24
    for key, case in meta["cases"].items():
        lh = handler(case["loss"], case["n_future"], tmp_path, aux)
        lh.train(case["mode"] == "train")
        prd, tar = golden_fields(case, C, H, W)
        prd.requires_grad_(True)
        if case.get("raises"):
            with pytest.raises(RuntimeError):
                lh(prd, tar, None)
            continue
        val = lh(prd, tar, None)
        ev = abs(float(val.detach()) - case["value"]) / abs(case["value"])
        val.backward()
        eg = relmax(prd.grad[:, ::9, ::5, ::7], torch.from_numpy(aux[f"gprd_{key}"]))
        print(f"{key} '{case['loss']}': value {float(val.detach()):.7f} rel err {ev:.2e}  gradient rel err {eg:.2e}")
        assert ev <= 2e-5 and eg < 1e-5, key
        assert int((prd.grad == 0).sum()) == case["grad_zeros"] == 2 * prd.shape[1] * 2 * W      # the pole rows, and nothing else


def test_unweighted_strings_are_one_number_and_squared_reaches_the_channel_factor_only(tmp_path):
    _, aux = golden()
    prd, tar = golden_fields({"seed": 1, "n_future": 0}, 73, 24, 48)
    vals = [handler(s, 0, tmp_path, aux)(prd, tar, None) for s in ("l1", "geometric l1", "squared geometric l1")]
    assert torch.equal(vals[0], vals[1]) and torch.equal(vals[0], vals[2])
    assert abs(float(vals[0]) - 2.8246057) <= 2e-5 * 2.8246057
    a, b = handler("weighted relative temp-std geometric l1", 0, tmp_path, aux), handler("weighted relative temp-std squared geometric l1", 0, tmp_path, aux)
    assert torch.equal(a.quad_rows, b.quad_rows) and not torch.equal(a.channel_weights, b.channel_weights)
    # l2 wins when both words occur, as in the reference's if / elif
    both, l2 = handler("squared geometric l1 l2", 0, tmp_path, aux), handler("squared geometric l2", 0, tmp_path, aux)
    assert both.p == 2 and both.squared and l2.p == 2 and handler("l1", 0, tmp_path, aux).p == 1


def test_gradient_is_exactly_zero_where_prd_equals_tar_and_on_the_pole_rows(tmp_path):
    _, aux = golden()
    lh = handler("weighted relative temp-std geometric l1", 0, tmp_path, aux)
    prd, tar = golden_fields({"seed": 3, "n_future": 0}, 73, 24, 48)
    prd[0, 5] = tar[0, 5]
    prd[1, 7, 3:9, ::5] = tar[1, 7, 3:9, ::5]
    prd.requires_grad_(True)
    lh(prd, tar, None).backward()
    g = prd.grad
    assert bool((g[0, 5] == 0).all()) and bool((g[1, 7, 3:9, ::5] == 0).all())
    assert bool((g[:, :, 0] == 0).all()) and bool((g[:, :, -1] == 0).all())
    inner = g[:, :, 1:-1].clone()
    inner[0, 5] = 1.0
    inner[1, 7, 2:8, ::5] = 1.0
    assert bool((inner != 0).all())                            # nothing else is zero
    S, _ = R.sums(prd.detach().numpy(), tar.numpy(), lh.quad_rows.numpy())
    _, _, coef, _ = R.loss(S, np.zeros_like(S), lh.channel_weights.reshape(-1).numpy(), False)
    ref = R.grad(prd.detach().numpy(), tar.numpy(), lh.quad_rows.numpy(), coef)
    assert np.abs(g.numpy() - ref).max() <= 1e-5 * np.abs(ref).max()


def test_fused_with_hands_the_head_no_l2_context(tmp_path):
    _, aux = golden()
    net = SimpleNamespace(_features_bhwc=None, _loss_ctx=None, out_chans=73)
    model = SimpleNamespace(module=SimpleNamespace(model=net))
    tar = torch.zeros(2, 73, 24, 48)
    l1 = handler("weighted absolute temp-std geometric l1", 0, tmp_path, aux).train()
    with l1.fused_with(model, tar):
        assert net._loss_ctx is None and l1._fused is None
    assert net._loss_ctx is None
    l2 = handler("weighted absolute temp-std squared geometric l2", 0, tmp_path, aux).train()
    with l2.fused_with(model, tar):
        assert net._loss_ctx is not None and l2._fused is net._loss_ctx          # (the l2 hand-over is what it was)
    assert net._loss_ctx is None


def test_l2_strings_construct_the_buffers_they_did(tmp_path):
    """channel_weights and quad_rows of the four l2 strings, bit for bit, from the formulas of the constructor before l1 existed"""
    from swin_v2_weather_amd.utils.grids import naive_quadrature_weights
    from swin_v2_weather_amd.utils.losses import auto_channel_weights
    _, aux = golden()
    for s in ("l2", "squared geometric l2", "weighted absolute temp-std squared geometric l2", "weighted relative temp-std geometric l2"):
        for nf in (0, 1):
            lh = handler(s, nf, tmp_path, aux)
            flags = set(s.split())
            cw = auto_channel_weights(NAMES, 73) if "weighted" in flags else torch.ones(73)
            cw = cw.reshape(1, -1, 1, 1)
            cw = cw / torch.sum(cw)
            if "temp-std" in flags:
                tvw = torch.from_numpy(aux["global_stds"]).reshape(1, -1, 1, 1) / (np.sqrt(1) * torch.from_numpy(aux["time_diff_stds"]).reshape(1, -1, 1, 1) + 1e-6)
                cw = cw * (tvw ** 2 if "squared" in flags else tvw)
            assert torch.equal(lh.channel_weights, cw.float()) and torch.equal(lh.quad_rows, naive_quadrature_weights(24, 48, True))
            assert lh.p == 2 and lh.squared == ("squared" in flags and "geometric" in flags) and lh.absolute == ("absolute" in flags)
            assert torch.equal(lh.multistep_weight, torch.full((nf + 1, 1, 1, 1), 1.0 / (nf + 1)))
            assert sorted(k for k, _ in lh.named_buffers()) == ["channel_weights", "multistep_weight", "quad_rows"]


@pytest.mark.parametrize("s", ["pole-masked geometric l1", "pole-masked l2", "geometric h1", "absolute geometric h1", "huber"])
def test_strings_that_keep_raising(tmp_path, s):
    _, aux = golden()
    with pytest.raises(ValueError):
        handler(s, 0, tmp_path, aux)
    # it is that word which raises: the same string with l1 in its place constructs
    ok = " ".join("l1" if w in ("pole-masked", "h1", "huber") else w for w in s.split() if w != "l2")
    assert handler(ok, 0, tmp_path, aux).p == 1


def test_legendre_gauss_rows_against_what_defines_the_rule(tmp_path):
    from swin_v2_weather_amd.utils.grids import GridQuadrature, legendre_gauss_quadrature_weights, naive_quadrature_weights
    for H, W in ((4, 8), (9, 12), (24, 48)):
        q = legendre_gauss_quadrature_weights(H, W, True)
        assert q.dtype == torch.float32 and tuple(q.shape) == (H,)
        assert bool((q > 0).all()) and torch.equal(q, q.flip(0))                                # positive, symmetric about the equator
        assert abs(float((q.double() * W).sum()) - 1.0) <= (H + 1) * 2.0 ** -24                 # every row rounded once to fp32
        un = legendre_gauss_quadrature_weights(H, W, False)
        assert abs(float((un.double() * W).sum()) - 4 * np.pi) <= (H + 1) * 2.0 ** -24 * 4 * np.pi
        # the rule itself: H nodes integrate x^k over [-1, 1] exactly for every k <= 2 H - 1 and not for k = 2 H
        x, w = np.polynomial.legendre.leggauss(H)
        assert np.array_equal(q.numpy(), (w * (2 * np.pi / W) / (4 * np.pi)).astype(np.float32))
        for k in range(2 * H):
            assert abs(np.sum(w * x ** k) - (0.0 if k % 2 else 2.0 / (k + 1))) <= 1e-13, (H, k)
        # k = 2 H: short by the rule's own error term 2^(2H+1) (H!)^4 / ((2H+1) ((2H)!)^2) = 1.2e-2, 1.2e-5, 1.1e-14 -- at H = 24 that is
        # below the 1e-13 of the exact degrees but fifty times the rounding of the sum (H terms of size <= 2 / H: ~ 2^-52), so the failure
        # is asked for as the term itself, to a tenth
        f = [float(math.factorial(n)) for n in (H, 2 * H)]
        short = 2.0 ** (2 * H + 1) * f[0] ** 4 / ((2 * H + 1) * f[1] ** 2)
        miss = 2.0 / (2 * H + 1) - np.sum(w * x ** (2 * H))
        print(f"H = {H}: x^{2 * H} is integrated short by {miss:.4e}, the rule's error term is {short:.4e}")
        assert miss > 0 and abs(miss - short) <= 0.1 * short
        gq = GridQuadrature("legendre-gauss", (H, W), normalize=True)
        assert torch.equal(gq.quad_weight[0, 0], q.unsqueeze(1).repeat(1, W))
    with pytest.raises(ValueError):
        GridQuadrature("clenshaw-curtiss", (8, 16))
    # LossHandler: the rule only where the string says geometric, for l1 and l2 alike
    _, aux = golden()
    lg, nv = legendre_gauss_quadrature_weights(24, 48, True), naive_quadrature_weights(24, 48, True)
    for s, want in (("geometric l1", lg), ("squared geometric l2", lg), ("l1", nv), ("l2", nv)):
        assert torch.equal(handler(s, 0, tmp_path, aux, grid="legendre_gauss").quad_rows, want), s
    # and the value of the statement with those rows against fp64
    lh = handler("weighted relative temp-std geometric l1", 0, tmp_path, aux, grid="legendre_gauss")
    prd, tar = golden_fields({"seed": 4, "n_future": 0}, 73, 24, 48)
    S, A = R.sums(prd.numpy(), tar.numpy(), lg.numpy())
    ref, bound, _, _ = R.loss(S, R.sum_bounds(A, 24 * 48), lh.channel_weights.reshape(-1).numpy(), False, k=2 * 73 + 1)
    assert abs(float(lh(prd, tar, None)) - ref) <= bound


def test_abi_version_sources_and_workspace_arithmetic():
    assert L.ABI_VERSION == 113 and "loss_l1.hip" in L.SOURCES
    lib = L.load()
    assert lib.swv2_version() == 113
    for (B, C, H, W) in ((1, 1, 1, 4), (2, 3, 5, 8), (1, 73, 720, 1440), (2, 73, 720, 1440), (1, 2100, 2, 4), (3, 5, 16, 32)):
        slices = lib.swv2_score_slices(B * C, H, W)
        assert lib.swv2_l1_ws_bytes(B * C, H, W) == B * C * slices * 8 and slices == R.plan_slices(B * C)
    for bad in ((0, 4, 4), (4, 0, 4), (4, 4, 0), (-1, 4, 4)):
        assert lib.swv2_l1_ws_bytes(*bad) == 0, bad
    # thread + 6 + 2 + fold + 6
    assert R.chain_length(1, 4, 2048) == 4 + 14 + 32 and R.chain_length(2, 4, 1) == 4 + 14 + 1
    assert R.chain_length(64, 64, 1) == 16 + 15 and R.chain_length(720, 1440, 14) == 4 * 73 + 15
    assert R.C_TERM == 2


def test_header_and_ctypes_agree_on_the_l1_entry_points():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "swv2.h")).read(), flags=re.S)
    kinds = {"int": ctypes.c_int, "long": ctypes.c_long, "size_t": ctypes.c_size_t}
    seen = []
    for ret, name, args in re.findall(r"\b(int|size_t)\s+(swv2_l1_[a-z_]+)\s*\(([^)]*)\)\s*;", txt):
        want = [ctypes.c_void_p if "*" in a else kinds[a.split()[0]] for a in (x.strip() for x in args.split(","))]
        res, argtypes = L.SYMBOLS[name]
        assert res is kinds[ret] and argtypes == want, name
        seen.append(name)
    assert sorted(seen) == ["swv2_l1_finalize", "swv2_l1_grad", "swv2_l1_sums", "swv2_l1_ws_bytes"]
    lib = L.load()
    assert all(hasattr(lib, n) for n in seen)


def test_every_refusal_returns_invalid_with_a_message_and_without_a_gpu():
    """Arguments are checked before anything is launched, so the pointers only have to be non-null here: a refused call touches nothing."""
    lib = L.load()
    P = 4096
    B, C, H, W = 2, 3, 8, 16
    span = C * H * W
    ok = lib.swv2_l1_ws_bytes(B * C, H, W)

    def sums(prd=P, ps=span, tar=P, ts=span, w=P, B=B, C=C, H=H, W=W, ws=P, wb=ok):
        return lib.swv2_l1_sums(prd, ps, tar, ts, w, B, C, H, W, ws, wb, None)

    def fin(ws=P, wb=ok, B=B, C=C, H=H, W=W, chw=None, s=P, loss=None, coef=None):
        return lib.swv2_l1_finalize(ws, wb, B, C, H, W, chw, 0, s, loss, coef, None)

    def grad(prd=P, tar=P, q=P, coef=P, d=P, BC=B * C, H=H, W=W):
        return lib.swv2_l1_grad(prd, tar, q, coef, d, BC, H, W, None)
    for call, word in ((lambda: sums(prd=None), b"null"), (lambda: sums(tar=None), b"null"), (lambda: sums(w=None), b"null"),
                       (lambda: sums(ws=None), b"null"), (lambda: sums(W=18), b"W % 4"), (lambda: sums(W=0), b"shape"), (lambda: sums(B=0), b"shape"),
                       (lambda: sums(prd=P + 4), b"aligned"), (lambda: sums(tar=P + 8), b"aligned"), (lambda: sums(ws=P + 4), b"aligned"),
                       (lambda: sums(ps=span + 1), b"stride"), (lambda: sums(ts=span + 3), b"stride"), (lambda: sums(ps=H * W), b"stride"),
                       (lambda: sums(wb=ok - 1), b"workspace"), (lambda: sums(wb=0), b"workspace"),
                       (lambda: sums(B=1 << 12, C=1 << 8), b"shape"), (lambda: sums(H=1 << 15, W=1 << 15), b"shape"),
                       (lambda: fin(ws=None), b"null"), (lambda: fin(s=None), b"null"), (lambda: fin(chw=P), b"null"),
                       (lambda: fin(chw=P, loss=P), b"null"), (lambda: fin(wb=ok - 8), b"workspace"), (lambda: fin(s=P + 4), b"aligned"),
                       (lambda: fin(ws=P + 8), b"aligned"), (lambda: fin(C=0), b"shape"),
                       (lambda: grad(prd=None), b"bad argument"), (lambda: grad(coef=None), b"bad argument"), (lambda: grad(W=18), b"W % 4"),
                       (lambda: grad(BC=65536), b"too large"), (lambda: grad(H=1 << 15, W=1 << 15), b"too large"),
                       (lambda: grad(d=P + 4), b"aligned"), (lambda: grad(H=0), b"bad argument")):
        assert call() == -1
        assert word in lib.swv2_last_error(), lib.swv2_last_error()
    from swin_v2_weather_amd import ops
    with pytest.raises(L.Swv2Error):
        ops.l1_sums(torch.zeros(1, 2, 4, 8), torch.zeros(1, 2, 4, 8), torch.ones(4), torch.zeros(64))          # CPU tensors


def test_forecast_scorer_mae_on_cpu_against_fp64():
    from swin_v2_weather_amd.utils.weighted_acc_rmse import ForecastScorer, MaeScores
    B, C, H, W = 2, 5, 9, 12
    rng = np.random.default_rng(7)
    prd, tar = rng.standard_normal((B, 15, H, W)).astype(np.float32), rng.standard_normal((B, 18, H, W)).astype(np.float32)
    stds = np.array([1.5, 2.0, 0.25, 9.0, 4.0], np.float32)
    sc = ForecastScorer(H, W, C, "cpu", stds=stds)
    r = sc.mae(torch.from_numpy(prd), torch.from_numpy(tar), coff_prd=5, coff_tar=7)
    assert isinstance(r, MaeScores) and tuple(r.mae.shape) == (B, C) and tuple(r.mae_mean.shape) == (C,) and tuple(r.sums.shape) == (B, C, 2)
    p, t, w = prd[:, 5:10], tar[:, 7:12], sc.w.numpy()
    S, A = R.sums(p, t, w)
    dS = R.sum_bounds(A, H * W)                                # torch: any order of H W terms
    rs = R.worst(np.abs(r.sums.numpy() - S), dS)
    m_ref, m_b = R.mae(S, dS, H, W)
    rm = R.worst(np.abs(r.mae.numpy() - m_ref), m_b)
    mm_ref, mm_b = R.batch_mean(r.mae.numpy(), stds)
    rmm = R.worst(np.abs(r.mae_mean.numpy() - mm_ref), mm_b)
    print(f"ForecastScorer.mae on CPU: worst error / bound  sums {rs:.3f}  mae {rm:.3f}  mae_mean {rmm:.3f}")
    assert rs <= 1.0 and rm <= 1.0 and rmm <= 1.0
    # score() is what it was: the same fields, no new member
    assert sc.score(torch.from_numpy(prd), torch.from_numpy(tar), 5, 7)._fields == ("rmse", "acc", "rmse_mean", "acc_mean", "sums")
