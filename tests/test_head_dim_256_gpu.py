"""GPU (-m gpu): 256-channel attention heads (embed 2048 / 8 heads; csrc/attn_d256.hip) and the rest of the block at that width,
against exact fp64 autograd and against the oracle in the kernels' rounding mode.  Bars as in tests/test_gpu_parity.py."""
import ctypes
import os

import numpy as np
import pytest
import torch

from oracle import swin_oracle as O
from swin_v2_weather_amd import _lib
from tests.test_gpu_parity import (BLOCK_LOGIT_TOL, ORACLE_LOGIT_TOL, _with_wide, block_cfg, emulate_kernels, from_heads, rb, rel,
                                   to_heads, worst_grad)

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def K():
    from swin_v2_weather_amd import _lib as L, ops
    from swin_v2_weather_amd.networks import swinv2_global as N, helpers
    L.load()
    return dict(L=L, ops=ops, N=N, helpers=helpers)


def _core_inputs(dev, ops, wh, ww, h, nwh, nww, shifted, seed=0):
    d = 256
    torch.manual_seed(seed)
    B, Lw, nW, Cc = 1, wh * ww, nwh * nww, h * d
    Lp, DP = ops.attn_geometry(Lw, d)
    assert (Lp, DP) == (176, 256)
    Bw = B * nW
    qkv = torch.randn(Bw, Lw, 3 * Cc)
    ls = torch.log(torch.tensor(10.0)) + 0.5 * torch.randn(h)
    ls[-1] = 5.0                                               # above the ln(100) clamp: zero gradient expected
    if h >= 8:
        ls[0], ls[1] = float(np.log(27.0)), float(np.log(30.0))
    gh, gw = nwh * wh, nww * ww
    sh = wh // 2 if (shifted and nwh > 1) else 0
    sw = ww // 2 if shifted else 0
    mask = O.shift_mask(gh, gw, wh, ww, sh, sw)
    mask_thr = (wh - sh) * ww if sh > 0 else 0
    q, k, v = qkv.reshape(Bw, Lw, 3, Cc).unbind(2)
    qh, kh = q.reshape(Bw, Lw, h, d), k.reshape(Bw, Lw, h, d)
    rq, rk = 1.0 / qh.norm(dim=-1).clamp_min(1e-12), 1.0 / kh.norm(dim=-1).clamp_min(1e-12)
    qn, kn, vb = rb(qh * rq.unsqueeze(-1)).reshape(Bw, Lw, Cc), rb(kh * rk.unsqueeze(-1)).reshape(Bw, Lw, Cc), rb(v)
    packed = torch.stack([qn, kn, vb], 2).reshape(Bw, Lw, 3 * Cc)
    qkvh = to_heads(packed, Bw, Lw, h, d, Lp, DP, 3).to(BF).to(dev).contiguous()
    rnorm = torch.zeros(Bw, h, 2, Lp)
    rnorm[:, :, 0, :Lw], rnorm[:, :, 1, :Lw] = rq.permute(0, 2, 1), rk.permute(0, 2, 1)
    go = rb(torch.randn(Bw, Lw, Cc))
    return dict(d=d, B=B, Lw=Lw, nW=nW, Cc=Cc, Lp=Lp, DP=DP, Bw=Bw, ls=ls, mask=mask, mask_thr=mask_thr, qn=qn, kn=kn, vb=vb,
                rq=rq, rk=rk, packed=packed, qkvh=qkvh, rnorm=rnorm.to(dev).contiguous(), go=go)


def _run(dev, ops, I, h, nwh, nww):
    Bw, Lw, Lp, DP, d = I["Bw"], I["Lw"], I["Lp"], I["DP"], I["d"]
    lsd = I["ls"].to(dev)
    oh = torch.full((Bw, h, Lp, DP), float("nan"), dtype=BF, device=dev)
    lse = torch.zeros(Bw, h, Lp, device=dev)
    ops.attn_fwd(ops.attn_args(I["qkvh"], lsd, None, oh, lse, Bw, h, Lw, d, nwh, nww, I["mask_thr"]))
    doh = to_heads(I["go"], Bw, Lw, h, d, Lp, DP, 1).squeeze(2).to(BF).to(dev).contiguous()
    dqkvh = torch.full((Bw, h, 3, Lp, DP), float("nan"), dtype=BF, device=dev)
    dls = torch.zeros(h, device=dev)
    ops.attn_bwd(ops.attn_args(I["qkvh"], lsd, None, oh, lse, Bw, h, Lw, d, nwh, nww, I["mask_thr"], doh=doh, rnorm=I["rnorm"],
                               dqkvh=dqkvh, dlogit=dls))
    return oh, lse, doh, dqkvh, dls


@pytest.mark.parametrize("wh,ww,h,nwh,nww,shifted", [
    (9, 18, 8, 2, 2, False), (9, 18, 2, 2, 2, True),         # the reference's 9 x 18 window: compile-time L = 162
    (10, 17, 1, 2, 2, True), (11, 16, 2, 2, 1, False),       # 170 / 176 tokens: run-time L
    (8, 16, 2, 2, 2, True), (8, 10, 8, 1, 2, False),         # 128 / 80 tokens: key tiles that hold padding only
])
def test_attention_core_d256(dev, K, wh, ww, h, nwh, nww, shifted):
    ops = K["ops"]
    I = _core_inputs(dev, ops, wh, ww, h, nwh, nww, shifted)
    Bw, Lw, Cc, d, Lp, B, nW = I["Bw"], I["Lw"], I["Cc"], I["d"], I["Lp"], I["B"], I["nW"]
    oh, lse, doh, dqkvh, dls = _run(dev, ops, I, h, nwh, nww)
    ref_in = I["packed"].double().requires_grad_(True)
    ls_ref = I["ls"].double().requires_grad_(True)
    q_, k_, v_ = ref_in.reshape(Bw, Lw, 3, h, d).permute(2, 0, 3, 1, 4)
    S = torch.einsum("bhqd,bhkd->bhqk", q_, k_) * torch.exp(torch.clamp(ls_ref, max=O.LOGIT_MAX)).view(1, h, 1, 1)
    mask = I["mask"]
    if mask is not None:
        S = (S.reshape(B, nW, h, Lw, Lw) + mask.double().view(1, nW, 1, Lw, Lw)).reshape(Bw, h, Lw, Lw)
    o_ref = torch.einsum("bhqk,bhkd->bqhd", torch.softmax(S, -1), v_).reshape(Bw, Lw, Cc)
    ohc = oh.float().cpu()
    assert not torch.isnan(ohc).any()
    assert rel(from_heads(ohc.unsqueeze(2), Bw, Lw, h, d, 1), o_ref) < 4e-3
    assert float(ohc[:, :, Lw:, :].abs().max() if Lp > Lw else 0) == 0            # padded query rows
    o_ref.backward(I["go"].double())
    dq = dqkvh.float().cpu()
    assert not torch.isnan(dq).any()
    assert float(dq[:, :, :, Lw:, :].abs().max() if Lp > Lw else 0) == 0           # padded rows of d(qkv)
    got = from_heads(dq, Bw, Lw, h, d, 3).reshape(Bw, Lw, 3, Cc)
    g = ref_in.grad.reshape(Bw, Lw, 3, Cc)

    def through_norm(gn, xn, r):
        gn, xn = gn.reshape(Bw, Lw, h, d), xn.reshape(Bw, Lw, h, d).double()
        return (r.unsqueeze(-1).double() * (gn - xn * (gn * xn).sum(-1, keepdim=True))).reshape(Bw, Lw, Cc)
    assert rel(got[:, :, 0], through_norm(g[:, :, 0], I["qn"], I["rq"])) < 1.5e-2
    assert rel(got[:, :, 1], through_norm(g[:, :, 1], I["kn"], I["rk"])) < 1.5e-2
    assert rel(got[:, :, 2], g[:, :, 2]) < 6e-3
    assert float(dls[-1]) == 0.0 and rel(dls, ls_ref.grad) < 0.15                  # clamp gate
    emulate_kernels(K, Lw, d, False, "row_max")
    try:
        ls_e = I["ls"].clone().requires_grad_(True)
        qe, ke, ve = (t.reshape(Bw, Lw, h, d).permute(0, 2, 1, 3).float() for t in (I["qn"], I["kn"], I["vb"]))
        oe = O.attention_core_normed(qe, ke, ve, ls_e, None, mask.float() if mask is not None else None)
        oe.backward(I["go"])
    finally:
        O.set_rounding(None)
    assert rel(dls, ls_e.grad) < ORACLE_LOGIT_TOL, (dls.cpu(), ls_e.grad)


def test_attention_d256_backward_is_deterministic(dev, K):
    ops = K["ops"]
    I = _core_inputs(dev, ops, 9, 18, 8, 2, 4, True, seed=3)
    _, _, _, d1, _ = _run(dev, ops, I, 8, 2, 4)
    _, _, _, d2, _ = _run(dev, ops, I, 8, 2, 4)
    assert torch.equal(d1, d2)


def test_bias_at_head_dim_256_is_unsupported(dev, K):
    ops, L = K["ops"], K["L"]
    I = _core_inputs(dev, ops, 9, 18, 1, 1, 1, False)
    Bw, Lp = I["Bw"], I["Lp"]
    oh = torch.zeros(Bw, 1, Lp, 256, dtype=BF, device=dev)
    lse = torch.zeros(Bw, 1, Lp, device=dev)
    bias = torch.zeros(1, 162, 162, device=dev)
    with pytest.raises(L.Swv2Error, match="head_dim=256"):
        ops.attn_fwd(ops.attn_args(I["qkvh"], I["ls"].to(dev), bias, oh, lse, Bw, 1, 162, 256, 1, 1, 0))


def chunk_rel(a, b, dim=-1, width=64):
    """worst relative l2 error over the 64-column pieces along `dim` (an error confined to one piece is not diluted)"""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return max(rel(x, y) for x, y in zip(a.split(width, dim), b.split(width, dim)))


def _both(run, kernel, families=(_lib.LINEAR_TILE_KERNELS, _lib.LINEAR_WIDE_KERNELS)):
    """run() under the 128-tile kernels (SWV2_GEMM_WIDE=0) and the wide ones (=1); returns the two result lists.  kernel(): the
    library's answer for the product run() launches (swv2_linear_kernel / swv2_linear_wgrad_kernel), which must be a tile kernel
    under =0 and a wide one under =1"""
    out = []
    for flag in ("0", "1"):
        res = []

        def go():
            assert kernel() in families[int(flag)], (flag, kernel())
            res.extend(t.clone() for t in run())
        _with_wide(flag, go)
        out.append(res)
    return out


def _linear_kernel(a, e, N):
    return lambda: _lib.load().swv2_linear_kernel(ctypes.byref(a), ctypes.byref(e), N)


def _wgrad_kernel(dy, x):
    """for ops.linear_wgrad(dy, x, ...) with its workspace (sized by swv2_linear_wgrad_ws_bytes: covers the wide plan for any slice count)"""
    lib = _lib.load()
    return lambda: lib.swv2_linear_wgrad_kernel(ctypes.byref(dy), ctypes.byref(x), 64, lib.swv2_linear_wgrad_ws_bytes(dy.rows, dy.cols, x.cols, 64))


_WGRAD = ((_lib.WGRAD_TILE,), (_lib.WGRAD_WIDE,))


def test_qkv_epilogue_normalisation_and_head_major_loaders_at_dp_256(dev, K):
    """The GEMM side of the 256-column head layout at C = 2048, 8 heads, against torch fp32: the qkv epilogue with head split
    (un-normalised bf16 values + squared norms in rnorm, four addends per row), swv2_qk_normalize, the head split of d(oh), the
    head-major operand in the proj forward and the d(qkv) -> dx product, and the two weight gradients that read it.  48 windows: 8 448
    rows, from which the wide kernels take the NT products (M >= 4 096) and the weight gradients (M >= 8 192, a multiple of 32) --
    every product asserts that the library's kernel query says so under SWV2_GEMM_WIDE=1, and the tile kernels under =0."""
    ops, L = K["ops"], K["L"]
    torch.manual_seed(31)
    h, DP, Lp, Lv, Bw, Cc = 8, 256, 176, 162, 48, 2048
    Mw = Bw * Lp
    valid = (torch.arange(Lp) < Lv).view(1, 1, 1, Lp, 1)
    xw = torch.randn(Mw, Cc)
    ri = torch.arange(Mw, dtype=torch.int32)
    ri[(torch.arange(Mw) % Lp) >= Lv] = -1                        # padded rows of a window: zero rows of the gather
    wq, bq = torch.randn(3 * h * DP, Cc) * 0.03, torch.randn(3 * h * DP)
    wqb = ops.prep_weight(wq.to(dev))
    qkvh = torch.empty(Bw, h, 3, Lp, DP, dtype=BF, device=dev)
    rn = torch.zeros(Bw, h, 2, Lp, device=dev)

    a_qkv = ops.op_f32(xw.to(dev), rowidx=ri.to(dev))
    e_qkv = ops.epilogue(L.EPI_QKV_HEADS, qkvh, bias=bq.to(dev), aux_out=rn, p=(h, 0, Lp, DP, Lv))

    def run_qkv():
        qkvh.fill_(float("nan"))
        rn.zero_()
        ops.linear(a_qkv, wqb, e_qkv, 3 * h * DP)
        return [qkvh, rn]
    (q0, r0), (q1, r1) = _both(run_qkv, _linear_kernel(a_qkv, e_qkv, 3 * h * DP))
    assert torch.equal(q0, q1) and rel(r0, r1) < 1e-6          # four float addends per norm: equal up to their order
    full = torch.where(valid, (rb(xw) @ rb(wq).T + bq).view(Bw, Lp, 3, h, DP).permute(0, 3, 2, 1, 4), torch.zeros(()))
    got = q1.float().cpu()
    assert not torch.isnan(got).any()
    assert chunk_rel(got, full) < 4e-3 and float(got[:, :, :, Lv:].abs().max()) == 0
    ss = (full[:, :, :2] ** 2).sum(-1)
    assert rel(r1, ss) < 1e-4 and float(r1[..., Lv:].abs().max()) == 0
    # swv2_qk_normalize: 1 / |.| into rnorm, q and k rows rescaled in place (v untouched)
    qkvh.copy_(q1)
    rn.copy_(r1)
    L.check(L.load().swv2_qk_normalize(qkvh.data_ptr(), rn.data_ptr(), Bw, h, Lp, Lv, DP, ops._stream()), "swv2_qk_normalize")
    torch.cuda.synchronize()
    nrm = full[:, :, :2].norm(dim=-1).clamp_min(1e-12)
    exp = full.clone()
    exp[:, :, :2] = full[:, :, :2] / nrm.unsqueeze(-1)
    got = qkvh.float().cpu()
    assert chunk_rel(got[:, :, :2], exp[:, :, :2]) < 4e-3 and torch.equal(qkvh[:, :, 2].cpu(), q1[:, :, 2].cpu())
    assert float(got[:, :, :, Lv:].abs().max()) == 0
    assert rel(rn.cpu(), torch.where(valid.view(1, 1, 1, Lp), 1.0 / nrm, torch.zeros(()))) < 1e-4
    # d(oh) = da1 Wp^T split into heads
    da1 = torch.randn(Mw, Cc).to(BF).to(dev)
    wp = torch.randn(h * DP, Cc) * 0.03
    doh = torch.empty(Bw, h, 1, Lp, DP, dtype=BF, device=dev)

    a_sp, e_sp = ops.op_bf16(da1), ops.epilogue(L.EPI_HEADS, doh, p=(h, 0, Lp, DP, Lv))

    def run_split():
        doh.fill_(float("nan"))
        ops.linear(a_sp, ops.prep_weight(wp.to(dev)), e_sp, h * DP)
        return [doh]
    (g0,), (g1,) = _both(run_split, _linear_kernel(a_sp, e_sp, h * DP))
    fullp = torch.where(valid, (da1.float().cpu() @ rb(wp).T).view(Bw, Lp, 1, h, DP).permute(0, 3, 2, 1, 4), torch.zeros(()))
    for g_ in (g0, g1):
        assert not torch.isnan(g_.float()).any() and chunk_rel(g_.float(), fullp) < 4e-3
    # head-major operand: proj forward (1 part, N = C) and d(qkv) -> dx (3 parts, N = C)
    for parts in (1, 3):
        src = torch.randn(Bw, h, parts, Lp, DP).to(BF).to(dev)
        wo = torch.randn(Cc, parts * h * DP) * 0.03
        wob = ops.prep_weight(wo.to(dev))
        rows = src.float().cpu().permute(0, 3, 2, 1, 4).reshape(Mw, parts * h * DP)
        ref = rows @ rb(wo).T
        o32 = torch.empty(Mw, Cc, device=dev)
        ob = torch.empty(Mw, Cc, dtype=BF, device=dev)
        a_h, e32, eb = ops.op_heads(src, Bw, h, parts, Lp, DP), ops.epilogue(L.EPI_F32, o32, ld=Cc), ops.epilogue(L.EPI_BF16, ob, ld=Cc)
        for g_ in _both(lambda: (ops.linear(a_h, wob, e32, Cc), [o32])[1], _linear_kernel(a_h, e32, Cc)):
            assert chunk_rel(g_[0], ref) < 1e-5
        for g_ in _both(lambda: (ops.linear(a_h, wob, eb, Cc), [ob])[1], _linear_kernel(a_h, eb, Cc)):
            assert chunk_rel(g_[0].float(), ref) < 4e-3
    # weight gradients: qkv (head-major dY x gathered fp32 rows) and proj (bf16 dY x head-major X)
    dq = torch.zeros(Bw, h, 3, Lp, DP)
    dq[:, :, :, :Lv] = torch.randn(Bw, h, 3, Lv, DP) * 0.5
    dqb = dq.to(BF).to(dev)
    xs = torch.randn(Bw * Lv, Cc)
    rg = torch.full((Mw,), -1, dtype=torch.int32)
    tok = torch.randperm(Bw * Lv).to(torch.int32)
    rg.view(Bw, Lp)[:, :Lv] = tok.view(Bw, Lv)

    dy_q, x_q = ops.op_heads(dqb, Bw, h, 3, Lp, DP), ops.op_f32(xs.to(dev), rows=Mw, rowidx=rg.to(dev))

    def run_wq():
        dW, db = torch.zeros(3 * h * DP, Cc, device=dev), torch.zeros(3 * h * DP, device=dev)
        ops.linear_wgrad(dy_q, x_q, dW, db)
        return [dW, db]
    rows = dqb.float().cpu().permute(0, 3, 2, 1, 4)[:, :Lv].reshape(Bw * Lv, 3 * h * DP)
    xg = rb(xs)[tok.long()]
    for dW, db in _both(run_wq, _wgrad_kernel(dy_q, x_q), _WGRAD):
        assert chunk_rel(dW, rows.T @ xg, dim=0) < 1e-5 and chunk_rel(db, rows.sum(0), dim=0) < 1e-5
    oh = torch.zeros(Bw, h, 1, Lp, DP)
    oh[:, :, :, :Lv] = torch.randn(Bw, h, 1, Lv, DP)
    ohb = oh.to(BF).to(dev)
    da = torch.zeros(Bw, Lp, Cc)
    da[:, :Lv] = torch.randn(Bw, Lv, Cc) * 0.5
    dab = da.reshape(Mw, Cc).to(BF).to(dev)

    dy_p, x_p = ops.op_bf16(dab), ops.op_heads(ohb, Bw, h, 1, Lp, DP)

    def run_wp():
        dW, db = torch.zeros(Cc, h * DP, device=dev), torch.zeros(Cc, device=dev)
        ops.linear_wgrad(dy_p, x_p, dW, db)
        return [dW, db]
    xo = ohb.float().cpu()[:, :, 0].permute(0, 2, 1, 3).reshape(Mw, h * DP)
    for dW, db in _both(run_wp, _wgrad_kernel(dy_p, x_p), _WGRAD):
        assert chunk_rel(dW, dab.float().cpu().T @ xo) < 1e-5 and rel(db, dab.float().cpu().sum(0)) < 1e-5


@pytest.mark.parametrize("Cc", [1544, 2048])
def test_layernorm_residual_up_to_2048(dev, K, Cc):
    """ln_residual forward / backward at C = 2048 (four 16-byte pieces per lane) and at 1544 (the fourth piece only on some lanes)
    against fp64 autograd, bars of test_layernorm_residual, d gamma / d beta also per 64-column piece"""
    ops = K["ops"]
    torch.manual_seed(4)
    M, B = 777, 3
    a, res, g, bt = torch.randn(M, Cc) * 2 + 0.5, torch.randn(M, Cc), torch.randn(Cc), torch.randn(Cc)
    scale = torch.tensor([0.0, 1.25, 1.25])
    y = torch.full((M, Cc), float("nan"), device=dev)
    mean, rstd = torch.empty(M, device=dev), torch.empty(M, device=dev)
    ab = a.to(BF).to(dev)
    ops.ln_residual_fwd(ab, res.to(dev), g.to(dev), bt.to(dev), scale.to(dev), None, y, mean, rstd, M, Cc, 0, M // B)
    ad, gd, bd = rb(a).double().requires_grad_(True), g.double().requires_grad_(True), bt.double().requires_grad_(True)
    sc = scale[(torch.arange(M) // (M // B)).clamp(max=B - 1)].double().view(-1, 1)
    ref = res.double() + sc * O.layer_norm(ad, gd, bd)
    dy = torch.randn(M, Cc)
    ref.backward(dy.double())
    da = torch.full((M, Cc), float("nan"), dtype=BF, device=dev)
    dg, db = torch.zeros(Cc, device=dev), torch.zeros(Cc, device=dev)
    ops.ln_residual_bwd(ab, dy.to(dev), g.to(dev), scale.to(dev), None, mean, rstd, da, dg, db, M, Cc, M // B)
    assert chunk_rel(y, ref) < 1e-6 and chunk_rel(da.float(), ad.grad) < 4e-3
    assert chunk_rel(dg, gd.grad) < 1e-5 and chunk_rel(db, bd.grad) < 1e-5


def _block_2048(K, sh, sw, drop_path):
    N = K["N"]
    torch.manual_seed(3)
    blk = N.SwinTransformerV2CrBlock(dim=2048, num_heads=8, feat_size=(18, 36), window_size=(9, 18), shift_size=(sh, sw),
                                     mlp_ratio=2.0, rel_pos=False, drop_path=drop_path)
    with torch.no_grad():
        blk.norm1.weight.uniform_(0.5, 1.0)
        blk.norm2.weight.uniform_(0.5, 1.0)
    return blk


@pytest.mark.parametrize("sh,sw,train", [(0, 0, False), (4, 9, False), (0, 0, True), (4, 9, True)],
                         ids=["unshifted_eval", "shifted_eval", "unshifted_train", "shifted_train"])
def test_block_at_embed_2048_against_oracle(dev, K, sh, sw, train):
    """One block at C = 2048, 8 heads of 256, hidden 4096 on an 18 x 36 grid with 9 x 18 windows: the unfused launch sequence (qkv
    epilogue + normalisation, attn_d256.hip, proj, LayerNorm at C = 2048, MLP as three launches, four single weight gradients: asserted
    on the runner's launch plan).  Train mode draws the
    DropPath scales (drop_path 0.3) and replays them through the oracle.  Forward and backward against the oracle in the kernels'
    rounding mode, bars of test_block_wide_heads_against_oracle."""
    gh, gw, wh, ww, Cc, h, B = 18, 36, 9, 18, 2048, 8, 2
    dp = 0.3 if train else 0.0
    blk = _block_2048(K, sh, sw, dp)
    sd = {k: v.detach().clone() for k, v in blk.state_dict().items()}
    x0 = torch.randn(B, gh, gw, Cc, generator=torch.Generator().manual_seed(1))
    gy0 = torch.randn(B, gh, gw, Cc, generator=torch.Generator().manual_seed(2))
    blk = blk.to(dev).train(train)
    x = x0.to(dev).requires_grad_(True)
    torch.manual_seed(1234)
    y = blk(x)
    y.backward(gy0.to(dev))
    run = blk._runner(B, x.device)
    assert run.plan.DP == 256
    lp = run.launch_plan
    assert (lp.mlp_fused, lp.proj_ln_fused, lp.ln_deferred, lp.wgrad_grouped, lp.wgrad_kernel, lp.grad_zero_in_kernel) == (0, 0, 0, 0, -1, 0)
    assert lp.steps("fwd") == ["rnorm_zero", "qkv", "qk_normalize", "attn_fwd", "proj", "ln1_fwd", "fc1", "fc2", "ln2_fwd"]
    assert lp.steps("bwd") == ["ln2_bwd", "wgrad_fc2", "dh", "wgrad_fc1", "dx1", "ln1_bwd", "wgrad_proj", "doh", "attn_bwd", "wgrad_qkv", "dx"]
    i = run.ACTS.index("hact")
    assert run.act_off[i + 1] - run.act_off[i] >= lp.need_hact_bytes == B * gh * gw * 4096 * 2
    dpo = None
    if train:
        torch.manual_seed(1234)                                  # replay the draws in the block's order
        s1, s2 = blk.drop_path1.scale(x).cpu(), blk.drop_path2.scale(x).cpu()
        assert all(v == 0.0 or abs(v - 1.0 / (1.0 - dp)) < 1e-6 for v in s1.tolist() + s2.tolist())
        dpo = (s1, s2)
    p = {"b." + k: v.clone().requires_grad_(v.dtype.is_floating_point) for k, v in sd.items()}
    xo = x0.clone().requires_grad_(True)
    cfg = block_cfg(gh, gw, wh, ww, sh, sw, Cc, h, False)
    emulate_kernels(K, wh * ww, Cc // h, False, "row_max")
    try:
        yo = O.block_forward(xo, p, "b.", cfg, 1, training=train, dp_override=dpo)
        yo.backward(gy0)
    finally:
        O.set_rounding(None)
    assert rel(y, yo) < 6e-3 and rel(x.grad, xo.grad) < 2e-2, (rel(y, yo), rel(x.grad, xo.grad))
    assert worst_grad(blk, {k[2:]: v.grad for k, v in p.items() if v.requires_grad}, logit_tol=BLOCK_LOGIT_TOL) < 4e-2


def test_model_at_embed_2048_with_the_yaml_settings(dev, K, tmp_path):
    """The yaml entry's settings -- embed 2048 / 8 heads / MLP ratio 2, residual skip, the invariant channels (orography + land mask)
    appended to the input, the channel-weighted loss 'weighted absolute temp-std squared geometric l2' with 'auto' weights, fused
    into the head epilogue as the Trainer runs it -- at depth 2 (one plain, one shifted block) on a 72 x 144 image: model output, loss
    value, input and parameter gradients through the loss against the oracle in the kernels' rounding mode."""
    from types import SimpleNamespace
    from swin_v2_weather_amd.utils.YParams import YParams
    from swin_v2_weather_amd.utils.losses import LossHandler
    yp = YParams(os.path.join(os.path.dirname(K["L"].__file__), "config", "swin.yaml"), "swin_73var_geo_depth24_e2048_mlp2_chweight_invar")
    assert yp.loss == "weighted absolute temp-std squared geometric l2" and yp.channel_weights == "auto" and yp.residual
    assert yp.add_orography and yp.add_landmask and yp.embed_dim == 2048 and yp.mlp_ratio == 2
    H, W, cout, depth = 72, 144, 12, 2
    n_invar = 1 * yp.add_orography + 2 * yp.add_landmask
    cin = cout + n_invar
    names = list(yp.channel_names)[:cout]
    pr = SimpleNamespace(nettype="swin", img_size=[H, W], patch_size=4, depth=depth, num_heads=yp.num_heads, n_in_channels=cin,
                         n_out_channels=cout, embed_dim=yp.embed_dim, window_ratio=8, drop_path_rate=0.0, full_pos_embed=True,
                         rel_pos=yp.rel_pos, mlp_ratio=yp.mlp_ratio, activation_ckpt=False, residual=yp.residual, n_future=0,
                         add_orography=yp.add_orography, add_landmask=yp.add_landmask)
    torch.manual_seed(5)
    model = K["helpers"].get_model(pr)
    with torch.no_grad():
        for n_, p_ in model.named_parameters():
            if n_.endswith("norm1.weight") or n_.endswith("norm2.weight"):
                p_.uniform_(0.5, 1.0)
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    g = torch.Generator().manual_seed(6)
    x0, t0 = torch.randn(1, cin, H, W, generator=g), torch.randn(1, cout, H, W, generator=g)
    gs = (0.5 + torch.rand(1, cout, 1, 1, generator=g)).numpy()
    td = (0.05 + 0.45 * torch.rand(1, cout, 1, 1, generator=g)).numpy()
    np.save(tmp_path / "gs.npy", gs)
    np.save(tmp_path / "td.npy", td)
    lh = LossHandler(SimpleNamespace(n_future=0, img_shape_x=H, img_shape_y=W, loss=yp.loss, channel_weights=yp.channel_weights,
                                     n_out_channels=cout, channel_names=names, out_channels=np.arange(cout),
                                     global_stds_path=str(tmp_path / "gs.npy"), time_diff_stds_path=str(tmp_path / "td.npy"), dt=1,
                                     model_grid_type="equiangular")).to(dev)
    model = model.to(dev).train()
    x, t = x0.to(dev).requires_grad_(True), t0.to(dev)
    with lh.fused_with(model, t):
        y = model(x)
    loss = lh(y, t, x)
    loss.backward()
    cfg = O.SwinCfg.from_params(pr)
    pk = [k for k in sd if k.endswith("pos_embed")][0]
    prefix = pk[:-len("pos_embed")]
    p = {k[len(prefix):]: v.clone().requires_grad_(v.dtype.is_floating_point) for k, v in sd.items()}
    xo = x0.clone().requires_grad_(True)
    chw = O.loss_channel_weights(yp.loss, cout, 0, names, "auto", torch.from_numpy(gs), torch.from_numpy(td), 1)
    emulate_kernels(K, 162, yp.embed_dim // yp.num_heads, False, "row_max")
    try:
        yo = O.model_forward(xo, p, cfg, training=True)
        lo = O.geometric_l2_loss(yo, t0, chw, yp.loss)
        lo.backward()
    finally:
        O.set_rounding(None)
    assert rel(y, yo) < 6e-3, rel(y, yo)
    assert abs(float(loss.detach()) - float(lo.detach())) < 1e-2 * abs(float(lo.detach())), (float(loss.detach()), float(lo.detach()))
    assert rel(x.grad, xo.grad) < 2e-2, rel(x.grad, xo.grad)
    ref = {prefix + k: v.grad for k, v in p.items() if v.requires_grad}
    assert worst_grad(model, ref, logit_tol=BLOCK_LOGIT_TOL) < 6e-2


def test_yaml_entry_trains_at_full_resolution(dev, K, tmp_path):
    """the yaml entry at 720 x 1440 with depth overridden to 2, local batch 1, three Trainer.train_step calls on synthetic data:
    finite losses; finite, non-zero gradients (the parameters move and stay finite)"""
    import os
    from types import SimpleNamespace
    from swin_v2_weather_amd.train import Trainer
    from swin_v2_weather_amd.utils.YParams import YParams
    cfg = "swin_73var_geo_depth24_e2048_mlp2_chweight_invar"
    p = YParams(os.path.join(os.path.dirname(K["L"].__file__), "config", "swin.yaml"), cfg)
    assert p.embed_dim == 2048 and list(p.img_size) == [720, 1440]
    p["depth"], p["batch_size"], p["max_epochs"] = 2, 1, 1
    p["synthetic_device_pool"], p["synthetic_steps_per_epoch"] = 2, 3
    p["exp_dir"], p["save_checkpoint"], p["log_to_screen"], p["log_to_wandb"] = str(tmp_path), False, False, False
    tr = Trainer(p, SimpleNamespace(sweep_id=None, config=cfg, run_num="00", enable_amp=True))
    tr.build()
    with torch.no_grad():                                        # LayerNorm weights away from the reference's init value 0
        for n_, q in tr.model.named_parameters():
            if n_.endswith("norm1.weight") or n_.endswith("norm2.weight"):
                q.uniform_(0.5, 1.0)
    named = [(n_, q) for n_, q in tr.model.named_parameters() if q.requires_grad]
    before = {n_: q.detach().clone() for n_, q in named}
    it = iter(tr.train_data_loader)
    losses, gmax = [], {n_: 0.0 for n_, _ in named}
    for _ in range(3):
        losses.append(float(tr.train_step(next(it))))
        for n_, q in named:                                      # the step's gradients (train_step sets them to None first)
            assert q.grad is not None and bool(torch.isfinite(q.grad).all()), n_
            gmax[n_] = max(gmax[n_], float(q.grad.abs().max()))
    torch.cuda.synchronize()
    assert all(np.isfinite(losses)), losses
    # every parameter has a non-zero gradient in at least one of the three steps (the yaml's drop_path_rate 0.1 may drop a
    # whole branch of the single sample in one step, and then that branch's gradients are exactly zero in that step), and moved
    assert [n_ for n_, v in gmax.items() if not v > 0] == []
    for n_, q in named:
        assert bool(torch.isfinite(q).all()) and not torch.equal(q.detach(), before[n_]), n_
