"""GPU (-m gpu): every attention kernel, element by element against fp64.

References, bounds (with their derivations) and the case table are in tests/attn_reference.py; tests/test_attn_exact_host.py checks
them without a GPU.  Every case first asks the library which kernels it will run for exactly these arguments (swv2_attn_fwd_kernel /
swv2_attn_bwd_kernel) and fails if they are not the ones the case is filed under -- the id of a case names both.  Then, for each of
the four input generators (normal / counting / peaked / adversarial mask):
  forward : o and lse against the reference, padding rows / columns exactly 0 (outputs prefilled with NaN);
  backward: fed oh = bf16(o_ref) and lse = fp32(lse_ref) computed on the host, so a backward failure never depends on the forward;
            dq, dk, dv, d logit_scale (on the normal generator also against its statistical bound), d bias against the reference; rows >= L of dqkvh exactly 0 (prefilled with NaN); guard elements
            around d logit_scale and d bias untouched; the three d bias destinations (atomics, workspace + reduce, partial tables);
  chained : on the normal generator the backward also runs from the forward kernel's own oh / lse, against the reference backward of
            those stored tensors.
SWV2_TEST_VERBOSE=1 prints the worst |error| / bound per output of every case (LABNOTES.md records them).
"""
import ctypes
import os

import pytest
import torch

from tests import attn_reference as R

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
GUARD = 12345.0


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def K():
    from swin_v2_weather_amd import _lib as L, ops
    L.load()
    return dict(L=L, ops=ops)


def _guarded(n, dev):
    """n zeros between two guard blocks of 64 floats"""
    buf = torch.full((n + 128,), GUARD, device=dev)
    buf[64:64 + n] = 0
    return buf, buf[64:64 + n]


def _guards_intact(buf, n):
    return bool((buf[:64] == GUARD).all()) and bool((buf[64 + n:] == GUARD).all())


@pytest.mark.parametrize("ci", range(len(R.CASES)), ids=[R.case_id(c) for c in R.CASES])
def test_attention_exact(dev, K, ci):
    c = R.CASES[ci]
    L_, ops = K["L"], K["ops"]
    lib = L_.load()
    B, (nwh, nww) = 2, c.nw
    Bw, Lw, d, h = B * nwh * nww, c.L, c.d, c.h
    thr = R.case_thr(c)
    Lp, DP = ops.attn_geometry(Lw, d)
    bias = R.make_bias(h, Lw) if c.bias else None
    bd = bias.to(dev).contiguous() if c.bias else None
    pk = ops.attn_pack_bias(bd) if c.bias == "packed" else None
    for gen in R.GENERATORS:
        x = R.generate(gen, Bw, h, Lw, d, thr, seed=ci)
        ref = R.forward_reference(x.qn, x.kn, x.v, x.tau, bias, nwh, nww, thr)
        qkvh = R.pad_heads((x.qn, x.kn, x.v), Lp, DP).to(BF).to(dev).contiguous()
        tau = x.tau.to(dev)
        # ---- forward
        oh = torch.full((Bw, h, Lp, DP), float("nan"), dtype=BF, device=dev)
        lse = torch.full((Bw, h, Lp), float("nan"), device=dev)
        a = ops.attn_args(qkvh, tau, bd, oh, lse, Bw, h, Lw, d, nwh, nww, thr, bias_pack=pk, max_chunks=c.mc)
        a.dbg = c.fdbg
        info = L_.AttnKernelInfo()
        assert lib.swv2_attn_fwd_kernel(ctypes.byref(a), ctypes.byref(info)) >= 0
        assert R.kernel_name(info, L_.ATTN_K_NAMES, False) == c.fwd, "the forward kernel the library picks is not the one this case is filed under"
        ops.attn_fwd(a)
        ohc, lsec = oh.float().cpu(), lse.cpu()
        rep = {}
        cS = R.CS_FOLDED if info.regime == 1 else R.CS_ROW_MAX(d)
        try:
            R.check_padding_fwd(ohc, lsec, Lw, d)
            R.check_forward(ohc[:, :, :Lw, :d], lsec[:, :, :Lw], ref, cS, info.regime == 1, rep)
            # ---- backward from the host's oh / lse
            runs = [("bwd", R.bf16(ref.o.float()), ref.lse.float())]
            if gen == "normal":
                runs.append(("chained", ohc[:, :, :Lw, :d], lsec[:, :, :Lw]))
            for tag, o_in, l_in in runs:
                sub = {}
                try:
                    _backward(dev, K, c, x, ref, bias, bd, pk, qkvh, tau, o_in, l_in, (Bw, Lp, DP, nwh, nww, thr), sub, gen == "normal")
                finally:
                    rep.update({f"{k}" if tag == "bwd" else f"{tag}.{k}": v for k, v in sub.items()})
        finally:
            if os.environ.get("SWV2_TEST_VERBOSE"):
                print(f"[attn-exact] {R.case_id(c)} {gen}: " + " ".join(f"{k}={v:.3g}" for k, v in rep.items()), flush=True)


def _backward(dev, K, c, x, ref, bias, bd, pk, qkvh, tau, o_in, l_in, geo, rep, random_data):
    L_, ops = K["L"], K["ops"]
    lib = L_.load()
    Bw, Lp, DP, nwh, nww, thr = geo
    Lw, d, h = c.L, c.d, c.h
    oh = R.pad_heads((o_in,), Lp, DP).squeeze(2).to(BF).to(dev).contiguous()
    lse = R.pad_rows(l_in, Lp).to(dev).contiguous()
    doh = R.pad_heads((x.dO,), Lp, DP).squeeze(2).to(BF).to(dev).contiguous()
    rnorm = torch.stack([R.pad_rows(x.rq, Lp), R.pad_rows(x.rk, Lp)], 2).to(dev).contiguous()
    dqkvh = torch.full((Bw, h, 3, Lp, DP), float("nan"), dtype=BF, device=dev)
    dl_buf, dl = _guarded(h, dev)
    db_buf = db = ws = None
    nchunk = min(Bw, c.mc)
    if c.bias:
        db_buf, db = _guarded(h * Lw * Lw, dev)
        if c.dest in ("ws", "partials"):
            nb = lib.swv2_attn_dbias_ws_bytes(h, Lw, nchunk)
            ws = torch.full((nb // 4 + 64,), float("nan"), device=dev)
            ws[nb // 4:] = GUARD
    a = ops.attn_args(qkvh, tau, bd, oh, lse, Bw, h, Lw, d, nwh, nww, thr, doh=doh, rnorm=rnorm, dqkvh=dqkvh, dlogit=dl,
                      dbias=None if (c.bias and c.dest == "partials") else db, bias_pack=pk, max_chunks=c.mc,
                      dbias_ws=ws[:-64] if ws is not None else None)
    a.dbg = c.bdbg
    if c.bias and c.dest == "partials":
        a.dbias_partials = 1
    info = L_.AttnKernelInfo()
    assert lib.swv2_attn_bwd_kernel(ctypes.byref(a), ctypes.byref(info)) >= 0
    assert R.kernel_name(info, L_.ATTN_K_NAMES, True) == c.bwd, "the backward kernel the library picks is not the one this case is filed under"
    ops.attn_bwd(a)
    g = dqkvh.float().cpu()
    R.check_padding_bwd(g, Lw)
    assert _guards_intact(dl_buf, h), "d logit_scale: guard elements written"
    dbias = None
    if c.bias:
        assert _guards_intact(db_buf, h * Lw * Lw), "d bias: guard elements written"
        if ws is not None:
            assert bool((ws[-64:] == GUARD).all()), "d bias workspace: guard elements written"
            # the workspace was prefilled with NaN: a launcher that fell back to atomics (workspace judged too small) would leave it so
            assert bool(torch.isfinite(ws[:-64]).all()), "d bias workspace: not every workgroup's table was written (atomics fallback?)"
        if c.dest == "partials":
            part = ws[:-64].view(nchunk, h, Lw, Lw)
            assert bool((db == 0).all()), "dbias_partials: d bias must stay untouched"
            dbias = part.double().sum(0).cpu()
        else:
            dbias = db.view(h, Lw, Lw).cpu()
    bw = R.backward_reference(ref, o_in, l_in, x.dO, x.rq, x.rk, bias is not None)
    R.check_backward(g[:, :, 0, :Lw, :d], g[:, :, 1, :Lw, :d], g[:, :, 2, :Lw, :d], dl.cpu(), dbias, ref, bw, R.CS_ROW_MAX(d),
                     R.MASK_EPS_AUG if info.aug else R.MASK_EPS_F32, rep, random_data=random_data)
