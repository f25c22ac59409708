"""CPU: utils/optim.HipLamb's torch path against the fp64 statement of LAMB (tests/lamb_reference.py), its apex-shaped surface, and the
host half of the swv2_lamb_* entry points (struct mirror, workspace arithmetic, refusals) -- no GPU call."""
import ctypes
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from swin_v2_weather_amd import _lib as L
from tests import lamb_reference as R
from tests.test_host_and_cabi import header_struct_fields

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MODES = {"default": {}, "l2": dict(adam_w_mode=False), "no_bias_correction": dict(bias_correction=False),
         "no_grad_averaging": dict(grad_averaging=False), "no_decay": dict(weight_decay=0.0),
         "nvlamb_no_decay": dict(weight_decay=0.0, use_nvlamb=True), "unclipped": dict(max_grad_norm=1e4), "scaled": dict(inv=1.0 / 128)}
SIZES = [1, 5, 4097, 12293]


def _inputs(seed, gscale):
    rng = np.random.default_rng(seed)
    ps = [(0.02 * rng.standard_normal(n)).astype(np.float32) for n in SIZES]
    ps[1][:] = 0.0                                                    # |p| = 0: the ratio is 1 on the first step
    gs = [[(gscale * np.exp(rng.uniform(-6, 0, n)) * rng.choice([-1.0, 1.0], n)).astype(np.float32) for n in SIZES] for _ in range(5)]
    return ps, gs


@pytest.mark.parametrize("mode", sorted(MODES))
def test_torch_path_follows_the_fp64_reference_for_five_steps(mode):
    """HipLamb on CPU parameters (its torch path: fp64 arithmetic rounded once) against the reference stepped in fp64 from the SAME fp32
    state each step: m, v and p within the kernel's bounds (it sits far inside: one rounding each)."""
    from swin_v2_weather_amd.utils.optim import HipLamb
    kw = dict(MODES[mode])
    inv = kw.pop("inv", 1.0)
    ps, gs = _inputs(3, 10.0 / inv)
    params = [torch.nn.Parameter(torch.from_numpy(p.copy())) for p in ps]
    opt = HipLamb(params, lr=2e-3, **kw)
    hk = dict(lr=2e-3, grad_inv_scale=inv, max_grad_norm=kw.get("max_grad_norm", 1.0), weight_decay=kw.get("weight_decay", 0.01),
              adam_w_mode=kw.get("adam_w_mode", True), bias_correction=kw.get("bias_correction", True),
              grad_averaging=kw.get("grad_averaging", True), use_nvlamb=kw.get("use_nvlamb", False))
    for it in range(5):
        h = R.Hyper(step=it + 1, **hk)
        old = [p.detach().numpy().copy() for p in params]
        ms = [opt.state[p]["exp_avg"].numpy().copy() if opt.state[p] else np.zeros_like(o) for p, o in zip(params, old)]
        vs = [opt.state[p]["exp_avg_sq"].numpy().copy() if opt.state[p] else np.zeros_like(o) for p, o in zip(params, old)]
        for p, g in zip(params, gs[it]):
            p.grad = torch.from_numpy(g.copy())
        opt.step(grad_inv_scale=inv)
        assert opt.param_groups[0]["step"] == it + 1 and opt.kernel_norms() is None
        g2 = R.grad_norm2(gs[it], inv)
        c = R.clip_divisor(g2, h.max_grad_norm)
        assert (c > 1.0) == (mode != "unclipped")
        for i, p in enumerate(params):
            assert torch.equal(p.grad, torch.from_numpy(gs[it][i]))                          # gradients are read only
            m_ref, v_ref, bm, bv, _ = R.moments(old[i], gs[it][i], ms[i], vs[i], h, c)
            m1, v1 = opt.state[p]["exp_avg"].numpy(), opt.state[p]["exp_avg_sq"].numpy()
            assert np.all(np.abs(m1 - m_ref) <= bm) and np.all(np.abs(v1 - v_ref) <= bv), (mode, it, i)
            a, u = R.update(old[i], m1, v1, h)
            r = R.trust_ratio(np.sum(R.d(old[i]) ** 2), np.sum(u ** 2), h)
            if mode == "no_decay" or (i == 1 and it == 0):
                assert r == 1.0
            p_ref, bp = R.apply(old[i], a, u, r, h)
            assert np.all(np.abs(p.detach().numpy() - p_ref) <= bp), (mode, it, i)
            assert not np.array_equal(p.detach().numpy(), old[i])


def test_surface_state_layout_and_state_dict_round_trip():
    from swin_v2_weather_amd.utils.optim import HipLamb
    with pytest.raises(RuntimeError):
        HipLamb([torch.nn.Parameter(torch.zeros(3))], amsgrad=True)
    o = HipLamb([torch.nn.Parameter(torch.zeros(3))])
    assert o.defaults == dict(lr=1e-3, bias_correction=True, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.01, grad_averaging=True,
                              max_grad_norm=1.0)
    assert (o.adam_w_mode, o.set_grad_none, o.use_nvlamb) == (1, True, False) and isinstance(o, torch.optim.Optimizer)

    def make():
        torch.manual_seed(0)
        a, b, c = (torch.nn.Parameter(torch.randn(s)) for s in ((7, 3), (4100,), (2,)))
        return [a, b, c], HipLamb([{"params": [a, c]}, {"params": [b], "weight_decay": 0.0}], lr=1e-2, max_grad_norm=5.0)
    pa, oa = make()
    pb, ob = make()
    g = torch.Generator().manual_seed(1)
    grads = [[torch.randn(p.shape, generator=g) for p in pa[:2]] for _ in range(4)]          # the third parameter never gets a gradient
    for it in range(4):
        for ps, o in ((pa, oa), (pb, ob)):
            for p, gr in zip(ps, grads[it]):
                p.grad = gr.clone()
            v0 = [p._version for p in ps[:2]]
            o.step()
            assert all(p._version > v for p, v in zip(ps[:2], v0))
        if it == 1:                                   # checkpoint after step 2 into a FRESH optimizer over the same parameters
            assert set(oa.state[pa[0]]) == {"exp_avg", "exp_avg_sq"} and pa[2] not in oa.state
            assert [g_["step"] for g_ in oa.param_groups] == [2, 2]
            sd = oa.state_dict()
            assert set(sd["state"]) == {0, 2} and set(sd["state"][0]) == {"exp_avg", "exp_avg_sq"}
            fresh = HipLamb([{"params": [pa[0], pa[2]]}, {"params": [pa[1]], "weight_decay": 0.0}], lr=1e-2, max_grad_norm=5.0)
            fresh.load_state_dict(sd)
            oa = fresh
    assert [g_["step"] for g_ in oa.param_groups] == [4, 4]
    for a, b in zip(pa, pb):
        assert torch.equal(a, b)                      # the restored optimizer continued bit for bit
    oa.zero_grad()
    assert all(p.grad is None for p in pa)


def test_a_copied_optimizer_steps_like_the_original_and_given_ratios_replace_the_norms():
    import copy
    from swin_v2_weather_amd.utils.optim import HipLamb
    torch.manual_seed(0)
    a = torch.nn.Parameter(torch.randn(300))
    o = HipLamb([a], lr=1e-2, adam_w_mode=False, use_nvlamb=True)
    a.grad = torch.randn(300)
    o.step()
    o2 = copy.deepcopy(o)                             # (copies the parameter too; launch tables are not part of an optimizer's state)
    b = o2.param_groups[0]["params"][0]
    assert (o2.adam_w_mode, o2.use_nvlamb, o2._table, o2.param_groups[0]["step"]) == (0, True, None, 1) and b is not a
    b.grad = a.grad.clone()
    o.step()
    o2.step()
    assert torch.equal(a, b) and torch.equal(o.state[a]["exp_avg_sq"], o2.state[b]["exp_avg_sq"])
    # ratios given from outside: r = 0 leaves p where it is, the moments still move
    before, m0 = a.detach().clone(), o.state[a]["exp_avg"].clone()
    with torch.no_grad():
        o._torch_group(o.param_groups[0], [a], torch.tensor(1.0, dtype=torch.float64), 1.0, ratios={a: 0.0})
    assert torch.equal(a, before) and not torch.equal(o.state[a]["exp_avg"], m0)


def test_other_dtypes_and_sparse_gradients_take_the_torch_path_too():
    from swin_v2_weather_amd.utils.optim import HipLamb
    torch.manual_seed(0)
    emb = torch.nn.Embedding(10, 4, sparse=True)
    half = torch.nn.Parameter(torch.randn(9).to(torch.bfloat16))
    o = HipLamb(list(emb.parameters()) + [half], lr=1e-2)
    emb(torch.tensor([1, 3])).sum().backward()
    half.grad = torch.ones(9, dtype=torch.bfloat16)
    w0, h0 = emb.weight.detach().clone(), half.detach().clone()
    o.step()
    assert emb.weight.grad.is_sparse and not torch.equal(emb.weight, w0) and not torch.equal(half, h0)
    assert torch.isfinite(emb.weight).all() and o.state[half]["exp_avg"].dtype == torch.bfloat16


def test_ctypes_item_follows_the_header_and_workspace_arithmetic():
    from swin_v2_weather_amd._lib import LambItem as _LambItem
    assert [f[0] for f in _LambItem._fields_] == header_struct_fields("swv2_lamb_item") == ["p", "g", "m", "v", "n", "chunk0"]
    assert ctypes.sizeof(_LambItem) == 48
    lib = L.load()
    assert lib.swv2_lamb_chunk() == 4096
    for ni, nc in ((1, 1), (7, 81), (160, 2700)):
        assert lib.swv2_lamb_ws_bytes(ni, nc) == 4 * (L.lamb_ws_item(ni) + 6 * nc)
    assert lib.swv2_lamb_ws_bytes(0, 5) == 0 and lib.swv2_lamb_ws_bytes(5, 0) == 0 and lib.swv2_lamb_ws_bytes(-1, -1) == 0
    hdr = open(os.path.join(ROOT, "include", "swv2.h")).read()
    assert "#define SWV2_LAMB_SUM_DEPTH %d\n" % L.LAMB_SUM_DEPTH in hdr and L.LAMB_SUM_DEPTH == R.D
    for name, val in (("ADAMW", L.LAMB_ADAMW), ("BIAS_CORRECTION", L.LAMB_BIAS_CORRECTION), ("GRAD_AVERAGING", L.LAMB_GRAD_AVERAGING),
                      ("NVLAMB", L.LAMB_NVLAMB), ("WS_GNORM2", L.LAMB_WS_GNORM2), ("WS_CLIP", L.LAMB_WS_CLIP), ("WS_BC1", L.LAMB_WS_BC1),
                      ("WS_BC2", L.LAMB_WS_BC2)):
        assert "#define SWV2_LAMB_%s %d\n" % (name, val) in hdr
    assert "#define SWV2_LAMB_WS_ITEM(i) (4 + 4 * (i))" in hdr and L.lamb_ws_item(3) == 16


def test_every_refusal_returns_invalid_with_a_message_and_without_a_gpu():
    """Arguments are checked before anything is launched, so the pointers only have to be non-null here: a refused call touches nothing."""
    lib = L.load()
    P = 4096                                         # any non-null, 4-byte aligned value: never dereferenced by a refused call
    ws_ok = lib.swv2_lamb_ws_bytes(2, 3)

    def norm(items=P, chunks=P, ni=2, nc=3, ws=P, wb=ws_ok):
        return lib.swv2_lamb_grad_norm(items, chunks, ni, nc, 1.0, ws, wb, None)

    def multi(items=P, chunks=P, ni=2, nc=3, i0=0, i1=2, c0=0, c1=3, step=1, flags=3, ws=P, wb=ws_ok):
        return lib.swv2_lamb_multi(items, chunks, ni, nc, i0, i1, c0, c1, 1e-3, 0.9, 0.999, 1e-6, 0.01, 1.0, 1.0, step, flags, None, ws, wb, None)
    for call, word in ((lambda: norm(items=None), b"null"), (lambda: norm(chunks=None), b"null"), (lambda: norm(nc=0), b"n_chunks"),
                       (lambda: norm(ni=0), b"n_items"), (lambda: norm(ws=None), b"workspace"), (lambda: norm(wb=ws_ok - 1), b"workspace"),
                       (lambda: multi(items=None), b"null"), (lambda: multi(chunks=None), b"null"), (lambda: multi(nc=0), b"n_chunks"),
                       (lambda: multi(nc=-4), b"n_chunks"), (lambda: multi(step=0), b"step"), (lambda: multi(step=-1), b"step"),
                       (lambda: multi(ws=None), b"workspace"), (lambda: multi(wb=ws_ok - 4), b"workspace"), (lambda: multi(wb=0), b"workspace"),
                       (lambda: multi(i1=3), b"items"), (lambda: multi(i0=2), b"items"), (lambda: multi(c0=-1), b"chunks"),
                       (lambda: multi(c1=4), b"chunks"), (lambda: multi(flags=16), b"flag")):
        assert call() == -1
        assert word in lib.swv2_last_error(), lib.swv2_last_error()
    with pytest.raises(L.Swv2Error):
        L.check(multi(step=0), "swv2_lamb_multi")


def test_cpu_trainer_with_fusedlamb_builds_hiplamb(tmp_path):
    from swin_v2_weather_amd.train import Trainer
    from swin_v2_weather_amd.utils.YParams import YParams
    from swin_v2_weather_amd.utils.optim import HipLamb
    from tests.test_ddp_gloo import _OracleLoss, _oracle_model, _params
    p = _params(str(tmp_path))
    p["optimizer_type"] = "FusedLAMB"
    assert YParams(os.path.join(ROOT, "swin_v2_weather_amd", "config", "swin.yaml"), "bench_tiny").optimizer_type == "adam"       # the yaml default stays
    tr = Trainer(p, SimpleNamespace(sweep_id=None, config="bench_tiny", run_num="00", enable_amp=False), model_factory=_oracle_model,
                 loss_factory=_OracleLoss, device="cpu")
    tr.build()
    assert isinstance(tr.optimizer, HipLamb) and tr.optimizer.defaults["max_grad_norm"] == 5.0
    assert tr.optimizer.defaults["lr"] == p.lr and len(tr.optimizer.param_groups) == 1
    g = torch.Generator().manual_seed(0)
    tr.model.train()
    before = [q.detach().clone() for q in tr.model.parameters()]
    loss = tr.train_step((torch.randn(2, 4, 24, 36, generator=g), torch.randn(2, 4, 24, 36, generator=g)))
    assert torch.isfinite(loss) and tr.optimizer.param_groups[0]["step"] == 1
    assert any(not torch.equal(a, b) for a, b in zip(before, tr.model.parameters()))


def test_chunk_pairs_lists_every_chunk_once_and_matches_the_two_loops_it_replaced():
    """utils/optim.chunk_pairs (the tables of HipAdam and HipLamb): tensors of 1 element, one short of a chunk, a chunk, one past it and
    three chunks -- every (item, chunk) once and in order, chunk0 = the running sum of the chunk counts."""
    from swin_v2_weather_amd.utils.optim import chunk_pairs
    numels, chunk = [1, 4095, 4096, 4097, 3 * 4096], 4096
    pairs, chunk0 = chunk_pairs(numels, chunk)
    counts = [sum(1 for i, _ in pairs if i == k) for k in range(len(numels))]
    assert counts == [1, 1, 1, 2, 3]
    assert chunk0 == [0, 1, 2, 3, 5]
    assert pairs == [(0, 0), (1, 0), (2, 0), (3, 0), (3, 1), (4, 0), (4, 1), (4, 2)]
    assert pairs == sorted(set(pairs)) and len(pairs) == sum(counts)
    for (i, c), n in ((pc, numels[pc[0]]) for pc in pairs):
        assert 0 <= c * chunk < n                                     # every chunk starts inside its tensor
    # HipAdam._table's loop, as it stood
    adam = []
    for i, n in enumerate(numels):
        adam += [(i, c) for c in range((n + chunk - 1) // chunk)]
    # HipLamb._tables_for's loop, as it stood (one group)
    lamb, lamb0, n_items = [], [], 0
    for n in numels:
        lamb0.append(len(lamb))
        lamb += [(n_items, c) for c in range((n + chunk - 1) // chunk)]
        n_items += 1
    assert pairs == adam == lamb and chunk0 == lamb0
    assert chunk_pairs([], chunk) == ([], [])
