"""The operand contract of the score families on the GPU: every wrapper of ops.py that takes blocks of planes in place gives, on each
layout the one rule (ops._planes_in_place) accepts, bit for bit what it gives on a fresh contiguous copy, and refuses each layout the
rule refuses without a launch.  B = 2, C = 3, H = 5, W = 8 (M = 3, K = 2): partial slices, more than one slice per plane, and the
smallest shape at which a wrong batch stride, member stride or channel offset changes the answer -- whatever surrounds a block is NaN.
Last, the collector the two rollouts share: the control of ensemble_rollout is score_rollout's answer on member 0."""
import functools

import pytest
import torch

from tests import regrid_reference as RR
from tests.plane_harness import dev, lib  # noqa: F401  (fixtures)
from tests.test_regrid_gpu import _setup, _tables

pytestmark = pytest.mark.gpu

B, C, H, W, M, K = 2, 3, 5, 8, 3, 2
HD, WD = 4, 6                                    # the regrid target: a width that is no multiple of 4 (C HD WD is one: the batch stride)
GRIDS = ((H, False, None, W), (HD, False, WD))
FAMILIES = ["score_sums", "l1_sums", "event_sums", "ens_sums", "ens_event_sums", "regrid", "plane_order_stats"]
LEAD = {"ens_sums": (M, B), "ens_event_sums": (M, B)}


@functools.lru_cache(maxsize=None)
def _data():
    """the operands of every case, on the CPU; made once, never modified"""
    from swin_v2_weather_amd.utils.weighted_acc_rmse import latitude_weights
    g = torch.Generator().manual_seed(11)
    return dict(prd=torch.randn(B, C, H, W, generator=g), tar=torch.randn(B, C, H, W, generator=g), ens=torch.randn(M, B, C, H, W, generator=g),
                clim=0.3 * torch.randn(C, H, W, generator=g), thr=0.5 * torch.randn(B, C, K, generator=g), w=latitude_weights(H),
                chw=torch.rand(C, generator=g) + 0.5, ranks=torch.tensor([0, 7, H * W - 1], dtype=torch.int32))


def _place(x, layout, dev, width=W):
    """x [..., b, C, h, width] as a device view of that layout; everything around the block is NaN"""
    lead, (b, _, h, _) = tuple(x.shape[:-4]), x.shape[-4:]
    if layout == "contiguous":
        return x.to(dev)
    if layout == "channels":                                   # channels 2:5 of a [.., 7, h, width] tensor
        wide = torch.full(lead + (b, 7, h, width), float("nan"), device=dev)
        wide[..., 2:5, :, :] = x.to(dev)
        return wide[..., 2:5, :, :]
    assert layout == "odd_batch_stride" and b == 1             # sample 1 of two whose batch stride is odd (legal: B == 1 never uses it)
    bs = 7 * h * width + 1
    ms = 2 * bs + 2                                            # the member stride stays a multiple of 4
    buf = torch.full(((lead[0] * ms if lead else 0) + 2 * bs + 8,), float("nan"), device=dev)
    size, stride = lead + (2, 7, h, width), ((ms,) if lead else ()) + (bs, h * width, width, 1)
    off = (-(bs + 2 * h * width)) % 4                          # so that the block itself starts on a 16-byte boundary
    blk = buf.as_strided(size, stride, off)[..., 1:2, 2:5, :, :]
    blk.copy_(x.to(dev))
    assert blk.stride(-4) == bs and bs % 4 != 0 and blk.data_ptr() % 16 == 0
    return blk


def _run(name, x, tar):
    """the wrapper and its finalize on the device views x (prediction [b, C, H, W], or members [M, b, C, H, W]) and tar (truth; the
    destination for regrid) -> the tuple of its results"""
    from swin_v2_weather_amd import ops
    d, dv = _data(), x.device
    b = x.shape[-4]
    w, clim = d["w"].to(dv), d["clim"].to(dv)
    thr = d["thr"][B - b:].to(dv).contiguous()                 # (b == 1: sample 1, as the operands)
    if name == "score_sums":
        ws = ops.score_workspace(b * C, H, W, dv)
        ops.score_sums(x, tar, w, ws, clim)
        return ops.score_finalize(ws, b, C, H, W)
    if name == "l1_sums":
        ws = ops.l1_workspace(b * C, H, W, dv)
        ops.l1_sums(x, tar, w, ws)
        return ops.l1_finalize(ws, b, C, H, W, d["chw"].to(dv))
    if name == "event_sums":
        ws = ops.event_workspace(b * C, H, W, K, dv)
        ops.event_sums(x, tar, thr, w, ws, clim)
        return ops.event_finalize(ws, K, b, C, H, W)
    if name == "ens_sums":
        ws = ops.ens_workspace(b * C, H, W, M, dv)
        ops.ens_sums(x, tar, w, ws)
        return ops.ens_finalize(ws, M, b, C, H, W)
    if name == "ens_event_sums":
        ws = ops.ens_event_workspace(b * C, H, W, M, K, dv)
        ops.ens_event_sums(x, tar, thr, w, ws, clim)
        return ops.ens_event_finalize(ws, M, K, b, C, H, W)
    if name == "regrid":
        ops.regrid(x, tar, *_tables(dv, _setup(*GRIDS)))
        return (tar.clone(),)
    assert name == "plane_order_stats"
    return ops.plane_order_stats(x, d["ranks"].to(dv))


def _operands(name, one):
    """(first operand, second operand) of the wrapper on the CPU; one: sample 1 alone (B = 1)"""
    d = _data()
    x = d["ens"] if name in LEAD else d["prd"]
    y = torch.zeros(B, C, HD, WD) if name == "regrid" else d["tar"]
    return (x[..., 1:, :, :, :], y[1:]) if one else (x, y)


@functools.lru_cache(maxsize=None)
def _reference(name, one, dev):
    """the wrapper on fresh contiguous copies; computed once per (wrapper, B), never modified"""
    x, y = _operands(name, one)
    return _run(name, x.contiguous().to(dev), y.contiguous().to(dev))


def _same(got, want):
    return len(got) == len(want) and all(torch.equal(a, b) for a, b in zip(got, want))


@pytest.mark.parametrize("layout", ["contiguous", "channels", "odd_batch_stride"])
@pytest.mark.parametrize("name", FAMILIES)
def test_every_accepted_layout_gives_the_bits_of_a_contiguous_copy(dev, lib, name, layout):
    one = layout == "odd_batch_stride"
    x, y = _operands(name, one)
    got = _run(name, _place(x, layout, dev), _place(y, layout, dev, WD if name == "regrid" else W))
    want = _reference(name, one, dev)
    assert all(bool(torch.isfinite(t.float()).all()) for t in want)              # (so that a NaN from outside a block cannot hide)
    assert _same(got, want)
    torch.cuda.synchronize()


@pytest.mark.parametrize("form", ["4d", "5d"])
@pytest.mark.parametrize("name", ["ens_sums", "ens_event_sums"])
def test_the_member_view_of_a_member_major_buffer(dev, lib, name, form):
    from swin_v2_weather_amd.utils.weighted_acc_rmse import _member_blocks
    d = _data()
    rows = torch.full((M * B, 7, H, W), float("nan"), device=dev)                # row m B + b is member m of sample b
    rows[:, 2:5] = d["ens"].reshape(M * B, C, H, W).to(dev)
    tar = _place(d["tar"], "channels", dev)
    e, t = _member_blocks(name, C, H, W, rows if form == "4d" else rows.view(M, B, 7, H, W), tar._base, M, 2, 2)
    assert e.data_ptr() == rows.data_ptr() + 2 * H * W * 4 and e.stride() == (B * 7 * H * W, 7 * H * W, H * W, W, 1)
    assert _same(_run(name, e, t), _reference(name, False, dev))


def _refused(x, why):
    """x [..., B, C, H, W] on the CPU -> a device tensor of its shape (but for the width) that the rule refuses for `why`"""
    dv = torch.device("cuda:0")
    if why == "misaligned":                                    # a view offset by one element
        return torch.zeros(x.numel() + 1, device=dv)[1:].view(x.shape)
    if why == "width 6":
        return torch.zeros(x.shape[:-1] + (6,), device=dv)
    if why == "batch stride":                                  # B = 2 samples C H W + 1 apart (members: a member stride that stays a multiple of 4)
        bs = C * H * W + 1
        stride = ((2 * bs + 2,) if x.dim() == 5 else ()) + (bs, H * W, W, 1)
        return torch.zeros(M * (2 * bs + 2) + 8, device=dv).as_strided(tuple(x.shape), stride)
    assert why == "transposed plane"
    return torch.zeros(x.shape[:-2] + (W, H), device=dv).transpose(-2, -1)


@pytest.mark.parametrize("why", ["misaligned", "width 6", "batch stride", "transposed plane"])
@pytest.mark.parametrize("name", FAMILIES)
def test_every_refused_layout_is_refused_without_a_launch(dev, lib, monkeypatch, name, why):
    from swin_v2_weather_amd import _lib as L
    x, y = _operands(name, False)
    bad = _refused(x, why)
    y = torch.zeros(y.shape[:-1] + (bad.shape[-1],), device=dev) if name != "regrid" else y.to(dev)      # (the truth follows the width)

    class SizesOnly:                                           # the workspace queries are host arithmetic; anything else would be a launch
        def __getattr__(self, entry):
            assert entry.endswith("_ws_bytes"), f"{entry}: the wrapper went on to the library"
            return getattr(lib, entry)
    monkeypatch.setattr(L, "load", SizesOnly)
    with pytest.raises(L.Swv2Error) as e:
        _run(name, bad, y)
    assert str(e.value).startswith(name + ": ")


def test_the_regrid_destination_is_exempt_from_alignment_and_width(dev, lib):
    from swin_v2_weather_amd import ops
    s, x = _setup(*GRIDS), _data()["prd"]
    y = torch.full((B * C * HD * WD + 1,), float("nan"), device=dev)[1:].view(B, C, HD, WD)
    assert WD % 4 and y.data_ptr() % 16 == 4 and ops.regrid_planes_ok(y, False) and not ops.regrid_planes_ok(y, True)
    got = _run("regrid", x.to(dev), y)
    assert _same(got, _reference("regrid", False, dev))
    assert RR.judge(got[0].cpu().numpy(), x.numpy(), s["Ar"], s["Br"], s["lat"][1], s["lon"][1], "destination off by one element, width 6") <= 1.0


def test_the_control_of_an_ensemble_rollout_is_score_rollout_on_member_0(dev, lib, tmp_path):
    from tests.test_score_gpu import _registry_model
    from swin_v2_weather_amd import inference
    from swin_v2_weather_amd.utils.weighted_acc_rmse import EventSpec, ForecastScorer
    model = _registry_model(dev, tmp_path)
    Mr, Br, Cout, Hr, Wr, steps = 3, 2, 5, 48, 72, 2
    g = torch.Generator(device=dev).manual_seed(3)
    x0 = torch.randn(Br, 9, Hr, Wr, device=dev, generator=g)
    cz = torch.rand(Br, steps - 1, Hr, Wr, device=dev, generator=g) * 2 - 1
    truth = torch.randn(Br, steps, Cout, Hr, Wr, device=dev, generator=g)
    scorer = ForecastScorer(Hr, Wr, Cout, dev, climatology=0.3 * torch.randn(Cout, Hr, Wr, device=dev, generator=g),
                            stds=torch.tensor([1.0, 2.0, 3.0, 4.0, 5.0]))
    for spec in (EventSpec("quantile", (0.5, 0.9), False), EventSpec("anomaly", (0.5,), True)):
        ens = inference.ensemble_rollout(model, x0, truth, steps, Mr, 0.05, 1, cz, 3, scorer, score_control=True, events=spec)
        member0 = inference.perturb_initial_condition(x0, Mr, 0.05, 1, 5)[:Br]
        want = inference.score_rollout(model, member0, truth, steps, cz, 3, scorer, events=spec)
        ctl = ens.control
        assert ctl.forecast is None and ctl.tqe is None and ctl.spectrum is None
        for f in ("rmse", "acc", "rmse_samples", "acc_samples"):
            assert torch.equal(getattr(ctl, f), getattr(want, f)), f
        ce, we = ctl.events, want.events
        assert ce.spec == we.spec == spec and len(ce.thresholds) == steps and all(torch.equal(a, b) for a, b in zip(ce.thresholds, we.thresholds))
        assert torch.equal(ce.table, we.table) and torch.equal(ce.n_invalid, we.n_invalid)
        assert set(ce.scores) == set(we.scores) and all(torch.equal(ce.scores[k], we.scores[k]) for k in we.scores)
