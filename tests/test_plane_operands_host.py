"""The operand contract of the score families, on the CPU: every wrapper of ops.py that takes blocks of planes in place refuses what the
one rule (ops._planes_in_place) refuses, under its own name and before it reaches the library; the scorers' two block cutters
(utils/weighted_acc_rmse._channel_blocks, _member_blocks) name the calling method in every refusal and return views."""
import pytest
import torch

from swin_v2_weather_amd import _lib as L
from swin_v2_weather_amd import ops
from swin_v2_weather_amd.utils import weighted_acc_rmse as S

B, C, H, W, M, K = 2, 3, 5, 8, 3, 2


def _good(*lead):
    return torch.zeros(*lead, C, H, W)


# what no wrapper takes, whatever else is right about it (on this machine every tensor is a CPU tensor, so the first one alone is refused
# for its device; the others also for what their names say)
BAD = {"cpu": lambda lead: _good(*lead),
       "fp64": lambda lead: _good(*lead).double(),
       "3d": lambda lead: torch.zeros(C, H, W),
       "empty": lambda lead: torch.zeros(*lead[:-1], 0, C, H, W)}

w, ws = torch.ones(H), torch.zeros(64)
thr = torch.zeros(B, C, K)
tables = [torch.zeros(4, dtype=torch.int32), torch.ones(4, dtype=torch.int32), torch.ones(4, 1), torch.zeros(6, dtype=torch.int32),
          torch.ones(6, dtype=torch.int32), torch.ones(6, 1)]
# wrapper -> (the leading dimensions of its first operand, the call on that operand)
WRAPPERS = {"score_sums": ((B,), lambda x: ops.score_sums(x, _good(B), w, ws)),
            "l1_sums": ((B,), lambda x: ops.l1_sums(x, _good(B), w, ws)),
            "event_sums": ((B,), lambda x: ops.event_sums(x, _good(B), thr, w, ws)),
            "ens_sums": ((M, B), lambda x: ops.ens_sums(x, _good(B), w, ws)),
            "ens_event_sums": ((M, B), lambda x: ops.ens_event_sums(x, _good(B), thr, w, ws)),
            "regrid": ((B,), lambda x: ops.regrid(x, torch.zeros(B, C, 4, 6), *tables)),
            "plane_order_stats": ((B,), lambda x: ops.plane_order_stats(x, torch.zeros(K, dtype=torch.int32)))}


@pytest.mark.parametrize("bad", list(BAD))
@pytest.mark.parametrize("name", list(WRAPPERS))
def test_every_wrapper_refuses_under_its_own_name_before_the_library(monkeypatch, name, bad):
    def no_library():
        raise AssertionError("the wrapper went on to the library")
    monkeypatch.setattr(L, "load", no_library)
    lead, call = WRAPPERS[name]
    with pytest.raises(L.Swv2Error) as e:
        call(BAD[bad](lead))
    assert str(e.value).startswith(name + ": ")


@pytest.mark.parametrize("bad", list(BAD))
def test_the_four_predicates_say_no_to_the_same_inputs(bad):
    x4, x5 = BAD[bad]((B,)), BAD[bad]((M, B))
    assert ops.score_planes_ok(x4) is False and ops.quantile_planes_ok(x4) is False and ops.ens_members_ok(x5) is False
    assert ops.regrid_planes_ok(x4, True) is False and ops.regrid_planes_ok(x4, False) is False


def test_the_second_operand_is_held_to_the_same_rule():
    for name, call in (("score_sums", lambda t: ops.score_sums(_good(B), t, w, ws)), ("ens_sums", lambda t: ops.ens_sums(_good(M, B), t, w, ws)),
                       ("regrid", lambda t: ops.regrid(_good(B), t, *tables))):
        with pytest.raises(L.Swv2Error) as e:
            call(torch.zeros(B, C, H, W, dtype=torch.float64))
        assert str(e.value).startswith(name + ": ")


def _wide(*lead, channels=7):
    g = torch.Generator().manual_seed(5)
    return torch.randn(*lead, channels, H, W, generator=g)


def test_channel_blocks_are_views_at_the_channel_offset():
    prd, tar = _wide(B), _wide(B, channels=5)
    p, t = S._channel_blocks("score", C, H, W, prd, tar, 2, 1)
    assert p.shape == t.shape == (B, C, H, W)
    assert p.data_ptr() == prd.data_ptr() + 2 * H * W * 4 and t.data_ptr() == tar.data_ptr() + 1 * H * W * 4
    assert p.stride() == prd.stride() and torch.equal(p, prd[:, 2:5])


def test_member_blocks_take_the_4d_and_the_5d_form_of_one_storage():
    rows, tar = _wide(M * B), _wide(B, channels=5)
    e4, t4 = S._member_blocks("ensemble_score", C, H, W, rows, tar, M, 2, 1)
    e5, t5 = S._member_blocks("ensemble_score", C, H, W, rows.view(M, B, 7, H, W), tar, M, 2, 1)
    for e, t in ((e4, t4), (e5, t5)):
        assert e.shape == (M, B, C, H, W) and t.shape == (B, C, H, W)
        assert e.data_ptr() == rows.data_ptr() + 2 * H * W * 4 and t.data_ptr() == tar.data_ptr() + 1 * H * W * 4
        assert e.stride() == (B * 7 * H * W, 7 * H * W, H * W, W, 1)
    assert torch.equal(e4, e5) and torch.equal(e4[1, 0], rows[B, 2:5])              # row m B + b is member m of sample b


# (the operands, what is wrong with them): every one is refused with a ValueError that names the calling method
def _member_cases():
    rows, tar = _wide(M * B), _wide(B, channels=5)
    return {"wrong C": (rows, tar, M, 5, 1),                                                       # only two channels are left from there
            "wrong H": (rows[:, :, :4], tar[:, :, :4], M, 2, 1),
            "batch not divisible by M": (rows[:5], tar, M, 2, 1),
            "M = 1": (rows[:B], tar, 1, 2, 1),
            "mismatched": (rows, tar[:1], M, 2, 1)}


@pytest.mark.parametrize("case", ["wrong C", "wrong H", "batch not divisible by M", "M = 1", "mismatched"])
def test_member_blocks_name_the_calling_method(case):
    ens, tar, m, ce, ct = _member_cases()[case]
    for who in ("ensemble_score", "ensemble_event_score"):
        with pytest.raises(ValueError, match=who):
            S._member_blocks(who, C, H, W, ens, tar, m, ce, ct)
        if ens.shape[0] % m == 0:                                                                  # the 5-D form of the same storage
            with pytest.raises(ValueError, match=who):
                S._member_blocks(who, C, H, W, ens.unflatten(0, (m, ens.shape[0] // m)), tar, m, ce, ct)


@pytest.mark.parametrize("case", ["wrong C", "wrong H", "mismatched"])
def test_channel_blocks_name_the_calling_method(case):
    prd, tar = _wide(B), _wide(B, channels=5)
    args = {"wrong C": (prd, tar, 5, 1), "wrong H": (prd[:, :, :4], tar[:, :, :4], 2, 1), "mismatched": (prd, tar[:1], 2, 1)}[case]
    for who in ("score", "mae", "quantile_error", "event_score"):
        with pytest.raises(ValueError, match=who):
            S._channel_blocks(who, C, H, W, *args)


def test_both_scorers_refuse_through_the_shared_cutters():
    """ForecastScorer and RegriddedScorer raise the same refusals: the adapter has no checks of its own to disagree with"""
    from swin_v2_weather_amd.utils import regrid as G
    fs = S.ForecastScorer(H, W, C, "cpu")
    rs = S.RegriddedScorer(G.Regridder(G.equiangular_grid(H, W, False), G.equiangular_grid(3, 4, False)), C)
    rows, tar = _wide(M * B), _wide(B, channels=5)
    for sc in (fs, rs):
        with pytest.raises(ValueError, match="score: blocks"):
            sc.score(rows[:B], tar, coff_prd=5)
        with pytest.raises(ValueError, match="ensemble_score: a batch of 5 rows"):
            sc.ensemble_score(rows[:5], tar, M, coff_ens=2, coff_tar=1)
        with pytest.raises(ValueError, match="ensemble_event_score: members"):
            sc.ensemble_event_score(rows, tar, M, torch.zeros(1), coff_ens=5, coff_tar=1)
    got = rs.ensemble_score(rows, tar, M, coff_ens=2, coff_tar=1)
    want = rs.inner.ensemble_score(rs.regridder(rows.view(M, B, 7, H, W)[:, :, 2:5]), rs.regridder(tar[:, 1:4]), M)
    assert all(torch.equal(a, b) for a, b in zip(got, want))
