"""CPU: the fp64 statement of the ensemble scores (tests/ensemble_reference.py) against a brute-force loop, the identity behind the
kernel's e2, `ensemble_scores_torch` and `ForecastScorer.ensemble_score` on their plain-torch path judged by that statement,
`perturb_initial_condition`, the command line's refusals and the host half of the swv2_ens_* entry points (workspace arithmetic, every
refusal, header / ctypes agreement) -- no GPU call."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from swin_v2_weather_amd import _lib as L
from swin_v2_weather_amd import inference
from swin_v2_weather_amd.utils import weighted_acc_rmse as M
from swin_v2_weather_amd.utils.weighted_acc_rmse import EnsembleScores, ensemble_scores_torch
from tests import ensemble_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _case(kind, m, B=2, C=3, H=5, W=6, seed=0):
    """members [m, B, C, H, W], truth [B, C, H, W] fp32 and row weights [H] (the fp32 latitude weights: negative pole rows included)"""
    rng = np.random.default_rng(100 * m + seed)
    ens = rng.standard_normal((m, B, C, H, W)).astype(np.float32)
    tar = rng.standard_normal((B, C, H, W)).astype(np.float32)
    if kind == "offset":
        ens, tar = ens + np.float32(1.0e4), tar + np.float32(1.0e4)
    if kind == "ties":                                        # a grid of 0.25, the truth equal to a member on every other row, zeros of both signs
        ens, tar = np.round(ens * 4) / 4, np.round(tar * 4) / 4
        tar[:, :, ::2] = ens[m // 2][:, :, ::2]
        ens[0, :, :, 1, :3], tar[:, :, 1, :3] = -0.0, 0.0
    if kind == "nan":
        ens[m - 1, 1, 2, 3, 4] = np.nan
    if kind == "constant":
        ens[:] = ens[0]
    return ens.astype(np.float32), tar.astype(np.float32), M.latitude_weights(H).numpy()


def _brute_force(ens, tar, w):
    """the definitions, one grid point at a time in Python floats: S [B, C, 4], hist [B, C, M + 1]"""
    m, B, C, H, W = ens.shape
    S, hist = np.zeros((B, C, 4)), np.zeros((B, C, m + 1), np.int64)
    for b in range(B):
        for c in range(C):
            acc = [[], [], [], []]
            for h in range(H):
                for x in range(W):
                    xs, y, q = [float(v) for v in ens[:, b, c, h, x]], float(tar[b, c, h, x]), float(w[h])
                    xbar = math.fsum(xs) / m
                    acc[0].append(q * (xbar - y) ** 2)
                    acc[1].append(q * math.fsum((v - xbar) ** 2 for v in xs) / (m - 1))
                    acc[2].append(q * math.fsum(abs(v - y) for v in xs))
                    acc[3].append(q * math.fsum(abs(xs[i] - xs[j]) for i in range(m) for j in range(i + 1, m)))
                    hist[b, c, sum(1 for v in ens[:, b, c, h, x] if v < tar[b, c, h, x])] += 1        # the fp32 compare
            S[b, c] = [sum(a) if any(math.isnan(t) for t in a) else math.fsum(a) for a in acc]
    return S, hist


@pytest.mark.parametrize("kind,m", [("normal", 2), ("normal", 5), ("offset", 16), ("ties", 6), ("nan", 4), ("constant", 4)])
def test_reference_equals_the_brute_force_loop(kind, m):
    ens, tar, w = _case(kind, m, B=2, C=3, H=5, W=6)
    S, dS, hist = R.sums(ens, tar, w, 30)
    Sb, hb = _brute_force(ens, tar, w)
    assert np.array_equal(hist, hb) and np.all(hist.sum(axis=-1) == 30)
    nan = np.isnan(Sb)
    assert np.array_equal(np.isnan(S), nan) and (nan.any() == (kind == "nan"))
    if kind == "nan":
        assert nan[1, 2].all() and nan.sum() == 4
    scale = np.abs(Sb[~nan]) + (1e-9 if kind == "offset" else 1e-300)          # (x - xbar)^2 of fields near 1e4: fp64 itself rounds at 1e4 2^-53
    assert np.all(np.abs(S[~nan] - Sb[~nan]) <= (1e-8 if kind == "offset" else 1e-12) * scale)
    assert np.all(dS[~nan] >= 0) and np.all(dS[~nan] <= 1e-4 * np.abs(S[~nan]) + 1e-30)     # bounds of a few hundred roundings, not more
    if kind == "constant":
        assert np.all(S[..., 1] == 0) and np.all(S[..., 3] == 0) and np.all(dS[..., 1] == 0) and np.all(dS[..., 3] == 0)
    if kind == "ties":
        assert (ens == tar[None]).mean() > 0.05                # the truth really sits on members: those members do not count (strict compare)
        assert hist[..., m].sum() < hist[..., : m].sum()


@pytest.mark.parametrize("m", [2, 3, 16, 17, 64])
def test_gap_identity_of_the_pairwise_sum(m):
    """sum_{m<n} |x_m - x_n| = sum_i i (M - i) (x_(i+1) - x_(i)) over the sorted members, all terms non-negative"""
    rng = np.random.default_rng(m)
    x = rng.standard_normal((m, 7, 11))
    x[:, 0, :3] = x[0, 0, :3]                                  # ties
    a, b = R.pairwise_e2(x), R.gap_e2(x)
    assert np.all(np.abs(a - b) <= 4 * m * 2.0 ** -53 * a) and np.all(b[0, :3] == 0)
    brute = sum(abs(x[i, 3, 5] - x[j, 3, 5]) for i in range(m) for j in range(i + 1, m))
    assert abs(a[3, 5] - brute) <= 1e-12 * brute


def _as_got(r):
    out = {k: getattr(r, k).numpy() for k in R.NAMES + ("sums", "hist")}
    out["means"] = np.stack([getattr(r, k + "_mean").numpy() for k in R.NAMES])
    return out


@pytest.mark.parametrize("kind,m", [("normal", 2), ("normal", 3), ("normal", 16), ("normal", 17), ("offset", 16), ("offset", 50), ("ties", 6),
                                    ("nan", 4), ("constant", 4)])
def test_ensemble_scores_torch_on_cpu_against_fp64(kind, m):
    """the plain-torch path, judged as sums of H W M terms in any order; W % 4 != 0"""
    ens, tar, w = _case(kind, m, B=2, C=3, H=5, W=6)
    scale = np.array([2.0, 0.5, 7.0], np.float32)
    r = ensemble_scores_torch(torch.from_numpy(ens), torch.from_numpy(tar), torch.from_numpy(w), torch.from_numpy(scale))
    assert isinstance(r, EnsembleScores) and r.hist.dtype == torch.int32 and r.crps.dtype == torch.float32
    assert tuple(r.sums.shape) == (2, 3, 4) and tuple(r.hist.shape) == (2, 3, m + 1) and tuple(r.crps_mean.shape) == (3,)
    R.judge(_as_got(r), ens, tar, w, 5 * 6 * m, scale, f"torch {kind} M={m}")
    if kind == "constant":
        assert bool((r.sums[..., 1] == 0).all()) and bool((r.sums[..., 3] == 0).all()) and torch.equal(r.crps, r.fair_crps)
    if kind == "nan":
        for k in R.NAMES:
            nan = torch.isnan(getattr(r, k))
            assert bool(nan[1, 2]) and int(nan.sum()) == 1 and bool(torch.isnan(getattr(r, k + "_mean"))[2]) and int(torch.isnan(getattr(r, k + "_mean")).sum()) == 1
    # the default weights are the latitude weights
    d = ensemble_scores_torch(torch.from_numpy(ens), torch.from_numpy(tar))
    again = ensemble_scores_torch(torch.from_numpy(ens), torch.from_numpy(tar), M.latitude_weights(5))
    assert torch.equal(d.sums.view(torch.int32), again.sums.view(torch.int32))          # (as bits: the NaN plane too)
    with pytest.raises(ValueError):
        ensemble_scores_torch(torch.from_numpy(ens[:1]), torch.from_numpy(tar))


def test_forecast_scorer_ensemble_score_torch_path_in_place_blocks():
    """CPU tensors: channels 1:4 of member-major rows against channels 2:5 of a wider truth; stds on the first three means; score() untouched"""
    m, B, C, H, W = 5, 2, 3, 5, 8
    rng = np.random.default_rng(9)
    rows = rng.standard_normal((m * B, C + 2, H, W)).astype(np.float32)
    wide = rng.standard_normal((B, C + 3, H, W)).astype(np.float32)
    stds = np.array([2.0, 0.5, 7.0], np.float32)
    sc = M.ForecastScorer(H, W, C, "cpu", stds=stds)
    before = sc.score(torch.from_numpy(rows[:B]), torch.from_numpy(wide), coff_prd=1, coff_tar=2)
    r = sc.ensemble_score(torch.from_numpy(rows), torch.from_numpy(wide), m, coff_ens=1, coff_tar=2)
    ens, tar = rows.reshape(m, B, C + 2, H, W)[:, :, 1:4], wide[:, 2:5]
    R.judge(_as_got(r), ens, tar, M.latitude_weights(H).numpy(), H * W * m, stds, "ensemble_score on cpu")
    r5 = sc.ensemble_score(torch.from_numpy(rows).view(m, B, C + 2, H, W), torch.from_numpy(wide), m, 1, 2)
    assert all(torch.equal(a, b) for a, b in zip(r, r5)) and len(sc._ws) == 0
    plain = M.ForecastScorer(H, W, C, "cpu").ensemble_score(torch.from_numpy(rows), torch.from_numpy(wide), m, 1, 2)
    assert torch.equal(plain.fair_crps_mean, r.fair_crps_mean) and torch.equal(plain.crps, r.crps)
    assert torch.equal(r.crps_mean, plain.crps_mean * torch.from_numpy(stds)) and torch.equal(r.spread_mean, plain.spread_mean * torch.from_numpy(stds))
    after = sc.score(torch.from_numpy(rows[:B]), torch.from_numpy(wide), coff_prd=1, coff_tar=2)
    assert torch.equal(before.sums, after.sums) and torch.equal(before.rmse_mean, after.rmse_mean)
    ratio = M.spread_skill_ratio(r.spread, r.ens_rmse, m)
    assert torch.allclose(ratio, math.sqrt((m + 1) / m) * r.spread / r.ens_rmse)
    for bad in (dict(n_members=3), dict(n_members=m, coff_ens=3), dict(n_members=1)):
        with pytest.raises(ValueError):
            sc.ensemble_score(torch.from_numpy(rows), torch.from_numpy(wide), **{"coff_ens": 1, "coff_tar": 2, **bad})


def test_perturb_initial_condition_control_noise_and_invariants():
    B, Cin, H, W, m, nf = 2, 7, 6, 8, 4, 4
    x0 = torch.randn(B, Cin, H, W, generator=torch.Generator().manual_seed(1))
    y = inference.perturb_initial_condition(x0, m, 0.25, 17, nf)
    assert tuple(y.shape) == (m * B, Cin, H, W) and y.dtype == x0.dtype
    assert torch.equal(y[:B], x0)                                                      # member 0: the control, bit for bit
    rep = x0.repeat(m - 1, 1, 1, 1)
    assert torch.equal(y[B:, nf:], rep[:, nf:])                                        # zenith and invariants: copied bit for bit
    noise = torch.randn((m - 1) * B, nf, H, W, generator=torch.Generator("cpu").manual_seed(17))
    assert torch.equal(y[B:, :nf], rep[:, :nf] + 0.25 * noise)                         # member-major: row m B + b
    assert torch.equal(y, inference.perturb_initial_condition(x0, m, 0.25, 17, nf))     # same seed, same bits
    assert not torch.equal(y, inference.perturb_initial_condition(x0, m, 0.25, 18, nf))
    assert torch.equal(inference.perturb_initial_condition(x0, m, 0.0, 17, nf), x0.repeat(m, 1, 1, 1))
    assert torch.equal(inference.perturb_initial_condition(x0, 1, 0.25, 17, nf), x0)
    with pytest.raises(ValueError):
        inference.perturb_initial_condition(x0, m, 0.25, 17, Cin + 1)


def test_parser_refuses_ensemble_flags_that_do_not_fit():
    ap = inference.build_parser()
    a = ap.parse_args(["--registry", "R", "--truth", "t.npy", "--ensemble", "16", "--perturbation", "0.05", "--seed", "3", "--member-batch", "4"])
    assert (a.ensemble, a.perturbation, a.seed, a.member_batch) == (16, 0.05, 3, 4)
    b = ap.parse_args(["--registry", "R", "--truth", "t.npy", "--out", "f.npy"])
    assert (b.ensemble, b.perturbation, b.seed, b.member_batch, b.out) == (None, None, None, None, "f.npy")      # without the flags nothing changes
    for bad in (["--ensemble", "4", "--perturbation", "0.1"],                                          # no --truth
                ["--truth", "t.npy", "--out", "f.npy", "--ensemble", "4", "--perturbation", "0.1"],    # --out
                ["--truth", "t.npy", "--ensemble", "4"],                                               # no amplitude
                ["--truth", "t.npy", "--ensemble", "1", "--perturbation", "0.1"], ["--truth", "t.npy", "--ensemble", "65", "--perturbation", "0.1"],
                ["--truth", "t.npy", "--ensemble", "4", "--perturbation", "0.1", "--member-batch", "0"],
                ["--truth", "t.npy", "--ensemble", "4", "--perturbation", "0.1", "--extremes"],
                ["--truth", "t.npy", "--perturbation", "0.1"], ["--truth", "t.npy", "--seed", "1"], ["--truth", "t.npy", "--member-batch", "2"]):
        with pytest.raises(SystemExit) as e:
            ap.parse_args(["--registry", "R"] + bad)
        assert e.value.code == 2, bad


def test_lead_time_table_gains_the_ensemble_columns():
    t = lambda *rows: torch.tensor(rows)                                                # noqa: E731
    ctl = inference.RolloutScores(t([1.0, 2.0], [3.0, 4.0]), None, None, None, None)
    z = torch.zeros(2, 1, 2)
    ens = inference.EnsembleRolloutScores(t([0.5, 0.6], [0.7, 0.8]), t([0.4, 0.5], [0.6, 0.7]), t([0.1, 0.2], [0.3, 0.4]), t([0.9, 1.0], [1.1, 1.2]),
                                          z, z, z, z, torch.zeros(2, 1, 2, 5, dtype=torch.int32), None)
    assert ens.control is None
    table = inference.lead_time_table(ctl, [("u10m", 0), ("v10m", 1)], ensemble=ens).splitlines()
    assert table[0].split() == ["lead_h", "rmse_u10m", "rmse_v10m", "crps_u10m", "crps_v10m", "spread_u10m", "spread_v10m", "ens_rmse_u10m", "ens_rmse_v10m"]
    assert [float(v) for v in table[2].split()] == pytest.approx([12.0, 3.0, 4.0, 0.7, 0.8, 0.3, 0.4, 1.1, 1.2])
    assert inference.lead_time_table(ctl, [("u10m", 0)]).splitlines()[0].split() == ["lead_h", "rmse_u10m"]


# ---- the host half of the entry points ------------------------------------------------------------------------------------
def test_abi_version_workspace_arithmetic_and_chain_lengths():
    assert L.ABI_VERSION == 113 and "ensemble.hip" in L.SOURCES
    lib = L.load()
    assert lib.swv2_version() == 113
    for (B, C, H, W) in ((1, 1, 1, 4), (2, 3, 5, 8), (1, 73, 720, 1440), (1, 2100, 2, 4), (3, 5, 16, 32)):
        slices = lib.swv2_score_slices(B * C, H, W)
        for m in (2, 8, 9, 16, 17, 50, 64):
            assert lib.swv2_ens_ws_bytes(B * C, H, W, m) == B * C * slices * (16 + 4 * (m + 1)) and slices == R.plan_slices(B * C)
    for bad in ((0, 4, 4, 4), (4, 0, 4, 4), (4, 4, 0, 4), (-1, 4, 4, 4), (4, 4, 4, 1), (4, 4, 4, 0), (4, 4, 4, 65), (4, 4, 4, -3)):
        assert lib.swv2_ens_ws_bytes(*bad) == 0, bad
    assert [R.capacity(m) for m in (2, 8, 9, 16, 17, 32, 33, 64)] == [8, 8, 16, 16, 32, 32, 64, 64]
    # thread + 6 + 2 + fold + 6: one vector of four points; a single slice of 1040 / 528 / 272 elements walked two or three times by the first threads
    assert R.chain_length(1, 4, 2048, 2) == 4 + 14 + 32 and R.chain_length(2, 4, 1, 2) == 4 + 14 + 1
    assert R.chain_length(4, 260, 1, 8) == 8 + 15 and R.chain_length(4, 260, 1, 16) == 8 + 15
    assert R.chain_length(4, 132, 1, 17) == 3 + 15 and R.chain_length(4, 68, 1, 33) == 2 + 15
    # the production plane: 73 planes -> 28 slices of 37 028 or 37 032 elements
    assert R.chain_length(720, 1440, 28, 16) == 4 * 37 + 15 and R.chain_length(720, 1440, 28, 50) == 145 + 15


def test_every_refusal_returns_invalid_with_a_message_and_without_a_gpu():
    """Arguments are checked before anything is launched, so the pointers only have to be non-null here: a refused call touches nothing."""
    lib = L.load()
    P = 4096                                          # any non-null, 16-byte aligned value: never dereferenced by a refused call
    m, B, C, H, W = 5, 2, 3, 8, 16
    span = C * H * W
    ok = lib.swv2_ens_ws_bytes(B * C, H, W, m)

    def sums(ens=P, ms=B * span, bs=span, tar=P, ts=span, w=P, m=m, B=B, C=C, H=H, W=W, ws=P, wb=ok):
        return lib.swv2_ens_sums(ens, ms, bs, tar, ts, w, m, B, C, H, W, ws, wb, None)

    def fin(ws=P, wb=ok, m=m, B=B, C=C, H=H, W=W, scale=None, s=P, h=P, er=P, sp=P, cr=P, fc=P, mn=P):
        return lib.swv2_ens_finalize(ws, wb, m, B, C, H, W, scale, s, h, er, sp, cr, fc, mn, None)
    for call, word in ((lambda: sums(ens=None), b"null"), (lambda: sums(tar=None), b"null"), (lambda: sums(w=None), b"null"),
                       (lambda: sums(ws=None), b"null"), (lambda: sums(m=1), b"members"), (lambda: sums(m=65), b"members"),
                       (lambda: sums(m=0), b"members"), (lambda: sums(W=18), b"W % 4"), (lambda: sums(W=0), b"shape"), (lambda: sums(B=0), b"shape"),
                       (lambda: sums(ens=P + 4), b"aligned"), (lambda: sums(tar=P + 8), b"aligned"), (lambda: sums(ws=P + 4), b"aligned"),
                       (lambda: sums(ms=B * span + 2), b"stride"), (lambda: sums(bs=span + 1), b"stride"), (lambda: sums(ts=span + 3), b"stride"),
                       (lambda: sums(bs=H * W), b"stride"), (lambda: sums(ts=H * W), b"stride"), (lambda: sums(wb=ok - 1), b"workspace"),
                       (lambda: sums(wb=0), b"workspace"), (lambda: sums(wb=lib.swv2_ens_ws_bytes(B * C, H, W, m - 1)), b"workspace"),
                       (lambda: sums(B=1 << 12, C=1 << 8), b"shape"), (lambda: sums(H=1 << 15, W=1 << 15), b"shape"),
                       (lambda: fin(ws=None), b"null"), (lambda: fin(s=None), b"null"), (lambda: fin(h=None), b"null"), (lambda: fin(er=None), b"null"),
                       (lambda: fin(sp=None), b"null"), (lambda: fin(cr=None), b"null"), (lambda: fin(fc=None), b"null"), (lambda: fin(mn=None), b"null"),
                       (lambda: fin(m=1), b"members"), (lambda: fin(m=65), b"members"), (lambda: fin(wb=ok - 16), b"workspace"),
                       (lambda: fin(s=P + 4), b"aligned"), (lambda: fin(ws=P + 8), b"aligned"), (lambda: fin(C=0), b"shape"),
                       (lambda: fin(B=1 << 12, C=1 << 8), b"shape")):
        assert call() == -1
        assert word in lib.swv2_last_error(), lib.swv2_last_error()
    with pytest.raises(L.Swv2Error):
        L.check(sums(W=18), "swv2_ens_sums")
    assert sums(B=1, bs=0, ts=0, wb=0) == -1 and b"workspace" in lib.swv2_last_error()      # B == 1: the batch strides are not looked at


def test_header_and_ctypes_agree_on_the_ensemble_entry_points():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "swv2.h")).read(), flags=re.S)
    kinds = {"int": ctypes.c_int, "long": ctypes.c_long, "size_t": ctypes.c_size_t}
    seen = []
    for ret, name, args in re.findall(r"\b(int|size_t)\s+(swv2_ens_[a-z_]+)\s*\(([^)]*)\)\s*;", txt):
        want = [ctypes.c_void_p if "*" in a else kinds[a.split()[0]] for a in (x.strip() for x in args.split(","))]
        res, argtypes = L.SYMBOLS[name]
        assert res is kinds[ret] and argtypes == want, name
        seen.append(name)
    assert sorted(seen) == ["swv2_ens_finalize", "swv2_ens_sums", "swv2_ens_ws_bytes"]
    assert [a.split()[-1].lstrip("*") for a in re.search(r"swv2_ens_sums\s*\(([^)]*)\)", txt).group(1).split(",")] == \
        ["ens", "ens_mstride", "ens_bstride", "tar", "tar_bstride", "w", "M", "B", "C", "H", "W", "ws", "ws_bytes", "stream"]
    lib = L.load()
    assert all(hasattr(lib, n) for n in seen)


def test_ops_wrappers_refuse_what_the_kernel_cannot_take():
    from swin_v2_weather_amd import ops
    x, y = torch.zeros(3, 1, 2, 4, 8), torch.zeros(1, 2, 4, 8)
    assert not ops.ens_members_ok(x)                          # a CPU tensor
    with pytest.raises(L.Swv2Error):
        ops.ens_sums(x, y, torch.ones(4), torch.zeros(64))
    with pytest.raises(L.Swv2Error):
        ops.ens_workspace(2, 4, 8, 65, "cpu")
