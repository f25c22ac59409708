"""Forecast events: the 2 x 2 contingency table of a forecast against the verifying analysis and its categorical scores, and the Brier
score, reliability table and ROC area of an ensemble's exceedance probabilities.  The definitions (include/swv2.h states them for the
kernels of csrc/events.hip; the statements here are the same definitions in plain torch, on any device, dtype and width):

    theta = thr[b][c][k], or fl32(base[c][h][w] + thr[b][c][k]) with a base field (one fp32 addition).  The event is x > theta, or
    x < theta with `below`; strict, in fp32 on the tensors as given.  A point is valid in its plane if the prediction (every member), the
    truth and the base are not NaN there; invalid points enter no cell and are counted per plane in n_invalid.
    deterministic   a = sum w [P and O]   b = sum w [P and not O]   c = sum w [not P and O]   d = sum w [not P and not O]   (four sums)
    ensemble        n = #{m : x_m event},  o = [truth event]:   S_e = sum w (n - M o)^2   S_f = sum w n (M - n)   S_o = sum w o   W_v = sum w
                    hist[0][j] = #{valid points with n = j}   hist[1][j] = #{... and o = 1}     (point counts, unweighted)

The scores are formed in fp64 from the tables, by the functions below alone; scores over a batch or over lead times are the scores of the
SUMMED tables, never means of scores.  The neighbourhood sums of the fractions skill score (csrc/fss.hip) are stated further down, beside
their functions.  None of this is compared with a verification package: the identities of tests/test_events_host.py
pin it.
"""
from collections import namedtuple

import torch

EVENT_MAX_K = 8               # thresholds per kernel call (more run in chunks)

EventSpec = namedtuple("EventSpec", "kind levels below", defaults=(False,))          # kind: "anomaly" | "quantile"
EventScores = namedtuple("EventScores", "table n_invalid scores pooled")
EnsembleEventScores = namedtuple("EnsembleEventScores", "sums wv hist n_invalid scores pooled reliability")
FSS_MAX_S = 8                 # scales per kernel call (more run in chunks)
FSS_MAX_R = 32                # the largest half-width of a neighbourhood, in grid points
NeighbourhoodScores = namedtuple("NeighbourhoodScores", "rows n_invalid scores pooled")
CONTINGENCY_NAMES = ("base_rate", "freq_bias", "pod", "far", "csi", "ets", "sedi")
BRIER_NAMES = ("brier", "fair_brier", "brier_skill")
RELIABILITY_NAMES = ("reliability", "resolution", "uncertainty", "roc_area")


def expand_thresholds(thresholds, B: int, Cc: int, device=None) -> torch.Tensor:
    """[K], [C, K] or [B, C, K] -> fp32 [B or 1, C, K] (a leading 1: shared by the samples)"""
    t = torch.as_tensor(thresholds, dtype=torch.float32)
    if device is not None:
        t = t.to(device)
    if t.dim() == 1:
        t = t.reshape(1, 1, -1).expand(1, Cc, -1)
    elif t.dim() == 2:
        t = t.unsqueeze(0)
    if t.dim() != 3 or t.shape[1] != Cc or t.shape[0] not in (1, B) or t.shape[2] < 1:
        raise ValueError(f"thresholds {tuple(torch.as_tensor(thresholds).shape)}: expected [K], [{Cc}, K] or [{B}, {Cc}, K]")
    return t.contiguous()


def _theta(thr, base, like):
    """the fp32 threshold field [B or 1, C, K, H or 1, W or 1]"""
    th = thr.to(device=like.device, dtype=torch.float32)[..., None, None]
    if base is not None:
        th = base.to(device=like.device, dtype=torch.float32).unsqueeze(0).unsqueeze(2) + th           # ONE fp32 addition
    return th


def _event(x, th, below: bool):
    return x < th if below else x > th


def event_table_torch(prd, tar, thresholds, w, base=None, below=False):
    """prd, tar [B, C, H, W] (any float dtype; compared in fp32), thresholds [K] | [C, K] | [B, C, K], w [H], base [C, H, W] | None ->
    (table [B, C, K, 4] = (a, b, c, d) in prd's dtype, n_invalid [B, C] int32)"""
    B, Cc, H, W = prd.shape
    if tar.shape != prd.shape:
        raise ValueError(f"event_table_torch: prediction {tuple(prd.shape)} / truth {tuple(tar.shape)}")
    thr = expand_thresholds(thresholds, B, Cc, prd.device)
    x, y = prd.to(torch.float32).unsqueeze(2), tar.to(torch.float32).unsqueeze(2)
    valid = ~(torch.isnan(prd) | torch.isnan(tar))
    if base is not None:
        valid = valid & ~torch.isnan(base.to(prd.device)).unsqueeze(0)
    th = _theta(thr, base, prd)
    P, O = _event(x, th, below), _event(y, th, below)
    q = (w.to(device=prd.device, dtype=prd.dtype).reshape(1, 1, -1, 1) * valid.to(prd.dtype)).unsqueeze(2)
    cells = [torch.sum(q * m.to(prd.dtype), dim=(-1, -2)) for m in (P & O, P & ~O, ~P & O, ~P & ~O)]
    return torch.stack(cells, dim=-1), (~valid).sum(dim=(-1, -2)).to(torch.int32)


def ensemble_event_sums_torch(ens, tar, thresholds, w, base=None, below=False):
    """ens [M, B, C, H, W], tar [B, C, H, W] -> (sums [B, C, K, 3] = (S_e, S_f, S_o), wv [B, C], hist [B, C, K, 2, M + 1] int32,
    n_invalid [B, C] int32); the member axis is walked one member at a time (no [M, ..., K] comparison tensor)"""
    M, B, Cc, H, W = ens.shape
    if M < 2 or tar.shape != ens.shape[1:]:
        raise ValueError(f"ensemble_event_sums_torch: members {tuple(ens.shape)} / truth {tuple(tar.shape)}, expected [M >= 2, B, C, H, W] / [B, C, H, W]")
    thr = expand_thresholds(thresholds, B, Cc, ens.device)
    K = thr.shape[2]
    dt = ens.dtype
    valid = ~(torch.isnan(tar) | torch.isnan(ens).any(dim=0))
    if base is not None:
        valid = valid & ~torch.isnan(base.to(ens.device)).unsqueeze(0)
    th = _theta(thr, base, ens)
    n = torch.zeros((B, Cc, K, H, W), dtype=torch.int64, device=ens.device)
    for m in range(M):
        n += _event(ens[m].to(torch.float32).unsqueeze(2), th, below)
    o = _event(tar.to(torch.float32).unsqueeze(2), th, below).to(torch.int64)
    q = (w.to(device=ens.device, dtype=dt).reshape(1, 1, -1, 1) * valid.to(dt))
    q5 = q.unsqueeze(2)
    s_e = torch.sum(q5 * ((n - M * o) ** 2).to(dt), dim=(-1, -2))
    s_f = torch.sum(q5 * (n * (M - n)).to(dt), dim=(-1, -2))
    s_o = torch.sum(q5 * o.to(dt), dim=(-1, -2))
    wv = torch.sum(q, dim=(-1, -2))
    v5 = valid.unsqueeze(2).to(torch.int64)
    hist = torch.zeros(B, Cc, K, 2, M + 1, dtype=torch.int64, device=ens.device)
    idx = n.reshape(B, Cc, K, H * W)
    hist[:, :, :, 0].scatter_add_(3, idx, v5.expand(B, Cc, K, H, W).reshape(B, Cc, K, H * W))
    hist[:, :, :, 1].scatter_add_(3, idx, (v5 * o).reshape(B, Cc, K, H * W))
    return torch.stack((s_e, s_f, s_o), dim=-1), wv, hist.to(torch.int32), (~valid).sum(dim=(-1, -2)).to(torch.int32)


# ---- scores, fp64 ------------------------------------------------------------------------------------------------------------------
def contingency_scores(table) -> dict:
    """table [..., 4] = (a, b, c, d) -> {name: fp64 [...]} for CONTINGENCY_NAMES.  0 / 0 is NaN in that entry only."""
    t = torch.as_tensor(table).to(torch.float64)
    a, b, c, d = t.unbind(dim=-1)
    n = a + b + c + d
    pod, pofd = a / (a + c), b / (b + d)
    a_r = (a + b) * (a + c) / n
    lf, lh, l1f, l1h = torch.log(pofd), torch.log(pod), torch.log(1 - pofd), torch.log(1 - pod)
    sedi = (lf - lh - l1f + l1h) / (lf + lh + l1f + l1h)
    return dict(base_rate=(a + c) / n, freq_bias=(a + b) / (a + c), pod=pod, far=b / (a + b), csi=a / (a + b + c),
                ets=(a - a_r) / (a + b + c - a_r), sedi=sedi)


def brier_scores(sums, wv, M: int) -> dict:
    """sums [..., K, 3] = (S_e, S_f, S_o), wv [...] -> {brier, fair_brier, brier_skill: fp64 [..., K]}"""
    s = torch.as_tensor(sums).to(torch.float64)
    v = torch.as_tensor(wv).to(torch.float64).unsqueeze(-1)
    s_e, s_f, s_o = s.unbind(dim=-1)
    m2 = float(M * M)
    brier = s_e / (m2 * v)
    obar = s_o / v
    return dict(brier=brier, fair_brier=(s_e - s_f / (M - 1.0)) / (m2 * v), brier_skill=1.0 - brier / (obar * (1.0 - obar)))


def reliability_scores(hist_fc, hist_ob) -> dict:
    """hist_fc, hist_ob [..., M + 1] point counts (forecast probability j / M issued; ... and the event observed) -> fp64 [...]:
    Murphy's reliability, resolution, uncertainty (brier = reliability - resolution + uncertainty, unweighted), and roc_area: the
    trapezoid rule over the points (F_t, H_t) of the M + 1 probability thresholds "warn if n >= t", closed by (0, 0) and (1, 1)."""
    nf = torch.as_tensor(hist_fc).to(torch.float64)
    no = torch.as_tensor(hist_ob).to(torch.float64)
    M1 = nf.shape[-1]
    p = torch.arange(M1, dtype=torch.float64, device=nf.device) / (M1 - 1.0)
    N = nf.sum(dim=-1, keepdim=True)
    obar = no.sum(dim=-1, keepdim=True) / N
    ok = torch.where(nf > 0, no / torch.where(nf > 0, nf, torch.ones_like(nf)), torch.zeros_like(nf))      # empty bins add nothing
    rel = (nf * (p - ok) ** 2).sum(dim=-1, keepdim=True) / N
    res = (nf * (ok - obar) ** 2).sum(dim=-1, keepdim=True) / N
    unc = obar * (1.0 - obar)
    # hits / false alarms with the warning "n >= t", t = M + 1 (never), M, ..., 0 (always): cumulative sums from the top
    zero = torch.zeros_like(N)
    hits = torch.cat([zero, torch.flip(no, dims=(-1,)).cumsum(dim=-1)], dim=-1)
    fals = torch.cat([zero, torch.flip(nf - no, dims=(-1,)).cumsum(dim=-1)], dim=-1)
    Hr, Fr = hits / hits[..., -1:], fals / fals[..., -1:]
    roc = ((Fr[..., 1:] - Fr[..., :-1]) * (Hr[..., 1:] + Hr[..., :-1]) * 0.5).sum(dim=-1)
    return dict(reliability=rel.squeeze(-1), resolution=res.squeeze(-1), uncertainty=unc.squeeze(-1), roc_area=roc)


# ---- neighbourhood verification: the fractions skill score (Roberts and Lean 2008) --------------------------------------------------
# include/swv2.h states this for csrc/fss.hip; the same in plain torch.  The event, theta, below, strictness, the fp32 comparison and
# validity are those above, except that an invalid point is NO EVENT IN EITHER FIELD (and stays in every denominator); it is counted in
# n_invalid.  A scale is a half-width r in grid points, 0 <= r <= 32, 2 r + 1 <= W.  The neighbourhood of (h, w): rows max(0, h - r) ..
# min(H - 1, h + r), columns w - r .. w + r modulo W (periodic longitude, the poles clip the box), N_h = rows of the clipped box * (2 r + 1)
# points; n_f / n_o = forecast / analysis events in it.
#     rows[B, C, K, S, H, 3] = (sum_w (n_f - n_o)^2, sum_w n_f^2, sum_w n_o^2)          int64, exact
#     q[h] = w[h] / N_h^2     FBS = sum_h q[h] rows[..., h, 0]     SF, SO likewise     FSS = 1 - FBS / (SF + SO)     (0 / 0 -> NaN there only)
# At r = 0 with the same weights (FBS, SF, SO) = (b + c, a + b, a + c) of the contingency table: the base rate f_o = SO_0 / (W sum w) comes
# from scale 0, and fss_uniform = 0.5 + f_o / 2 is the level from which a forecast counts as useful.  Scores over a batch or over lead
# times are the scores of the SUMMED rows.
def check_scales(scales, W: int) -> tuple:
    """the scales as a tuple of ints, or ValueError: strictly ascending, within 0 .. FSS_MAX_R, 2 r + 1 <= W"""
    sc = tuple(int(r) for r in scales)
    if not sc or any(float(r) != float(s) for r, s in zip(sc, scales)):
        raise ValueError(f"scales {tuple(scales)}: expected at least one integer half-width")
    if any(b <= a for a, b in zip(sc, sc[1:])) or sc[0] < 0 or sc[-1] > FSS_MAX_R:
        raise ValueError(f"scales {sc}: expected strictly ascending half-widths within 0 .. {FSS_MAX_R}")
    if 2 * sc[-1] + 1 > W:
        raise ValueError(f"scales {sc}: a box of 2 * {sc[-1]} + 1 columns is wider than the grid's {W}")
    return sc


def _box_count(e, r: int):
    """e [..., H, W] int64 -> the number of ones in the box of half-width r around every point (columns modulo W, rows clipped)"""
    H, W = e.shape[-2:]
    if r == 0:
        return e
    F = torch.nn.functional
    c = F.pad(torch.cat((e[..., W - r:], e, e[..., :r]), dim=-1).cumsum(dim=-1), (1, 0))
    row = c[..., 2 * r + 1:] - c[..., :W]                                    # [..., H, W]: the window sums of every row
    c = F.pad(F.pad(row, (0, 0, r, r)).cumsum(dim=-2), (0, 0, 1, 0))
    return c[..., 2 * r + 1:, :] - c[..., :H, :]


def fss_rows_torch(prd, tar, thresholds, scales, base=None, below=False):
    """prd, tar [B, C, H, W] (any float dtype; compared in fp32), thresholds [K] | [C, K] | [B, C, K], scales: half-widths (check_scales),
    base [C, H, W] | None -> (rows [B, C, K, S, H, 3] int64, n_invalid [B, C] int32); counted in int64 with cumulative sums: exact"""
    B, Cc, H, W = prd.shape
    if tar.shape != prd.shape:
        raise ValueError(f"fss_rows_torch: prediction {tuple(prd.shape)} / truth {tuple(tar.shape)}")
    sc = check_scales(scales, W)
    thr = expand_thresholds(thresholds, B, Cc, prd.device)
    valid = ~(torch.isnan(prd) | torch.isnan(tar))
    if base is not None:
        valid = valid & ~torch.isnan(base.to(prd.device)).unsqueeze(0)
    th = _theta(thr, base, prd)
    v5 = valid.unsqueeze(2)
    P = (_event(prd.to(torch.float32).unsqueeze(2), th, below) & v5).to(torch.int64)
    O = (_event(tar.to(torch.float32).unsqueeze(2), th, below) & v5).to(torch.int64)
    rows = []
    for r in sc:
        nf, no = _box_count(P, r), _box_count(O, r)
        rows.append(torch.stack((((nf - no) ** 2).sum(dim=-1), (nf * nf).sum(dim=-1), (no * no).sum(dim=-1)), dim=-1))       # [B, C, K, H, 3]
    return torch.stack(rows, dim=3), (~valid).sum(dim=(-1, -2)).to(torch.int32)


def box_sizes(H: int, scales) -> torch.Tensor:
    """N_h [S, H] int64: the points of the box around a point of row h (the poles clip its rows, the longitude wraps)"""
    h = torch.arange(H, dtype=torch.int64)
    return torch.stack([((h + int(r)).clamp(max=H - 1) - (h - int(r)).clamp(min=0) + 1) * (2 * int(r) + 1) for r in scales], dim=0)


def fss_scores(rows, w, scales, W: int, fields: int = 1) -> dict:
    """rows [..., S, H, 3] int64 (summed over the `fields` samples or lead times that are pooled), row weights w [H], the scales of axis S
    (scales[0] = 0: the base rate is read there) and the grid's width -> {fss [..., S], fbs [..., S] (= FBS), fss_uniform [...],
    base_rate [...] = SO_0 / (fields W sum w)} in fp64"""
    r = torch.as_tensor(rows)
    sc = tuple(int(s) for s in scales)
    if r.dim() < 3 or r.shape[-1] != 3 or r.shape[-3] != len(sc) or sc[0] != 0:
        raise ValueError(f"fss_scores: rows {tuple(r.shape)} for scales {sc}: expected [..., {len(sc)}, H, 3] and scales[0] = 0")
    w64 = torch.as_tensor(w).to(device=r.device, dtype=torch.float64).reshape(-1)
    q = w64 / box_sizes(r.shape[-2], sc).to(device=r.device, dtype=torch.float64) ** 2          # [S, H]
    fbs, sf, so = ((r[..., j].to(torch.float64) * q).sum(dim=-1) for j in range(3))            # the dot products over H
    base_rate = so[..., 0] / (w64.sum() * float(W) * float(fields))
    return dict(fss=1.0 - fbs / (sf + so), fbs=fbs, fss_uniform=0.5 + 0.5 * base_rate, base_rate=base_rate)


def useful_scale(fss, fss_uniform, scales) -> torch.Tensor:
    """fss [..., S], fss_uniform [...] -> int64 [...]: the smallest scale with fss >= fss_uniform, or -1 (a NaN score is never useful)"""
    f = torch.as_tensor(fss)
    ok = f >= torch.as_tensor(fss_uniform).to(f.device).unsqueeze(-1)
    sc = torch.as_tensor([int(s) for s in scales], dtype=torch.int64, device=f.device)
    first = ok.to(torch.int64).argmax(dim=-1)                               # the first True where there is one
    return torch.where(ok.any(dim=-1), sc[first], torch.full_like(first, -1))


# ---- ensemble neighbourhood verification: the probabilistic FSS (Schwartz et al. 2010, Duc et al. 2013) and eFSS / dFSS (Dey et al. 2014) ----
# include/swv2.h states this for swv2_fss_ens_rows; the same in plain torch.  Event, theta, below, strictness, the fp32 comparison, base
# field and box are those above.  A point is valid if no member, nor the truth, nor the base is NaN there (+-inf are valid); an invalid point
# is an event in NO member and not in the analysis, and is counted in n_invalid.  With e_m the event bit of member m and o the analysis':
#     c = sum_m e_m (0 .. M)     N_f = sum_box c = sum_m n_f^m     n_o = sum_box o
#     rows[B, C, K, S, H, 3] = (sum_w (N_f - M n_o)^2, sum_w N_f^2, sum_w n_o^2)          int64, exact
#     q[h] = w[h] / N_h^2     FBS = sum_h q rows[.., 0] / M^2     SF = sum_h q rows[.., 1] / M^2     SO = sum_h q rows[.., 2]
#     pfss = 1 - FBS / (SF + SO): the FSS of the neighbourhood ensemble probability N_f / (M N_h) against the analysis' fraction n_o / N_h
# base_rate, fss_uniform and useful_scale as for one forecast.  Boxes are in grid points, M >= 2 (the kernel: 2 .. 64), and ties between
# members are not randomised: the probability is the plain member fraction.  Beside it the spread-skill pair of Dey et al. (2014), from the
# DETERMINISTIC rows: member_rows = sum_m rows(member m vs analysis) -> eFSS, the skill of the mean member; dispersion_rows =
# sum_{m >= 1} rows(member m vs member 0) -> dFSS, the spatial agreement between the members and the control.  eFSS ~ dFSS per scale is the
# spatial analogue of spread ~ error.
EnsembleNeighbourhoodScores = namedtuple("EnsembleNeighbourhoodScores", "rows n_invalid scores pooled member_rows dispersion_rows member_scores "
                                         "dispersion_scores", defaults=(None, None, None, None))


def fss_ens_rows_torch(ens, tar, thresholds, scales, base=None, below=False):
    """ens [M, B, C, H, W], tar [B, C, H, W] (any float dtype; compared in fp32), thresholds, scales, base, below as fss_rows_torch ->
    (rows [B, C, K, S, H, 3] int64, n_invalid [B, C] int32); the member axis is walked one member at a time, counted in int64: exact"""
    if ens.dim() != 5 or ens.shape[0] < 2 or tar.shape != ens.shape[1:]:
        raise ValueError(f"fss_ens_rows_torch: members {tuple(ens.shape)} / truth {tuple(tar.shape)}, expected [M >= 2, B, C, H, W] / [B, C, H, W]")
    M, B, Cc, H, W = ens.shape
    sc = check_scales(scales, W)
    thr = expand_thresholds(thresholds, B, Cc, ens.device)
    valid = ~torch.isnan(tar)
    for m in range(M):
        valid = valid & ~torch.isnan(ens[m])
    if base is not None:
        valid = valid & ~torch.isnan(base.to(ens.device)).unsqueeze(0)
    th = _theta(thr, base, ens)
    v5 = valid.unsqueeze(2)
    c = torch.zeros((B, Cc, thr.shape[2], H, W), dtype=torch.int64, device=ens.device)
    for m in range(M):
        c += _event(ens[m].to(torch.float32).unsqueeze(2), th, below) & v5
    O = (_event(tar.to(torch.float32).unsqueeze(2), th, below) & v5).to(torch.int64)
    rows = []
    for r in sc:
        nf, no = _box_count(c, r), _box_count(O, r)
        rows.append(torch.stack((((nf - M * no) ** 2).sum(dim=-1), (nf * nf).sum(dim=-1), (no * no).sum(dim=-1)), dim=-1))       # [B, C, K, H, 3]
    return torch.stack(rows, dim=3), (~valid).sum(dim=(-1, -2)).to(torch.int32)


def fss_ens_scores(rows, w, scales, W: int, M: int, fields: int = 1) -> dict:
    """rows [..., S, H, 3] int64 of fss_ens_rows_torch / swv2_fss_ens_rows (summed over the `fields` samples or lead times that are pooled)
    for M members -> {pfss [..., S], fbs [..., S] (= FBS), fss_uniform [...], base_rate [...]} in fp64: fss_scores with the two forecast
    sums over M^2"""
    r = torch.as_tensor(rows)
    sc = tuple(int(s) for s in scales)
    if r.dim() < 3 or r.shape[-1] != 3 or r.shape[-3] != len(sc) or sc[0] != 0 or int(M) < 2:
        raise ValueError(f"fss_ens_scores: rows {tuple(r.shape)} for scales {sc}, M = {M}: expected [..., {len(sc)}, H, 3], scales[0] = 0 and M >= 2")
    w64 = torch.as_tensor(w).to(device=r.device, dtype=torch.float64).reshape(-1)
    q = w64 / box_sizes(r.shape[-2], sc).to(device=r.device, dtype=torch.float64) ** 2          # [S, H]
    fbs, sf, so = ((r[..., j].to(torch.float64) * q).sum(dim=-1) for j in range(3))            # the dot products over H
    m2 = float(int(M) * int(M))
    fbs, sf = fbs / m2, sf / m2
    base_rate = so[..., 0] / (w64.sum() * float(W) * float(fields))
    return dict(pfss=1.0 - fbs / (sf + so), fbs=fbs, fss_uniform=0.5 + 0.5 * base_rate, base_rate=base_rate)


def quantile_thresholds(truth, q) -> torch.Tensor:
    """truth [B, C, H, W], levels q [K] in [0, 1] -> [B, C, K] fp32: the analysis' own spatial quantiles per plane (plane_quantiles)"""
    from .weighted_acc_rmse import plane_quantiles
    return plane_quantiles(truth, torch.as_tensor(q, dtype=torch.float32).reshape(-1)).permute(1, 2, 0).to(torch.float32).contiguous()
