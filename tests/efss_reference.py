"""The neighbourhood sums of the probabilistic fractions skill score, stated independently in numpy for tests/test_efss_host.py and
tests/test_efss_gpu.py on the events and the box count of tests/fss_reference.py: the box counts of the members are taken one member at a
time and added, then the three row sums.  No cumulative sum, and nothing is shared with swin_v2_weather_amd.  Everything is an integer: the
judge is equality."""
import functools

import numpy as np

from tests import fss_reference as R


@functools.lru_cache(maxsize=None)
def members(M, B, C, H, W):
    """the forecast of fields(B, C, H, W) + 0.5 N(0, 1) per member, fp32 [M, B, C, H, W]; made once per shape and never modified"""
    from tests.test_fss_host import fields                    # the shared field construction of the neighbourhood suites (numpy only)
    prd = fields(B, C, H, W)[0]
    rng = np.random.default_rng(11 * M + H + W)
    ens = (prd[None] + 0.5 * rng.standard_normal((M, B, C, H, W), dtype=np.float32)).astype(np.float32)
    ens.setflags(write=False)
    return ens


def member_events(ens, tar, thr, base=None, below=False):
    """-> (E [M, B, C, K, H, W] bool: the event in every member, O [B, C, K, H, W] bool: in the analysis, n_invalid [B, C] int32); a point
    with a NaN in ANY member, the truth or the base is an event in no member and not in the analysis"""
    ens, tar = np.asarray(ens, np.float32), np.asarray(tar, np.float32)
    bad = np.isnan(tar)
    for x in ens:
        bad = bad | np.isnan(x)
    if base is not None:
        bad = bad | np.isnan(np.asarray(base, np.float32))[None]
    keep = ~bad[:, :, None]
    Es = []
    for x in ens:
        P, O, _ = R.events(x, tar, thr, base, below)
        Es.append(P & keep)
    return np.stack(Es), O & keep, bad.sum(axis=(-1, -2)).astype(np.int32)


def counts(ens, tar, thr, base=None, below=False):
    """c [B, C, K, H, W] int64: the members with the event at every point"""
    return member_events(ens, tar, thr, base, below)[0].sum(axis=0).astype(np.int64)


def box_sum(c, r):
    """c [..., H, W] int64 -> the sum of c over the box of fss_reference.box_count, as two explicit passes: 2 r + 1 rolls in longitude, then
    2 r + 1 shifted, clipped slices in latitude (for the large planes, where (2 r + 1)^2 passes per member take minutes)"""
    c = np.asarray(c, np.int64)
    H = c.shape[-2]
    row = np.zeros_like(c)
    for dw in range(-r, r + 1):
        row += np.roll(c, -dw, axis=-1)
    n = np.zeros_like(c)
    for dh in range(-r, r + 1):
        lo, hi = max(0, -dh), min(H, H - dh)
        if lo < hi:
            n[..., lo:hi, :] += row[..., lo + dh:hi + dh, :]
    return n


def rows(ens, tar, thr, scales, base=None, below=False, two_pass=False):
    """-> (rows [B, C, K, S, H, 3] int64 = (sum_w (N_f - M n_o)^2, sum_w N_f^2, sum_w n_o^2), n_invalid [B, C] int32).  N_f is the sum of
    the members' box counts (fss_reference.box_count, one member at a time); two_pass: box_sum of the point counts instead"""
    E, O, ninv = member_events(ens, tar, thr, base, below)
    M = E.shape[0]
    out = []
    for r in scales:
        if two_pass:
            nf, no = box_sum(E.sum(axis=0), int(r)), box_sum(O, int(r))
        else:
            no = R.box_count(O, int(r))
            nf = np.zeros_like(no)
            for e in E:                                       # N_f = sum_m n_f^m
                nf += R.box_count(e, int(r))
        out.append(np.stack((((nf - M * no) ** 2).sum(-1), (nf * nf).sum(-1), (no * no).sum(-1)), axis=-1))
    return np.stack(out, axis=3), ninv


def scores(Rw, w, scales, W, M, fields=1):
    """fp64: {pfss, fbs [..., S], fss_uniform, base_rate [...]} from rows [..., S, H, 3] summed over `fields` samples; scales[0] == 0"""
    assert scales[0] == 0
    q = np.asarray(w, np.float64)[None, :] / R.box_sizes(Rw.shape[-2], scales).astype(np.float64) ** 2
    fbs, sf, so = ((Rw[..., j].astype(np.float64) * q).sum(-1) for j in range(3))
    fbs, sf = fbs / float(M * M), sf / float(M * M)
    with np.errstate(invalid="ignore", divide="ignore"):
        pfss = 1.0 - fbs / (sf + so)
    base_rate = so[..., 0] / (np.asarray(w, np.float64).sum() * W * fields)
    return dict(pfss=pfss, fbs=fbs, fss_uniform=0.5 + 0.5 * base_rate, base_rate=base_rate)
