"""The neighbourhood sums of the fractions skill score, stated independently in numpy for tests/test_fss_host.py and tests/test_fss_gpu.py:
the box count is an explicit loop over the (2 r + 1)^2 offsets -- np.roll in longitude, shifted and clipped slices in latitude -- with no
cumulative sum, and nothing is shared with swin_v2_weather_amd/utils/events.py.  Everything is an integer: the judge is equality."""
import numpy as np


def thresholds_3d(thr, B, C):
    """[K] | [C, K] | [B, C, K] -> fp32 [B or 1, C, K]"""
    t = np.asarray(thr, np.float32)
    if t.ndim == 1:
        t = np.broadcast_to(t[None, None, :], (1, C, t.shape[0]))
    elif t.ndim == 2:
        t = t[None]
    assert t.ndim == 3 and t.shape[1] == C and t.shape[0] in (1, B)
    return t


def events(prd, tar, thr, base=None, below=False):
    """-> (P, O [B, C, K, H, W] bool: the event in the forecast / the analysis, an invalid point being no event; n_invalid [B, C])"""
    prd, tar = np.asarray(prd, np.float32), np.asarray(tar, np.float32)
    B, C, H, W = prd.shape
    th = thresholds_3d(thr, B, C)[..., None, None]
    valid = ~(np.isnan(prd) | np.isnan(tar))
    if base is not None:
        b = np.asarray(base, np.float32)
        valid &= ~np.isnan(b)[None]
        with np.errstate(invalid="ignore"):
            th = (b[None, :, None] + th).astype(np.float32)          # one fp32 addition
    with np.errstate(invalid="ignore"):
        x, y = prd[:, :, None], tar[:, :, None]
        P, O = (x < th, y < th) if below else (x > th, y > th)
    v = valid[:, :, None]
    return P & v, O & v, (~valid).sum(axis=(-1, -2)).astype(np.int32)


def box_count(e, r):
    """e [..., H, W] bool -> int64: the events in rows max(0, h - r) .. min(H - 1, h + r), columns w - r .. w + r modulo W.  One addition
    per offset (dh, dw) of the box; the running count is kept in int16 (at most 65 * 65 = 4225) for speed and widened at the end."""
    e = e.astype(np.int16)
    H = e.shape[-2]
    n = np.zeros_like(e)
    for dw in range(-r, r + 1):
        shifted = np.roll(e, -dw, axis=-1)                    # shifted[..., w] = e[..., (w + dw) mod W]
        for dh in range(-r, r + 1):
            lo, hi = max(0, -dh), min(H, H - dh)              # the rows h whose neighbour h + dh exists
            if lo < hi:
                n[..., lo:hi, :] += shifted[..., lo + dh:hi + dh, :]
    return n.astype(np.int64)


def rows(prd, tar, thr, scales, base=None, below=False):
    """-> (rows [B, C, K, S, H, 3] int64 = (sum_w (n_f - n_o)^2, sum_w n_f^2, sum_w n_o^2), n_invalid [B, C] int32)"""
    P, O, ninv = events(prd, tar, thr, base, below)
    out = []
    for r in scales:
        nf, no = box_count(P, int(r)), box_count(O, int(r))
        out.append(np.stack((((nf - no) ** 2).sum(-1), (nf * nf).sum(-1), (no * no).sum(-1)), axis=-1))
    return np.stack(out, axis=3), ninv


def populated(R, H, W, scales):
    """the reference's own verdict that a case is not degenerate: all three sums of a (plane, threshold, scale), added over its rows, are
    positive -- in every plane where a plane has the points for it (160 or more), somewhere in the batch otherwise"""
    tot = R.sum(axis=-2)                                      # [B, C, K, S, 3]
    return bool((tot > 0).all()) if H * W >= 160 else bool((tot.sum(axis=(0, 1)) > 0).all())


def box_sizes(H, scales):
    h = np.arange(H)
    return np.stack([(np.minimum(H - 1, h + r) - np.maximum(0, h - r) + 1) * (2 * r + 1) for r in scales]).astype(np.int64)


def scores(R, w, scales, W):
    """fp64: {fss, fbs [..., S], fss_uniform, base_rate [...]} from rows [..., S, H, 3]; scales[0] == 0"""
    assert scales[0] == 0
    q = np.asarray(w, np.float64)[None, :] / box_sizes(R.shape[-2], scales).astype(np.float64) ** 2
    fbs, sf, so = ((R[..., j].astype(np.float64) * q).sum(-1) for j in range(3))
    with np.errstate(invalid="ignore", divide="ignore"):
        fss = 1.0 - fbs / (sf + so)
    base_rate = so[..., 0] / (np.asarray(w, np.float64).sum() * W)
    return dict(fss=fss, fbs=fbs, fss_uniform=0.5 + 0.5 * base_rate, base_rate=base_rate)
