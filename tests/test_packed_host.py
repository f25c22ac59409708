"""CPU: the int16 packing rule of utils/packed.py against its independent restatement and error bound (tests/packed_reference.py), the
folder format, the packer's cpu path, statistics over a packed folder, and the host half of the five swv2 entry points -- no GPU call."""
import os

import numpy as np
import pytest

from swin_v2_weather_amd import _lib as L
from swin_v2_weather_amd.utils import dataset_stats as S
from swin_v2_weather_amd.utils import pack_dataset as D
from swin_v2_weather_amd.utils import packed as P
from swin_v2_weather_amd.utils.host_pipeline import SyntheticYearSource, YearArraySource
from tests import packed_reference as R

DIST = R.distributions()


def _chan(x):
    return np.asarray(x, np.float32).reshape(1, 1, -1)


def _params_of(x):
    lo, hi, mi = P.finite_range(_chan(x))
    off, sc = P.pack_params(lo, hi)
    return off, sc, mi, lo, hi


@pytest.mark.parametrize("name", sorted(DIST))
def test_rule_equals_the_restatement_and_stays_within_the_bound(name):
    x = DIST[name]
    off, sc, mi, lo, hi = _params_of(x)
    r_off, r_sc, r_mi = R.params(x)
    assert off.dtype == sc.dtype == np.float32 and off[0].tobytes() == r_off.tobytes() and sc[0].tobytes() == r_sc.tobytes() and mi[0] == r_mi == 0
    assert not np.signbit(off[0])                                  # -0 never reaches the sidecar
    q = P.pack_array(_chan(x), off, sc)
    assert q.dtype == np.int16 and np.array_equal(q.reshape(-1), R.pack(x, r_off, r_sc))
    xh = P.unpack_array(q, off, sc)
    assert xh.dtype == np.float32 and xh.tobytes() == R.unpack(q, r_off, r_sc).tobytes()
    assert q.min() >= -32767 and q.max() <= 32767                 # -32768 only for non-finite input: there is none here
    if name == "constant":
        assert sc[0] == 1.0 and off[0] == x[0] and np.all(q == 0) and np.array_equal(xh.reshape(-1), x)
    elif name == "subnormal":                                     # the quotient is positive but below the normal range: the step is FLT_MIN,
        assert sc[0] == np.finfo(np.float32).tiny and hi[0] - lo[0] < sc[0] and np.all(np.abs(q) <= 1)      # wider than the whole channel
    elif name == "two_adjacent":                                  # the midpoint rounds onto one of the two values: that one is code 0
        assert sorted(set(q.reshape(-1).tolist())) in ([0, 32767], [-32767, 0])
    else:
        assert q.min() == -32767 and q.max() == 32767             # the codes span the whole range
    err = np.abs(x.astype(np.float64) - xh.reshape(-1).astype(np.float64))
    b = R.bound(off[0], sc[0], lo[0], hi[0])
    print(f"{name}: offset {off[0]!r} scale {sc[0]!r} worst error / bound {err.max() / b:.3f}")
    assert np.all(err <= b)


def test_ties_go_to_even():
    x, want = R.ties()
    off, sc, _, _, _ = _params_of(x)
    assert off[0] == 0.0 and sc[0] == 1.0
    assert np.array_equal(P.pack_array(_chan(x), off, sc).reshape(-1), want)
    assert np.array_equal(R.pack(x, 0.0, 1.0), want)


@pytest.mark.parametrize("name", ["normal", "geopotential", "huge"])
def test_non_finite_values_round_trip_to_nan_and_are_counted(name):
    x, n_bad = R.with_missing(DIST[name])
    off, sc, mi, lo, hi = _params_of(x)
    assert mi[0] == n_bad == R.params(x)[2] and np.isfinite(off[0]) and np.isfinite(sc[0])
    q = P.pack_array(_chan(x), off, sc).reshape(-1)
    bad = ~np.isfinite(x)
    assert np.array_equal(q == -32768, bad) and np.array_equal(q, R.pack(x, off[0], sc[0]))
    xh = P.unpack_array(q.reshape(1, 1, -1), off, sc).reshape(-1)
    assert np.array_equal(np.isnan(xh), bad)
    assert np.all(np.abs(x[~bad].astype(np.float64) - xh[~bad]) <= R.bound(off[0], sc[0], lo[0], hi[0]))


def test_all_missing_and_mixed_channels():
    x = np.stack([np.full((4, 8), np.nan, np.float32), np.full((4, 8), -0.0, np.float32), DIST["normal"][:32].reshape(4, 8)])
    x[0, 0, 0] = np.inf
    lo, hi, mi = P.finite_range(x)
    assert lo[0] == np.inf and hi[0] == -np.inf and list(mi) == [32, 0, 0]
    off, sc = P.pack_params(lo, hi)
    assert off[0] == 0.0 and sc[0] == 1.0 and off[1] == 0.0 and not np.signbit(off[1]) and sc[1] == 1.0
    q = P.pack_array(x, off, sc)
    assert np.all(q[0] == -32768) and np.all(q[1] == 0) and q[2].min() == -32767 and q[2].max() == 32767
    assert np.all(np.isnan(P.unpack_array(q, off, sc)[0]))
    with pytest.raises(ValueError):
        P.pack_array(x.astype(np.float64), off, sc)
    with pytest.raises(ValueError):
        P.unpack_array(q.astype(np.int32), off, sc)


@pytest.mark.parametrize("name", sorted(DIST))
def test_packing_the_unpacked_values_again(name):
    """pack(unpack(pack(x))).  What holds, and why:
    (a) with FRESH parameters (what the packer does on an unpacked folder) the codes are not guaranteed equal: the decoded extremes may
        lie inside [lo, hi], so the range and with it the scale may shrink.  The decoded values x1 are a channel like any other, so the
        second round trip x2 stays within the bound of the NEW parameters of x1, and x2 within the sum of both bounds of x.
    (b) with the SAME parameters the codes come back exactly wherever the rounding of the final addition is small against a step,
        2^-22 max(|lo|, |hi|) <= scale: the position of x1 before rint is then off by at most 2^-24 |x1| / scale <= 1/4 step from the
        addition plus 3 * 2^-9 from the subtraction, the quotient and the product (packed_reference), less than the half step rint
        forgives.  Where the ulp of the values exceeds a step (two adjacent floats) several codes decode to one float and only (a)
        holds."""
    x = DIST[name]
    off, sc, _, lo, hi = _params_of(x)
    q = P.pack_array(_chan(x), off, sc)
    x1 = P.unpack_array(q, off, sc).reshape(-1)
    off1, sc1, _, lo1, hi1 = _params_of(x1)
    b = R.bound(off[0], sc[0], lo[0], hi[0])
    assert lo[0] - b <= lo1[0] <= hi1[0] <= hi[0] + b            # (a channel that decodes to one value gets the constant channel's scale 1)
    x2 = P.unpack_array(P.pack_array(_chan(x1), off1, sc1), off1, sc1).reshape(-1)
    b0, b1 = R.bound(off[0], sc[0], lo[0], hi[0]), R.bound(off1[0], sc1[0], lo1[0], hi1[0])
    assert np.all(np.abs(x1.astype(np.float64) - x2) <= b1) and np.all(np.abs(x.astype(np.float64) - x2) <= b0 + b1)
    if 2.0 ** -22 * max(abs(float(lo[0])), abs(float(hi[0]))) <= float(sc[0]):
        assert name != "two_adjacent"
        assert np.array_equal(P.pack_array(_chan(x1), off, sc), q)
    else:
        assert name == "two_adjacent"


# ---- the format ------------------------------------------------------------------------------------------------------
def _write_fp32_folder(path, n_years=2, n=5, shape=(3, 9, 16), seed=3, missing=False):
    os.makedirs(path, exist_ok=True)
    rng = np.random.default_rng(seed)
    arrays = []
    for y in range(n_years):
        a = (rng.standard_normal((n,) + shape) * (1.0 + 4.0 * y) + np.array([0.0, 250.0, 2e5]).reshape(1, 3, 1, 1)[:, :shape[0]]).astype(np.float32)
        if missing:
            a[1, 0, 2, 3], a[3, 2, 0, 0] = np.nan, np.inf
        np.save(os.path.join(path, f"era5_{1979 + y}.npy"), a)
        arrays.append(a)
    return arrays


def test_sidecar_round_trip_and_refusals(tmp_path):
    npy = str(tmp_path / "era5_1979.npy")
    off = np.array([0.0, -1.5e38, 2e5], np.float32)
    sc = np.array([np.finfo(np.float32).tiny, 9e33, 0.09], np.float32)
    mi = np.array([0, 7, 1 << 40], np.int64)
    side = P.write_sidecar(npy, off, sc, mi)
    assert side.endswith("era5_1979.pack.npz") and not side.endswith(".npy") and not side.endswith(".h5")
    got = P.read_sidecar(npy, 3)
    assert all(g.dtype == w.dtype and g.tobytes() == w.tobytes() for g, w in zip(got, (off, sc, mi)))
    with pytest.raises(ValueError, match="shape"):
        P.read_sidecar(npy, 4)                                     # mis-shaped: another channel count
    with pytest.raises(FileNotFoundError, match="sidecar"):
        P.read_sidecar(str(tmp_path / "era5_1980.npy"))
    with open(side, "wb") as f:
        np.savez(f, offset=off, scale=sc, missing=mi, version=np.int64(P.VERSION + 1))
    with pytest.raises(ValueError, match="version"):
        P.read_sidecar(npy, 3)
    with open(side, "wb") as f:
        np.savez(f, offset=off, scale=sc[:2], missing=mi, version=np.int64(P.VERSION))
    with pytest.raises(ValueError, match="shape"):
        P.read_sidecar(npy, 3)
    with open(side, "wb") as f:
        np.savez(f, offset=off, scale=sc)
    with pytest.raises(ValueError, match="not a pack sidecar"):
        P.read_sidecar(npy, 3)


def test_open_year_source_picks_each_class_and_a_broken_packed_folder_raises(tmp_path):
    arrays = _write_fp32_folder(str(tmp_path / "f32"))
    src = P.open_year_source(str(tmp_path / "f32"))
    assert type(src) is YearArraySource and not getattr(src, "packed", False)
    buf = np.empty((3, 9, 16), np.float32)
    src.read(1, 4, buf)
    assert buf.tobytes() == arrays[1][4].tobytes()                # the fp32 path reads the file's bytes, as before
    D.pack_folder(str(tmp_path / "f32"), str(tmp_path / "i16"), device="cpu", log=lambda *_: None)
    ps = P.open_year_source(str(tmp_path / "i16"))
    assert type(ps) is P.PackedYearSource and ps.packed and not ps.pinned
    assert ps.years == src.years == [1979, 1980] and ps.n_samples_year == [5, 5] and ps.shape == (3, 9, 16)
    q = np.empty((3, 9, 16), np.int16)
    ps.read(1, 4, q)
    off, sc = ps.params(1)
    assert np.array_equal(q, P.pack_array(arrays[1][4], off, sc))
    ps.read_f32(1, 4, buf)
    assert buf.tobytes() == P.unpack_array(q, off, sc).tobytes()
    os.remove(str(tmp_path / "i16" / "era5_1980.pack.npz"))
    with pytest.raises(FileNotFoundError, match="sidecar"):
        P.open_year_source(str(tmp_path / "i16"))
    P.write_sidecar(str(tmp_path / "i16" / "era5_1980.npy"), off[:2], sc[:2], np.zeros(2, np.int64))
    with pytest.raises(ValueError, match="shape"):
        P.PackedYearSource(str(tmp_path / "i16"))


def test_pack_source_is_the_packer_in_memory():
    src = SyntheticYearSource(n_years=2, n_samples=3, shape=(2, 5, 8), seed=9)
    src.slab(1, 0).mul_(7.0).add_(100.0)
    ps = P.pack_source(src)
    assert ps.packed and not ps.pinned and ps.years == src.years and ps.n_samples_year == [3, 3] and ps.shape == (2, 5, 8)
    for y in range(2):
        allx = np.stack([src.slab(y, t).numpy() for t in range(3)])
        lo, hi, mi = P.finite_range(allx)
        off, sc = P.pack_params(lo, hi)
        assert ps.params(y)[0].tobytes() == off.tobytes() and ps.params(y)[1].tobytes() == sc.tobytes() and not ps.missing(y).any()
        assert np.array_equal(ps.slab(y, 1).numpy(), P.pack_array(allx[1], off, sc))
    assert ps.params(0)[1].tobytes() != ps.params(1)[1].tobytes()
    toff, tsc = P.param_tables(ps)
    assert toff.shape == tsc.shape == (2, 2) and tsc[1].tobytes() == ps.params(1)[1].tobytes()


# ---- the packer and the statistics -------------------------------------------------------------------------------------
def test_cpu_cli_packs_and_unpacks_a_folder(tmp_path, capsys):
    arrays = _write_fp32_folder(str(tmp_path / "f32"), missing=True)
    np.save(tmp_path / "stds.npy", np.array([1.0, 2.0, 3e3], np.float32).reshape(1, 3, 1, 1))
    assert D.main(["--data", str(tmp_path / "f32"), "--out", str(tmp_path / "i16"), "--device", "cpu", "--stds", str(tmp_path / "stds.npy")]) == 0
    out = capsys.readouterr().out
    assert "scale/std" in out and "missing 1" in out and out.count("channel") == 6
    assert sorted(os.listdir(tmp_path / "i16")) == ["era5_1979.npy", "era5_1979.pack.npz", "era5_1980.npy", "era5_1980.pack.npz"]
    with pytest.raises(FileExistsError):
        D.main(["--data", str(tmp_path / "f32"), "--out", str(tmp_path / "i16"), "--device", "cpu"])
    assert D.main(["--data", str(tmp_path / "f32"), "--out", str(tmp_path / "i16"), "--device", "cpu", "--overwrite", "--years", "1980"]) == 0
    assert D.main(["unpack", "--data", str(tmp_path / "i16"), "--out", str(tmp_path / "back")]) == 0
    ps = P.PackedYearSource(str(tmp_path / "i16"))
    for y, a in enumerate(arrays):
        q = np.load(tmp_path / "i16" / f"era5_{1979 + y}.npy")
        assert q.dtype == np.int16 and q.shape == a.shape and q.flags["C_CONTIGUOUS"]
        lo, hi, mi = P.finite_range(a)
        off, sc = P.pack_params(lo, hi)
        assert ps.params(y)[0].tobytes() == off.tobytes() and ps.params(y)[1].tobytes() == sc.tobytes() and np.array_equal(ps.missing(y), mi)
        assert list(mi) == [1, 0, 1]
        assert np.array_equal(q, P.pack_array(a, off, sc))
        back = np.load(tmp_path / "back" / f"era5_{1979 + y}.npy")
        assert back.dtype == np.float32 and np.array_equal(np.isnan(back), ~np.isfinite(a))
        for c in range(3):
            ok = np.isfinite(a[:, c])
            assert np.all(np.abs(a[:, c][ok].astype(np.float64) - back[:, c][ok]) <= R.bound(off[c], sc[c], lo[c], hi[c]))
    with pytest.raises(ValueError, match="packed already"):
        D.pack_folder(str(tmp_path / "i16"), str(tmp_path / "again"), device="cpu")


def test_interrupted_pack_leaves_no_folder_that_opens_as_packed(tmp_path, monkeypatch):
    _write_fp32_folder(str(tmp_path / "f32"), n_years=1)

    def boom(*a, **k):
        raise OSError("disk full")
    monkeypatch.setattr(P, "write_sidecar", boom)
    with pytest.raises(OSError):
        D.pack_folder(str(tmp_path / "f32"), str(tmp_path / "i16"), device="cpu", log=lambda *_: None)
    assert not [f for f in os.listdir(tmp_path / "i16") if f.endswith(".npy")]
    with pytest.raises(FileNotFoundError):
        P.open_year_source(str(tmp_path / "i16"))


def test_dataset_stats_on_a_packed_folder_equal_those_of_its_unpacked_folder(tmp_path):
    _write_fp32_folder(str(tmp_path / "f32"))
    D.pack_folder(str(tmp_path / "f32"), str(tmp_path / "i16"), device="cpu", log=lambda *_: None)
    D.unpack_folder(str(tmp_path / "i16"), str(tmp_path / "back"), log=lambda *_: None)
    assert S.main(["--data", str(tmp_path / "i16"), "--out", str(tmp_path / "s_packed"), "--device", "cpu"]) == 0
    assert S.main(["--data", str(tmp_path / "back"), "--out", str(tmp_path / "s_f32"), "--device", "cpu"]) == 0
    for name in S.FILES:
        a, b = np.load(tmp_path / "s_packed" / name), np.load(tmp_path / "s_f32" / name)
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), name
    assert np.load(tmp_path / "s_packed" / "global_means.npy").shape == (1, 3, 1, 1)


# ---- the entry points, host half ---------------------------------------------------------------------------------------
def test_workspace_arithmetic_and_abi_version():
    lib = L.load()
    assert L.ABI_VERSION == 113 and lib.swv2_version() == 113
    for C, H, W, slices in ((73, 721, 1440, 28), (3, 9, 16, 682), (5, 33, 132, 409), (2048, 4, 4, 1), (4000, 4, 4, 1)):
        assert lib.swv2_pack_range_ws_bytes(C, H, W) == C * slices * 16 and lib.swv2_stats_slices(C, H, W) == slices
    for bad in ((0, 4, 4), (4, 0, 4), (4, 4, 0), (-1, 4, 4)):
        assert lib.swv2_pack_range_ws_bytes(*bad) == 0


def test_every_refusal_returns_invalid_with_a_message_and_without_a_gpu():
    """Arguments are checked before anything is launched, so the pointers only have to be non-null here: a refused call touches nothing."""
    lib = L.load()
    P_ = 4096                                         # any non-null, 16-byte aligned value: never dereferenced by a refused call
    ok = lib.swv2_pack_range_ws_bytes(3, 8, 16)

    def sel(raw=P_, out=P_, chan=P_, mean=P_, std=P_, off=P_, sc=P_, row=P_, B=2, S=2, Csel=3, Craw=5, Hraw=9, Wraw=16, H=8, W=12, Ct=7, coff=1):
        return lib.swv2_era5_select_normalize_i16(raw, out, chan, mean, std, off, sc, row, B, S, Csel, Craw, Hraw, Wraw, H, W, Ct, coff, None)

    def unp(raw=P_, out=P_, off=P_, sc=P_, C=3, H=8, W=16):
        return lib.swv2_era5_unpack_i16(raw, out, off, sc, C, H, W, None)

    def pck(slab=P_, out=P_, off=P_, sc=P_, C=3, H=8, W=16):
        return lib.swv2_era5_pack_i16(slab, out, off, sc, C, H, W, None)

    def rng(slab=P_, C=3, H=8, W=16, first=1, r=P_, m=P_, ws=P_, wb=ok):
        return lib.swv2_pack_range(slab, C, H, W, first, r, m, ws, wb, None)
    cases = [(lambda k=k: sel(**{k: None}), b"null") for k in ("raw", "out", "chan", "mean", "std", "off", "sc", "row")]
    cases += [(lambda k=k: sel(**{k: 0}), b"sizes") for k in ("B", "S", "Csel", "Craw", "H", "W")]
    cases += [(lambda: sel(B=-1), b"sizes"), (lambda: sel(H=10), b"sizes"), (lambda: sel(W=20), b"sizes"),
              (lambda: sel(W=10), b"multiples of 4"), (lambda: sel(Wraw=18, W=16), b"multiples of 4"),
              (lambda: sel(raw=P_ + 4), b"8-byte aligned"), (lambda: sel(raw=P_ + 2), b"8-byte aligned"), (lambda: sel(out=P_ + 8), b"16-byte aligned"),
              (lambda: sel(coff=2), b"channel range"), (lambda: sel(coff=-1), b"channel range"), (lambda: sel(Ct=5, coff=0), b"channel range"),
              (lambda: sel(B=300, S=100, Ct=400, coff=0), b"planes")]
    for fn in (unp, pck):
        first, second = ("raw", "out") if fn is unp else ("out", "slab")
        cases += [(lambda fn=fn, k=k: fn(**{k: None}), b"null") for k in (first, second, "off", "sc")]
        cases += [(lambda fn=fn, k=k: fn(**{k: 0}), b"sizes") for k in ("C", "H", "W")]
        cases += [(lambda fn=fn: fn(W=18), b"W % 4"), (lambda fn=fn: fn(C=70000), b"sizes"), (lambda fn=fn: fn(H=1 << 15, W=1 << 15), b"sizes"),
                  (lambda fn=fn, k=first: fn(**{k: P_ + 4}), b"8-byte aligned"), (lambda fn=fn, k=second: fn(**{k: P_ + 8}), b"16-byte aligned")]
    cases += [(lambda k=k: rng(**{k: None}), b"null") for k in ("slab", "r", "m", "ws")]
    cases += [(lambda k=k: rng(**{k: 0}), b"shape") for k in ("C", "H", "W")]
    cases += [(lambda: rng(W=18), b"W % 4"), (lambda: rng(slab=P_ + 8), b"aligned"), (lambda: rng(m=P_ + 4), b"aligned"), (lambda: rng(ws=P_ + 4), b"aligned"),
              (lambda: rng(r=P_ + 2), b"aligned"), (lambda: rng(wb=ok - 1), b"workspace"), (lambda: rng(wb=0), b"workspace"),
              (lambda: rng(C=1 << 21), b"shape")]
    for call, word in cases:
        assert call() == -1
        assert word in lib.swv2_last_error(), lib.swv2_last_error()
    with pytest.raises(L.Swv2Error):
        L.check(unp(W=18), "swv2_era5_unpack_i16")


def test_ops_wrappers_refuse_cpu_tensors_and_wrong_dtypes():
    import torch
    from swin_v2_weather_amd import ops
    q, x, p = torch.zeros(2, 4, 8, dtype=torch.int16), torch.zeros(2, 4, 8), torch.ones(2)
    with pytest.raises(L.Swv2Error):
        ops.era5_unpack_i16(q, x, p, p)
    with pytest.raises(L.Swv2Error):
        ops.era5_pack_i16(x, q, p, p)
    with pytest.raises(L.Swv2Error):
        ops.pack_range(x, torch.zeros(2, 2), torch.zeros(2, dtype=torch.int64), torch.zeros(64, dtype=torch.uint8), True)
    with pytest.raises(L.Swv2Error):
        ops.era5_select_normalize_i16(q.view(1, 1, 2, 4, 8), x.view(1, 2, 4, 8), torch.zeros(2, dtype=torch.int32), p, p, p.view(1, 2), p.view(1, 2),
                                      torch.zeros(1, 1, dtype=torch.int32))
