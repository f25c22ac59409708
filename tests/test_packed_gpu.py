"""GPU: the int16 packing kernels (csrc/packed.hip) byte for byte against the numpy statement of utils/packed.py, the host pipeline over
packed sources end to end, the packer and the statistics on the device."""
import os

import numpy as np
import pytest
import torch

from swin_v2_weather_amd.utils import dataset_stats as S
from swin_v2_weather_amd.utils import pack_dataset as D
from swin_v2_weather_amd.utils import packed as P
from tests import packed_reference as R
from tests.plane_harness import SENTINEL, Guarded, dev, lib  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

# (B, S, Craw, Hraw, Wraw, H, W)
SHAPES = [(2, 2, 7, 21, 40, 20, 36),        # cropped, every row 16-byte aligned
          (2, 1, 3, 5, 44, 5, 44),          # rows alternate in 16-byte alignment
          (1, 1, 2, 3, 1440, 3, 1440),      # the grid-stride loop at the real width (8 codes per lane)
          (1, 2, 1, 2, 4, 1, 4)]            # one vector per plane


@pytest.fixture(scope="module")
def ops(lib):
    from swin_v2_weather_amd import ops as o
    return o


def _f32(g, k):
    return g.ints(k).view(torch.float32)


def _same(a, b):
    """equal as numbers, NaN at the same places"""
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


@pytest.mark.parametrize("shape", SHAPES)
def test_select_normalize_i16_equals_the_numpy_statement(dev, ops, shape):
    B, S, Craw, Hraw, Wraw, H, W = shape
    rng = np.random.default_rng(sum(shape))
    rows = B * S + 1
    q = rng.integers(-32767, 32768, size=(B, S, Craw, Hraw, Wraw)).astype(np.int16)
    flat = q.reshape(-1)
    special = np.array([32767, -32767, 0, -32768], np.int16)
    flat[rng.choice(flat.size, size=min(flat.size, 8), replace=False)] = np.resize(special, min(flat.size, 8))
    flat[0], flat[-1] = -32768, 32767
    off = (rng.standard_normal((rows, Craw)) * 100).astype(np.float32)
    sc = (10.0 ** rng.uniform(-5, 1, (rows, Craw))).astype(np.float32)
    slab_row = rng.permutation(rows)[:B * S].astype(np.int32).reshape(B, S)          # every (b, s) another row, not in order
    Csel = min(Craw, 4)
    chan = rng.permutation(Craw)[:Csel].astype(np.int32)
    mean = (rng.standard_normal(Csel) * 10).astype(np.float32)
    std = (0.5 + rng.random(Csel)).astype(np.float32)
    coff, Ct = 1, S * Csel + 3
    g = Guarded(dev, out=B * Ct * H * W)
    out = _f32(g, "out").view(B, Ct, H, W)
    t = lambda a: torch.from_numpy(a).to(dev)
    qd, offd, scd = t(q), t(off), t(sc)
    ops.era5_select_normalize_i16(qd, out, t(chan), t(mean), t(std), offd, scd, t(slab_row), coff=coff)
    torch.cuda.synchronize()
    # the numpy statement: unpack every slab with the row of its (b, s), then crop / select / z-score as data_loader_era5 does
    xh = np.stack([np.stack([P.unpack_array(q[b, s], off[slab_row[b, s]], sc[slab_row[b, s]]) for s in range(S)]) for b in range(B)])
    ref = xh[:, :, chan, :H, :W].copy()
    with np.errstate(invalid="ignore"):
        ref -= mean.reshape(1, 1, -1, 1, 1)
        ref /= std.reshape(1, 1, -1, 1, 1)
    got = out.cpu().numpy()
    assert _same(got[:, coff:coff + S * Csel], ref.reshape(B, S * Csel, H, W))
    assert np.array_equal(np.isnan(got[:, coff:coff + S * Csel]).reshape(B, S, Csel, H, W), (q[:, :, chan, :H, :W] == -32768))
    ints = g.ints("out").view(B, Ct, H, W)
    assert bool((ints[:, :coff] == SENTINEL).all()) and bool((ints[:, coff + S * Csel:] == SENTINEL).all())      # other channels untouched
    assert g.guards_intact()
    # and the fp32 kernel on what unpack_i16 makes of the same slabs
    f32 = torch.empty(B, S, Craw, Hraw, Wraw, device=dev)
    for b in range(B):
        for s in range(S):
            r = int(slab_row[b, s])
            ops.era5_unpack_i16(qd[b, s], f32[b, s], offd[r], scd[r])
    assert f32.cpu().numpy().tobytes() == xh.tobytes()
    out2 = torch.full((B, Ct, H, W), -7.0, device=dev)
    ops.era5_select_normalize(f32, out2, t(chan), t(mean), t(std), coff=coff)
    assert _same(out2.cpu().numpy()[:, coff:coff + S * Csel], got[:, coff:coff + S * Csel])


def _distribution_slab(H, W):
    """one channel per distribution of the host test, plus the ties, non-finite values and an all-missing channel: [C, H, W] fp32"""
    n = H * W
    chans = [np.resize(v, n) for _, v in sorted(R.distributions(n=max(n, 64)).items())]
    tx, _ = R.ties()
    chans.append(np.resize(np.concatenate([tx[-2:], tx[:-2][::max(1, (tx.size - 2) // (n - 2))]]), n))      # keeps +-32767: offset 0, scale 1
    chans.append(R.with_missing(np.resize(R.distributions(n=max(n, 64), seed=5)["normal"], n))[0])
    chans.append(np.full(n, np.nan, np.float32))
    return np.stack(chans).astype(np.float32).reshape(len(chans), H, W)


@pytest.mark.parametrize("H,W", [(40, 52), (5, 44), (1, 4)])      # planes of 8k (8 codes per lane), 8k + 4 (4 per lane), one vector
def test_pack_i16_and_unpack_i16_bytes_equal_numpy(dev, ops, H, W):
    x = _distribution_slab(H, W)
    C = x.shape[0]
    lo, hi, mi = P.finite_range(x)
    off, sc = P.pack_params(lo, hi)
    if H * W >= 200:
        assert off[-3] == 0.0 and sc[-3] == 1.0                   # the ties channel
    assert mi[-1] == H * W and mi[-2] >= 3
    want_q = P.pack_array(x, off, sc)
    want_x = P.unpack_array(want_q, off, sc)
    t = lambda a: torch.from_numpy(a).to(dev)
    g = Guarded(dev, q=(C * H * W // 2, torch.int32), x=C * H * W)
    q = g.ints("q").view(torch.int16).view(C, H, W)
    xo = _f32(g, "x").view(C, H, W)
    ops.era5_pack_i16(t(x), q, t(off), t(sc))
    ops.era5_unpack_i16(q, xo, t(off), t(sc))
    torch.cuda.synchronize()
    assert q.cpu().numpy().tobytes() == want_q.tobytes()
    assert xo.cpu().numpy().tobytes() == want_x.tobytes()
    assert g.guards_intact()


def _range_run(dev, ops, lib, slabs):
    C, H, W = slabs[0].shape
    ws_bytes = lib.swv2_pack_range_ws_bytes(C, H, W)
    g = Guarded(dev, rng=C * 2, missing=(C, torch.float64), ws=(ws_bytes // 4, torch.int32))
    rng, missing, ws = _f32(g, "rng").view(C, 2), g.ints("missing").view(torch.int64), g.ints("ws").view(torch.uint8)
    for i, x in enumerate(slabs):
        ops.pack_range(torch.from_numpy(x).to(dev), rng, missing, ws, first=i == 0)
    torch.cuda.synchronize()
    assert g.guards_intact()
    return rng.cpu().numpy(), missing.cpu().numpy()


@pytest.mark.parametrize("C,H,W", [(3, 9, 16), (5, 33, 132), (700, 48, 64)])
def test_pack_range_running_fold_equals_numpy(dev, ops, lib, C, H, W):
    """three slabs folded into one range; (3, 9, 16): 144 elements for 682 slices, most of them empty; a channel that is all NaN in every
    slab; (700, 48, 64): two slices of 1536 elements each, more than one vector per thread"""
    assert (lib.swv2_stats_slices(C, H, W) * 4 > H * W) == ((C, H, W) == (3, 9, 16))
    rng = np.random.default_rng(C * H)
    slabs = []
    for k in range(3):
        x = (rng.standard_normal((C, H, W)) * (1 + k) + 10.0 * np.arange(C).reshape(C, 1, 1)).astype(np.float32)
        x[0] = R.with_missing(x[0], seed=k)[0]
        x[C - 1] = np.nan
        if k == 1:
            x[1, H - 1, W - 1], x[1, 0, 0] = -0.0, 1e30           # the last and the first element of a plane
        slabs.append(x)
    got_r, got_m = _range_run(dev, ops, lib, slabs)
    lo, hi, mi = P.finite_range(np.stack(slabs))
    assert lo[C - 1] == np.inf and hi[C - 1] == -np.inf and mi[C - 1] == 3 * H * W and mi[0] > 0
    assert np.array_equal(got_r[:, 0], lo) and np.array_equal(got_r[:, 1], hi) and np.array_equal(got_m, mi)
    again_r, again_m = _range_run(dev, ops, lib, slabs)
    assert again_r.tobytes() == got_r.tobytes() and again_m.tobytes() == got_m.tobytes()
    one_r, one_m = _range_run(dev, ops, lib, slabs[2:])                # first != 0 overwrites what the sentinel fill left
    l2, h2, m2 = P.finite_range(slabs[2])
    assert np.array_equal(one_r[:, 0], l2) and np.array_equal(one_r[:, 1], h2) and np.array_equal(one_m, m2)


# ---- the pipeline ------------------------------------------------------------------------------------------------------
class _Params(dict):
    __getattr__ = dict.__getitem__


def _two_year_source(pinned=False):
    from swin_v2_weather_amd.utils import host_pipeline as hp
    src = hp.SyntheticYearSource(n_years=2, n_samples=9, shape=(6, 21, 40), seed=5, pinned=pinned)
    for t in range(9):
        src.slab(1, t).mul_(3.0).add_(50.0)                       # the second year gets other parameters
    return src


@pytest.mark.parametrize("leg", ["staged", "pinned", "files"])
def test_host_pipeline_end_to_end_on_packed_sources(dev, ops, leg, tmp_path):
    """test_host_pipeline_end_to_end over int16 sources: every batch of two epochs equals the synchronous numpy computation on the
    unpacked codes exactly, through the staging ring, the zero-copy path and year files written by the packer"""
    from swin_v2_weather_amd.utils import host_pipeline as hp
    from swin_v2_weather_amd.utils.data_loader_era5 import cos_zenith
    Craw, Hraw, Wraw, H, W, B, nf = 6, 21, 40, 20, 40, 2, 1
    f32 = _two_year_source()
    if leg == "files":
        for y in range(2):
            np.save(tmp_path / f"era5_{f32.years[y]}.npy", np.stack([f32.slab(y, t).numpy() for t in range(9)]))
        D.pack_folder(str(tmp_path), str(tmp_path / "i16"), device="cuda:0", log=lambda *_: None)
        src = P.open_year_source(str(tmp_path / "i16"))
        assert type(src) is P.PackedYearSource
    else:
        src = P.pack_source(f32, pinned=leg == "pinned")
    assert src.packed and src.pinned == (leg == "pinned") and src.years == f32.years and src.shape == (Craw, Hraw, Wraw)
    assert src.params(0)[1].tobytes() != src.params(1)[1].tobytes()
    codes = np.empty((Craw, Hraw, Wraw), np.int16)

    def field(y, t):
        src.read(y, t, codes)
        return P.unpack_array(codes, *src.params(y))
    means = np.arange(Craw, dtype=np.float32).reshape(1, Craw, 1, 1) * 0.1
    stds = (1.0 + np.arange(Craw, dtype=np.float32)).reshape(1, Craw, 1, 1)
    np.save(tmp_path / "m.npy", means)
    np.save(tmp_path / "s.npy", stds)
    chans = np.array([0, 2, 3, 5])
    params = _Params(local_batch_size=B, dt=1, n_future=nf, img_size=(H, W), in_channels=chans, out_channels=chans, add_zenith=True,
                     seed=11, data_num_shards=2, data_shard_id=1, global_means_path=str(tmp_path / "m.npy"),
                     global_stds_path=str(tmp_path / "s.npy"), num_data_workers=4)
    stat = torch.randn(3, H, W)
    pipe = hp.Era5HostPipeline(params, src, dev, train=True, static_features=stat, ring=3)
    assert pipe.packed and pipe.raw[0][0].dtype == torch.int16 and (pipe.direct or pipe.pin[0][1].dtype == torch.int16)
    assert len(pipe) == (18 // 2) // B
    busy = torch.randn(1024, 1024, device=dev)
    for epoch in range(2):
        order = hp.epoch_order(18, 2, 1, 11, epoch, True)
        for i, batch in enumerate(pipe):
            inp, tar, tz = batch
            for b in range(B):
                y, t = hp.locate(int(order[i * B + b]), [0, 9], [9, 9], 1, nf)
                x = (field(y, t)[chans, :H, :W] - means[0, chans]) / stds[0, chans]
                assert np.array_equal(inp[b, :4].cpu().numpy(), x)
                assert float((inp[b, 4].cpu() - cos_zenith(src.years[y], 6.0 * t, H, W)).abs().max()) < 2e-5
                assert torch.equal(inp[b, 5:].cpu(), stat)
                for s_ in range(nf + 1):
                    tt = (field(y, t + 1 + s_)[chans, :H, :W] - means[0, chans]) / stds[0, chans]
                    assert np.array_equal(tar[b, 4 * s_: 4 * s_ + 4].cpu().numpy(), tt)
                    assert float((tz[b, s_].cpu() - cos_zenith(src.years[y], 6.0 * (t + 1 + s_), H, W)).abs().max()) < 2e-5
            busy = busy @ busy * 1e-3                          # keep the compute stream busy past the next __next__
        assert i == len(pipe) - 1


def test_reader_failure_in_a_packed_source_reaches_the_consumer(dev, ops):
    from swin_v2_weather_amd.utils import host_pipeline as hp
    src = P.pack_source(hp.SyntheticYearSource(n_years=1, n_samples=12, seed=1, shape=(3, 21, 40)))
    good = src.read

    def read(year_idx, t, out):
        if t == 5:
            raise OSError("bad time slab")
        return good(year_idx, t, out)
    src.read = read
    params = _Params(local_batch_size=2, dt=1, n_future=0, img_size=(20, 36), in_channels=[0, 1, 2], out_channels=[0, 1, 2], add_zenith=False,
                     seed=3, data_num_shards=1, data_shard_id=0, num_data_workers=2)
    pipe = hp.Era5HostPipeline(params, src, dev, train=False, steps_per_epoch=6)
    with pytest.raises(RuntimeError, match="producer thread failed"):
        for _ in pipe:
            pass


# ---- the packer and the statistics on the device -----------------------------------------------------------------------
def _write_folder(path):
    os.makedirs(path, exist_ok=True)
    rng = np.random.default_rng(7)
    for y in range(2):
        a = (rng.standard_normal((5, 3, 9, 16)) * (1.0 + 4.0 * y) + np.array([0.0, 250.0, 2e5]).reshape(1, 3, 1, 1)).astype(np.float32)
        np.save(os.path.join(path, f"era5_{1979 + y}.npy"), a)


def test_packer_on_the_device_writes_the_bytes_of_the_cpu_packer(dev, ops, tmp_path):
    _write_folder(str(tmp_path / "f32"))
    a = np.load(tmp_path / "f32" / "era5_1980.npy")
    a[1, 0, 2, 3], a[3, 2, 0, 0], a[4, 2, 8, 15] = np.nan, np.inf, -np.inf
    np.save(tmp_path / "f32" / "era5_1980.npy", a)
    assert D.main(["--data", str(tmp_path / "f32"), "--out", str(tmp_path / "gpu"), "--device", "cuda:0"]) == 0
    assert D.main(["--data", str(tmp_path / "f32"), "--out", str(tmp_path / "cpu"), "--device", "cpu"]) == 0
    assert sorted(os.listdir(tmp_path / "gpu")) == sorted(os.listdir(tmp_path / "cpu")) and len(os.listdir(tmp_path / "gpu")) == 4
    for y in (1979, 1980):
        assert open(tmp_path / "gpu" / f"era5_{y}.npy", "rb").read() == open(tmp_path / "cpu" / f"era5_{y}.npy", "rb").read()
        with np.load(tmp_path / "gpu" / f"era5_{y}.pack.npz") as zg, np.load(tmp_path / "cpu" / f"era5_{y}.pack.npz") as zc:
            assert sorted(zg.files) == sorted(zc.files)
            assert all(zg[k].dtype == zc[k].dtype and zg[k].tobytes() == zc[k].tobytes() for k in zg.files)
    assert list(P.PackedYearSource(str(tmp_path / "gpu")).missing(1)) == [1, 0, 2]


def test_dataset_stats_on_the_device_over_a_packed_folder_equal_its_unpacked_folder(dev, ops, tmp_path):
    _write_folder(str(tmp_path / "f32"))
    D.pack_folder(str(tmp_path / "f32"), str(tmp_path / "i16"), device="cuda:0", log=lambda *_: None)
    D.unpack_folder(str(tmp_path / "i16"), str(tmp_path / "back"), log=lambda *_: None)
    a = S.compute_stats(str(tmp_path / "i16"), "cuda:0").finalize()
    b = S.compute_stats(str(tmp_path / "back"), "cuda:0").finalize()
    assert set(a) == {n[:-4] for n in S.FILES}
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), k
    pinned = S.compute_stats(None, "cuda:0", source=P.pack_source(P.open_year_source(str(tmp_path / "f32")), pinned=True)).finalize()
    assert all(pinned[k].tobytes() == a[k].tobytes() for k in a)              # the zero-copy path, and pack_source == the packer


def test_get_data_loader_opens_a_packed_folder_by_its_content(dev, ops, tmp_path):
    """no yaml key: the same call gives the int16 pipeline over the packed folder and the fp32 pipeline over the fp32 one, and their
    batches are those of the folder `unpack` writes"""
    from swin_v2_weather_amd.utils.data_loader_era5 import get_data_loader
    _write_folder(str(tmp_path / "f32"))
    D.pack_folder(str(tmp_path / "f32"), str(tmp_path / "i16"), device="cpu", log=lambda *_: None)
    D.unpack_folder(str(tmp_path / "i16"), str(tmp_path / "back"), log=lambda *_: None)
    params = _Params(local_batch_size=2, dt=1, n_future=0, img_size=(8, 16), in_channels=[0, 2], out_channels=[0, 2], add_zenith=False,
                     add_landmask=False, add_orography=False, seed=3, data_num_shards=1, data_shard_id=0, num_data_workers=2)
    got = {}
    for name in ("i16", "back"):
        pipe, ds, sampler = get_data_loader(params, str(tmp_path / name), False, True)
        assert sampler is pipe and pipe.packed == (name == "i16") and len(ds) == 10
        got[name] = [(inp.cpu().clone(), tar.cpu().clone()) for inp, tar, _ in pipe]
    assert len(got["i16"]) == len(got["back"]) == 5
    assert all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for a, b in zip(got["i16"], got["back"]))
