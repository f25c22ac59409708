"""GPU (-m gpu): swv2_stats_accumulate / swv2_stats_finalize through the C ABI into guarded, sentinel-filled buffers, judged element by
element against the statement and the bounds of tests/stats_reference.py; then utils/dataset_stats.compute_stats on cuda:0 over year
files."""
import numpy as np
import pytest
import torch

from tests import stats_reference as R
from tests.plane_harness import SENTINEL, Guarded, dev, lib  # noqa: F401  (dev, lib: fixtures)

pytestmark = pytest.mark.gpu


def _run(lib, dev, slabs, pivot, fill=SENTINEL):
    """feed the device slabs of ONE year file in order (first on the first slab, prev null on the first slab), finalize;
    -> Guarded with part / tsum / folded / time_means"""
    from swin_v2_weather_amd import _lib as L
    C, H, W = slabs[0].shape
    slices = lib.swv2_stats_slices(C, H, W)
    wsb = lib.swv2_stats_ws_bytes(C, H, W)
    assert slices == R.plan_slices(C) and wsb == C * slices * 48
    g = Guarded(dev, fill, part=(wsb // 8, torch.float64), tsum=(C * H * W, torch.float64), folded=(C * 6, torch.float64),
                time_means=(C * H * W, torch.float32))
    st = torch.cuda.current_stream().cuda_stream
    for t, x in enumerate(slabs):
        L.check(lib.swv2_stats_accumulate(x.data_ptr(), slabs[t - 1].data_ptr() if t else None, pivot.data_ptr(), g["tsum"].data_ptr(),
                                          g["part"].data_ptr(), wsb, C, H, W, int(t == 0), st), "swv2_stats_accumulate")
    L.check(lib.swv2_stats_finalize(g["part"].data_ptr(), wsb, g["tsum"].data_ptr(), pivot.data_ptr(), C, H, W, len(slabs),
                                    g["folded"].data_ptr(), g["time_means"].data_ptr(), st), "swv2_stats_finalize")
    torch.cuda.synchronize()
    return g


@pytest.fixture(scope="module")
def runs(lib, dev):
    """one guarded run per shape, shared by the tests below (inputs and references: R.case, computed once)"""
    cache = {}

    def get(shape):
        if shape not in cache:
            years, pivot, _, _ = R.case(*shape, R.SHAPES[shape])
            slabs = [torch.tensor(years[0][t]).to(dev) for t in range(years[0].shape[0])]
            cache[shape] = (_run(lib, dev, slabs, torch.from_numpy(pivot).to(dev)), slabs)
        return cache[shape]
    return get


@pytest.mark.parametrize("shape", list(R.SHAPES), ids=lambda s: "x".join(map(str, s)))
def test_kernels_element_by_element_against_the_statement(runs, shape):
    from swin_v2_weather_amd.utils.dataset_stats import vectors_from_folded
    C, H, W = shape
    T = R.SHAPES[shape]
    years, pivot, ref, ref_state = R.case(C, H, W, T)
    g, _ = runs(shape)
    assert g.guards_intact(), "a kernel wrote outside its buffers"
    for k in ("part", "tsum", "folded", "time_means"):
        assert g.written(k), f"{k}: slots the plan names were left unwritten"
    folded, tsum = g["folded"].cpu().numpy().reshape(C, 6), g["tsum"].cpu().numpy().reshape(C, H, W)
    rs, rt = R.judge_state(folded, tsum, ref_state, R.chain_length(H, W, R.plan_slices(C), T), T, tag=f"{shape}")
    assert rs <= 1.0 and rt <= 1.0
    gm, gs, td = vectors_from_folded(folded, pivot, T, (T - 1) * H * W, H, W)
    vec = lambda a: a.astype(np.float32).reshape(1, C, 1, 1)
    got = dict(global_means=vec(gm), global_stds=vec(gs), time_diff_stds=vec(td),
               time_means=g["time_means"].cpu().numpy().reshape(1, C, H, W))
    u = R.judge_written(got, ref, tag=f"{shape}")
    assert max(u.values()) <= 1.0


def test_two_runs_agree_bit_for_bit_and_first_ignores_what_the_workspace_held(lib, dev, runs):
    for shape in ((3, 5, 8), (73, 16, 32), (1024, 49, 104)):
        years, pivot, _, _ = R.case(*shape, R.SHAPES[shape])
        g1, slabs = runs(shape)
        p = torch.from_numpy(pivot).to(dev)
        g2 = _run(lib, dev, slabs, p)
        assert torch.equal(g1.raw, g2.raw), shape                                # every output and the workspace, as bits
        g0 = _run(lib, dev, slabs, p, fill=0)                                    # a zeroed workspace instead of a dirty one
        assert g0.guards_intact()
        for k in ("part", "tsum", "folded", "time_means"):
            assert torch.equal(g0[k].view(torch.int32), g1[k].view(torch.int32)), (shape, k)


def test_argument_errors_return_the_code_without_a_launch(lib, dev):
    C, H, W = 2, 4, 8
    wsb = lib.swv2_stats_ws_bytes(C, H, W)
    g = Guarded(dev, part=(wsb // 8, torch.float64), tsum=(C * H * W, torch.float64), folded=(C * 6, torch.float64),
                time_means=(C * H * W, torch.float32))
    x = torch.zeros(C, H, W, device=dev)
    p = torch.zeros(C, dtype=torch.float64, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    a = (x.data_ptr(), None, p.data_ptr(), g["tsum"].data_ptr(), g["part"].data_ptr())
    assert lib.swv2_stats_accumulate(*a, wsb - 8, C, H, W, 1, st) == -1 and b"workspace" in lib.swv2_last_error()
    assert lib.swv2_stats_accumulate(*a, wsb, C, 3, 5, 1, st) == -1 and b"H * W % 4" in lib.swv2_last_error()
    assert lib.swv2_stats_accumulate(x.data_ptr() + 4, *a[1:], wsb, C, H, W, 1, st) == -1 and b"aligned" in lib.swv2_last_error()
    assert lib.swv2_stats_accumulate(None, *a[1:], wsb, C, H, W, 1, st) == -1 and b"null" in lib.swv2_last_error()
    assert lib.swv2_stats_finalize(g["part"].data_ptr(), wsb, g["tsum"].data_ptr(), p.data_ptr(), C, H, W, 0, g["folded"].data_ptr(),
                                   g["time_means"].data_ptr(), st) == -1 and b"T <= 0" in lib.swv2_last_error()
    torch.cuda.synchronize()
    assert bool((g.raw == SENTINEL).all())                                        # nothing ran
    from swin_v2_weather_amd.utils.dataset_stats import DatasetStats
    with pytest.raises(ValueError, match="multiple of 4"):
        DatasetStats(2, 3, 5, dev, np.zeros(2))


def _write_years(folder, years, first=1979):
    folder.mkdir()
    for k, a in enumerate(years):
        np.save(folder / f"{first + k}.npy", a)
    return str(folder)


def test_compute_stats_on_year_files_equals_the_cpu_path_and_stays_inside_a_file(dev, lib, tmp_path):
    from swin_v2_weather_amd.utils import dataset_stats as DS
    C, H, W, counts = 5, 5, 8, (3, 4)
    # the second file's slabs lie 1e4 above the first's: a difference across the file boundary would swamp time_diff_stds
    years = R.make_years(C, H, W, counts, seed=9, jump=1.0e4)
    data = _write_years(tmp_path / "data", years)
    T, N_d = 7, 5 * H * W
    on_gpu, on_cpu = DS.compute_stats(data, dev), DS.compute_stats(data, "cpu")
    assert on_gpu.on_kernels and not on_cpu.on_kernels and np.array_equal(on_gpu.pivot, on_cpu.pivot)
    sg, sc = on_gpu.state(), on_cpu.state()
    assert (sg["T"], sg["N_d"]) == (sc["T"], sc["N_d"]) == (T, N_d)
    ref_state = R.state(years, on_gpu.pivot)
    rs, rt = R.judge_state(sg["folded"], sg["tsum"], ref_state, R.chain_length(H, W, R.plan_slices(C), T), T, tag="compute_stats cuda")
    assert rs <= 1.0 and rt <= 1.0
    rs, rt = R.judge_state(sc["folded"], sc["tsum"], ref_state, R.chain_any_order(H, W, T), T, c_term=3, tag="compute_stats cpu")
    assert rs <= 1.0 and rt <= 1.0
    ref = R.statement(years)
    got, cpu = on_gpu.finalize(), on_cpu.finalize()
    assert max(R.judge_written(got, ref, tag="compute_stats cuda").values()) <= 1.0
    assert max(R.judge_written(cpu, ref, tag="compute_stats cpu").values()) <= 1.0
    for k in got:                                                                 # both within 1 ulp of one value: at most 2 apart
        assert got[k].shape == cpu[k].shape and R.ulps(got[k], cpu[k].astype(R.LD)) <= 2.0, k
    # no difference across the boundary: the statement over ONE file holding all seven slabs (one difference of 1e4 per element) is far away
    crossing = [np.concatenate(years)]
    assert R.ulps(got["time_diff_stds"], R.statement(crossing)["time_diff_stds"]) > 1000
    # a state written by the GPU run merges and loads like any other: shards of one folder, one on each path
    a = DS.compute_stats(data, dev, years=[1979]).state()
    b = DS.compute_stats(data, "cpu", years=[1980]).state()
    merged = DS.DatasetStats.merge([a, b]).finalize()
    assert max(R.judge_written(merged, ref, tag="merged cuda + cpu").values()) <= 1.0
    cont = DS.DatasetStats(C, H, W, dev, on_gpu.pivot).load_state(a)              # go on from a loaded state on the device
    slabs = [torch.tensor(years[1][t]).to(dev) for t in range(counts[1])]
    for t, x in enumerate(slabs):
        cont.update(x, slabs[t - 1] if t else None)
    assert max(R.judge_written(cont.finalize(), ref, tag="continued on cuda").values()) <= 1.0


def test_a_failing_producer_fails_the_streaming_call_and_a_pinned_source_streams_in_place(dev, lib):
    from swin_v2_weather_amd.utils import dataset_stats as DS

    class Broken(DS.SyntheticYearSource):
        def read(self, y, t, out):
            if t == 2:
                raise OSError("unreadable slab")
            super().read(y, t, out)
    with pytest.raises(OSError, match="unreadable"):
        DS.compute_stats(None, dev, source=Broken(n_years=1, n_samples=4, shape=(2, 4, 8)))
    # through the ring (more slabs than ring slots) and in place from a page-locked source: the same bits
    ring = DS.compute_stats(None, dev, source=DS.SyntheticYearSource(n_years=2, n_samples=5, shape=(3, 6, 8)), ring=2)
    direct = DS.compute_stats(None, dev, source=DS.SyntheticYearSource(n_years=2, n_samples=5, shape=(3, 6, 8), pinned=True))
    assert ring.T == direct.T == 10 and ring.N_d == 8 * 48
    a, b = ring.finalize(), direct.finalize()
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
