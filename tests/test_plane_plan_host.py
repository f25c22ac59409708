"""CPU: the plane-streaming entry points (scores, statistics, ensemble scores, order statistics) stand on ONE plan, csrc/plane_stream.h,
and tests/plane_reference.py mirrors it -- no GPU call."""
from swin_v2_weather_amd import _lib as L
from tests import plane_reference as P
from tests.test_dataset_stats_host import PLAN as STATS_PLAN
from tests.test_score_host import PLAN as SCORE_PLAN


def test_every_entry_point_answers_with_the_one_plan():
    lib = L.load()
    for planes in (1, 3, 146, 219, 1024, 2047, 2048, 2100):
        slices = P.plan_slices(planes)
        assert lib.swv2_score_slices(planes, 4, 4) == lib.swv2_stats_slices(planes, 4, 4) == slices, planes
        assert lib.swv2_score_ws_bytes(planes, 4, 4) == planes * slices * 16 and lib.swv2_stats_ws_bytes(planes, 4, 4) == planes * slices * 48
        for m in (2, 16, 50, 64):
            assert lib.swv2_ens_ws_bytes(planes, 4, 4, m) == planes * slices * (16 + 4 * (m + 1)), (planes, m)
        assert lib.swv2_quantile_ws_bytes(planes, 4, 4, 7) == planes * 35856              # histogram and state per plane, whatever the slices


def test_slice_bounds_tile_every_plane_of_the_plan_tables_on_multiples_of_four():
    shapes = [((B * C, H, W), s) for (B, C, H, W), s in SCORE_PLAN.items()] + list(STATS_PLAN.items())
    for (planes, H, W), slices in shapes:
        assert P.plan_slices(planes) == slices, (planes, H, W)
        b = P.slice_bounds(H * W, slices)
        assert len(b) == slices and b[0][0] == 0 and b[-1][1] == H * W
        assert all(lo % 4 == 0 and lo <= hi for lo, hi in b) and all(x[1] == y[0] for x, y in zip(b, b[1:]))
