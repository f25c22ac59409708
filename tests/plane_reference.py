"""The plan of the plane-streaming kernels (csrc/plane_stream.h) mirrored in Python, and the pieces every fp64 reference of those kernels
uses to turn a count of roundings into a bound.  Imported by score_reference, stats_reference, quantile_reference and ensemble_reference;
each of those keeps its own chain_length and C_TERM, which describe its kernel.

    slices = planes >= 2048 ? 1 : 2048 / planes;  slice s = [plane * s // slices // 4 * 4, plane * (s + 1) // slices // 4 * 4), the last to the end
    u = one rounding of the sums' format, g(k) = k u / (1 - k u): the usual bound of k accumulated roundings
"""
import numpy as np

U = 2.0 ** -24         # one fp32 rounding (stats_reference, whose sums are fp64, passes its own)
BLOCKS = 2048          # PLANE_MAX_BLOCKS of csrc/plane_stream.h


def gamma(k: float, u: float = U) -> float:
    assert k * u < 0.01
    return k * u / (1.0 - k * u)


def plan_slices(planes: int) -> int:
    """swv2_score_slices / swv2_stats_slices: the published plan"""
    return 1 if planes >= BLOCKS else BLOCKS // planes


def slice_bounds(plane: int, slices: int):
    """element range [lo, hi) of every slice of a plane of `plane` elements"""
    lo = [plane * s // slices // 4 * 4 for s in range(slices)]
    return list(zip(lo, lo[1:] + [plane]))


def worst(err, bound) -> float:
    """largest error / bound ratio (0 / 0 counts as 0, x / 0 as inf): what every test prints before it asserts"""
    err, bound = np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(err == 0, 0.0, err / bound)
    return float(np.max(r)) if r.size else 0.0
