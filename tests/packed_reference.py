"""An independent numpy restatement of the int16 packing rule of swin_v2_weather_amd/utils/packed.py, the distributions the host and GPU
suites pack, and the error bound.

The rule.  For one (year file, channel) with lo / hi the smallest / largest finite fp32 value:
    offset = fp32((lo64 + hi64) / 2) + 0.0f          scale = fp32((hi64 - lo64) / 65534)
    scale = 1 when hi == lo or nothing is finite (offset lo, or 0); scale = FLT_MIN when the quotient is positive but below the normal range
    q  = clamp(rint(fl(fl(x - offset) / scale)), -32767, 32767),  -32768 for a non-finite x          (fl: one fp32 rounding)
    xh = fl(fl(float(q) * scale) + offset),  NaN for q = -32768

The bound.  For a finite x of the channel
    |x - xh| <= (1/2 + 2^-7) * scale + 2^-23 * max(|lo|, |hi|).
Write u = 2^-24 (the unit roundoff) and count in units of scale ("steps").  |x - offset| is at most half the range, 32767 steps and a
little, so d = fl(x - offset) is off by at most u * 32768 = 2^-9 steps, and so is r = fl(d / scale) once more: before rint the position is
wrong by at most 2 * 2^-9 steps.  rint adds at most half a step.  The product fl(q * scale), |q| <= 32767, adds at most 2^-9 steps (where
it is subnormal its error is at most 2^-150, below any step, scale being at least FLT_MIN).  Together 1/2 + 3 * 2^-9 < 1/2 + 2^-7 steps.
Two things are not proportional to scale.  The final addition rounds a value of magnitude at most max(|lo|, |hi|) (up to the error just
counted): at most u * max(|lo|, |hi|), doubled to cover a result one binade up.  And offset itself is the rounded midpoint, off by at
most u * max(|lo|, |hi|): x - offset can then exceed 32767.5 steps at one end of the range, where the clamp to +-32767 loses what rint
would not have.  Each of the two is at most 2^-24 * max(|lo|, |hi|) in the cases that matter, 2^-23 * max(|lo|, |hi|) together.  On a
channel of two adjacent floats that last term is the whole bound, one ulp, and it is reached: both values decode to the one the midpoint
rounded to or to its neighbour.
"""
import numpy as np

F32 = np.float32
TINY = float(np.finfo(np.float32).tiny)
MISSING = -32768


def params(x):
    """(offset, scale, missing) of one channel's values, from scalars"""
    x = np.asarray(x, F32).reshape(-1)
    fin = x[np.isfinite(x)]
    missing = int(x.size - fin.size)
    if fin.size == 0:
        return F32(0.0), F32(1.0), missing
    lo, hi = float(fin.min()), float(fin.max())               # python floats: fp64
    offset = F32((lo + hi) / 2.0) + F32(0.0)
    if hi == lo:
        return offset, F32(1.0), missing
    quot = (hi - lo) / 65534.0
    scale = F32(quot)
    if float(scale) < TINY:
        scale = F32(TINY)
    return offset, scale, missing


def pack(x, offset, scale):
    x = np.asarray(x, F32)
    offset, scale = F32(offset), F32(scale)
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.subtract(x, offset, dtype=F32)
        r = np.divide(d, scale, dtype=F32)
        k = np.minimum(np.maximum(np.rint(r), F32(-32767.0)), F32(32767.0))
    q = np.full(x.shape, MISSING, np.int16)
    ok = np.isfinite(x)
    q[ok] = k[ok].astype(np.int16)
    return q


def unpack(q, offset, scale):
    q = np.asarray(q, np.int16)
    p = np.multiply(q.astype(F32), F32(scale), dtype=F32)
    v = np.add(p, F32(offset), dtype=F32)
    v[q == MISSING] = np.nan
    return v


def bound(offset, scale, lo, hi):
    """the bound above, fp64"""
    return (0.5 + 2.0 ** -7) * float(scale) + 2.0 ** -23 * max(abs(float(lo)), abs(float(hi)))


def distributions(n=1 << 16, seed=0):
    """name -> fp32 values: the cases the bound was checked on"""
    rng = np.random.default_rng(seed)
    one = np.float32(1.0)
    d = {
        "normal": rng.standard_normal(n),
        "geopotential": 2e5 + 3e3 * rng.standard_normal(n),
        "cubed_exponential": rng.exponential(1e-3, n) ** 3,
        "lognormal_six_decades": 1e-6 * np.exp(np.log(1e6) * rng.random(n)),
        "constant": np.full(n, 273.15),
        "two_adjacent": np.where(rng.random(n) < 0.5, one, np.nextafter(one, np.float32(2.0))),
        "huge": np.concatenate([[-3e38, 3e38, 0.0, 1e30], 3e38 * (2 * rng.random(n - 4) - 1)]),
        "subnormal": np.concatenate([[1e-40, 3e-40, 2e-40, 0.0], 3e-40 * rng.random(n - 4)]),
    }
    return {k: np.asarray(v).astype(F32) for k, v in d.items()}


def ties():
    """(values, codes): lo = -32767, hi = 32767 give offset 0 and scale 1, so k + 1/2 sits exactly half a step between the codes k and
    k + 1 and must go to the even one"""
    k = np.arange(-32767, 32767, dtype=np.int64)
    x = np.concatenate([(k + 0.5).astype(F32), np.array([-32767.0, 32767.0], F32)])
    even = np.where(k % 2 == 0, k, k + 1)
    return x, np.concatenate([even, [-32767, 32767]]).astype(np.int16)


def with_missing(x, seed=1):
    """a copy of x with NaN, +Inf and -Inf at seeded places; -> (values, number of them)"""
    rng = np.random.default_rng(seed)
    x = np.array(x, F32)
    idx = rng.choice(x.size, size=max(3, x.size // 50), replace=False)
    x.reshape(-1)[idx[0::3]] = np.nan
    x.reshape(-1)[idx[1::3]] = np.inf
    x.reshape(-1)[idx[2::3]] = -np.inf
    return x, idx.size
