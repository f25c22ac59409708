"""CPU: the fp64 statement of Adam (tests/adam_reference.py) against torch.optim.Adam itself, an fp32 numpy twin of the kernels' arithmetic
inside the derived bounds on the GPU test's own inputs, eight defective twins outside them, the host wrappers' fp32 scalars (glibc's powf)
inside their error terms, and the host half of swv2_adam_multi / swv2_adam_step (struct mirror, refusals) -- no GPU call."""
import ctypes
import ctypes.util

import numpy as np
import pytest
import torch

from swin_v2_weather_amd import _lib as L
from tests import adam_reference as R
from tests.test_host_and_cabi import header_struct_fields

F = np.float32
_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.powf.restype, _libm.powf.argtypes = ctypes.c_float, [ctypes.c_float, ctypes.c_float]


def c_powf(b, t):
    """the function the host wrappers call"""
    return F(_libm.powf(float(b), float(t)))


def np_powf(b, t):
    return np.power(F(b), F(t))


def host_scalars(lr, beta1, beta2, step, powf=c_powf):
    """(step_size, bc2_sqrt) as swv2_adam_multi / swv2_adam_step form them, every operation in fp32"""
    bc1, bc2 = F(1) - powf(F(beta1), step), F(1) - powf(F(beta2), step)
    ss, bs = F(lr) / bc1, np.sqrt(bc2)
    assert ss.dtype == np.float32 and bs.dtype == np.float32
    return ss, bs


def fma(a, b, c):
    """fp32 fma: the product of two fp32 values is exact in fp64, the sum rounds to fp64 and then to fp32 (a double rounding in rare
    ties: a twin, not a bit-exact model)"""
    return (R.d(a) * R.d(b) + R.d(c)).astype(np.float32)


def twin_step(p, g, m, v, hyper, step, contraction="none", defect=None):
    """one step of the kernels' arithmetic in fp32 numpy -> (p', m', v').  contraction: which product of a * b + c * d the compiler fused
    ("none": adam_kernel as compiled today; "first" / "second": the two fmas adam_multi_kernel's walks may get).  defect: one of DEFECTS."""
    lr, b1, b2, eps, inv = (F(x) for x in hyper)
    ss, bs = host_scalars(lr, b1, b2, step)
    if defect == "step_size_without_bias_correction":
        ss = lr
    gi = g if defect == "inv_not_applied" else g * inv
    w1, w2 = F(1) - b1, F(1) - b2
    a = w2 * gi
    sq = a if defect == "v_from_g_not_g_squared" else None
    with np.errstate(invalid="ignore", divide="ignore"):
        if contraction == "none":
            m1 = b1 * m + w1 * gi
            v1 = b2 * v + (sq if sq is not None else a * gi)
        elif contraction == "first":
            m1 = fma(b1, m, w1 * gi)
            v1 = fma(b2, v, sq if sq is not None else a * gi)
        else:
            m1 = fma(w1, gi, b1 * m)
            v1 = (sq + b2 * v) if sq is not None else fma(a, gi, b2 * v)
        if defect == "bc2_sqrt_multiplies":
            den = np.sqrt(v1) * bs + eps
        elif defect == "eps_inside_the_square_root":
            den = np.sqrt(v1 + eps) / bs
        else:
            den = np.sqrt(v1) / bs + eps
        p1 = p - ss * m1 / den
    assert p1.dtype == m1.dtype == v1.dtype == np.float32
    n = p.size
    keep = np.zeros(n, bool)                        # elements a defective walk never reaches
    if defect == "tail_not_updated":
        keep[n - n % 4:] = True
    if defect == "last_of_partial_chunk_dropped" and n % R.CHUNK:
        keep[-1] = True
    if defect == "second_chunk_starts_at_4095" and n > R.CHUNK:     # element 4095 is updated by both workgroups
        i = slice(R.CHUNK - 1, R.CHUNK)
        q = twin_step(p1[i], g[i], m1[i], v1[i], hyper, step, contraction)
        p1[i], m1[i], v1[i] = q
    return np.where(keep, p, p1), np.where(keep, m, m1), np.where(keep, v, v1)


DEFECTS = ["tail_not_updated", "last_of_partial_chunk_dropped", "second_chunk_starts_at_4095", "inv_not_applied", "bc2_sqrt_multiplies",
           "step_size_without_bias_correction", "eps_inside_the_square_root", "v_from_g_not_g_squared"]


def run_twin(name, contraction="none", defect=None):
    """the chained steps of one case on every tensor, each step from the twin's own state -> worst error / bound per output"""
    inp = R.case_inputs(name)
    worst = dict(m=0.0, v=0.0, p=0.0)
    for i in range(len(R.SIZES)):
        st = (inp["p"][i], inp["m"][i], inp["v"][i])
        for k, step in enumerate(inp["steps"]):
            new = twin_step(*st[:1], inp["grads"][k][i], *st[1:], inp["hypers"][k], step, contraction, defect)
            for key, val in R.judge(st, inp["grads"][k][i], new, inp["hypers"][k], step).items():
                worst[key] = max(worst[key], val)
            st = new
    return worst


def test_the_fp64_statement_is_torch_adam_in_float64():
    """five chained steps of torch.optim.Adam on float64 CPU tensors against `step_torch` with nothing rounded (cast=float): p, exp_avg
    and exp_avg_sq to 1e-12.  `step_abi` is the same arithmetic on other scalars."""
    rng = np.random.default_rng(0)
    sizes = [1, 5, 4097]
    lrs = [2e-3, 1e-3, 3e-3, 5e-4, 2e-3]
    for betas in ((0.9, 0.95), (0.9, 0.999)):
        ps = [torch.nn.Parameter(torch.from_numpy(0.02 * rng.standard_normal(n))) for n in sizes]
        opt = torch.optim.Adam(ps, lr=lrs[0], betas=betas, eps=1e-8)
        ref = [(p.detach().numpy().copy(), np.zeros(n), np.zeros(n)) for p, n in zip(ps, sizes)]
        for step, lr in enumerate(lrs, 1):
            opt.param_groups[0]["lr"] = lr
            gs = [R.GSCALE * np.exp(rng.uniform(-6, 0, n)) * rng.choice([-1.0, 1.0], n) for n in sizes]
            for p, g in zip(ps, gs):
                p.grad = torch.from_numpy(g.copy())
            opt.step()
            ref = [R.step_torch(*r[:1], g, *r[1:], lr, betas[0], betas[1], 1e-8, step, cast=float) for r, g in zip(ref, gs)]
            for p, r in zip(ps, ref):
                got = (p.detach().numpy(), opt.state[p]["exp_avg"].numpy(), opt.state[p]["exp_avg_sq"].numpy())
                for a, b in zip(got, r):
                    assert np.max(np.abs(a - b)) <= 1e-12 * np.max(np.abs(b)), (betas, step)
        assert all(float(opt.state[p]["step"]) == 5.0 for p in ps)
    # and with the fp32 values of the hyper-parameters as its doubles, the ABI's statement is that same function
    x = [rng.standard_normal(9) for _ in range(3)] + [rng.random(9)]
    h = [R.f32(t) for t in (2e-3, 0.9, 0.999, 1e-8)]
    for a, b in zip(R.step_abi(x[0], x[1], x[2], x[3], *h, 7, 0.5), R.step_torch(x[0], x[1], x[2], x[3], *h, 7, 0.5, cast=float)):
        assert np.max(np.abs(a - b)) <= 1e-12 * np.max(np.abs(b))


@pytest.mark.parametrize("contraction", ["none", "first", "second"])
@pytest.mark.parametrize("name", sorted(R.CASES))
def test_fp32_twin_sits_inside_the_bounds_on_the_gpu_tests_inputs(name, contraction):
    w = run_twin(name, contraction)
    print("adam twin worst error/bound  %-24s %-6s " % (name, contraction) + "  ".join("%s %.3f" % kv for kv in sorted(w.items())))
    assert all(val <= 1.0 for val in w.values()), (name, contraction, w)


@pytest.mark.parametrize("defect", DEFECTS)
def test_defective_twins_land_outside_the_bounds_on_the_gpu_tests_inputs(defect):
    """on the two cases that start at step 1 with gradients scaled by 1024 (the bias corrections differ from 1 there, and inv from 1; at
    step 1000 both corrections are 1 in fp32 and three of the defects are invisible by construction)"""
    for name in ("b95_inv1024th_step1", "b999_inv1024th_step1"):
        w = run_twin(name, "none", defect)
        print("adam defective twin  %-36s %-22s " % (defect, name) + "  ".join("%s %.3g" % kv for kv in sorted(w.items())))
        assert max(w.values()) > 1.0, (defect, name, w)


def test_distance_between_the_two_statements_is_printed_and_the_twin_sits_within_bound_plus_gap():
    """what tests/test_adam_gpu.py asserts of the kernels against torch's statement, here of the twin: within (bound + gap), the gap in u
    printed per beta pair.  Printed here: (0.9, 0.95) m 3.7 u, v 3.7 u, p 2.3 u; (0.9, 0.999) m 3.7 u, v 216.8 u, p 111.9 u."""
    for name in ("b95_inv1024th_step1", "b999_inv1024th_step1", "b999_inv1_step1000"):
        inp = R.case_inputs(name)
        gap, worst = {}, {}
        for i in range(len(R.SIZES)):
            st = (inp["p"][i], inp["m"][i], inp["v"][i])
            for k, step in enumerate(inp["steps"]):
                g, h = inp["grads"][k][i], inp["hypers"][k]
                new = twin_step(st[0], g, st[1], st[2], h, step)
                for key, val in R.torch_gap(st, g, new, h, step)[0].items():
                    gap[key] = max(gap.get(key, 0.0), val)
                for key, val in R.judge_against_torch(st, g, new, h, step).items():
                    worst[key] = max(worst.get(key, 0.0), val)
                st = new
        print("adam statements  %-22s gap to torch's statement  " % name + "  ".join("%s %.1f u" % kv for kv in sorted(gap.items())) +
              "   twin error / (bound + gap)  " + "  ".join("%s %.3f" % kv for kv in sorted(worst.items())))
        assert all(val <= 1.0 for val in worst.values()), (name, worst)


def test_inputs_plant_what_the_cases_promise():
    for name in R.CASES:
        inp = R.case_inputs(name)
        for i, n in enumerate(R.SIZES):
            z = R.zero_positions(n)
            assert all(np.all(gk[i][z] == 0) for gk in inp["grads"]) and np.all(inp["m"][i][z] == 0) and np.all(inp["v"][i][z] == 0)
            if n % R.CHUNK and n > 1:                 # the carried tail
                assert all(abs(gk[i][-1]) >= 99 * np.abs(gk[i][:-1]).max() for gk in inp["grads"]) and n - 1 not in z
            gi = np.abs(inp["grads"][0][i].astype(np.float64) * inp["hypers"][0][4])
            assert gi[gi > 0].min() >= R.GSCALE * np.exp(-6) * 0.99           # normal range throughout: (1 - beta2) g^2 >= 6e-13
    assert len({h[0] for h in R.case_inputs("b95_inv1_step1")["hypers"]}) == len(R.LRS)
    assert sum(len(R.zero_positions(n)) for n in R.SIZES) > 40000 and len(R.zero_positions(1)) == 0


def test_host_scalars_sit_inside_their_error_terms_and_the_distance_to_torchs_is_printed():
    """swv2_adam_*'s step_size and bc2_sqrt (fp32 arithmetic on glibc's powf, and on numpy's power for comparison) against the ABI
    statement's exact scalars: within e1, e2 of adam_reference for steps 1 .. 3000.  Against torch's scalars (doubles rounded once) the
    distance is printed in u: that is the cost of a float ABI, bounded by nothing here.
    Printed by this test (u = 2^-24, largest over the steps; glibc's powf and numpy's power give the same figures):
        (0.9, 0.95)   step_size 5.3 u (step 3)    bc2_sqrt   2.5 u (step 21)
        (0.9, 0.999)  step_size 5.3 u (step 3)    bc2_sqrt 163.6 u (step 2: 1e-5 relative)"""
    for betas in ((0.9, 0.95), (0.9, 0.999)):
        for powf, label in ((c_powf, "glibc powf"), (np_powf, "numpy power")):
            worst = dict(e1=0.0, e2=0.0)
            far = dict(step_size=(0.0, 0), bc2_sqrt=(0.0, 0))
            for step in range(1, 3001):
                ss, bs = host_scalars(2e-3, betas[0], betas[1], step, powf)
                s, t = R.abi_scalars(2e-3, betas[0], betas[1], 1e-8, step), R.torch_scalars(2e-3, betas[0], betas[1], 1e-8, step)
                e1, e2 = R.scalar_errors(betas[0], betas[1], step)
                worst["e1"] = max(worst["e1"], abs(float(ss) - s["step_size"]) / s["step_size"] / e1)
                worst["e2"] = max(worst["e2"], abs(float(bs) - s["bc2_sqrt"]) / s["bc2_sqrt"] / e2)
                for k, val in (("step_size", float(ss)), ("bc2_sqrt", float(bs))):
                    dist = abs(val - t[k]) / t[k] / R.U
                    if dist > far[k][0]:
                        far[k] = (dist, step)
            print("adam host scalars %s %-11s: error / allowed  step_size %.3f  bc2_sqrt %.3f;  distance to torch's  step_size %.1f u (step %d)  "
                  "bc2_sqrt %.1f u (step %d)" % (betas, label, worst["e1"], worst["e2"], *far["step_size"], *far["bc2_sqrt"]))
            assert worst["e1"] <= 1.0 and worst["e2"] <= 1.0
    # the kernel's own 1.f - beta against torch's fp32(1 - beta): exact for the ABI statement, 1.3e-5 away from torch's at 0.999
    assert float(F(1) - F(0.999)) == 1.0 - R.f32(0.999) and abs(float(F(1) - F(0.999)) / R.f32(1 - 0.999) - 1) > 1e-5


def test_ctypes_item_follows_the_header_and_refusals_need_no_gpu():
    assert [f[0] for f in L.AdamItem._fields_] == header_struct_fields("swv2_adam_item") == ["p", "g", "m", "v", "n"]
    assert ctypes.sizeof(L.AdamItem) == 40
    lib = L.load()
    assert lib.swv2_adam_chunk() == R.CHUNK
    P = 4096                                         # any non-null value: never dereferenced by a refused call
    multi = lambda items=P, chunks=P, nc=3, step=1: lib.swv2_adam_multi(items, chunks, nc, 1e-3, 0.9, 0.95, 1e-8, step, 1.0, None)
    flat = lambda p=P, g=P, m=P, v=P, n=8, step=1: lib.swv2_adam_step(p, g, m, v, n, 1e-3, 0.9, 0.95, 1e-8, step, 1.0, None)
    for call, word in ((lambda: multi(items=None), b"adam_multi"), (lambda: multi(chunks=None), b"adam_multi"), (lambda: multi(nc=0), b"adam_multi"),
                       (lambda: multi(step=0), b"adam_multi"), (lambda: flat(p=None), b"adam_step"), (lambda: flat(g=None), b"adam_step"),
                       (lambda: flat(m=None), b"adam_step"), (lambda: flat(v=None), b"adam_step"), (lambda: flat(n=0), b"adam_step"),
                       (lambda: flat(step=0), b"adam_step"), (lambda: flat(step=-3), b"adam_step")):
        assert call() == -1
        assert word in lib.swv2_last_error(), lib.swv2_last_error()
