"""GPU (-m gpu): swv2_adam_multi and swv2_adam_step (csrc/rowops.hip) through the C ABI, element by element against the fp64 statement of
tests/adam_reference.py, whose docstring derives every bound used here; then utils/optim.HipAdam against the same statement, parameter by
parameter from the optimizer's own state.

Every p, g, m, v sits between 16-byte guards of a sentinel; tensor 5 has all four buffers starting one element in (the scalar walk over
four chunks, one of them partial), tensor 2 only its gradient (one unaligned pointer of four leaves the 16-byte walk).  Steps are chained,
each from the state the kernel itself left, and p' is judged from the kernel's own stored m', v'.  Each case prints its worst error / bound
per output (-s); those figures, the bit-equality notes and the distances to torch.optim.Adam below are records of one MI355X run with
this compiler (LABNOTES, "Adam and the remaining row kernels element by element"), asserted nowhere.

Records (MI355X):
    worst error / bound  swv2_adam_multi   m 0.967  v 0.980  p 0.995   (8 cases x 4 steps x 7 tensors)
                         swv2_adam_step    m 0.956  v 0.985  p 0.972   (the grid-cap case included)
                         HipAdam           kernel steps m 0.933  v 0.493  p 0.979;  torch steps m 0.485  v 0.929  p 0.902
    distance between the ABI's statement and torch.optim.Adam's on these inputs (u = 2^-24, relative to |beta1 m| + |(1 - beta1) g^|, to v'
    and to the size of the update; the same for both entry points):
                         betas (0.9, 0.95)   m 3.7 u  v   3.7 u  p   2.3 u
                         betas (0.9, 0.999)  m 3.7 u  v 216.8 u  p 111.9 u     (v: 1.f - 0.999f against fp32(1 - 0.999), 1.3e-5)
    swv2_adam_multi's 16-byte walk against swv2_adam_step on one aligned tensor of 3 * 4096 + 5 elements, same state: NOT bit-equal,
                         m' differs in 726, v' in 2456, p' in 654 of the 12 293 elements (each by a last-place rounding, inside the bounds)
    swv2_adam_multi's 16-byte walk against its scalar walk (the same tensor one element into its buffers): NOT bit-equal, the same
                         726 / 2456 / 654 elements: the scalar walk and swv2_adam_step agree bit for bit (0 elements differ), the 16-byte
                         walk contracts otherwise
"""
import ctypes

import numpy as np
import pytest
import torch

from swin_v2_weather_amd import _lib as L
from tests import adam_reference as R
from tests.plane_harness import dev, lib  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

CHUNK, SIZES = R.CHUNK, R.SIZES
SENT = -123456.75            # guard value around every p, g, m, v
GUARD = 4                    # guard elements on each side: 16 bytes, so the interior keeps the buffer's alignment
SHIFT = {5: dict(p=1, g=1, m=1, v=1), 2: dict(g=1)}


class Bed:
    """p, g, m, v of a list of tensors between guards and the launch tables of swv2_adam_multi over all of them"""

    def __init__(self, dev, sizes, shift=None):
        assert ctypes.sizeof(L.AdamItem) == 40
        self.dev, self.sizes = dev, sizes
        self.buf, self.view = {}, {}
        for i, n in enumerate(sizes):
            for k in "pgmv":
                s = (shift or {}).get(i, {}).get(k, 0)
                b = torch.full((n + 2 * GUARD + s,), SENT, dtype=torch.float32, device=dev)
                self.buf[k, i], self.view[k, i] = b, b[GUARD + s:GUARD + s + n]
                assert self.view[k, i].data_ptr() % 16 == 4 * s
        rows = [[self.view[k, i].data_ptr() for k in "pgmv"] + [n] for i, n in enumerate(sizes)]
        pairs = [(i, c) for i, n in enumerate(sizes) for c in range((n + CHUNK - 1) // CHUNK)]
        self.n_chunks = len(pairs)
        self.items = torch.tensor(rows, dtype=torch.int64).to(dev)           # 5 x 8 bytes = one swv2_adam_item per row
        self.chunks = torch.tensor(pairs, dtype=torch.int32).to(dev)

    def put(self, k, i, x):
        self.view[k, i].copy_(torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)))

    def get(self, k, i):
        return self.view[k, i].cpu().numpy().copy()

    def state(self, i):
        return tuple(self.get(k, i) for k in "pmv")

    def guards_intact(self):
        for (k, i), b in self.buf.items():
            s = b.numel() - self.sizes[i] - 2 * GUARD
            b = b.cpu()
            if not (bool((b[:GUARD + s] == SENT).all()) and bool((b[GUARD + s + self.sizes[i]:] == SENT).all())):
                return False
        return True

    def multi(self, lib, hyper, step):
        lr, b1, b2, eps, inv = hyper
        L.check(lib.swv2_adam_multi(self.items.data_ptr(), self.chunks.data_ptr(), self.n_chunks, lr, b1, b2, eps, step, inv,
                                    torch.cuda.current_stream(self.dev).cuda_stream), "swv2_adam_multi")
        torch.cuda.synchronize(self.dev)

    def flat(self, lib, hyper, step, i=0):
        lr, b1, b2, eps, inv = hyper
        L.check(lib.swv2_adam_step(*(self.view[k, i].data_ptr() for k in "pgmv"), self.sizes[i], lr, b1, b2, eps, step, inv,
                                   torch.cuda.current_stream(self.dev).cuda_stream), "swv2_adam_step")
        torch.cuda.synchronize(self.dev)


def run_chain(dev, lib, name, sizes, shift, entry, label, n_steps=None):
    """the chained steps of one case through one entry point ("multi" / "flat"); asserts everything the module docstring lists and returns
    (worst error / bound per output, largest statement gap per output in u)"""
    inp = R.case_inputs(name, sizes)
    bed = Bed(dev, sizes, shift)
    for i in range(len(sizes)):
        for k in "pmv":
            bed.put(k, i, inp[k][i])
    launch = (lambda h, s: bed.multi(lib, h, s)) if entry == "multi" else (lambda h, s: bed.flat(lib, h, s))
    worst, wtorch, gap = {}, {}, {}
    steps = list(zip(inp["steps"], inp["hypers"], inp["grads"]))[:n_steps]
    for k, (step, hyper, grads) in enumerate(steps):
        for i in range(len(sizes)):
            bed.put("g", i, grads[i])
        old = [bed.state(i) for i in range(len(sizes))]
        launch(hyper, step)
        assert bed.guards_intact(), "a guard was written"
        new = [bed.state(i) for i in range(len(sizes))]
        for i, n in enumerate(sizes):
            assert np.array_equal(bed.get("g", i).view(np.uint32), grads[i].view(np.uint32)), "gradient %d was written" % i
            z = R.zero_positions(n)
            assert np.array_equal(new[i][0][z].view(np.uint32), inp["p"][i][z].view(np.uint32)), "p moved where g = 0 and v = 0"
            assert np.all(new[i][1][z] == 0) and np.all(new[i][2][z] == 0)
            for key, val in R.judge(old[i], grads[i], new[i], hyper, step).items():
                worst[key] = max(worst.get(key, 0.0), val)
            for key, val in R.judge_against_torch(old[i], grads[i], new[i], hyper, step).items():
                wtorch[key] = max(wtorch.get(key, 0.0), val)
            for key, val in R.torch_gap(old[i], grads[i], new[i], hyper, step)[0].items():
                gap[key] = max(gap.get(key, 0.0), val)
            if n > 1:
                assert not np.array_equal(new[i][0], old[i][0])
        if k == 1:                     # the same step again from the same state: the same bits everywhere
            for i in range(len(sizes)):
                for key, x in zip("pmv", old[i]):
                    bed.put(key, i, x)
            launch(hyper, step)
            assert bed.guards_intact()
            for i in range(len(sizes)):
                for a, b in zip(bed.state(i), new[i]):
                    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), "a second run differs"
    print("adam worst error/bound  %-10s %-24s " % (label, name) + "  ".join("%s %.3f" % kv for kv in sorted(worst.items())) +
          "   against torch's statement (bound + gap) " + "  ".join("%s %.3f" % kv for kv in sorted(wtorch.items())) +
          "   gap to torch's statement " + "  ".join("%s %.1f u" % kv for kv in sorted(gap.items())))
    assert set(worst) == {"m", "v", "p"}
    for key in worst:
        assert worst[key] <= 1.0, (label, name, key, worst[key])
        assert wtorch[key] <= 1.0, (label, name, key, wtorch[key])
    return worst, gap


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_adam_multi_against_fp64(dev, lib, name):
    run_chain(dev, lib, name, SIZES, SHIFT, "multi", "multi")


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_adam_step_against_fp64(dev, lib, name):
    """the same checks on one flat buffer: three whole rounds of 256 threads x 16 and a ragged end"""
    run_chain(dev, lib, name, [3 * CHUNK + 5], None, "flat", "step")


def test_adam_step_beyond_the_grid_cap(dev, lib):
    """n = 8192 * 256 + 5: the grid is capped at 8192 workgroups of 256 threads, so five threads take a second element (8 MB per array)"""
    run_chain(dev, lib, "b999_inv1024th_step1", [R.GRID_CAP + 5], None, "flat", "step>cap", n_steps=2)


def test_entry_points_and_walks_on_the_same_tensor(dev, lib):
    """One tensor of 3 * 4096 + 5 elements from one state through swv2_adam_multi aligned (the 16-byte walk and a scalar tail), through
    swv2_adam_step, and through swv2_adam_multi one element into its buffers (the scalar walk): each within the bounds.  How many elements
    differ between them is printed and recorded in the module docstring; the compiler is free to contract b1 m + (1 - b1) g differently on
    each walk (csrc/rowops.hip says it does), so bit equality is a record of this compiler and not a contract."""
    n = 3 * CHUNK + 5
    inp = R.case_inputs("b999_inv1_step1000", [n])
    hyper, step, g = inp["hypers"][0], inp["steps"][0], inp["grads"][0][0]
    old = (inp["p"][0], inp["m"][0], inp["v"][0])
    out = {}
    for label, shift, entry in (("multi", None, "multi"), ("step", None, "flat"), ("multi_scalar", {0: dict(p=1, g=1, m=1, v=1)}, "multi")):
        bed = Bed(dev, [n], shift)
        for k, x in zip("pmvg", old + (g,)):
            bed.put(k, 0, x)
        (bed.multi if entry == "multi" else bed.flat)(lib, hyper, step)
        assert bed.guards_intact()
        out[label] = bed.state(0)
        w = R.judge(old, g, out[label], hyper, step)
        assert all(val <= 1.0 for val in w.values()), (label, w)
    for one, other in (("multi", "step"), ("multi", "multi_scalar"), ("step", "multi_scalar")):
        diff = {k: int(np.sum(a.view(np.uint32) != b.view(np.uint32))) for k, a, b in zip("pmv", out[one], out[other])}
        print("adam bits  %-5s against %-12s of %d elements differ:  " % (one, other, n) + "  ".join("%s' %d" % (k, diff[k]) for k in "mvp"))


# ---------------------------------------------------------------------------------------------------------------
# HipAdam
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("betas", [(0.9, 0.95), (0.9, 0.999)], ids=["b95", "b999"])
def test_hipadam_parameter_by_parameter_against_fp64(dev, lib, betas):
    """Five steps of HipAdam over three groups, gradients scaled by 128 (grad_inv_scale = 1 / 128), each parameter judged from the state
    the optimizer itself held before the step, with the kernels' bounds:
      group 0 (lr 2e-3, then 1e-3 from step 2): A [4097], B [5] and C [33]; C gets its first gradient at step 3.  Steps 1, 2 run the
              kernel; from step 3 the step counters disagree and the group takes torch's path, C at its own step 1
      group 1 (lr 5e-4, then 2e-4 from step 4): D [3 * 4096 + 5], the kernel throughout
      group 2 (lr 1e-3): E, a transposed (non-dense) parameter: torch's path throughout
    A kernel step is held to the ABI's statement, a torch step to torch's statement (its op sequence rounds no more often than the
    kernel's, so the same bounds hold around its own scalars).  Gradient tensors are allocated anew before every step but the second
    (pointer rows change, the table is uploaded again), which writes into the tensors of the first."""
    from swin_v2_weather_amd.utils.optim import HipAdam
    rng = np.random.default_rng(17)
    inv, scale = 1.0 / 128, 128.0
    mk = lambda n: torch.nn.Parameter(torch.from_numpy(R.draw_p(rng, n)).to(dev))
    A, B, C_, D = mk(4097), mk(5), mk(33), mk(3 * CHUNK + 5)
    E = torch.nn.Parameter(torch.from_numpy(R.draw_p(rng, 48).reshape(6, 8)).to(dev).t())
    assert not E.is_contiguous()
    params = [A, B, C_, D, E]
    opt = HipAdam([dict(params=[A, B, C_], lr=2e-3), dict(params=[D], lr=5e-4), dict(params=[E], lr=1e-3)], betas=betas, eps=R.EPS)
    group_of = {id(p): gi for gi, g_ in enumerate(opt.param_groups) for p in g_["params"]}
    taken = {id(p): 0 for p in params}
    keepalive, worst = [], {}
    flat = lambda t: t.detach().cpu().numpy().ravel().copy()
    for it in range(1, 6):
        if it == 2:
            opt.param_groups[0]["lr"] = 1e-3
        if it == 4:
            opt.param_groups[1]["lr"] = 2e-4
        live = [p for p in params if p is not C_ or it >= 3]
        for p in live:
            g = torch.from_numpy(R.draw_g(rng, p.numel(), R.GSCALE * scale).reshape(tuple(p.shape))).to(dev)
            if it == 2:
                p.grad.copy_(g)
            else:
                keepalive.append(p.grad)
                p.grad = g
        old = {id(p): (flat(p), flat(opt.state[p]["exp_avg"]) if opt.state[p] else np.zeros(p.numel(), np.float32),
                       flat(opt.state[p]["exp_avg_sq"]) if opt.state[p] else np.zeros(p.numel(), np.float32), flat(p.grad),
                       int(opt.state[p]["step"]) if opt.state[p] else 0) for p in live}
        rows0 = opt._tables[1].rows if 1 in opt._tables else None
        opt.step(grad_inv_scale=inv)
        torch.cuda.synchronize(dev)
        on_kernel = {0: it <= 2, 1: True, 2: False}
        assert {gi: gi in opt._tables for gi in range(3)} == on_kernel, (it, sorted(opt._tables))
        assert (opt._tables[1].rows != rows0) == (it != 2), "the pointer rows of group 1 and the re-allocation of its gradients disagree"
        for p in live:
            gi = group_of[id(p)]
            p0, m0, v0, g0, s0 = old[id(p)]
            taken[id(p)] += 1
            assert int(opt.state[p]["step"]) == s0 + 1 == taken[id(p)]
            if on_kernel[gi]:
                assert np.array_equal(flat(p.grad).view(np.uint32), g0.view(np.uint32)), "the kernel's path wrote a gradient"
            hyper = (opt.param_groups[gi]["lr"], betas[0], betas[1], R.EPS, inv)
            new = (flat(p), flat(opt.state[p]["exp_avg"]), flat(opt.state[p]["exp_avg_sq"]))
            for key, val in R.judge((p0, m0, v0), g0, new, hyper, s0 + 1, "abi" if on_kernel[gi] else "torch").items():
                tag = ("kernel " if on_kernel[gi] else "torch ") + key
                worst[tag] = max(worst.get(tag, 0.0), val)
    print("adam worst error/bound  HipAdam %s  " % (betas,) + "  ".join("%s %.3f" % kv for kv in sorted(worst.items())))
    assert set(worst) == {"kernel m", "kernel v", "kernel p", "torch m", "torch v", "torch p"}
    assert all(val <= 1.0 for val in worst.values()), worst
    sd = opt.state_dict()["state"]
    assert {k: float(s["step"]) for k, s in sd.items()} == {0: 5.0, 1: 5.0, 2: 3.0, 3: 5.0, 4: 5.0}
