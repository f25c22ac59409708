"""GPU (-m gpu): every weight-gradient path, element by element, against fp64.

A block's four weight gradients (fc2, fc1, proj, qkv and their bias gradients) run on one of four kernel families:
  * slab        -- gemm_tn_slab.hip, swv2_block_wgrad(items, 0, ...) for the block shapes of SL_SETS (C 128 / 192);
                   per-workgroup partial tiles in bf16, folded in fp32
  * grouped     -- gemm_tn_group_kernel, swv2_block_wgrad(items, 8 / 16, ...) (and slices 0 at every other width)
  * single      -- gemm_tn_kernel, swv2_linear_wgrad_ws per product, fp32 atomics (no workspace) or per-slice partials
  * wide        -- gemm_tn_wide_kernel (gemm_tn_wide.hip), swv2_linear_wgrad_ws with SWV2_GEMM_WIDE=1 when N, K >= 512 (multiples of 256),
                   M >= 8192 and a multiple of 32
The items use the block's operand kinds: 0 fc2 (BF16, BF16_GELU), 1 fc1 (BF16, F32), 2 proj (BF16, HEADS with kmap),
3 qkv (HEADS with nmap, F32 gathered through rowidx with -1 rows).

Part 1 (exact): integer operands for which no rounding can happen anywhere.  dY and X rows are one-hot (every row
reaches exactly one output element, so a dropped, doubled or misplaced row changes that element), the products are
+-1 .. +-64 and no output element sums more than 256 in absolute value: every partial sum over ANY subset of rows is an
integer of magnitude <= 256, exact in bf16 and fp32, whatever slice plan or partial precision a path uses.  Every path
must then equal the fp64 reference bit for bit (torch.equal), on every element of dW and db, accumulated onto an integer
baseline, with guard rows around dW / db that no launch may touch.

Part 2 (random data, per element): X columns scaled from 1e-4 to 1 and dY columns from 1e-3 to 1, so that most dW
entries are small.  The reference is fp64 of exactly what the kernels read (X rounded to bf16, the GELU operand as the
library's own bf16(GELU(pre)), read from the library by the gelu_lut fixture).  With A[n, k] = sum_m |dY[m, n]| |X[m, k]|:
  * fp32-partial paths (single, grouped, wide):  |dW - ref| <= C32 * A
  * slab (bf16 partials):                        |dW - ref| <= 2^-8 * A  (each partial rounded once: <= 2^-9 of itself)
  * bias gradients: the same with A = sum_m |dY[m, n]| (every path keeps its bias partials in fp32: C32)

Every result is filed under a path name, and the error bar follows from the name (_family); before each launch the library is asked
which kernel it will run for exactly these arguments (swv2_block_wgrad_kernel / swv2_linear_wgrad_kernel), and the answer must be
the one the name claims: a slab that declines (workspace, shape, CU count) fails the test instead of borrowing the looser bar.
The slab's row slices come from the library too (swv2_block_wgrad_plan, the function the launch switches on): the slice-aligned
cancellation test builds its data on them, and one case checks that planning for "the current device" is planning for its CU count.

Conventions of the product the operands follow (swv2_block_bwd): the padded rows t >= L of a window are zero in the
head-major operands and in the proj product's dY (their bias gradient counts every row); the padded head columns
(j >= head dim) hold anything -- here large finite values -- and are dropped through nmap / kmap.
"""
import ctypes
import math

import pytest
import torch

from tests.mlp_reference import bf16_bits_all, gelu64, library_gelu_lut, lut_of

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
F64 = torch.float64
L_WIN, LP = 162, 176                 # one 9 x 18 window; swv2_attn_geometry(162, 16 / 24 / 64) pads it to 176 rows
BIG = 2.0 ** 100                     # padded head columns: finite, exact in bf16, far above every real value
GUARD = 12345.0                      # guard rows / entries around dW and db
# fp32-partial paths: |dW - ref| <= C32 * A per element.  Measured on an MI355X over every case of
# test_random_operands_per_element_bound: worst dW 1.29e-7 A (single-product tile kernel, atomics and workspace), 9.8e-8 A
# (grouped), 1.7e-8 A (wide); worst db 1.3e-8 (the slab's fp32 bias partials included).  2^-20 = 9.5e-7 leaves a margin of 7x.
C32 = 2.0 ** -20
# slab: each bf16 partial carries <= 2^-9 of its own magnitude, so 2^-8 A holds by construction.  Measured: 1.4e-3 A on random
# data, 1.5e-3 A when every slice's partial is coherent and the total cancels (test_slab_on_cancelling_data)
C_SLAB = 2.0 ** -8

# block shapes: the two slab shape sets (gemm_tn_slab.hip SL_SETS) and one width at which the wide kernel takes the
# fp32-X, head-major and gathered products (no slab set: swv2_block_wgrad(items, 0) runs the grouped tile kernel)
SETS = {
    "c128": dict(C=128, hid=512, h=8, hd=16, DP=16, slab=True),
    "c192": dict(C=192, hid=768, h=8, hd=24, DP=32, slab=True),
    "c512": dict(C=512, hid=1024, h=8, hd=64, DP=64, slab=False),
}

# Row counts (M = token rows of items 0 / 1; Bw = windows of items 2 / 3, which have Bw * 176 head-major rows).  The slab's
# planner (sl_plan) splits sl_cus() workgroups over the four products in proportion to their bytes, S = min(sl, T) row slices
# of T = ceil(rows / SR) stages (SR = 32; 64 for proj at C 128), then hands the rounding remainder out one slice at a time.
# Branches reached at 256 CUs (an MI355X), per shape set [c128 | c192]; S = slices of items 0..3 (swv2_block_wgrad_plan reports them;
# tests/test_wgrad_plan_host.py pins four of these rows and sweeps every CU count):
#   (162, 1)      one window of one sample: all four clamped to S = T = [6 6 3 6 | 6 6 6 6], remainder loop finds no product to grow
#   (324, 2)      two windows: all clamped, S = T = [11 11 6 11 | 11 11 11 11]
#   (31, 1)       SR - 1: items 0 / 1 a SINGLE ragged stage (T = 1, S = 1); all clamped
#   (32, 1)       SR: a single full stage; all clamped
#   (33, 1)       SR + 1: two stages, the second holding one row; all clamped
#   (4383, 27)    SR * 137 - 1, odd window count: unclamped [91 70 25 70 | 41 35 20 42], c192 takes two slices back from proj
#   (4384, 27)    SR * 137: same plan, no ragged stage
#   (4385, 27)    SR * 137 + 1: T = 138 with a one-row last stage
#   (4374, 27)    ragged, as in the block tests: unclamped, no remainder at c128; at c192 [40 35 22 42], no remainder
#   (4374, 1)     items 2 / 3 tiny: c128 clamps fc2 to T = 137 and the remainder loop GROWS proj, qkv, fc1 ([137 112 2 5]);
#                 c192 takes one slice from qkv and gives one to proj ([67 58 2 2])
#   (162, 800)    items 0 / 1 tiny beside full-size windows: their share rounds to 0 slices (raised to 1), remainder loop SHRINKS proj
#   (129600, 800) full size: one block at local batch 2 (180 x 360 patches, 800 windows), no remainder
CASES = [(162, 1), (324, 2), (31, 1), (32, 1), (33, 1), (4383, 27), (4384, 27), (4385, 27), (4374, 27), (4374, 1), (162, 800),
         (129600, 800)]
WIDE_CASES = [(8192, 48), (8224, 50)]          # wide kernel: M and Bw * 176 multiples of 32, >= 8192
SINGLE = [(1, False), (7, False), (64, False), (1, True), (7, True), (64, True)]      # (splits, workspace)
GELU_INT = [3.0, 4.0, 5.0, 6.0, 7.0, 8.0, 9.0, 10.0, 11.0, 12.0, 13.0, 14.0, 15.0, 16.0, 24.0, 32.0]   # bf16(GELU(x)) == x
GELU_ZERO = [0.0, -20.0]                                                            # bf16(GELU(x)) == 0


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def K():
    from swin_v2_weather_amd import _lib as L, ops
    L.load()
    return dict(L=L, ops=ops)


@pytest.fixture(scope="module")
def gelu_lut(dev, K):
    """the library's own bf16(GELU(x)) for all 65 536 bf16 patterns x, as fp32 [65536] indexed by the pattern (shared with the fused
    MLP's tests: tests/mlp_reference.py)"""
    return library_gelu_lut(K["ops"], K["L"], dev)


# ---------------------------------------------------------------------------------------------------------------
# The GELU operand: the library against fp64 erf-GELU on every bf16 input
# ---------------------------------------------------------------------------------------------------------------
def test_gelu_operand_on_every_bf16_input(dev, K, gelu_lut):
    """bf16(GELU(x)) of the GELU-on-load operand (table for 2^-14 <= |x| < 16, the erf_parts formula elsewhere) against fp64
    erf-GELU for all 65 536 bf16 patterns.  On [-3, 3] within one bf16 ulp.  Below -3, 1 + erf(x / sqrt 2) cancels in fp32
    (PyTorch's own fp32 GELU cancels the same way) and the rational erf's absolute error (1.5e-7) becomes relative: the bar
    there is 2^-8 |ref| + 2^-21 |x| (an absolute error of 4.8e-7 on 1 + erf, 2.4 x the fp32 + approximation budget)."""
    pats = bf16_bits_all(dev)
    x = pats.double()
    got = gelu_lut.double()
    ref = gelu64(pats.float())
    fin = torch.isfinite(x)
    # non-finite inputs: +inf -> +inf, -inf -> NaN (-inf * 0, as fp64 erf-GELU), every NaN -> NaN
    pinf, ninf = x == math.inf, x == -math.inf
    assert got[pinf].item() == math.inf and torch.isnan(got[ninf]).all() and torch.isnan(ref[ninf]).all()
    assert torch.isnan(got[torch.isnan(x)]).all()
    assert torch.isfinite(got[fin]).all()
    xf, gf, rf = x[fin], got[fin], ref[fin]
    # every output is a bf16 value (the operand the MFMAs read)
    assert torch.equal(gf.float().to(BF).double(), gf)
    err = (gf - rf).abs()
    # distance in bf16 ulps from bf16(fp64 GELU), the correctly rounded operand
    rq = rf.to(BF).double()
    ulps = (gf - rq).abs() / torch.exp2(torch.floor(torch.log2(rq.abs().clamp_min(2.0 ** -126))) - 7)
    core = xf.abs() <= 3
    sub = xf.abs() < 2.0 ** -126
    tail = ~core
    band = (xf >= -4) & (xf < -3)
    print(f"\n[gelu] [-3, 3]: worst {float(ulps[core & ~sub].max()):.3g} ulps, {int((ulps[core & ~sub] > 0).sum())} of "
          f"{int((core & ~sub).sum())} inputs not correctly rounded; [-4, -3): worst {float(ulps[band].max()):.3g} ulps; outside [-3, 3] "
          f"worst err / (2^-8 |ref| + 2^-21 |x|) {float((err[tail] / (2.0 ** -8 * rf[tail].abs() + 2.0 ** -21 * xf[tail].abs())).max()):.3g}; "
          f"subnormal inputs worst |err| {float(err[sub].max()):.3g}")
    # +-0 -> 0; subnormal inputs: within the smallest normal (fp32 denormals may flush in the formula path)
    assert torch.equal(gf[xf == 0], torch.zeros_like(gf[xf == 0]))
    assert float(err[sub].max()) <= 2.0 ** -126
    assert float(ulps[core & ~sub].max()) <= 1.0
    bar = 2.0 ** -8 * rf.abs() + 2.0 ** -21 * xf.abs()
    assert bool((err[tail] <= bar[tail]).all()), float((err[tail] / bar[tail]).max())
    # the table's edges and what lies just outside them (formula fallback): 2^-14 and the bf16 below it, the last entry below 16,
    # 16 itself and beyond -- all already in the sweep, named here
    edges = torch.tensor([2.0 ** -14, 2.0 ** -14 - 2.0 ** -22, 16.0 - 2.0 ** -4, 16.0, 16.125, 1e4, 3e38], dtype=torch.float32, device=dev)
    for v in torch.cat([edges, -edges]).to(BF):
        g_ = float(lut_of(gelu_lut, v.view(1)))
        r_ = float(gelu64(v.float().view(1)))
        assert abs(g_ - r_) <= 2.0 ** -8 * abs(r_) + 2.0 ** -21 * abs(float(v)), (float(v), g_, r_)
    # the pre-activations of the exact cases below: their bf16(GELU) is an integer in fp64 and in the library
    ints = torch.tensor(GELU_INT + GELU_ZERO, dtype=BF, device=dev)
    want = torch.tensor(GELU_INT + [0.0, 0.0], dtype=F64, device=dev)
    assert torch.equal(gelu64(ints.float()).float().to(BF).double(), want)
    assert torch.equal(lut_of(gelu_lut, ints).double(), want)


# ---------------------------------------------------------------------------------------------------------------
# Operands of the four products
# ---------------------------------------------------------------------------------------------------------------
class Prod:
    """one product: its two operands (library form), the dense logical operands as the kernels read them (fp64: dY [R][N],
    X [R][K], after GELU / bf16 rounding / gather), the output maps and the dW / db buffers (with guard rows)"""

    def __init__(self, dy_op, x_op, dyd, xd, nmap, kmap, nout, kout, keep):
        self.dy_op, self.x_op, self.dyd, self.xd = dy_op, x_op, dyd, xd
        self.nmap, self.kmap, self.nout, self.kout, self.keep = nmap, kmap, nout, kout, keep

    def buffers(self, dev, base_w, base_b):
        bw = torch.full((self.nout + 2, self.kout), GUARD, dtype=torch.float32, device=dev)
        bb = torch.full((self.nout + 8,), GUARD, dtype=torch.float32, device=dev)
        bw[1:self.nout + 1] = base_w
        bb[4:self.nout + 4] = base_b
        return bw, bb, bw[1:self.nout + 1], bb[4:self.nout + 4]

    def reference(self, base_w, base_b):
        """(dW, db, A, Ab) in fp64 in the OUTPUT index space (nmap / kmap applied; dropped columns discarded)"""
        dev = self.dyd.device
        vn = (self.nmap >= 0).nonzero().flatten() if self.nmap is not None else torch.arange(self.dyd.shape[1], device=dev)
        vk = (self.kmap >= 0).nonzero().flatten() if self.kmap is not None else torch.arange(self.xd.shape[1], device=dev)
        on = self.nmap[vn].long() if self.nmap is not None else vn
        ok = self.kmap[vk].long() if self.kmap is not None else vk
        dy, x = self.dyd[:, vn], self.xd[:, vk]
        out = [torch.zeros(self.nout, self.kout, dtype=F64, device=dev) for _ in range(2)]
        outb = [torch.zeros(self.nout, dtype=F64, device=dev) for _ in range(2)]
        out[0][on.view(-1, 1), ok.view(1, -1)] = dy.T @ x
        out[1][on.view(-1, 1), ok.view(1, -1)] = dy.abs().T @ x.abs()
        outb[0][on] = dy.sum(0)
        outb[1][on] = dy.abs().sum(0)
        return out[0] + base_w.double(), outb[0] + base_b.double(), out[1], outb[1]


def _colscale(n, lo, hi, g, dev):
    return torch.exp(torch.empty(n, device=dev, dtype=F64).uniform_(math.log(lo), math.log(hi), generator=g))


def _dense_values(R, N, K, valid_rows, vn, vk, mode, xvals, g, dev, sign=None):
    """dense logical dY [R][N] and X [R][K] (fp64, zero outside valid rows / columns).  exact: one-hot rows, the (n, k) pairs
    dealt from a random permutation so that no pair is hit more than ceil(rows / pairs) times; random: scaled normals."""
    dy = torch.zeros(R, N, dtype=F64, device=dev)
    x = torch.zeros(R, K, dtype=F64, device=dev)
    nv = valid_rows.numel()
    if mode == "exact":
        P = vn.numel() * vk.numel()
        perm = torch.randperm(P, generator=g, device=dev)
        p = perm[torch.arange(nv, device=dev) % P]
        n, k = vn[p % vn.numel()], vk[p // vn.numel()]
        mag = torch.randint(1, 3, (nv,), generator=g, device=dev).double()
        sg = torch.randint(0, 2, (nv,), generator=g, device=dev).double() * 2 - 1
        dy[valid_rows, n] = mag * sg
        xv = torch.tensor(xvals, dtype=F64, device=dev)
        x[valid_rows, k] = xv[torch.randint(0, len(xvals), (nv,), generator=g, device=dev)]
        assert int(-(-nv // P)) * 2 * float(xv.abs().max()) <= 256          # every |partial| <= 256 (the exactness premise)
    else:
        dy[valid_rows.view(-1, 1), vn.view(1, -1)] = (torch.randn(nv, vn.numel(), generator=g, device=dev, dtype=F64) *
                                                      _colscale(vn.numel(), 1e-3, 1.0, g, dev))
        x[valid_rows.view(-1, 1), vk.view(1, -1)] = (torch.randn(nv, vk.numel(), generator=g, device=dev, dtype=F64) *
                                                     _colscale(vk.numel(), 1e-4, 1.0, g, dev))
        if sign is not None:                # cancellation: |X|, |dY| with a sign per row
            x = x.abs()
            dy = dy.abs() * sign.view(-1, 1)
    return dy, x


def _rb(t):
    return t.to(BF).double()


def make_block(K, sd, M, Bw, mode, seed, lut, dev, signs=(None, None, None, None)):
    """the four products of one block shape at M token rows (items 0, 1) and Bw windows (items 2, 3); signs: per item, an
    optional sign per row (random mode: |dY| * sign, |X|)"""
    ops = K["ops"]
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    C, hid, h, hd, DP = sd["C"], sd["hid"], sd["h"], sd["hd"], sd["DP"]
    Mw = Bw * LP
    rows_tok = torch.arange(M, device=dev)
    t_of = torch.arange(Mw, device=dev) % LP
    rows_win = (t_of < L_WIN).nonzero().flatten()                     # valid window rows
    allc = lambda n: torch.arange(n, device=dev)                       # noqa: E731
    j = torch.arange(DP, device=dev)
    one = torch.where(j.view(1, -1) < hd, torch.arange(h, device=dev).view(-1, 1) * hd + j.view(1, -1), torch.full((1, 1), -1, device=dev)).reshape(-1)
    proj_map = one.to(torch.int32)                                     # [h DP] -> head * hd + j, or -1
    qkv_map = torch.cat([torch.where(one >= 0, one + part * C, one) for part in range(3)]).to(torch.int32)
    ints = [float(v) for v in range(1, 9)] + [float(-v) for v in range(1, 9)]
    prods = []

    # item 0, fc2: dY = d(a2) bf16 [M][C], X = GELU(hpre), hpre bf16 [M][hid]
    dy, xg = _dense_values(M, C, hid, rows_tok, allc(C), allc(hid), mode, GELU_INT, g, dev, signs[0])
    dy = _rb(dy)
    if mode == "exact":                # pre-activation = the GELU value itself; the non-hot entries 0 or -20 (table / formula zeros)
        z = torch.tensor(GELU_ZERO, dtype=F64, device=dev)[torch.randint(0, 2, xg.shape, generator=g, device=dev)]
        pre = torch.where(xg != 0, xg, z).to(BF)
    else:
        pre = xg.to(BF)
    dyb = dy.to(BF).contiguous()
    xe = lut_of(lut, pre).double()
    if mode == "exact":
        assert torch.equal(xe, xg)
    prods.append(Prod(ops.op_bf16(dyb), ops.op_bf16(pre, gelu=True), dy, xe, None, None, C, hid, (dyb, pre)))

    # item 1, fc1: dY = d(h) bf16 [M][hid], X = x1 fp32 [M][C] (read as bf16)
    dy, x = _dense_values(M, hid, C, rows_tok, allc(hid), allc(C), mode, ints, g, dev, signs[1])
    dy = _rb(dy)
    dyb, xf = dy.to(BF).contiguous(), x.float().contiguous()
    prods.append(Prod(ops.op_bf16(dyb), ops.op_f32(xf), dy, _rb(xf), None, None, hid, C, (dyb, xf)))

    # item 2, proj: dY = d(a1) bf16 [Mw][C] (zero on padded rows), X = oh head-major [Bw][h][1][Lp][DP] (padded columns BIG)
    vk = (proj_map >= 0).nonzero().flatten()
    dy, x = _dense_values(Mw, C, h * DP, rows_win, allc(C), vk, mode, ints, g, dev, signs[2])
    dy = _rb(dy)
    x = _rb(x)
    xs = x.clone()
    pad_k = (proj_map < 0).nonzero().flatten()
    xs[rows_win.view(-1, 1), pad_k.view(1, -1)] = BIG
    oh = xs.view(Bw, LP, h, DP).permute(0, 2, 1, 3).unsqueeze(2).to(BF).contiguous()
    dyb = dy.to(BF).contiguous()
    prods.append(Prod(ops.op_bf16(dyb), ops.op_heads(oh, Bw, h, 1, LP, DP), dy, xs, None, proj_map, C, C, (dyb, oh, proj_map)))

    # item 3, qkv: dY = d(qkv) head-major [Bw][h][3][Lp][DP] (padded columns BIG), X = x fp32 token rows gathered through rowidx
    vn = (qkv_map >= 0).nonzero().flatten()
    # rowidx: valid window rows -> a permutation of the token rows; -1 on padded rows and on every 8th valid row (chosen at random)
    ntok = Bw * L_WIN
    perm = torch.randperm(ntok, generator=g, device=dev)
    rowidx = torch.full((Mw,), -1, dtype=torch.int64, device=dev)
    rowidx[rows_win] = perm
    drop = rows_win[torch.rand(rows_win.numel(), generator=g, device=dev) < 0.125]
    rowidx[drop] = -1
    dy, x = _dense_values(Mw, 3 * h * DP, C, rows_win, vn, allc(C), mode, ints, g, dev, signs[3])
    dy = _rb(dy)
    x[drop] = 0.0                                                      # a -1 row reads as zeros (its dY still counts in db)
    xtok = torch.full((ntok, C), 5.0, dtype=torch.float32, device=dev)   # token rows no window row reads: junk
    keep_r = rowidx >= 0
    xtok[rowidx[keep_r]] = x[keep_r].float()
    dys = dy.clone()
    pad_n = (qkv_map < 0).nonzero().flatten()
    dys[rows_win.view(-1, 1), pad_n.view(1, -1)] = BIG
    dqkv = dys.view(Bw, LP, 3, h, DP).permute(0, 3, 2, 1, 4).to(BF).contiguous()
    ri = rowidx.to(torch.int32)
    xe = torch.where(keep_r.view(-1, 1), _rb(xtok[rowidx.clamp_min(0)]), torch.zeros((), dtype=F64, device=dev))
    prods.append(Prod(ops.op_heads(dqkv, Bw, h, 3, LP, DP), ops.op_f32(xtok, rows=Mw, rowidx=ri), dys, xe, qkv_map, None, 3 * C, C,
                      (dqkv, xtok, ri, qkv_map)))
    return prods


# ---------------------------------------------------------------------------------------------------------------
# The paths
# ---------------------------------------------------------------------------------------------------------------
def run_block(K, sd, prods, slices, bases, dev, path):
    """swv2_block_wgrad; `path` is the name the caller files the result under, and the library must say that this launch runs the
    kernel the name claims: "slab" -> the slab kernel, "grouped..." -> the grouped tile kernel"""
    L = K["L"]
    lib = L.load()
    items = (L.WgradItem * 4)()
    bufs = []
    for i, p in enumerate(prods):
        bw, bb, w, b = p.buffers(dev, *bases[i])
        bufs.append((bw, bb, w, b))
        items[i].dy, items[i].x = p.dy_op, p.x_op
        items[i].dW, items[i].db = w.data_ptr(), b.data_ptr()
        items[i].nmap = p.nmap.data_ptr() if p.nmap is not None else None
        items[i].kmap = p.kmap.data_ptr() if p.kmap is not None else None
        items[i].ldw = p.kout
    nb = lib.swv2_block_wgrad_ws_bytes(sd["C"], sd["hid"], sd["h"] * sd["DP"], slices)
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    assert lib.swv2_block_wgrad_kernel(items, slices, nb) == (L.BLOCK_WGRAD_SLAB if path == "slab" else L.BLOCK_WGRAD_GROUPED), (path, slices)
    L.check(lib.swv2_block_wgrad(items, slices, ctypes.c_void_p(ws.data_ptr()), nb, None), "swv2_block_wgrad")
    torch.cuda.synchronize()
    return bufs


def run_single(K, p, splits, workspace, base, dev, family):
    """swv2_linear_wgrad(_ws) through ops.linear_wgrad; `family` ("wide" / anything else: the tile kernel) is what the caller's
    path name claims for this product, checked against the library's answer for the launch's own arguments"""
    L = K["L"]
    lib = L.load()
    nb = lib.swv2_linear_wgrad_ws_bytes(p.dy_op.rows, p.dy_op.cols, p.x_op.cols, splits) if workspace else 0      # (as ops.linear_wgrad sizes it)
    assert lib.swv2_linear_wgrad_kernel(ctypes.byref(p.dy_op), ctypes.byref(p.x_op), splits, nb) == \
        (L.WGRAD_WIDE if family == "wide" else L.WGRAD_TILE), (family, splits, workspace)
    bw, bb, w, b = p.buffers(dev, *base)
    K["ops"].linear_wgrad(p.dy_op, p.x_op, w, b, nmap=p.nmap, kmap=p.kmap, splits=splits, workspace=workspace)
    torch.cuda.synchronize()
    return bw, bb, w, b


def all_results(K, sd, prods, bases, dev, monkeypatch, wide):
    """{path name: [(bw, bb, w, b) per product]}"""
    res = {}
    for blk in (0, 8, 16):
        name = ("slab" if sd["slab"] else "grouped0") if blk == 0 else f"grouped{blk}"
        res[name] = run_block(K, sd, prods, blk, bases, dev, name)
    flags = ("0", "1") if wide else (None,)
    for fl in flags:
        if fl is not None:
            monkeypatch.setenv("SWV2_GEMM_WIDE", fl)
        for s, wsp in SINGLE:
            name = f"{'ws' if wsp else 'atomic'}{s}" + ("" if fl is None else ("/wide" if fl == "1" and wsp else f"/gemm_wide={fl}"))
            res[name] = [run_single(K, p, s, wsp, bases[i], dev, _family(name, i)) for i, p in enumerate(prods)]
        if fl is not None:
            monkeypatch.delenv("SWV2_GEMM_WIDE")
    return res


def _bases(prods, mode, seed, dev):
    g = torch.Generator(device=dev)
    g.manual_seed(seed + 99)
    if mode != "exact":
        return [(torch.zeros(p.nout, p.kout, device=dev), torch.zeros(p.nout, device=dev)) for p in prods]
    return [(torch.randint(-64, 65, (p.nout, p.kout), generator=g, device=dev).float(),
             torch.randint(-64, 65, (p.nout,), generator=g, device=dev).float()) for p in prods]


def _guards_intact(bw, bb, nout):
    return bool((bw[0] == GUARD).all() and (bw[nout + 1] == GUARD).all() and (bb[:4] == GUARD).all() and (bb[nout + 4:] == GUARD).all())


def _first_bad(got, ref, n=5):
    bad = (got.double() != ref).nonzero()
    return int(bad.shape[0]), [(tuple(int(v) for v in ix), float(got[tuple(ix)]), float(ref[tuple(ix)])) for ix in bad[:n]]


# ---------------------------------------------------------------------------------------------------------------
# Part 1: exact arithmetic
# ---------------------------------------------------------------------------------------------------------------
def _exact_case(K, dev, monkeypatch, gelu_lut, tag, M, Bw, wide):
    sd = SETS[tag]
    seed = 1000 * M + Bw + 7 * len(tag)
    prods = make_block(K, sd, M, Bw, "exact", seed, gelu_lut, dev)
    bases = _bases(prods, "exact", seed, dev)
    refs = [p.reference(*bases[i]) for i, p in enumerate(prods)]
    res = all_results(K, sd, prods, bases, dev, monkeypatch, wide)
    fails = []
    for path, outs in res.items():
        for i, (bw, bb, w, b) in enumerate(outs):
            rw, rb_ = refs[i][0], refs[i][1]
            if not _guards_intact(bw, bb, prods[i].nout):
                fails.append((path, i, "guard rows written"))
            if not torch.equal(w.double(), rw):
                fails.append((path, i, "dW", _first_bad(w, rw)))
            if not torch.equal(b.double(), rb_):
                fails.append((path, i, "db", _first_bad(b, rb_)))
    assert not fails, (tag, M, Bw, fails[:12])


@pytest.mark.parametrize("tag", ["c128", "c192"])
@pytest.mark.parametrize("M,Bw", CASES)
def test_exact_integer_operands_bit_for_bit(dev, K, monkeypatch, gelu_lut, tag, M, Bw):
    """slab (slices 0), grouped tile kernel (slices 8, 16) and the single-product kernel (splits 1 / 7 / 64, atomics and workspace)
    on integer operands: every element of dW and db equals the fp64 reference exactly, accumulated onto an integer baseline"""
    _exact_case(K, dev, monkeypatch, gelu_lut, tag, M, Bw, wide=False)


@pytest.mark.parametrize("M,Bw", WIDE_CASES)
def test_exact_integer_operands_wide_kernel(dev, K, monkeypatch, gelu_lut, M, Bw):
    """C 512 / hidden 1024 / 8 heads of 64: fc1, proj and qkv take the wide kernel (SWV2_GEMM_WIDE=1, workspace) or the
    128 x 128 tile kernel (=0); fc2's GELU operand and the atomic path always the tile kernel; slices 0 the grouped tile kernel"""
    _exact_case(K, dev, monkeypatch, gelu_lut, "c512", M, Bw, wide=True)


# ---------------------------------------------------------------------------------------------------------------
# Part 2: random data, per element, small elements included
# ---------------------------------------------------------------------------------------------------------------
def _family(path, item):
    """the kernel family a path name claims for item (run_block / run_single check the claim against the library)"""
    if "/wide" in path and item > 0:          # (fc2's GELU operand is not a wide-kernel kind: the tile kernel runs it)
        return "wide"
    return path.split("/")[0].rstrip("0123456789")


def _check_per_element(res, prods, refs, tag, M, Bw):
    """asserts the per-element bounds; returns the worst |err| / A per (path family, dW | db)"""
    worst, fails = {}, []

    def _record(path, item, kind, r):
        key = (_family(path, item), kind)
        worst[key] = max(worst.get(key, 0.0), r)

    for path, outs in res.items():
        for i, (bw, bb, w, b) in enumerate(outs):
            rw, rb_, A, Ab = refs[i]
            if not _guards_intact(bw, bb, prods[i].nout):
                fails.append((path, i, "guard rows written"))
            c = C_SLAB if path == "slab" else C32
            ew, eb = (w.double() - rw).abs(), (b.double() - rb_).abs()
            # (A = 0 only where every product is zero: the result must then be exactly zero)
            rw_ = float((ew / A.clamp_min(1e-300)).max())
            rb2 = float((eb / Ab.clamp_min(1e-300)).max())
            _record(path, i, "dW", rw_)
            _record(path, i, "db", rb2)
            if not bool((ew <= c * A).all()):
                fails.append((path, i, "dW", rw_, c))
            if not bool((eb <= C32 * Ab).all()):
                fails.append((path, i, "db", rb2, C32))
    assert not fails, (tag, M, Bw, fails[:12])
    return worst


RANDOM_CASES = [("c128", 162, 1), ("c128", 4374, 27), ("c128", 129600, 800), ("c192", 162, 1), ("c192", 4374, 27),
                ("c192", 129600, 800), ("c512", 8192, 48)]


@pytest.mark.parametrize("tag,M,Bw", RANDOM_CASES)
def test_random_operands_per_element_bound(dev, K, monkeypatch, gelu_lut, tag, M, Bw):
    """every path on random operands with a wide dynamic range: per-element bound against A = sum |dY| |X|.  The slab runs
    (its result is not bit-equal to the grouped tile kernel's: other summation order and bf16 partials), and the wide kernel
    runs at C 512 (not bit-equal to the tile kernel's either)."""
    sd = SETS[tag]
    seed = 31 * M + Bw + len(tag)
    prods = make_block(K, sd, M, Bw, "random", seed, gelu_lut, dev)
    bases = _bases(prods, "random", seed, dev)
    res = all_results(K, sd, prods, bases, dev, monkeypatch, wide=tag == "c512")
    worst = _check_per_element(res, prods, [p.reference(*bases[i]) for i, p in enumerate(prods)], tag, M, Bw)
    if sd["slab"]:
        assert any(not torch.equal(res["slab"][i][2], res["grouped8"][i][2]) for i in range(4)), "the slab kernel did not run"
    else:
        assert any(not torch.equal(res["ws64/wide"][i][2], res["ws64/gemm_wide=0"][i][2]) for i in (1, 2, 3)), "the wide kernel did not run"
    print(f"\n[wgrad per element] {tag} M={M} Bw={Bw}: " + ", ".join(f"{k[0]} {k[1]} {v:.3g}" for k, v in sorted(worst.items())))


# ---------------------------------------------------------------------------------------------------------------
# The slab on cancelling data
# ---------------------------------------------------------------------------------------------------------------
def shape_items(L, sd, M, Bw):
    """the four items of swv2_block_wgrad for a block shape at M token rows and Bw windows, shapes only: every pointer is a stand-in
    (the kernel and plan queries dereference none), so this needs no GPU"""
    C, hid, h, DP = sd["C"], sd["hid"], sd["h"], sd["DP"]
    fake = 0x10000

    def op(kind, rows, cols, ld, gather=False, p=(0, 0, 0, 0)):
        o = L.Operand()
        o.kind, o.ptr, o.rowidx, o.ld, o.rows, o.cols = kind, fake, fake if gather else None, ld, rows, cols
        o.p = (ctypes.c_int * 4)(*p)
        return o

    def heads(parts):
        return op(L.OP_HEADS, Bw * LP, parts * h * DP, parts, p=(h, 0, LP, DP))

    pairs = [(op(L.OP_BF16, M, C, C), op(L.OP_BF16_GELU, M, hid, hid)), (op(L.OP_BF16, M, hid, hid), op(L.OP_F32, M, C, C)),
             (op(L.OP_BF16, Bw * LP, C, C), heads(1)), (heads(3), op(L.OP_F32, Bw * LP, C, C, gather=True))]
    items = (L.WgradItem * 4)()
    for i, (dy, x) in enumerate(pairs):
        items[i].dy, items[i].x, items[i].dW, items[i].ldw = dy, x, fake, x.cols
    return items


def slab_plan(L, sd, M, Bw, cus):
    """the library's plan of swv2_block_wgrad(items, 0, ...) for this shape with a workspace of swv2_block_wgrad_ws_bytes on `cus` CUs
    (0: the current device's): swv2_block_wgrad_plan, the function the launch itself switches on.  Returns (plan, workspace bytes)"""
    lib = L.load()
    nb = lib.swv2_block_wgrad_ws_bytes(sd["C"], sd["hid"], sd["h"] * sd["DP"], 0)
    plan = L.BlockWgradPlan()
    L.check(lib.swv2_block_wgrad_plan(shape_items(L, sd, M, Bw), 0, nb, cus, ctypes.byref(plan)), "swv2_block_wgrad_plan")
    return plan, nb


@pytest.mark.parametrize("tag,M,Bw", [("c128", 162, 1), ("c192", 4374, 27)])
def test_plan_query_for_the_current_device(K, tag, M, Bw):
    """cus = 0 plans for the current device as the launch sees it: its CU count, at most 320"""
    L = K["L"]
    here, _ = slab_plan(L, SETS[tag], M, Bw, 0)
    want, _ = slab_plan(L, SETS[tag], M, Bw, min(torch.cuda.get_device_properties(0).multi_processor_count, 320))
    assert here.kernel == want.kernel == L.BLOCK_WGRAD_SLAB
    assert (list(here.S), list(here.SR), list(here.wgs), here.bytes) == (list(want.S), list(want.SR), list(want.wgs), want.bytes)


@pytest.mark.parametrize("tag", ["c128", "c192"])
@pytest.mark.parametrize("how", ["halves", "slices"])
def test_slab_on_cancelling_data(dev, K, monkeypatch, gelu_lut, tag, how):
    """|X| and |dY| with a sign per row, so that large partials cancel in the total.  halves: + on the first half of the rows,
    - on the second; slices: + on the stages of the first half of the slab's row slices, - on the others (slice s owns the
    stages s, s + S, s + 2 S ...: every slice's partial is then coherent, the worst case for bf16 partials).  The per-element
    bound 2^-8 A holds; the measured cost of the bf16 partials is printed, as |err| / A and |err| / |ref|."""
    sd = SETS[tag]
    M, Bw = 4374, 27
    Mw = Bw * LP
    rows = [M, M, Mw, Mw]
    if how == "halves":
        signs = [torch.where(torch.arange(R, device=dev) < R // 2, 1.0, -1.0).double() for R in rows]
    else:
        plan, _ = slab_plan(K["L"], sd, M, Bw, 0)          # the slices of the launch below (the current device's CUs)
        assert plan.kernel == K["L"].BLOCK_WGRAD_SLAB
        S, SR = list(plan.S), list(plan.SR)
        signs = [torch.where(((torch.arange(R, device=dev) // SR[i]) % S[i]) < S[i] // 2, 1.0, -1.0).double() for i, R in enumerate(rows)]
    prods = make_block(K, sd, M, Bw, "random", 77, gelu_lut, dev, signs=signs)
    bases = _bases(prods, "random", 77, dev)
    refs = [p.reference(*bases[i]) for i, p in enumerate(prods)]
    res = {"slab": run_block(K, sd, prods, 0, bases, dev, "slab"), "grouped8": run_block(K, sd, prods, 8, bases, dev, "grouped8")}
    _check_per_element(res, prods, refs, tag, M, Bw)
    line = []
    for path, outs in res.items():
        wa, wr = 0.0, 0.0
        for i, (_, _, w, _) in enumerate(outs):
            rw, _, A, _ = refs[i]
            e = (w.double() - rw).abs()
            wa = max(wa, float((e / A.clamp_min(1e-300)).max()))
            wr = max(wr, float((e / rw.abs().clamp_min(1e-300)).max()))
        line.append(f"{path}: worst |err|/A {wa:.3g}, |err|/|ref| {wr:.3g}")
    print(f"\n[slab cancellation] {tag} {how}: " + "; ".join(line))
