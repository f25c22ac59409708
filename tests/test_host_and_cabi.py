"""CPU: host-side logic of the product package and the C-ABI surface (no compute calls -- there is no GPU here)."""
import ctypes
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import swin_oracle as O
from swin_v2_weather_amd import _lib as L
from swin_v2_weather_amd.networks import helpers, swinv2_global as N
from swin_v2_weather_amd.utils.YParams import YParams, load_yaml
from swin_v2_weather_amd.utils.data_loader_era5 import GetDataset, get_data_loader
from swin_v2_weather_amd.utils.grids import GridQuadrature, naive_quadrature_weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
CFG = os.path.join(ROOT, "swin_v2_weather_amd", "config", "swin.yaml")


# ---- C ABI -------------------------------------------------------------------------------------------------
def header_symbols():
    txt = open(os.path.join(ROOT, "include", "swv2.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(swv2_[a-z0-9_]+)\s*\(", txt)))


def test_library_builds_loads_and_exports_every_declared_symbol():
    L.build_library()
    lib = L.load()
    names = header_symbols()
    assert len(names) >= 15
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/swv2.h but not exported"
    assert set(names) == set(L.SYMBOLS), "ctypes binding table and header disagree"
    # the ABI revision: header, library and ctypes mirrors agree (a stale .so is refused by L.load())
    hdr = int(re.search(r"#define SWV2_VERSION (\d+)", open(os.path.join(ROOT, "include", "swv2.h")).read()).group(1))
    assert lib.swv2_version() == hdr == L.ABI_VERSION


def header_struct_fields(name):
    """member names of `struct <name>` in include/swv2.h, in declaration order"""
    txt = open(os.path.join(ROOT, "include", "swv2.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    body = re.search(r"typedef struct(?: %s)? \{([^{}]*)\} %s;" % (name, name), txt, flags=re.S).group(1)
    out = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        first, *rest = decl.split(",")
        out.append(re.findall(r"([A-Za-z_][A-Za-z0-9_]*)\s*(?:\[[^\]]*\])?\s*$", first.strip())[0])
        out += [re.sub(r"\[.*", "", r_).replace("*", "").strip() for r_ in rest]
    return out


def test_ctypes_structs_follow_the_header_field_order():
    """the ctypes mirrors (swin_v2_weather_amd/_lib.py) and the stub printed in INTEGRATION.md list exactly the members of
    the C structs, in order -- a missing member shifts every later pointer by one slot (`bias_pack`)"""
    pairs = {"swv2_attn_args": L.AttnArgs, "swv2_operand": L.Operand, "swv2_epilogue": L.Epilogue, "swv2_block_desc": L.BlockDesc,
             "swv2_mlp_args": L.MlpArgs, "swv2_mlp_bwd_args": L.MlpBwdArgs, "swv2_proj_ln_args": L.ProjLnArgs,
             "swv2_proj_ln_bwd_args": L.ProjLnBwdArgs, "swv2_ln_args": L.LnArgs,
             "swv2_wgrad_item": L.WgradItem, "swv2_block_plan_t": L.BlockPlan, "swv2_attn_kernel_t": L.AttnKernelInfo,
             "swv2_block_wgrad_plan_t": L.BlockWgradPlan}
    pairs["swv2_adam_item"] = L.AdamItem
    for cname, cls in pairs.items():
        assert [f[0] for f in cls._fields_] == header_struct_fields(cname), cname
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    stub = doc[doc.index("class AttnArgs(C.Structure)"):doc.index("lib.swv2_attn_fwd.argtypes")]
    names = re.findall(r'"([A-Za-z_][A-Za-z0-9_]*)"', stub)
    assert names == header_struct_fields("swv2_attn_args")


def test_argument_errors_are_reported_without_touching_the_gpu():
    lib = L.load()
    assert lib.swv2_attn_fwd(None, None) == -1            # SWV2_ERR_INVALID
    assert b"null" in lib.swv2_last_error()
    lp, dp = ctypes.c_int(), ctypes.c_int()
    assert lib.swv2_attn_geometry(162, 16, ctypes.byref(lp), ctypes.byref(dp)) == 0 and (lp.value, dp.value) == (176, 16)
    assert lib.swv2_attn_geometry(54, 24, ctypes.byref(lp), ctypes.byref(dp)) == 0 and (lp.value, dp.value) == (64, 32)
    assert lib.swv2_attn_geometry(54, 96, ctypes.byref(lp), ctypes.byref(dp)) == 0 and (lp.value, dp.value) == (64, 96)    # yaml default 768 / 8: unpadded
    assert lib.swv2_attn_geometry(162, 80, ctypes.byref(lp), ctypes.byref(dp)) == 0 and (lp.value, dp.value) == (176, 96)
    assert lib.swv2_attn_geometry(162, 112, ctypes.byref(lp), ctypes.byref(dp)) == 0 and (lp.value, dp.value) == (176, 128)
    assert lib.swv2_attn_geometry(162, 48, ctypes.byref(lp), ctypes.byref(dp)) == 0 and (lp.value, dp.value) == (176, 64)
    assert lib.swv2_attn_geometry(400, 16, ctypes.byref(lp), ctypes.byref(dp)) == -1
    assert lib.swv2_attn_geometry(54, 160, ctypes.byref(lp), ctypes.byref(dp)) == -1
    assert lib.swv2_block_wgrad(None, 0, None, 0, None) == -1 and lib.swv2_adam_multi(None, None, 0, 1e-3, 0.9, 0.95, 1e-8, 1, 1.0, None) == -1
    # the larger of the 128 x 128 tile kernel's partial tiles (40 slices x 12 tiles) and the slab kernel's bound (one workgroup per CU, at
    # most 320 -- a pure host function: no HIP call, the same on every device -- with the largest partial output, + the partial bias rows)
    assert lib.swv2_block_wgrad_ws_bytes(128, 512, 128, 0) == max(40 * 12 * 128 * 128 * 4, 320 * 128 * 512 * 4 + 320 * 512 * 4 + 1024)
    assert lib.swv2_block_wgrad_ws_bytes(96, 384, 96, 0) == 48 * 10 * 128 * 128 * 4       # (no slab instantiation: 48 slices x (3 + 3 + 1 + 3) tiles)
    with pytest.raises(L.Swv2Error):
        L.check(lib.swv2_linear(None, None, None, 4, None), "swv2_linear")


def test_weight_gradient_workspace_budget_covers_the_wide_path():
    """Host-only sizing (no GPU call): from N, K = 512 the 256 x 256 weight-gradient kernel writes S = 256 / tiles partial [N][K]
    matrices + S * (K / 256) bias-gradient rows and casts an fp32 X operand to a bf16 [M][K] copy -- all inside the workspace the
    caller sizes with swv2_linear_wgrad_ws_bytes; narrow shapes and ragged row counts keep the 128-tile plan."""
    lib = L.load()
    lib.swv2_linear_wgrad_ws_bytes.restype = ctypes.c_size_t
    up = lambda b: (b + 255) // 256 * 256
    for (M, N, K) in ((64800, 768, 3072), (70400, 3072, 768), (70400, 768, 1024)):
        S = max(1, 256 // ((N // 256) * (K // 256)))
        need = up(S * N * K * 4) + up(S * (K // 256) * N * 4) + up(M * K * 2)
        assert lib.swv2_linear_wgrad_ws_bytes(M, N, K, 16) >= need, (M, N, K)
    narrow = lib.swv2_linear_wgrad_ws_bytes(129600, 384, 128, 40)
    assert 0 < narrow <= 40 * 3 * 128 * 128 * 4                                   # 3 tiles x 40 slices of 64 KB: the 128-tile plan only
    assert lib.swv2_linear_wgrad_ws_bytes(64801, 768, 3072, 16) < 64801 * 3072 * 2      # ragged M: no wide path, no cast buffer
    assert lib.swv2_linear_wgrad_ws_bytes(0, 768, 768, 8) == 0


# ---- kernel selection (swv2_linear_kernel / swv2_linear_wgrad_kernel / swv2_block_wgrad_kernel) ---------------------------
_FAKE = 0x10000          # stands for "a pointer is present": the queries dereference no data pointer


def _op(kind, rows, cols, ld, gather=False, p=(0, 0, 0, 0)):
    o = L.Operand()
    o.kind, o.ptr, o.rowidx, o.ld, o.rows, o.cols = kind, _FAKE, _FAKE if gather else None, ld, rows, cols
    o.p = (ctypes.c_int * 4)(*p)
    return o


def _op_heads(Bw, h, parts, Lp, DP):
    return _op(L.OP_HEADS, Bw * Lp, parts * h * DP, parts, p=(h, 0, Lp, DP))


def _epi(kind, ld=0, aux=False, scatter=False, p=(0, 0, 0, 0, 0)):
    e = L.Epilogue()
    e.kind, e.out, e.aux, e.rowidx, e.ld = kind, _FAKE, _FAKE if aux else None, _FAKE if scatter else None, ld
    e.p = (ctypes.c_int * 5)(*p)
    return e


def _block_products(B, C, hid, h, DP, fused):
    """the descriptors swv2_block_fwd / swv2_block_bwd build (csrc/block.hip) for one block on the 180 x 360 patch grid of the
    721 x 1440 fields in 9 x 18 windows (WindowPlan: 400 windows per sample, 162 tokens padded to 176 rows), local batch B"""
    Lw, Lp, BT, Bw = 162, 176, B * 180 * 360, B * 400
    Mw = Bw * Lp
    hp = (h, 0, Lp, DP, Lw)
    linear = {
        "qkv": (_op(L.OP_F32, Mw, C, C, gather=True), _epi(L.EPI_QKV_HEADS, p=hp), 3 * h * DP),
        "proj": (_op_heads(Bw, h, 1, Lp, DP), _epi(L.EPI_BF16, C), C),
        "fc1": (_op(L.OP_F32, BT, C, C), _epi(L.EPI_BF16_GELU, hid), hid),
        "fc2": (_op(L.OP_BF16, BT, hid, hid), _epi(L.EPI_BF16, C), C),
        "d_fc2": (_op(L.OP_BF16, BT, C, C), _epi(L.EPI_GELU_GRAD, hid, aux=True), hid),
        "dx1": (_op(L.OP_BF16, BT, hid, hid), _epi(L.EPI_F32, C, aux=True), C),
        "d_oh": (_op(L.OP_BF16, Mw, C, C), _epi(L.EPI_HEADS, p=hp), h * DP),
        "dx": (_op_heads(Bw, h, 3, Lp, DP), _epi(L.EPI_F32, C, aux=True, scatter=True), C),
        "head": (_op(L.OP_F32, BT, C, C), _epi(L.EPI_UNPATCH, p=(73, 720, 1440, 0, 0)), 73 * 16),
        "head_loss": (_op(L.OP_F32, BT, C, C), _epi(L.EPI_UNPATCH_LOSS, p=(73, 720, 1440, 0, 0)), 73 * 16),
    }
    # items 0 .. 3 of swv2_block_wgrad; the fused MLP path keeps no GELU output: fc2's X operand is GELU(hpre) on load
    wgrad = [(_op(L.OP_BF16, BT, C, C), _op(L.OP_BF16_GELU if fused else L.OP_BF16, BT, hid, hid)),
             (_op(L.OP_BF16, BT, hid, hid), _op(L.OP_F32, BT, C, C)),
             (_op(L.OP_BF16, Mw, C, C), _op_heads(Bw, h, 1, Lp, DP)),
             (_op_heads(Bw, h, 3, Lp, DP), _op(L.OP_F32, Mw, C, C, gather=True))]
    return linear, wgrad


def test_kernel_selection_for_the_products_the_model_launches(monkeypatch):
    """The selection the launchers switch on, pinned for the products of the four block shapes the repository runs.  The expected
    kernels were read off the launch ladders as they stood before the selection functions existed (swv2_linear: resident-weight
    shapes, then the wide condition N % 256 == 0, N, K >= 512, M >= 4096 with LDS-DMA staging for raw bf16 / head-major operands,
    then 64-row tiles for the loss epilogue and where the qkv / dx products fill 768 workgroup slots better; weight gradients: wide
    from N, K >= 512 in multiples of 256 with a raw-bf16 or fp32 X, the slab at its two block shapes).  No GPU: the slab query
    sees the library's 256-CU fallback."""
    lib = L.load()
    monkeypatch.delenv("SWV2_GEMM_WIDE", raising=False)
    Q128, Q192, DX128, DMA, WIDE, T64, T128 = (L.LINEAR_RESIDENT_QKV128, L.LINEAR_RESIDENT_QKV192X3, L.LINEAR_RESIDENT_DX128,
                                               L.LINEAR_WIDE_DMA, L.LINEAR_WIDE, L.LINEAR_TILE64, L.LINEAR_TILE128)
    order = ("qkv", "proj", "fc1", "fc2", "d_fc2", "dx1", "d_oh", "dx", "head", "head_loss")
    shapes = {
        # (local batch, C, hidden, heads, head columns, fused MLP): linear kernels in `order`, single weight gradients, block
        "bench C 128": ((2, 128, 512, 8, 16, True), (Q128, T128, T128, T128, T128, T128, T128, DX128, T128, T64),
                        [L.WGRAD_TILE] * 4, L.BLOCK_WGRAD_SLAB),
        "geo C 192": ((2, 192, 768, 8, 32, True), (Q192, T128, T128, T128, T128, T128, T128, DMA, T128, T64),
                      [L.WGRAD_TILE] * 4, L.BLOCK_WGRAD_SLAB),
        "yaml default C 768": ((1, 768, 3072, 8, 96, False), (WIDE, DMA, WIDE, DMA, DMA, DMA, DMA, DMA, T128, T64),
                               [L.WGRAD_WIDE] * 4, L.BLOCK_WGRAD_GROUPED),
        "embed 2048": ((1, 2048, 4096, 8, 256, False), (WIDE, DMA, WIDE, DMA, DMA, DMA, DMA, DMA, T128, T64),
                       [L.WGRAD_WIDE] * 4, L.BLOCK_WGRAD_GROUPED),
    }

    def wgrad_ws(dy, x):
        return lib.swv2_linear_wgrad_ws_bytes(dy.rows, dy.cols, x.cols, 128)

    for name, (cfg, want_linear, want_wgrad, want_block) in shapes.items():
        linear, wgrad = _block_products(*cfg)
        got = tuple(lib.swv2_linear_kernel(ctypes.byref(a), ctypes.byref(e), n) for a, e, n in (linear[k] for k in order))
        assert got == want_linear, (name, dict(zip(order, got)))
        got = [lib.swv2_linear_wgrad_kernel(ctypes.byref(dy), ctypes.byref(x), 128, wgrad_ws(dy, x)) for dy, x in wgrad]
        assert got == want_wgrad, (name, got)
        # without a workspace (swv2_linear_wgrad: atomics) only the tile kernel runs
        assert all(lib.swv2_linear_wgrad_kernel(ctypes.byref(dy), ctypes.byref(x), 64, 0) == L.WGRAD_TILE for dy, x in wgrad), name
        items = (L.WgradItem * 4)()
        for i, (dy, x) in enumerate(wgrad):
            items[i].dy, items[i].x, items[i].dW, items[i].ldw = dy, x, _FAKE, x.cols
        _, C_, hid, h, DP, _ = cfg
        ws = lib.swv2_block_wgrad_ws_bytes(C_, hid, h * DP, 0)
        assert lib.swv2_block_wgrad_kernel(items, 0, ws) == want_block, name
        assert lib.swv2_block_wgrad_kernel(items, 8, ws) == L.BLOCK_WGRAD_GROUPED, name      # an explicit slice count: the tile kernel

    # the embed-768 fc2 gradient with the fused path's GELU-on-load operand is not a wide-kernel kind
    _, wg = _block_products(1, 768, 3072, 8, 96, True)
    assert lib.swv2_linear_wgrad_kernel(ctypes.byref(wg[0][0]), ctypes.byref(wg[0][1]), 128, wgrad_ws(*wg[0])) == L.WGRAD_TILE
    # SWV2_GEMM_WIDE=0: the wide rows fall to the tile kernels (64-row tiles where 2 200 workgroups fill 3 x 768 slots, 128-row ones
    # where 550 / 1 100 workgroups fill 768 / 1 536 equally)
    monkeypatch.setenv("SWV2_GEMM_WIDE", "0")
    lin192, _ = _block_products(2, 192, 768, 8, 32, True)
    lin768, wg768 = _block_products(1, 768, 3072, 8, 96, False)
    assert lib.swv2_linear_kernel(ctypes.byref(lin192["dx"][0]), ctypes.byref(lin192["dx"][1]), 192) == T64
    assert lib.swv2_linear_kernel(ctypes.byref(lin768["qkv"][0]), ctypes.byref(lin768["qkv"][1]), 2304) == T128
    assert lib.swv2_linear_kernel(ctypes.byref(lin768["fc2"][0]), ctypes.byref(lin768["fc2"][1]), 768) == T128
    assert all(lib.swv2_linear_wgrad_kernel(ctypes.byref(dy), ctypes.byref(x), 128, wgrad_ws(dy, x)) == L.WGRAD_TILE for dy, x in wg768)
    monkeypatch.delenv("SWV2_GEMM_WIDE")
    # argument errors come back as negative codes
    assert lib.swv2_linear_kernel(None, None, 4) == -1 and lib.swv2_block_wgrad_kernel(None, 0, 0) == -1
    assert lib.swv2_linear_kernel(ctypes.byref(_op(L.OP_BF16_CSCALE, 64, 64, 64)), ctypes.byref(_epi(L.EPI_BF16, 64)), 64) == -1


# ---- the block's launch plan (swv2_block_plan) ---------------------------------------------------------------------------------
def _block_desc(B, C, hid, h, bias=False, grid=(180, 360), **over):
    """a descriptor as _BlockRunner fills it (geometry + requests, 9 x 18 windows on `grid` patches) with everything the full plan
    needs on offer: workspace and gradient carve present (the plan tests pointers for presence only), capacities = the reported
    needs.  `over` overrides fields afterwards."""
    lib = L.load()
    d = L.BlockDesc()
    lp, dp = ctypes.c_int(), ctypes.c_int()
    assert lib.swv2_attn_geometry(162, C // h, ctypes.byref(lp), ctypes.byref(dp)) == 0
    d.B, d.T, d.C, d.heads, d.head_dim, d.hidden = B, grid[0] * grid[1], C, h, C // h, hid
    d.L, d.Lp, d.DP, d.nwh, d.nww = 162, lp.value, dp.value, grid[0] // 9, grid[1] // 18
    d.fuse_mlp = d.fuse_proj_ln = d.wgrad_group = 1
    d.wgrad_splits = 128
    d.wgrad_ws = d.grad_zero = _FAKE
    if bias:
        d.bias = d.bias_pack = _FAKE
    for k in ("fuse_mlp", "fuse_proj_ln", "wgrad_group"):
        if k in over:
            setattr(d, k, over.pop(k))
    need = L.block_plan(d)
    d.ln_ws_floats, d.wgrad_ws_bytes = need.need_ln_ws_floats, need.need_wgrad_ws_bytes
    for k, v in over.items():
        setattr(d, k, v)
    return d


# the step sequences below were read off swv2_block_fwd / swv2_block_bwd as they stood before swv2_block_plan existed (nested ifs over
# fuse_mlp && swv2_mlp_supported, fuse_proj_ln && swv2_proj_ln_supported, defer, group), not off the plan function
_FWD_FUSED = ["qkv", "attn_fwd", "proj_ln_fwd", "mlp_fwd"]
_BWD_FUSED = ["mlp_bwd", "proj_ln_bwd", "attn_bwd", "dx", "wgrad_group"]
_FWD_SEPARATE_WIDE = ["rnorm_zero", "qkv", "qk_normalize", "attn_fwd", "proj", "ln1_fwd", "fc1", "fc2", "ln2_fwd"]
_BWD_SEPARATE = ["ln2_bwd", "wgrad_fc2", "dh", "wgrad_fc1", "dx1", "ln1_bwd", "wgrad_proj", "doh", "attn_bwd", "wgrad_qkv", "dx"]
_BWD_FUSED_SINGLE = ["mlp_bwd", "wgrad_fc2", "wgrad_fc1", "proj_ln_bwd", "wgrad_proj", "attn_bwd", "wgrad_qkv", "dx", "ln_fold"]
_FWD_STEPS = {"rnorm_zero", "qkv", "qk_normalize", "pack_bias", "attn_fwd", "proj", "ln1_fwd", "proj_ln_fwd", "fc1", "fc2", "ln2_fwd", "mlp_fwd"}
_BLOCK_SHAPES = {       # (local batch, C, hidden, heads) of test_kernel_selection_for_the_products_the_model_launches
    "bench C 128": (2, 128, 512, 8), "geo C 192": (2, 192, 768, 8), "yaml default C 768": (1, 768, 3072, 8), "embed 2048": (1, 2048, 4096, 8)}


def _with_pack(steps):
    i = steps.index("attn_fwd")
    return steps[:i] + ["pack_bias"] + steps[i:]


@pytest.mark.parametrize("name", list(_BLOCK_SHAPES))
@pytest.mark.parametrize("bias", [False, True])
def test_block_plan_of_the_shapes_the_model_runs(name, bias):
    """The default plan of the four block shapes the repository runs, with and without a CPB table (every one of them accepts one:
    swv2_attn_fwd_regime >= 0).  C 128 / 192: forward 4 launches, backward 4 + the grouped weight gradients (the slab kernel), one
    deferred LayerNorm fold riding on their reduction, gradients zeroed in kernel, no hact.  C 768 / 2048 (no fused instantiation,
    wide head slots): 9 forward steps with the rnorm memset and swv2_qk_normalize, 11 backward launches."""
    lib = L.load()
    B, C, hid, h = _BLOCK_SHAPES[name]
    assert lib.swv2_attn_fwd_regime(162, C // h, int(bias), 0) >= 0
    p = L.block_plan(_block_desc(B, C, hid, h, bias))
    small = C <= 192
    fwd = _FWD_FUSED if small else _FWD_SEPARATE_WIDE
    assert p.steps("fwd") == (_with_pack(fwd) if bias else fwd)
    assert p.steps("bwd") == (_BWD_FUSED if small else _BWD_SEPARATE)
    assert (p.mlp_fused, p.proj_ln_fused, p.ln_deferred, p.wgrad_grouped, p.grad_zero_in_kernel) == ((1,) * 5 if small else (0,) * 5)
    assert p.wgrad_kernel == (L.BLOCK_WGRAD_SLAB if small else -1)
    assert p.need_hact_bytes == (0 if small else B * 180 * 360 * hid * 2)
    # attention workgroups per head: 64; 32 with a table (forward: per-workgroup table load; backward: swv2_attn_bias_chunks of >= 32
    # windows); without one at the 176-row window the backward runs 256 / heads
    assert (p.attn_fwd_chunks, p.attn_bwd_chunks) == ((32, 32) if bias else (64, 256 // h))
    assert p.dbias_dest == (L.DBIAS_WGRAD_WS if bias else L.DBIAS_NONE)
    if bias:
        # the stage's one-launch CPB pipeline: table prepacked, the workgroups' d bias tables stay in the stage's buffer
        q = L.block_plan(_block_desc(B, C, hid, h, True, bias_prepacked=1, dbias_part=_FAKE))
        assert q.steps("fwd") == fwd and q.steps("bwd") == p.steps("bwd") and q.dbias_dest == L.DBIAS_PART
        assert L.block_plan(_block_desc(B, C, hid, h, True, wgrad_ws=None)).dbias_dest == L.DBIAS_ATOMICS


def test_block_plan_follows_each_switch_and_capacity():
    """one request off at a time at the benchmark shape, then every capacity fallback: each loses exactly the decision that needs it"""
    lib = L.load()
    cfg = _BLOCK_SHAPES["bench C 128"]
    B, C, hid, h = cfg
    p = L.block_plan(_block_desc(*cfg, fuse_mlp=0))         # (wgrad_group stays 1: the grouped launch needs the fused path's operands)
    assert p.steps("fwd") == ["qkv", "attn_fwd", "proj_ln_fwd", "fc1", "fc2", "ln2_fwd"]
    assert p.steps("bwd") == ["ln2_bwd", "wgrad_fc2", "dh", "wgrad_fc1", "dx1", "proj_ln_bwd", "wgrad_proj", "attn_bwd", "wgrad_qkv", "dx"]
    assert (p.mlp_fused, p.proj_ln_fused, p.ln_deferred, p.wgrad_grouped, p.wgrad_kernel, p.grad_zero_in_kernel) == (0, 1, 0, 0, -1, 0)
    assert p.need_hact_bytes == B * 180 * 360 * hid * 2
    p = L.block_plan(_block_desc(*cfg, fuse_proj_ln=0))
    assert p.steps("fwd") == ["qkv", "attn_fwd", "proj", "ln1_fwd", "mlp_fwd"]
    assert p.steps("bwd") == ["mlp_bwd", "ln1_bwd", "doh", "attn_bwd", "dx", "wgrad_group"]
    assert (p.mlp_fused, p.proj_ln_fused, p.ln_deferred, p.wgrad_grouped, p.wgrad_kernel, p.grad_zero_in_kernel) == (1, 0, 0, 1, L.BLOCK_WGRAD_SLAB, 1)
    p = L.block_plan(_block_desc(*cfg, wgrad_group=0))      # the deferred fold is then a launch of its own
    assert p.steps("fwd") == _FWD_FUSED and p.steps("bwd") == _BWD_FUSED_SINGLE
    assert (p.mlp_fused, p.proj_ln_fused, p.ln_deferred, p.wgrad_grouped, p.wgrad_kernel) == (1, 1, 1, 0, -1)

    # capacities.  The needs do not move with them
    full = L.block_plan(_block_desc(*cfg))
    needs = lambda q: (q.need_hact_bytes, q.need_ln_ws_floats, q.need_wgrad_ws_bytes)
    BT, Mw = B * 180 * 360, B * 400 * 176
    assert full.need_ln_ws_floats == max(L.LN_BWD_MAX_BLOCKS * 2 * C, lib.swv2_mlp_bwd_ws_floats(BT, C) + lib.swv2_proj_ln_bwd_ws_floats(Mw, C))
    group_ws = lib.swv2_block_wgrad_ws_bytes(C, hid, h * 16, 0)
    assert full.need_wgrad_ws_bytes == max([group_ws] + [lib.swv2_linear_wgrad_ws_bytes(m, n, k, 128) for m, n, k in
                                                         ((BT, C, hid), (BT, hid, C), (Mw, C, h * 16), (Mw, 3 * h * 16, C))])
    # one float short of both LayerNorms' rows side by side: not deferred -- each fused kernel folds its own rows inside its launcher
    # (as the separate LayerNorm kernels always do), so no fold step appears; everything else stays
    p = L.block_plan(_block_desc(*cfg, ln_ws_floats=lib.swv2_mlp_bwd_ws_floats(BT, C) + lib.swv2_proj_ln_bwd_ws_floats(Mw, C) - 1))
    assert (p.ln_deferred, p.wgrad_grouped) == (0, 1) and p.steps("bwd") == _BWD_FUSED and needs(p) == needs(full)
    # one byte short of the grouped launch's workspace, none, or a NULL pointer: four single products + the fold as its own step
    for over in (dict(wgrad_ws_bytes=group_ws - 1), dict(wgrad_ws_bytes=0), dict(wgrad_ws=None)):
        p = L.block_plan(_block_desc(*cfg, **over))
        assert (p.ln_deferred, p.wgrad_grouped, p.wgrad_kernel) == (1, 0, -1) and p.steps("bwd") == _BWD_FUSED_SINGLE, over
        assert needs(p) == needs(full)
    assert L.block_plan(_block_desc(*cfg, wgrad_ws_bytes=group_ws)).wgrad_grouped == 1
    # no gradient carve on offer: the caller zeroes
    p = L.block_plan(_block_desc(*cfg, grad_zero=None))
    assert p.grad_zero_in_kernel == 0 and p.steps("bwd") == _BWD_FUSED


def test_block_plan_invariants_and_step_table():
    lib = L.load()
    from swin_v2_weather_amd import ops
    # the step table: every (name, launch id) bench.py's kernel names resolve through is a step with that id; the rest is unbracketed
    table, s = {}, 1
    while lib.swv2_block_step_name(s):
        table[lib.swv2_block_step_name(s).decode()] = lib.swv2_block_step_id(s)
        s += 1
    assert {n: i for n, i in table.items() if i} == ops.BLOCK_KERNEL_IDS
    assert sorted(n for n, i in table.items() if not i) == ["ln_fold", "pack_bias", "qk_normalize", "rnorm_zero"]
    assert sorted(set(ops.BLOCK_KERNEL_IDS.values())) == list(range(1, 8)) + list(range(11, 23))
    assert lib.swv2_block_step_id(0) == lib.swv2_block_step_id(s) == -1 and lib.swv2_block_step_name(0) is None
    # NULL arguments
    assert lib.swv2_block_plan(None, None) == -1 and lib.swv2_block_plan(None, ctypes.byref(L.BlockPlan())) == -1
    assert lib.swv2_block_plan(ctypes.byref(_block_desc(1, 32, 128, 2, grid=(18, 36))), None) == -1
    assert lib.swv2_block_plan(ctypes.byref(L.BlockDesc()), ctypes.byref(L.BlockPlan())) == -1        # no geometry
    lp, dp = ctypes.c_int(), ctypes.c_int()
    seen = 0
    for C in (32, 64, 96, 128, 192, 768, 2048):
        for h in (1, 2, 4, 6, 8, 16):
            if C % h or lib.swv2_attn_geometry(162, C // h, ctypes.byref(lp), ctypes.byref(dp)):
                continue
            for bits in range(8):
                req = dict(fuse_mlp=bits & 1, fuse_proj_ln=bits >> 1 & 1, wgrad_group=bits >> 2 & 1)
                d = _block_desc(1, C, 4 * C, h, bias=bool(h & 2), grid=(18, 36), **req)
                p = L.block_plan(d)
                seen += 1
                fwd, bwd = p.steps("fwd"), p.steps("bwd")
                # written out, not asked of swv2_mlp_supported / swv2_proj_ln_supported: the MLP branch has a fused instantiation at
                # every C of this sweep up to 192 (hidden 4 C) and none at 768 / 2048; proj + LN1 has none there either, and has one
                # at the shapes the GPU fixtures and the benchmark run (C 32 with 2 heads, C 128 and 192 with 8)
                assert p.mlp_fused == int(req["fuse_mlp"] and C <= 192), (C, h, req)
                assert not p.proj_ln_fused or (req["fuse_proj_ln"] and C <= 192), (C, h, req)
                if (C, h) in ((32, 2), (128, 8), (192, 8)):
                    assert p.proj_ln_fused == req["fuse_proj_ln"], (C, h, req)
                # the decisions are the step lists: a fused kernel stands in both directions exactly where its separate ones do not
                assert bool(p.mlp_fused) == ("mlp_fwd" in fwd) == ("mlp_bwd" in bwd) == ("fc1" not in fwd) == ("dh" not in bwd), (C, h, req)
                assert bool(p.proj_ln_fused) == ("proj_ln_fwd" in fwd) == ("proj_ln_bwd" in bwd) == ("proj" not in fwd) == ("doh" not in bwd)
                assert bool(p.wgrad_grouped) == ("wgrad_group" in bwd) == ("wgrad_qkv" not in bwd), (C, h, req)
                assert (p.need_hact_bytes == 0) == bool(p.mlp_fused), (C, h, req)
                assert not p.ln_deferred or (p.mlp_fused and p.proj_ln_fused), (C, h, req)
                assert not p.wgrad_grouped or (p.mlp_fused and req["wgrad_group"]), (C, h, req)
                assert (p.wgrad_kernel >= 0) == bool(p.wgrad_grouped)
                for phase, steps in (("fwd", fwd), ("bwd", bwd)):
                    n = getattr(p, "n_" + phase)
                    assert 0 < n <= L.BLOCK_MAX_STEPS and all(lib.swv2_block_step_id(s) >= 0 for s in getattr(p, phase)[:n])
                assert set(fwd) <= _FWD_STEPS and not set(bwd) & _FWD_STEPS, (C, h, req)
    assert seen >= 8 * 20


def test_model_refuses_cpu_tensors():
    m = N.SwinTransformerV2Cr(img_size=(24, 36), patch_size=4, depths=(1,), num_heads=(2,), in_chans=3, out_chans=3,
                              embed_dim=16, img_window_ratio=4, full_pos_embed=True, rel_pos=False)
    with pytest.raises(L.Swv2Error):
        m(torch.zeros(1, 3, 24, 36))


# ---- config ------------------------------------------------------------------------------------------------
def test_every_config_parses_and_floats_resolve():
    cfgs = load_yaml(CFG)
    assert len(cfgs) >= 15
    for name in cfgs:
        p = YParams(CFG, name)
        assert isinstance(p.lr, float), name                       # `1E-3` / `1e-4` are floats, not strings
        assert p.nettype == 'swin' and p['img_size'] == [720, 1440] or name == 'bench_tiny'
        assert len(p.in_channels) == 73 and len(p.channel_names) == 73
    p = YParams(CFG, 'swin_73var_geo_depth12_chweight_invar_2step')
    assert p.n_future == 1 and p.lr == 1e-4 and p.residual is True and p.add_landmask is True and 'finetune' in p
    p['n_in_channels'] = 77
    p.foo = 1
    assert p.n_in_channels == 77 and p.params['foo'] == 1 and p['foo'] == 1
    p.update_params({'depth': 3})
    assert p.depth == 3 and p['depth'] == 3


# ---- model surface -----------------------------------------------------------------------------------------
def small_params(**kw):
    d = dict(nettype='swin', img_size=[72, 144], patch_size=4, depth=2, num_heads=2, n_in_channels=5, n_out_channels=5,
             embed_dim=32, window_ratio=8, drop_path_rate=0.1, full_pos_embed=True, rel_pos=True, mlp_ratio=4,
             activation_ckpt=False, residual=False, n_future=0, add_orography=False, add_landmask=False)
    d.update(kw)
    return SimpleNamespace(**d)


def test_state_dict_names_and_shapes_match_reference_fixture():
    fx = np.load(os.path.join(GOLD, "model_relpos_residual.npz"))
    cin, cout, H, W, C, depth, h, ratio, relpos, residual, seed = [int(v) for v in fx["meta"]]
    m = N.swinv2net(small_params(n_in_channels=cin, n_out_channels=cout, residual=True))
    sd = m.state_dict()
    ref = {k[2:]: fx[k].shape for k in fx.files if k.startswith("p:")}
    assert set(sd) == set(ref)
    for k, shp in ref.items():
        assert tuple(sd[k].shape) == tuple(shp), k
    # non-persistent buffers stay out of checkpoints; wrappers add the 'model.' prefix (helpers.py:11,22)
    w = helpers.get_model(small_params())
    assert all(k.startswith("model.") for k in w.state_dict())
    assert isinstance(helpers.get_model(small_params(n_future=1)), helpers.MultiStepWrapper)
    with pytest.raises(Exception, match="not implemented"):
        helpers.get_model(small_params(nettype='afno'))


def test_constructor_draws_parameters_in_reference_order():
    """Same seed => same initial weights as the reference: checked against checksums recorded while generating the
    loss-curve fixture from the real reference."""
    import json
    path = os.path.join(GOLD, "losscurve_tiny.json")
    if not os.path.exists(path):
        pytest.skip("loss-curve fixture not generated yet")
    meta = json.load(open(path))
    c = meta["cfg"]
    torch.manual_seed(meta["seed"])
    m = N.SwinTransformerV2Cr(img_size=tuple(c["img_size"]), patch_size=4, depths=(c["depth"],), num_heads=(c["num_heads"],),
                              in_chans=c["in_chans"], out_chans=c["out_chans"], embed_dim=c["embed_dim"],
                              img_window_ratio=c["window_ratio"], drop_path_rate=0.0, full_pos_embed=True, rel_pos=False,
                              mlp_ratio=4, residual=False)
    for k, (s, a) in meta["init_checksums"].items():
        v = m.state_dict()[k].double()
        assert abs(float(v.sum()) - s) <= 1e-9 * max(1.0, abs(a)) and abs(float(v.abs().sum()) - a) <= 1e-9 * max(1.0, a), k


def test_block_geometry_mask_and_window_plan_tables():
    fx = np.load(os.path.join(GOLD, "masks.npz"))
    blk = N.SwinTransformerV2CrBlock(dim=8, num_heads=1, feat_size=(18, 36), window_size=(9, 18), shift_size=(4, 9), rel_pos=False)
    assert torch.equal(blk.attn_mask, torch.from_numpy(fx["18_36_9_18_4_9"]))
    blk = N.SwinTransformerV2CrBlock(dim=8, num_heads=1, feat_size=(9, 36), window_size=(9, 18), shift_size=(4, 9), rel_pos=True)
    assert blk.shift_size == (0, 9) and float(blk.attn_mask.abs().max()) == 0.0      # W shift only: all-zero mask
    # float32 log of small integers, computed on the host: the CPU's vector math may round the last bit either way (one ulp)
    got, exp = blk.attn.relative_coordinates_log, torch.from_numpy(fx["relcoords_9_18"])
    ulp = torch.nextafter(exp.abs(), torch.tensor(float("inf"))) - exp.abs()
    assert torch.equal(got.sign(), exp.sign()) and bool(((got - exp).abs() <= ulp).all())
    # the kernels' index table = oracle gather index (+ batch offset), -1 on the padded rows; closed-form mask threshold
    from swin_v2_weather_amd.ops import WindowPlan
    import swin_v2_weather_amd.ops as ops
    orig = ops.attn_geometry
    ops.attn_geometry = lambda Lw, d: (64 if Lw <= 64 else 176, 16 if d <= 16 else 32)       # no library call needed
    try:
        plan = WindowPlan(2, 12, 18, 6, 9, 3, 4, 2, 12, torch.device("cpu"))
    finally:
        ops.attn_geometry = orig
    idx = O.window_token_index(12, 18, 6, 9, 3, 4)
    tab = plan.rowidx.view(2, 4, 64)
    assert torch.equal(tab[0, :, :54].long(), idx) and torch.equal(tab[1, :, :54].long(), idx + 12 * 18)
    assert int(tab[:, :, 54:].max()) == -1 and plan.mask_thr == (6 - 3) * 9
    mask = O.shift_mask(12, 18, 6, 9, 3, 4)
    tok = torch.arange(54)
    closed = torch.where((tok.view(-1, 1) >= plan.mask_thr) != (tok.view(1, -1) >= plan.mask_thr), -100.0, 0.0)
    assert torch.equal(mask[-1], closed) and float(mask[0].abs().max()) == 0.0
    # head padding maps (d = 12 -> DP = 16)
    assert plan.proj_map.tolist()[:16] == list(range(12)) + [-1] * 4 and plan.qkv_map.numel() == 3 * 2 * 16
    assert plan.qkv_map[2 * 16 + 1] == 24 + 1          # part 1 (k), head 0, j = 1 -> C + 1


def test_quadrature_and_loss_weights_match_fixture():
    fx = np.load(os.path.join(GOLD, "loss_aux.npz"))
    q = naive_quadrature_weights(24, 48)
    torch.testing.assert_close(q.unsqueeze(1).repeat(1, 48), torch.from_numpy(fx["quad_24_48"]), rtol=1e-6, atol=1e-10)
    gq = GridQuadrature('naive', (24, 48), crop_shape=(24, 48), normalize=True)
    x = torch.randn(2, 3, 24, 48)
    torch.testing.assert_close(gq(x), (x * torch.from_numpy(fx["quad_24_48"])).sum((-2, -1)))
    from swin_v2_weather_amd.utils.losses import auto_channel_weights
    names = YParams(CFG, 'swin_73var').channel_names
    torch.testing.assert_close(auto_channel_weights(names, 73), O.auto_channel_weights(names, 73))


# ---- synthetic ERA5 loader: the reference's index arithmetic (data_loader_era5.py:149-181) -------------------
def loader_params(**kw):
    p = YParams(CFG, 'bench_tiny')
    p['n_in_channels'], p['n_out_channels'] = 73, 73
    p['in_channels'], p['out_channels'] = np.arange(73), np.arange(73)
    p['img_size'] = [16, 24]
    p['synthetic_device_pool'] = 0
    p['synthetic_samples_per_year'] = 10
    p['local_batch_size'], p['num_data_workers'] = 2, 0
    for k, v in kw.items():
        p[k] = v
    return p


def test_dataset_index_arithmetic_and_tensor_contract():
    p = loader_params(n_future=1, add_zenith=True)
    ds = GetDataset(p, "unused", train=True)
    assert len(ds) == 20
    # known answers from the cited lines: local = idx % (N - dt*(n_future+1)); local < dt -> += dt
    assert ds.index(0) == (0, 1) and ds.index(7) == (0, 7) and ds.index(8) == (0, 1) and ds.index(9) == (0, 1)
    assert ds.index(13) == (1, 3) and ds.index(19) == (1, 1)
    inp, tar, zi, zt = ds[3]
    assert inp.shape == (73, 16, 24) and tar.shape == (146, 16, 24) and zi.shape == (1, 16, 24) and zt.shape == (2, 16, 24)
    # the target slab is the next two time steps of the same virtual file: tar[:73] of sample 3 == inp of sample 4
    inp4 = ds[4][0]
    assert torch.equal(tar[:73], inp4)
    assert float(zi.abs().max()) <= 1.0
    loader, dataset, sampler = get_data_loader(p, "unused", distributed=False, train=True)
    batch = next(iter(loader))
    assert batch[0].shape == (2, 73, 16, 24) and batch[1].shape == (2, 146, 16, 24) and sampler is None


# ---- host input pipeline: index arithmetic, sources, invariant fields -------------------------------------
def test_pipeline_epoch_order_and_boundary_handling():
    """known answers written from utils/dali_era5_es_helper.py:163-186 (seeded permutation per epoch, contiguous shard slice,
    year lookup by offsets, the two boundary rules)"""
    from swin_v2_weather_amd.utils import host_pipeline as hp
    n, shards, seed = 103, 4, 333
    full = np.random.default_rng(seed=seed + 2).permutation(n)
    parts = [hp.epoch_order(n, shards, r, seed, 2, True) for r in range(shards)]
    assert all(len(p_) == n // shards for p_ in parts)
    assert np.array_equal(np.concatenate(parts), full[: (n // shards) * shards])            # disjoint, in permutation order
    assert not np.array_equal(hp.epoch_order(n, shards, 0, seed, 3, True), parts[0])        # re-drawn per epoch
    assert np.array_equal(hp.epoch_order(n, shards, 1, seed, 0, False), np.arange(25, 50))  # validation: identity order
    offs, ny = [0, 1460, 2924], [1460, 1464, 1460]
    assert hp.locate(0, offs, ny, 1, 0) == (0, 1)                   # local < step  -> += step
    assert hp.locate(1459, offs, ny, 1, 0) == (0, 1458)             # local >= n - step (nf + 1) -> n - step (nf + 1) - 1
    assert hp.locate(1460, offs, ny, 1, 1) == (1, 1)
    assert hp.locate(2923, offs, ny, 1, 1) == (1, 1461)
    assert hp.locate(2000, offs, ny, 2, 3) == (1, 540)
    assert hp.locate(2925, offs, ny, 2, 3) == (2, 3)                # local 1 < step 2 -> 3


def test_year_array_source_and_static_features_from_files(tmp_path):
    from swin_v2_weather_amd.utils import host_pipeline as hp
    from swin_v2_weather_amd.utils.preprocess_utils import build_static_features
    rng = np.random.default_rng(0)
    for yr, n in ((1980, 5), (1979, 4)):
        np.save(tmp_path / f"era5_{yr}.npy", rng.standard_normal((n, 3, 9, 16)).astype(np.float32))
    src = hp.YearArraySource(str(tmp_path))
    assert src.years == [1979, 1980] and src.n_samples_year == [4, 5] and src.shape == (3, 9, 16)
    out = np.empty((3, 9, 16), np.float32)
    src.read(1, 2, out)
    assert np.array_equal(out, np.load(tmp_path / "era5_1980.npy")[2])
    # invariant fields from files (conditioning_inputs.py:23-40, preprocess_utils.py:15-45)
    lsm = (rng.random((1, 9, 16)) < 0.4).astype(np.int64)
    z = rng.standard_normal((1, 9, 16)).astype(np.float32) * 3000.0
    np.save(tmp_path / "lsm.npy", lsm)
    np.save(tmp_path / "orog.npy", z)
    p = SimpleNamespace(img_size=(8, 16), add_landmask=True, add_orography=True)
    pd = {"landmask_path": str(tmp_path / "lsm.npy"), "orography_path": str(tmp_path / "orog.npy")}

    class P(dict):
        __getattr__ = dict.__getitem__
    sf = build_static_features(P(img_size=(8, 16), add_landmask=True, add_orography=True, **pd))
    assert sf.shape == (1, 3, 8, 16)
    assert torch.equal(sf[0, 0], torch.from_numpy((lsm[0] == 0).astype(np.float32))[:8])       # one_hot: channel 0 = class 0
    assert torch.equal(sf[0, 1], torch.from_numpy((lsm[0] == 1).astype(np.float32))[:8])
    o = torch.from_numpy(z[0])
    o = ((o - o.min()) / (o.max() - o.min()))[:8]
    assert torch.allclose(sf[0, 2], (o - o.mean()) / (o.std() + 1e-6), atol=1e-6)
    del p


def test_year_array_source_reads_hdf5_year_files(tmp_path, h5py_mod):
    """the reference's storage format (data_loader_era5.py:65-95: one `<name>_<year>.h5` per year with a 'fields' dataset):
    round trip through YearArraySource's HDF5 branch.  h5py is an optional dependency that this image does not ship: the
    branch then runs against tests/conftest.py's stand-in module (File -> datasets with .shape and [t]) instead of being skipped."""
    h5py = h5py_mod
    from swin_v2_weather_amd.utils import host_pipeline as hp
    rng = np.random.default_rng(2)
    data = {}
    for yr, n in ((2017, 3), (2016, 4)):
        data[yr] = rng.standard_normal((n, 5, 9, 16)).astype(np.float32)
        with h5py.File(tmp_path / f"era5_{yr}.h5", "w") as f:
            f.create_dataset("fields", data=data[yr])
    src = hp.YearArraySource(str(tmp_path))
    assert src.years == [2016, 2017] and src.n_samples_year == [4, 3] and src.shape == (5, 9, 16)
    out = np.empty((5, 9, 16), np.float32)
    for y, t in ((0, 3), (1, 0), (1, 2)):
        src.read(y, t, out)
        assert np.array_equal(out, data[src.years[y]][t])


def test_year_array_source_without_h5py_fails_loudly(tmp_path, monkeypatch):
    """an `.h5` year file on a box without h5py must raise where the file is opened (and, inside the pipeline's producer thread,
    reach the training loop as an exception -- ADVICE r2 -- instead of a silent hang)"""
    import builtins
    from swin_v2_weather_amd.utils import host_pipeline as hp
    (tmp_path / "era5_2016.h5").write_bytes(b"not really hdf5")
    real_import = builtins.__import__

    def no_h5py(name, *a, **k):
        if name == "h5py":
            raise ImportError("No module named 'h5py'")
        return real_import(name, *a, **k)
    monkeypatch.setattr(builtins, "__import__", no_h5py)
    with pytest.raises((ImportError, OSError)):
        src = hp.YearArraySource(str(tmp_path))
        src.read(0, 0, np.empty((1, 1, 1), np.float32))


def test_unsupported_attention_geometry_fails_at_construction():
    """head dims above 128 (e.g. the upstream 2048 / 8 = 256 variant) and windows above 176 tokens have no kernel: the model
    constructor says so instead of the first forward; the yaml default width 768 / 8 = 96 builds."""
    kw = dict(img_size=(48, 72), patch_size=4, depths=(1,), in_chans=3, out_chans=3, img_window_ratio=8, full_pos_embed=True, rel_pos=False)
    N.SwinTransformerV2Cr(num_heads=(8,), embed_dim=768, **kw)
    with pytest.raises(L.Swv2Error, match="head_dim"):
        N.SwinTransformerV2Cr(num_heads=(8,), embed_dim=2048, **kw)
    with pytest.raises(L.Swv2Error, match="window area"):
        N.SwinTransformerV2Cr(num_heads=(2,), embed_dim=32, **dict(kw, img_window_ratio=2))


def test_hip_adam_on_cpu_parameters_takes_torchs_path():
    """utils/optim.HipAdam never drops a parameter it cannot update with the HIP kernel: CPU tensors (no GPU here) and
    option combinations the kernel does not implement go through torch.optim.Adam's own step -- same numbers as torch's
    optimizer, same state_dict layout."""
    from swin_v2_weather_amd.utils.optim import HipAdam
    torch.manual_seed(0)
    pa = [torch.nn.Parameter(torch.randn(5, 3)), torch.nn.Parameter(torch.randn(7))]
    pb = [torch.nn.Parameter(p.detach().clone()) for p in pa]
    oa = HipAdam(pa, lr=1e-2, betas=(0.9, 0.95), weight_decay=0.01)
    ob = torch.optim.Adam(pb, lr=1e-2, betas=(0.9, 0.95), weight_decay=0.01)
    for _ in range(3):
        for a, b in zip(pa, pb):
            g = torch.randn_like(a)
            a.grad, b.grad = g.clone(), g.clone()
        oa.step()
        ob.step()
    for a, b in zip(pa, pb):
        assert torch.equal(a, b)
    sa, sb = oa.state_dict(), ob.state_dict()
    assert sa["state"].keys() == sb["state"].keys() and all(float(sa["state"][k]["step"]) == 3.0 for k in sa["state"])


def test_bench_launch_contract_without_a_gpu():
    """`python bench.py --gpus N` as the driver invokes it: with WORLD_SIZE unset and N > 1 the process
    becomes the launcher of N child ranks before any GPU call and returns THEIR exit code (here: non-zero, no GPU, and no
    JSON line); with a launcher environment whose size differs from --gpus it refuses instead of printing a smaller job."""
    import subprocess
    import sys
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")         # the ranks see no GPU, also on a host that has one
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    bench = os.path.join(ROOT, "bench.py")
    r = subprocess.run([sys.executable, bench, "--gpus", "2", "--backend", "gloo", "--steps", "1", "--warmup", "0"], env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode != 0 and not r.stdout.strip()
    assert b"needs an MI355X" in r.stderr            # printed by the CHILD ranks: the launch happened
    r = subprocess.run([sys.executable, bench, "--gpus", "8"], env=dict(env, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0"),
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode != 0 and not r.stdout.strip() and b"WORLD_SIZE=1" in r.stderr


def test_ddp_bucket_plan_overlaps_backward_and_isolates_pos_embed():
    """train.py:186-190 / north star "gradient all-reduce overlapped with backward": at the shipped bucket cap the BASELINE cfg-2
    model's block gradients (0.79 MB per block, ready block by block, last block first) form >= 4 buckets that are launched while
    earlier blocks are still in backward, no such bucket exceeds the cap by more than one block, and pos_embed (33.2 MB, ready
    right after block 0) closes a bucket of its own tail instead of collecting the whole model (round 3's cap of 12 MB gave
    [1.13, 42.77] MB: 97 % of the bytes started at the end of backward)."""
    p = SimpleNamespace(nettype="swin", img_size=[720, 1440], patch_size=4, depth=12, num_heads=8, n_in_channels=73, n_out_channels=73,
                        embed_dim=128, window_ratio=80, drop_path_rate=0.1, full_pos_embed=True, rel_pos=False, mlp_ratio=4,
                        activation_ckpt=False, residual=False, n_future=0, add_orography=False, add_landmask=False)
    model = helpers.get_model(p)
    cap = helpers.DDP_BUCKET_CAP_MB
    sizes, where = helpers.ddp_bucket_plan(model)
    # >= 4 block buckets before pos_embed's (an explicit bucket_cap_mb also caps the FIRST bucket: torch's 1 MB first-bucket limit
    # applies only with the default cap -- found in round 5 by comparing this plan with the reducer's own report, ddp_observed_buckets)
    assert where >= 4, (sizes, where)
    block_mb = sum(q.numel() for n, q in model.named_parameters() if ".blocks.0." in n) * 4 / 1e6
    assert all(s <= cap * 1.048576 + block_mb for s in sizes[:where]), sizes
    pos_mb = model.model.pos_embed.numel() * 4 / 1e6
    assert sizes[where] <= pos_mb + cap * 1.048576 + block_mb, sizes  # pos_embed + at most the open bucket it closes
    assert abs(sum(sizes) - sum(q.numel() for q in model.parameters()) * 4 / 1e6) < 0.1
    old, old_where = helpers.ddp_bucket_plan(model, 12)
    assert len(old) <= 3 and old[old_where] > 40                      # what the fix replaces
    import inspect
    from swin_v2_weather_amd import train as T
    assert "DDP_BUCKET_CAP_MB" in inspect.getsource(T.Trainer.__init__) or "DDP_BUCKET_CAP_MB" in inspect.getsource(T)


def _kernel_resources(source, tmp_path):
    """{kernel symbol: {"ScratchSize [bytes/lane]": n, "VGPRs Spill": n}} from the compiler's own resource report of one csrc file
    (cross-compiled for gfx950, no GPU needed)"""
    import subprocess
    src = os.path.join(L.CSRC, source)
    r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Rpass-analysis=kernel-resource-usage",
                        "-c", src, "-o", str(tmp_path / (source + ".o"))], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    seen = {}
    name = None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            continue
        m = re.search(r"(ScratchSize \[bytes/lane\]|VGPRs Spill): (\d+)", line)
        if m and name:
            seen.setdefault(name, {})[m.group(1)] = int(m.group(2))
    return seen


def test_dma_kernels_with_hand_counted_waits_use_no_scratch(tmp_path):
    """csrc/gemm_tn_slab.hip retires its LDS-DMA loads with hand-counted `s_waitcnt vmcnt(N)`: a register spill is a VMEM operation
    the count does not know about (a reload would be waited for too early or too late).  The compiler's own resource report must
    show 0 bytes of scratch and 0 spilled VGPRs for both slab kernels (cross-compiled for gfx950, no GPU needed)."""
    seen = _kernel_resources("gemm_tn_slab.hip", tmp_path)
    slab = {k: v for k, v in seen.items() if "gemm_tn_slab_c" in k}
    assert len(slab) == 2, sorted(seen)
    for k, v in slab.items():
        assert v.get("ScratchSize [bytes/lane]") == 0 and v.get("VGPRs Spill") == 0, (k, v)


def test_wide_weight_gradient_kernels_use_no_scratch(tmp_path):
    """the same for csrc/gemm_tn_wide.hip: the three gemm_tn_wide_kernel instantiations (bf16 x bf16, bf16 x head-major, head-major x
    bf16) keep three stages of LDS-DMA in flight and wait on `s_waitcnt vmcnt(8)` by hand"""
    seen = _kernel_resources("gemm_tn_wide.hip", tmp_path)
    wide = {k: v for k, v in seen.items() if "gemm_tn_wide_kernel" in k}
    assert len(wide) == 3, sorted(seen)
    for k, v in wide.items():
        assert v.get("ScratchSize [bytes/lane]") == 0 and v.get("VGPRs Spill") == 0, (k, v)


def test_rollout_loss_hand_over_bookkeeping():
    """host logic of LossHandler.fused_with for rollouts (utils/losses.py::_LossCtx): the per-step sums are concatenated in channel order only
    when EVERY channel block of the concatenated prediction was offered exactly once for this result buffer; anything else falls back to the
    two-pass kernels (returns None).  Also: the residual pitch helper mirrors SWV2_LOSS_RESID_PITCH of the header."""
    from swin_v2_weather_amd.utils.losses import _LossCtx
    from swin_v2_weather_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "swv2.h")).read()
    assert "#define SWV2_LOSS_RESID_PITCH(N) (((N) + 63) / 64 * 64)" in hdr
    assert [L.loss_resid_pitch(n) for n in (64, 80, 1168, 1216)] == [64, 128, 1216, 1216]
    B, Cout, S = 2, 3, 3
    result = torch.zeros(B, S * Cout, 4, 8)
    tar = torch.zeros(B, S * Cout, 4, 8)
    sums = [torch.full((8, B, Cout, 2), float(s)) for s in range(S)]
    lc = _LossCtx(tar, torch.ones(4))
    assert lc.rollout_sums(result, Cout) is None                      # nothing offered
    for s in (2, 0, 1):                                                  # any order
        lc.offer_step(result, s * Cout, sums[s])
    got = lc.rollout_sums(result, Cout)
    assert got is not None and tuple(got.shape) == (8, B, S * Cout, 2)
    assert [float(got[0, 0, c, 0]) for c in range(S * Cout)] == [0.0] * 3 + [1.0] * 3 + [2.0] * 3
    assert lc.rollout_sums(result.clone(), Cout) is None                # another buffer
    lc.offer_step(result, 0, sums[0])                                    # a block offered twice (e.g. a recomputed forward)
    assert lc.rollout_sums(result, Cout) is None
    lc2 = _LossCtx(tar, torch.ones(4))
    lc2.offer_step(result, 0, sums[0]); lc2.offer_step(result, 2 * Cout, sums[2])     # a step declined
    assert lc2.rollout_sums(result, Cout) is None
    other = torch.zeros_like(result)
    lc2.offer_step(other, 0, sums[0])                                    # a new result buffer starts a new collection
    assert lc2.result_ptr == other.data_ptr() and len(lc2.steps) == 1


@pytest.mark.skipif(os.environ.get("SWV2_TEST_SANITIZERS", "0") == "0",
                    reason="opt-in (SWV2_TEST_SANITIZERS=1): rebuilds every source with host-side ASAN + UBSAN, ~3 minutes on 8 cores; "
                           "profiles/r06_sanitize_host.txt is the committed run")
def test_host_halves_under_address_and_ub_sanitizers():
    """The host halves of the C ABI (argument checks, workspace arithmetic, block orchestration, error strings) under AddressSanitizer +
    UndefinedBehaviorSanitizer: tools/sanitize_host.sh builds csrc/*.hip with -Xarch_host -fsanitize=address,undefined and runs the
    host-side tests of this file against that library (SWV2_LIB).  CPU only: the GPU pool refuses sanitizer runs."""
    import subprocess
    r = subprocess.run([os.path.join(ROOT, "tools", "sanitize_host.sh")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=1800)
    out = r.stdout.decode()
    assert r.returncode == 0 and " passed" in out and "ERROR: AddressSanitizer" not in out and "runtime error" not in out, out[-3000:]


# ---- attention kernel selection (swv2_attn_fwd_kernel / swv2_attn_bwd_kernel) ---------------------------------------------------
def _attn_query(Lw, d, bias=None, dbg=0, bwd=False):
    """-> (return code, "FAMILY<LT,DK,LFIX>+variants") for a geometry; bias: None / "raw" / "packed" (presence only: nothing is read)"""
    from tests import attn_reference as R
    a = L.AttnArgs()
    a.L, a.head_dim, a.dbg = Lw, d, dbg
    a.bias = _FAKE if bias else None
    a.bias_pack = _FAKE if bias == "packed" else None
    info = L.AttnKernelInfo()
    lib = L.load()
    rc = (lib.swv2_attn_bwd_kernel if bwd else lib.swv2_attn_fwd_kernel)(ctypes.byref(a), ctypes.byref(info))
    return rc, (R.kernel_name(info, L.ATTN_K_NAMES, bwd) if rc >= 0 else None), info


def test_attention_kernel_selection_is_pinned_for_every_case_of_the_exact_tests():
    """The answer of swv2_attn_fwd_kernel / swv2_attn_bwd_kernel -- the function swv2_attn_fwd / swv2_attn_bwd dispatch on -- for every
    row of the case table of tests/test_attn_exact_gpu.py (tests/attn_reference.py::CASES), without a GPU; every first-generation
    instantiation and every other family is reached by a row."""
    from tests import attn_reference as R
    lib = L.load()
    seen_f, seen_b = set(), set()
    for c in R.CASES:
        rc, name, info = _attn_query(c.L, c.d, c.bias, c.fdbg)
        assert rc == info.family and name == c.fwd, (R.case_id(c), name)
        lp, dp = ctypes.c_int(), ctypes.c_int()
        assert lib.swv2_attn_geometry(c.L, c.d, ctypes.byref(lp), ctypes.byref(dp)) == 0 and (info.Lp, info.DP) == (lp.value, dp.value)
        assert (info.LT, info.DK) == (info.Lp // 16, info.DP // 16)
        if c.fdbg == 0 and c.bias != "raw":         # swv2_attn_fwd_regime is the same answer (it speaks of a packed table)
            assert lib.swv2_attn_fwd_regime(c.L, c.d, int(bool(c.bias)), 0) == info.regime
        assert info.regime == int(name.startswith("FWD3"))
        seen_f.add(name)
        rc, name, info = _attn_query(c.L, c.d, c.bias, c.bdbg, bwd=True)
        assert rc == info.family and name == c.bwd, (R.case_id(c), name)
        seen_b.add(name)
    rows = ["<11,1,162>", "<4,1,54>", "<4,1,0>", "<4,2,0>", "<11,1,0>", "<11,2,162>", "<11,2,0>", "<4,4,0>", "<4,6,0>", "<11,6,0>", "<4,8,0>",
            "<11,4,0>", "<11,8,0>"]                  # SWV2_ATTN_ROWS of csrc/attn.hip
    for r in rows:
        assert "FIRST_GEN" + r in seen_f, r
        assert any(n.startswith("FIRST_GEN" + r) for n in seen_b), r
    # every first-generation instantiation, forward and backward, without a table, with a raw and with a packed one, at the smallest and the
    # largest window area of its layout (the rows specialised for one area: that area)
    for (LT, DK, LFIX) in R.FIRST_GEN_ROWS:
        name = f"FIRST_GEN<{LT},{DK},{LFIX}>"
        areas = {LFIX} if LFIX else ({9, 64} if LT == 4 else {65, 176})
        for form in (None, "raw", "packed"):
            for attr in ("fwd", "bwd"):
                got = {c.L for c in R.CASES if c.bias == form and getattr(c, attr).split("+")[0] == name}
                assert areas <= got, (name, form, attr, got)
    assert sorted(f"<{a},{b},{c}>" for a, b, c in R.FIRST_GEN_ROWS) == sorted(rows)
    for fam in ("FWD3<", "FWD3W<", "FWD3B<", "WIDE<", "D256<"):
        assert any(n.startswith(fam) for n in seen_f), fam
    for fam in ("STREAM<", "WIDE<", "D256<"):
        assert any(n.startswith(fam) for n in seen_b), fam
    for var in ("+aug", "+aug+biaslds", "+biaslds", "+qg"):
        assert any(n.startswith("FIRST_GEN") and n.endswith(">" + var) for n in seen_b), var


def test_attention_kernel_selection_switches_and_refusals():
    q = lambda *a, **k: _attn_query(*a, **k)[1]          # noqa: E731
    # each dbg switch, where it selects another kernel -- and where it does not apply
    assert q(162, 16) == "FWD3<11,1,162>" and q(162, 16, dbg=L.ATTN_FIRST_GEN) == "FIRST_GEN<11,1,162>"
    assert q(170, 24) == "FWD3W<11,2,0>" and q(170, 24, dbg=L.ATTN_FIRST_GEN) == "FIRST_GEN<11,2,0>"
    assert q(162, 16, "packed") == "FWD3B<11,1,162>" and q(162, 16, "packed", dbg=L.ATTN_FIRST_GEN) == q(162, 16, "raw") == "FIRST_GEN<11,1,162>"
    assert q(159, 16) == "FIRST_GEN<11,1,0>" and q(160, 16) == "FWD3<11,1,0>"          # attn2.hip's L >= 160 rule
    assert q(162, 96) == "WIDE<11,6,162>" and q(162, 96, dbg=L.ATTN_FIRST_GEN) == "FIRST_GEN<11,6,0>" and q(162, 96, "raw") == "FIRST_GEN<11,6,0>"
    assert q(162, 100) == "FIRST_GEN<11,8,0>" and q(64, 96) == "FIRST_GEN<4,6,0>" and q(65, 96) == "WIDE<11,6,0>"
    assert q(162, 256) == q(162, 256, dbg=L.ATTN_FIRST_GEN) == "D256<11,16,162>"
    assert q(162, 16, bwd=True) == "STREAM<11,1,162>+aug"
    assert q(162, 16, dbg=L.ATTN_BWD_TWO_PHASE, bwd=True) == "FIRST_GEN<11,1,162>+aug"
    assert q(162, 16, dbg=L.ATTN_PLAIN_STATS, bwd=True) == "FIRST_GEN<11,1,162>"
    assert q(162, 16, dbg=L.ATTN_FIRST_GEN, bwd=True) == "STREAM<11,1,162>+aug"            # (a forward switch)
    assert q(54, 16, dbg=L.ATTN_BWD_TWO_PHASE, bwd=True) == q(54, 16, bwd=True) == "FIRST_GEN<4,1,54>+aug"
    assert q(54, 24, bwd=True) == "FIRST_GEN<4,2,0>+aug" and q(54, 24, dbg=L.ATTN_PLAIN_STATS, bwd=True) == "FIRST_GEN<4,2,0>"
    assert q(162, 16, "packed", bwd=True) == "FIRST_GEN<11,1,162>+aug+biaslds"
    assert q(162, 16, "packed", dbg=L.ATTN_PLAIN_STATS, bwd=True) == "FIRST_GEN<11,1,162>+biaslds"
    assert q(170, 16, "packed", bwd=True) == "FIRST_GEN<11,1,0>+biaslds"                   # operand statistics with a table need a fixed L
    assert q(162, 96, bwd=True) == "WIDE<11,6,162>" and q(162, 96, dbg=L.ATTN_FIRST_GEN, bwd=True) == "FIRST_GEN<11,6,0>+qg"
    assert q(162, 64, bwd=True) == "FIRST_GEN<11,4,0>" and q(162, 128, bwd=True) == "FIRST_GEN<11,8,0>+qg"
    assert q(162, 256, dbg=L.ATTN_PLAIN_STATS | L.ATTN_BWD_TWO_PHASE, bwd=True) == "D256<11,16,162>"
    # refused geometries: negative return, a message, nothing launched (there is no GPU here)
    lib = L.load()
    for bwd in (False, True):
        for (Lw, d, bias) in ((162, 132, None), (162, 192, None), (162, 252, None), (162, 256, "raw"), (162, 256, "packed"), (64, 256, None),
                              (9, 256, None), (177, 16, None), (400, 16, None), (162, 18, None)):
            rc, name, _ = _attn_query(Lw, d, bias, bwd=bwd)
            assert rc < 0 and name is None and lib.swv2_last_error(), (Lw, d, bias, bwd)
    assert lib.swv2_attn_fwd_kernel(None, None) == -1
    a = L.AttnArgs()
    a.L, a.head_dim = 162, 16
    assert lib.swv2_attn_fwd_kernel(ctypes.byref(a), None) == L.ATTN_K_FWD3           # `out` is optional
