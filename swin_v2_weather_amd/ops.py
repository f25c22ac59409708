"""Thin tensor-level wrappers over the C ABI (include/swv2.h).

PyTorch is used for device memory, streams and autograd bookkeeping only; every arithmetic op of the hot path is a
HIP kernel in libswv2.so.  All wrappers enqueue on torch's current stream.
"""
from __future__ import annotations

import ctypes as C
import functools
import math
from typing import Optional

import torch

from . import _lib as L

BF16 = torch.bfloat16


def _p(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ---- optional per-kernel event timing (bench.py): HIP events on the launch stream around selected entry points ----
_TIMED = None          # None or dict name -> list of (start_event, end_event)


_EVERY = 1
_EVPOOL = []            # event pairs whose hipEvent_t handles exist already (materialised OUTSIDE any timed region)


def prewarm_events(n):
    """Create n HIP event pairs now (an event's handle is created by its first record, which is a packet on the stream)."""
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); b.record()
        _EVPOOL.append((a, b))


def _event_pair():
    if _EVPOOL:
        return _EVPOOL.pop()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); b.record()                       # materialise the hipEvent_t handles (re-recorded by the library)
    return a, b


def start_kernel_timing(names, every=1):
    """Bracket launches of the named kernels with HIP event pairs on the launch stream.  `every` = N: only every N-th eligible
    block call gets a pair -- an event record between two kernels is a packet the next kernel waits behind (measured: one pair per
    block call, 24 per step, costs 3.3 % of the benchmark step), so a timed region samples instead of bracketing everything."""
    global _TIMED, _EVERY
    _TIMED = {n: [] for n in names}
    _EVERY = max(1, int(every))
    _RR["fwd"] = _RR["bwd"] = 0


def stop_kernel_timing():
    """-> {name: (launches, mean_ms)}; synchronises."""
    global _TIMED
    rec, _TIMED = _TIMED, None
    torch.cuda.synchronize()
    out = {n: (len(ev), sum(a.elapsed_time(b) for a, b in ev) / max(len(ev), 1)) for n, ev in (rec or {}).items()}
    for ev in (rec or {}).values():
        _EVPOOL.extend(ev)
    return out


BLOCK_KERNEL_IDS = {"qkv": 1, "attn_fwd": 2, "proj": 3, "ln1_fwd": 4, "fc1": 5, "fc2": 6, "ln2_fwd": 7, "ln2_bwd": 11,
                    "wgrad_fc2": 12, "dh": 13, "wgrad_fc1": 14, "dx1": 15, "ln1_bwd": 16, "wgrad_proj": 17, "doh": 18,
                    "attn_bwd": 19, "wgrad_qkv": 20, "dx": 21,
                    # fused kernels share the launch slot of the first kernel they replace
                    "proj_ln_fwd": 3, "mlp_fwd": 5, "mlp_bwd": 13, "proj_ln_bwd": 16,
                    # the four weight gradients of a block as one grouped launch + its partial-tile reduction
                    "wgrad_group": 22}


_RR = {"fwd": 0, "bwd": 0}


def block_event_pair(phase, desc):
    """If kernels of this phase ("fwd": launch ids 1-7, "bwd": 11-22; swv2_block_step_id holds the same table) are being timed (start_kernel_timing), attach a
    fresh HIP event pair to the block descriptor so that swv2_block_fwd/bwd brackets exactly ONE launch on the launch
    stream; with several requested kernels of a phase the calls take turns (round robin over the blocks of the step)."""
    desc.ev_kernel = 0
    rec = _TIMED
    if rec is None:
        return
    mine = [n for n in rec if BLOCK_KERNEL_IDS.get(n, 0) and ((BLOCK_KERNEL_IDS[n] < 10) == (phase == "fwd"))]
    if not mine:
        return
    turn = _RR[phase]
    _RR[phase] += 1
    if turn % _EVERY:
        return
    n = mine[(turn // _EVERY) % len(mine)]
    a, b = _event_pair()
    desc.ev_kernel, desc.ev_start, desc.ev_stop = BLOCK_KERNEL_IDS[n], a.cuda_event, b.cuda_event
    rec[n].append((a, b))


def _timed(name, fn, *args):
    rec = _TIMED
    if rec is None or name not in rec:
        return fn(*args)
    a, b = _event_pair()
    a.record()
    r = fn(*args)
    b.record()
    rec[name].append((a, b))
    return r


def _chk(t: torch.Tensor, dtype, name: str):
    if t.dtype != dtype or not t.is_contiguous() or not t.is_cuda:
        raise L.Swv2Error(f"{name}: expected a contiguous CUDA {dtype} tensor, got {t.dtype} "
                          f"contiguous={t.is_contiguous()} device={t.device}")
    return t


def attn_geometry(Lwin: int, head_dim: int):
    lp, dp = C.c_int(), C.c_int()
    L.check(L.load().swv2_attn_geometry(Lwin, head_dim, C.byref(lp), C.byref(dp)), "swv2_attn_geometry")
    return lp.value, dp.value


# ---- operand / epilogue builders ---------------------------------------------------------------------------
def operand(kind, t, rows, cols, ld=0, rowidx=None, aux=(None, None, None, None), p=(0, 0, 0, 0)) -> L.Operand:
    o = L.Operand()
    o.kind, o.ptr, o.rowidx = kind, _p(t), _p(rowidx)
    o.aux0, o.aux1, o.aux2, o.aux3 = (_p(a) for a in aux)
    o.ld, o.rows, o.cols = ld, rows, cols
    o.p = (C.c_int * 4)(*p)
    o._keep = (t, rowidx, aux)
    return o


def op_f32(x2d: torch.Tensor, rows=None, rowidx=None):
    _chk(x2d, torch.float32, "op_f32")
    return operand(L.OP_F32, x2d, rows if rows is not None else x2d.shape[0], x2d.shape[1], x2d.shape[1], rowidx)


def op_bf16(x2d: torch.Tensor, rows=None, rowidx=None, gelu=False):
    _chk(x2d, BF16, "op_bf16")
    return operand(L.OP_BF16_GELU if gelu else L.OP_BF16, x2d, rows if rows is not None else x2d.shape[0],
                   x2d.shape[1], x2d.shape[1], rowidx)


def op_bf16_cscale(x2d: torch.Tensor, coef: torch.Tensor, rows_per_sample: int, cols: int = 0):
    """bf16 rows scaled on load by coef[row // rows_per_sample][col // 16] (fp32 [B, cols / 16]); `cols` < x2d.shape[1]: only the first
    `cols` columns of every row are the operand (the loss epilogue's residual: rows padded to whole cache lines)"""
    _chk(x2d, BF16, "op_bf16_cscale"); _chk(coef, torch.float32, "op_bf16_cscale coef")
    cols = cols or x2d.shape[1]
    if coef.dim() != 2 or coef.shape[1] * 16 != cols or coef.shape[0] * rows_per_sample != x2d.shape[0] or cols > x2d.shape[1]:
        raise L.Swv2Error(f"op_bf16_cscale: coef {tuple(coef.shape)} does not match rows {x2d.shape[0]} / {rows_per_sample}, cols {cols}")
    return operand(L.OP_BF16_CSCALE, x2d, x2d.shape[0], cols, x2d.shape[1], aux=(coef, None, None, None),
                   p=(rows_per_sample, 0, coef.shape[1], 0))


def op_heads(t: torch.Tensor, Bw, heads, parts, Lp, DP):
    _chk(t, BF16, "op_heads")
    return operand(L.OP_HEADS, t, Bw * Lp, parts * heads * DP, parts, p=(heads, 0, Lp, DP))


def op_patch(x4d: torch.Tensor):
    _chk(x4d, torch.float32, "op_patch")
    B, Cin, H, W = x4d.shape
    return operand(L.OP_PATCH, x4d, B * (H // 4) * (W // 4), Cin * 16, 0, p=(Cin, H, W, 0))


def op_merge_ln(x4d, mean, rstd, gamma, beta):
    B, H, W, Cc = x4d.shape
    return operand(L.OP_MERGE_LN, x4d, B * (H // 2) * (W // 2), 4 * Cc, 0, aux=(mean, rstd, gamma, beta), p=(H, W, Cc, 0))


def epilogue(kind, out, ld=0, bias=None, aux=None, aux_out=None, rowidx=None, p=(0, 0, 0, 0, 0), loss=None) -> L.Epilogue:
    """loss (EPI_UNPATCH_LOSS) = (tar [B, Ct, H, W] fp32, quadrature row weights [H], per-group partial sums
    [ceil(M / LOSS_GROUP_ROWS), 2, Cout, 2] fp32, residual bf16 [M, N], first target channel[, base]); `out` (or, in rollouts, the
    tensor `base` that `out` is a channel slice of, with p[4] = its channels per sample), the residual and a second destination
    `aux_out` must have LOSS_DUMP_BYTES of allocated memory behind them; follow the launch with loss_part_reduce"""
    e = L.Epilogue()
    e.kind, e.out, e.bias, e.aux, e.aux_out, e.rowidx, e.ld = kind, _p(out), _p(bias), _p(aux), _p(aux_out), _p(rowidx), ld
    e.p = (C.c_int * 5)(*p)
    e._keep = (out, bias, aux, aux_out, rowidx, loss)
    if loss is not None:
        tar, qw, part, resid, coff = loss[:5]
        base = loss[5] if len(loss) > 5 else None
        _chk(tar, torch.float32, "loss target"); _chk(qw, torch.float32, "quadrature weights")
        _chk(resid, BF16, "loss residual"); _chk(part, torch.float32, "loss partial sums")
        if resid.dim() != 2 or resid.shape[1] % 64:
            raise L.Swv2Error(f"loss epilogue: residual rows must be padded to whole 128-byte lines (ops._lib.loss_resid_pitch), got {tuple(resid.shape)}")
        behind = [(out if base is None else base, "out"), (resid, "residual")] + ([(aux_out, "second destination")] if aux_out is not None else [])
        for t_, nm in behind:      # room behind the tensors for the masked lanes' stores
            room = t_.untyped_storage().nbytes() - (t_.storage_offset() + t_.numel()) * t_.element_size()
            if room < L.LOSS_DUMP_BYTES:
                raise L.Swv2Error(f"loss epilogue: {nm} needs {L.LOSS_DUMP_BYTES} bytes of allocated scratch behind it ({room} found)")
        e.loss_tar, e.loss_qw, e.loss_part, e.loss_resid = _p(tar), _p(qw), _p(part), _p(resid)
        dump = 0
        if base is not None:      # floats from `out` to the end of the tensor it is a slice of
            dump = (base.data_ptr() + base.numel() * 4 - out.data_ptr()) // 4
        e.q = (C.c_int * 3)(tar.shape[1], coff, dump)
    return e


def linear(a: L.Operand, w_bf16: torch.Tensor, e: L.Epilogue, N: int, tag: str = "linear"):
    _chk(w_bf16, BF16, "linear weight")
    if w_bf16.shape[0] != N or w_bf16.shape[1] != a.cols:
        raise L.Swv2Error(f"linear: weight {tuple(w_bf16.shape)} does not match N={N} K={a.cols}")
    L.check(_timed(tag, L.load().swv2_linear, C.byref(a), _p(w_bf16), C.byref(e), N, _stream()), "swv2_linear")


def linear_wgrad(dy: L.Operand, x: L.Operand, dW: torch.Tensor, db: Optional[torch.Tensor], nmap=None, kmap=None,
                 splits: int = 0, workspace: bool = True):
    """dW += dY^T X.  workspace=True: per-slice partial tiles + reduce kernel (deterministic, no atomics on dW), the
    partials live in a torch allocation that is released (stream-ordered) after the call; False: fp32 atomics on dW.
    splits = 0: as many row slices as fill the chip in ONE round (two 70 KB workgroups per CU = 512): the PatchEmbed / head
    gradients (10 output tiles) ran 1280 workgroups = 2.5 rounds at 128 slices and wrote 84 MB of partial tiles."""
    _chk(dW, torch.float32, "dW")
    ldw = dW.shape[-1] if dW.dim() == 2 else dW[0].numel()
    lib = L.load()
    if splits <= 0:
        tiles = ((dy.cols + 127) // 128) * ((x.cols + 127) // 128)
        splits = max(8, (512 // tiles) // 8 * 8)
        if tiles < 3:                       # the library doubles the slice count of small outputs itself
            splits = max(8, splits // 16 * 8)
    if not workspace:
        L.check(lib.swv2_linear_wgrad(C.byref(dy), C.byref(x), _p(dW), _p(db), _p(nmap), _p(kmap), ldw, splits, _stream()),
                "swv2_linear_wgrad")
        return
    nbytes = lib.swv2_linear_wgrad_ws_bytes(dy.rows, dy.cols, x.cols, splits)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dW.device)
    L.check(lib.swv2_linear_wgrad_ws(C.byref(dy), C.byref(x), _p(dW), _p(db), _p(nmap), _p(kmap), ldw, splits, _p(ws), nbytes,
                                     _stream()), "swv2_linear_wgrad_ws")


def prep_weight(w: torch.Tensor, transpose=False, row_map=None, out_rows=None, col_map=None, out_cols=None):
    """fp32 [rows][cols] parameter -> bf16 [out_rows][out_cols] (cast / transpose / permute / zero-pad)."""
    w2 = w.detach().reshape(w.shape[0], -1)
    _chk(w2, torch.float32, "prep_weight")
    rows, cols = w2.shape
    r_t, c_t = (cols, rows) if transpose else (rows, cols)
    out_rows = out_rows if out_rows is not None else r_t
    out_cols = out_cols if out_cols is not None else c_t
    out = torch.empty(out_rows, out_cols, dtype=BF16, device=w.device)
    L.check(L.load().swv2_prep_weight(_p(w2), rows, cols, int(transpose), _p(row_map), out_rows, _p(col_map), out_cols,
                                      _p(out), _stream()), "swv2_prep_weight")
    return out


class PrepBatch:
    """Collects parameter preparations (prep_weight's arguments) and runs them as ONE swv2_prep_multi launch.  `add` returns
    the output tensor at once (a given `out` of the right shape / dtype is reused, so the pointers handed to the kernels
    stay stable); `launch` must be called before anything reads the outputs.  The device tables are cached per job-list
    identity: in steady state (same parameters, same outputs every step) nothing is uploaded."""

    _tables = {}

    def __init__(self):
        self.jobs, self.keep, self.done = [], [], []

    def on_launched(self, fn):
        """fn() runs after the launch that covers the jobs added so far has been enqueued successfully"""
        self.done.append(fn)

    def add(self, w: torch.Tensor, transpose=False, row_map=None, out_rows=None, col_map=None, out_cols=None, out=None, f32=False):
        w2 = w.detach().reshape(w.shape[0], -1)
        _chk(w2, torch.float32, "PrepBatch.add")
        rows, cols = w2.shape
        r_t, c_t = (cols, rows) if transpose else (rows, cols)
        out_rows = out_rows if out_rows is not None else r_t
        out_cols = out_cols if out_cols is not None else c_t
        dt = torch.float32 if f32 else BF16
        if out is None or out.dtype != dt or tuple(out.shape) != (out_rows, out_cols) or out.device != w.device or not out.is_contiguous():
            out = torch.empty(out_rows, out_cols, dtype=dt, device=w.device)
        self.jobs.append((_p(w2), rows, cols, int(transpose), _p(row_map), out_rows, _p(col_map), out_cols, _p(out), int(f32)))
        self.keep.append((w2, row_map, col_map, out))
        return out

    def launch(self):
        if not self.jobs:
            for fn in self.done:
                fn()
            self.done = []
            return
        lib = L.load()
        key = tuple(self.jobs)
        t = PrepBatch._tables.get(key)
        dev = self.keep[0][3].device
        if t is None:
            arr = (L.PrepItem * len(self.jobs))()
            pairs = []
            for i, j in enumerate(self.jobs):
                arr[i] = L.PrepItem(*j)                        # (w, rows, cols, transpose, row_map, out_rows, col_map, out_cols, out, f32)
                pairs += [(i, c) for c in range(lib.swv2_prep_item_chunks(j[5], j[7], j[3]))]
            host = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).clone()
            t = (host.to(dev), torch.tensor(pairs, dtype=torch.int32).to(dev), len(pairs))
            if len(PrepBatch._tables) > 64:
                PrepBatch._tables.clear()
            PrepBatch._tables[key] = t
        L.check(lib.swv2_prep_multi(_p(t[0]), _p(t[1]), t[2], _stream()), "swv2_prep_multi")
        for fn in self.done:
            fn()
        self.jobs, self.keep, self.done = [], [], []


def ln_residual_fwd(a, res, gamma, beta, scale, rowidx, y, mean, rstd, M, Cc, res_mod, rows_per_sample, eps=1e-5):
    g = L.LnArgs()
    g.a, g.res, g.gamma, g.beta, g.scale, g.rowidx = _p(a), _p(res), _p(gamma), _p(beta), _p(scale), _p(rowidx)
    g.y, g.mean, g.rstd = _p(y), _p(mean), _p(rstd)
    g.M, g.C, g.res_mod, g.rows_per_sample, g.eps = M, Cc, res_mod, rows_per_sample, eps
    L.check(L.load().swv2_ln_residual_fwd(C.byref(g), _stream()), "swv2_ln_residual_fwd")


def ln_residual_bwd(a, dy, gamma, scale, rowidx, mean, rstd, da, dgamma, dbeta, M, Cc, rows_per_sample):
    g = L.LnArgs()
    g.a, g.dy, g.gamma, g.scale, g.rowidx = _p(a), _p(dy), _p(gamma), _p(scale), _p(rowidx)
    g.mean, g.rstd, g.da, g.dgamma, g.dbeta = _p(mean), _p(rstd), _p(da), _p(dgamma), _p(dbeta)
    ws = torch.empty(L.LN_BWD_MAX_BLOCKS * 2 * Cc, dtype=torch.float32, device=a.device)
    g.ws = _p(ws)
    g.M, g.C, g.res_mod, g.rows_per_sample, g.eps = M, Cc, 0, rows_per_sample, 1e-5
    L.check(L.load().swv2_ln_residual_bwd(C.byref(g), _stream()), "swv2_ln_residual_bwd")


def attn_args(qkvh, logit_scale, bias, oh, lse, Bw, heads, Lwin, head_dim, nwh, nww, mask_thr, doh=None, rnorm=None,
              dqkvh=None, dlogit=None, dbias=None, max_chunks=64, bias_pack=None, dbias_ws=None) -> L.AttnArgs:
    a = L.AttnArgs()
    a.qkvh, a.logit_scale, a.bias, a.oh, a.lse = _p(qkvh), _p(logit_scale), _p(bias), _p(oh), _p(lse)
    a.bias_pack = _p(bias_pack)
    a.doh, a.rnorm, a.dqkvh, a.dlogit_scale, a.dbias = _p(doh), _p(rnorm), _p(dqkvh), _p(dlogit), _p(dbias)
    a.Bw, a.heads, a.L, a.head_dim, a.nwh, a.nww, a.mask_thr, a.max_chunks = Bw, heads, Lwin, head_dim, nwh, nww, mask_thr, max_chunks
    if dbias_ws is not None:        # scratch for the workgroups' d bias tables (swv2_attn_dbias_ws_bytes); the caller keeps it alive
        a.dbias_ws, a.dbias_ws_bytes = _p(dbias_ws), dbias_ws.numel() * dbias_ws.element_size()
    return a


def attn_pack_bias(bias: torch.Tensor) -> torch.Tensor:
    """[heads][L][L] fp32 CPB table -> the attention kernels' pre-packed layouts (one uint8 buffer)."""
    heads, Lw = bias.shape[0], bias.shape[1]
    out = torch.empty(L.load().swv2_attn_pack_bias_bytes(heads, Lw), dtype=torch.uint8, device=bias.device)
    L.check(L.load().swv2_attn_pack_bias(_p(bias), heads, Lw, _p(out), _stream()), "swv2_attn_pack_bias")
    return out


def attn_fwd(a: L.AttnArgs):
    L.check(_timed("attn_fwd", L.load().swv2_attn_fwd, C.byref(a), _stream()), "swv2_attn_fwd")


def attn_bwd(a: L.AttnArgs):
    L.check(_timed("attn_bwd", L.load().swv2_attn_bwd, C.byref(a), _stream()), "swv2_attn_bwd")


def batch_sum(inp: torch.Tensor, out: torch.Tensor, accumulate=False):
    B = inp.shape[0]
    n = inp[0].numel()
    L.check(L.load().swv2_batch_sum(_p(inp), _p(out), B, n, int(accumulate), _stream()), "swv2_batch_sum")


def merge_stats(x, mean, rstd, eps=1e-5):
    B, H, W, Cc = x.shape
    L.check(L.load().swv2_merge_stats(_p(x), _p(mean), _p(rstd), B, H, W, Cc, eps, _stream()), "swv2_merge_stats")


def merge_ln_bwd(x, dn, gamma, mean, rstd, dx, dgamma, dbeta):
    B, H, W, Cc = x.shape
    L.check(L.load().swv2_merge_ln_bwd(_p(x), _p(dn), _p(gamma), _p(mean), _p(rstd), _p(dx), _p(dgamma), _p(dbeta),
                                       B, H, W, Cc, _stream()), "swv2_merge_ln_bwd")


def loss_sums(prd, tar, qw, sums, ws=None):
    """sums [B, C, 2] = (sum q (prd - tar)^2, sum q tar^2) per plane, written in full; prd, tar contiguous fp32 [B, C, H, W]; ws: a
    loss_workspace to reuse (allocated here otherwise)"""
    B, Cc, H, W = prd.shape
    if ws is None:
        ws = loss_workspace(B * Cc, H, W, prd.device)
    L.check(L.load().swv2_loss_sums(_p(prd), _p(tar), _p(qw), _p(sums), B * Cc, H, W, _p(ws), ws.numel() * 4, _stream()), "swv2_loss_sums")


def loss_finalize(sums, chw, absolute: bool, squared: bool, loss, coef):
    """sums [B, C, 2] or [layers, B, C, 2] (layers added in order)"""
    layers = sums.shape[0] if sums.dim() == 4 else 1
    BC, Cc = sums.shape[-3] * sums.shape[-2], chw.numel()
    L.check(L.load().swv2_loss_finalize(_p(sums), layers, _p(chw), BC, Cc, int(absolute), int(squared), _p(loss), _p(coef), _stream()),
            "swv2_loss_finalize")


def loss_part_reduce(part, M, T, B, Cout, coff, sums):
    """per-group partial sums of the head's loss epilogue -> sums [LOSS_PART_SLICES, B, Ct, 2] (channels coff .. coff + Cout)"""
    L.check(L.load().swv2_loss_part_reduce(_p(part), M, T, B, Cout, sums.shape[2], coff, _p(sums), _stream()), "swv2_loss_part_reduce")


def loss_resid_to_image(resid, coef, out, Cout: int, add=None):
    """out[:, :Cout] = coef[b, c] * un-patchify(resid) (+ add[:, :Cout]); resid bf16 [B * T, Cout * 16], out fp32 [B, Cs, H, W] contiguous,
    add fp32 [B, Cadd, H, W] contiguous or None"""
    _chk(resid, BF16, "loss residual"); _chk(coef, torch.float32, "coef"); _chk(out, torch.float32, "out")
    B, Cs, H, W = out.shape
    if resid.shape[1] != L.loss_resid_pitch(Cout * 16):
        raise L.Swv2Error(f"loss_resid_to_image: residual rows of {resid.shape[1]} elements, expected the padded pitch {L.loss_resid_pitch(Cout * 16)}")
    if add is not None:
        _chk(add, torch.float32, "add")
    L.check(L.load().swv2_loss_resid_to_image(_p(resid), _p(coef), _p(add), _p(out), B, Cout, H, W, Cs, add.shape[1] if add is not None else 0,
                                              _stream()), "swv2_loss_resid_to_image")


def loss_finalize_sums(sums, chw, absolute: bool, squared: bool):
    """[B, C, 2] (or [layers, B, C, 2]) quadrature sums -> (loss [1], coef [B, C] = 2 d loss / d S0) in one launch"""
    B, Cc = sums.shape[-3:-1]
    buf = torch.empty(B * Cc + 1, dtype=torch.float32, device=sums.device)
    coef, loss = buf[:B * Cc].view(B, Cc), buf[B * Cc:]
    loss_finalize(sums, chw, absolute, squared, loss, coef)
    return loss, coef


def loss_grad(prd, tar, qw, coef, dprd):
    B, Cc, H, W = prd.shape
    L.check(L.load().swv2_loss_grad(_p(prd), _p(tar), _p(qw), _p(coef), _p(dprd), B * Cc, H, W, _stream()), "swv2_loss_grad")


def score_slices(planes: int, H: int, W: int) -> int:
    """slices per plane of swv2_score_sums' plan (host-only)"""
    return int(L.load().swv2_score_slices(planes, H, W))


# ---- blocks of planes read in place (DESIGN "Blocks of planes read in place"): the operand contract of every score family ----------------
ENS_MAX_MEMBERS = 64          # the M cap of swv2_ens_sums
EVENT_MAX_K = 8               # the threshold cap of swv2_event_sums / swv2_event_ens_sums
FSS_MAX_S = 8                 # the scale cap of swv2_fss_rows (its threshold cap is EVENT_MAX_K, its largest half-width 32)
QUANTILE_MAX_RANKS = 256      # the K cap of swv2_plane_order_stats
REGRID_MAX_BAND = 32          # the KH / KW cap of swv2_regrid


def _planes_in_place(t: torch.Tensor, lead: int = 1, vec=True) -> bool:
    """THE rule.  A CUDA fp32 block of planes a kernel takes where it lies: `lead` leading dimensions ([B], or [M, B] for the member view
    with 2 <= M <= ENS_MAX_MEMBERS and a member stride that is a multiple of 4), then [C, H, W] with contiguous planes; the batch
    stride, unless B == 1 (where nobody uses it), a multiple of 4 that steps over the C planes of a sample.  vec: how the kernel touches
    the planes -- True: 16-byte vectors that never straddle a row (aligned, W % 4 == 0); "plane": 16-byte vectors through the
    flattened plane (aligned, H * W % 4 == 0, H * W < 2^30); False: single elements (no further rule)."""
    if not (t.is_cuda and t.dtype == torch.float32 and t.dim() == lead + 3 and t.numel() > 0):
        return False
    B, (Cc, H, W), bs = t.shape[lead - 1], t.shape[lead:], t.stride(lead - 1)
    if tuple(t.stride()[lead:]) != (H * W, W, 1) or not (B == 1 or (bs % 4 == 0 and bs >= Cc * H * W)):
        return False
    if lead == 2 and not (2 <= t.shape[0] <= ENS_MAX_MEMBERS and t.stride(0) % 4 == 0):
        return False
    whole = {True: W % 4 == 0, "plane": (H * W) % 4 == 0 and H * W < 2 ** 30, False: None}[vec]
    return whole is None or (whole and t.data_ptr() % 16 == 0)


def _plane_block(who: str, t: torch.Tensor, lead: int = 1, vec=True):
    """t under _planes_in_place, or Swv2Error -> what the C call takes of it: (pointer, batch stride), for the member view (pointer,
    member stride, batch stride).  The batch stride handed on is the tensor's, or the span of one sample where B == 1."""
    if not _planes_in_place(t, lead, vec):
        dims = "[M, B, C, H, W] members, 2 <= M <= %d," % ENS_MAX_MEMBERS if lead == 2 else "[B, C, H, W]"
        rule = {True: ", 16-byte aligned, W % 4 == 0", "plane": ", 16-byte aligned, H * W % 4 == 0", False: ""}[vec]
        raise L.Swv2Error(f"{who}: expected a CUDA fp32 {dims} block of planes to take in place (contiguous planes{rule}; strides above the "
                          f"planes multiples of 4 that step over a sample, unless B == 1), got {tuple(t.shape)} {t.dtype} strides {t.stride()} "
                          f"on {t.device}, address % 16 = {t.data_ptr() % 16 if t.numel() else 0}")
    bs = t.stride(lead - 1) if t.shape[lead - 1] > 1 else math.prod(t.shape[lead:])
    return (t.data_ptr(), bs) if lead == 1 else (t.data_ptr(), t.stride(0), bs)


def _plane_blocks(who: str, x: torch.Tensor, tar: torch.Tensor, lead: int = 1):
    """the operand pair of the sum kernels: x ([B, ...], or the member view with lead = 2) and the truth [B, C, H, W] of the same planes on
    the same device -> _plane_block of each"""
    px, pt = _plane_block(who, x, lead), _plane_block(who, tar)
    if x.shape[lead - 1:] != tar.shape or x.device != tar.device:
        raise L.Swv2Error(f"{who}: blocks {tuple(x.shape)} on {x.device} / {tuple(tar.shape)} on {tar.device} do not name the same planes")
    return px, pt


def _row_weights(who: str, w: torch.Tensor, H: int):
    if _chk(w, torch.float32, "row weights").numel() != H:
        raise L.Swv2Error(f"{who}: {w.numel()} row weights for {H} rows")


def _plane_workspace(who: str, nbytes: int, dtype, device, limits: str = "") -> torch.Tensor:
    """nbytes (the answer of the family's swv2_*_ws_bytes) as a fresh tensor of dtype; a family that answers 0 for arguments outside its
    limits names them, and 0 is refused with that text"""
    if limits and not nbytes:
        raise L.Swv2Error(f"{who}: {limits}")
    return torch.empty(int(nbytes) // dtype.itemsize, dtype=dtype, device=device)


def score_workspace(planes: int, H: int, W: int, device) -> torch.Tensor:
    """the caller's workspace of swv2_score_sums / swv2_score_finalize for `planes` = B * C planes: allocate once, reuse"""
    return _plane_workspace("score_workspace", L.load().swv2_score_ws_bytes(planes, H, W), torch.float32, device)


def score_planes_ok(t: torch.Tensor) -> bool:
    """what swv2_score_sums takes in place: a CUDA fp32 [B, C, H, W] tensor or channel block of one (contiguous planes, W % 4 == 0)"""
    return _planes_in_place(t)


def score_sums(prd, tar, w, ws, clim=None):
    """the four weighted sums of every (b, c) plane of prd / tar (each [B, C, H, W] or a channel block `x[:, a:b]` of a wider contiguous
    tensor, scored in place) as slice partials in ws (score_workspace); w [H] row weights, clim [C, H, W] or None"""
    (pp, pbs), (tp, tbs) = _plane_blocks("score_sums", prd, tar)
    B, Cc, H, W = prd.shape
    _row_weights("score_sums", w, H); _chk(ws, torch.float32, "score workspace")
    if clim is not None and (_chk(clim, torch.float32, "climatology").shape != (Cc, H, W)):
        raise L.Swv2Error(f"score_sums: climatology {tuple(clim.shape)}, expected {(Cc, H, W)}")
    L.check(L.load().swv2_score_sums(pp, pbs, tp, tbs, _p(clim), _p(w), B, Cc, H, W, _p(ws), ws.numel() * 4, _stream()), "swv2_score_sums")


def score_finalize(ws, B: int, Cc: int, H: int, W: int, scale=None):
    """slice partials -> (sums [B, C, 4], rmse [B, C], acc [B, C], rmse_mean [C] (x scale [C] if given), acc_mean [C]), one launch;
    the five results are views of one fresh buffer"""
    _chk(ws, torch.float32, "score workspace")
    if scale is not None and _chk(scale, torch.float32, "scale").numel() != Cc:
        raise L.Swv2Error(f"score_finalize: scale of {scale.numel()} values for {Cc} channels")
    n = B * Cc
    buf = torch.empty(6 * n + 2 * Cc, dtype=torch.float32, device=ws.device)
    sums, rmse, acc = buf[:4 * n].view(B, Cc, 4), buf[4 * n:5 * n].view(B, Cc), buf[5 * n:6 * n].view(B, Cc)
    rmse_mean, acc_mean = buf[6 * n:6 * n + Cc], buf[6 * n + Cc:]
    L.check(L.load().swv2_score_finalize(_p(ws), ws.numel() * 4, B, Cc, H, W, _p(scale), _p(sums), _p(rmse), _p(acc), _p(rmse_mean),
                                         _p(acc_mean), _stream()), "swv2_score_finalize")
    return sums, rmse, acc, rmse_mean, acc_mean


def forecast_scores(prd, tar, w, clim=None, scale=None, ws=None):
    """score_sums + score_finalize; ws: a score_workspace to reuse (allocated here otherwise)"""
    B, Cc, H, W = prd.shape
    if ws is None:
        ws = score_workspace(B * Cc, H, W, prd.device)
    score_sums(prd, tar, w, ws, clim)
    return score_finalize(ws, B, Cc, H, W, scale)


def l1_workspace(planes: int, H: int, W: int, device) -> torch.Tensor:
    """the caller's workspace of swv2_l1_sums / swv2_l1_finalize for `planes` = B * C planes: allocate once, reuse"""
    return _plane_workspace("l1_workspace", L.load().swv2_l1_ws_bytes(planes, H, W), torch.float32, device)


def loss_workspace(planes: int, H: int, W: int, device) -> torch.Tensor:
    """the caller's workspace of swv2_loss_sums for `planes` = B * C planes: allocate once, reuse"""
    return _plane_workspace("loss_workspace", L.load().swv2_loss_ws_bytes(planes, H, W), torch.float32, device)


def l1_sums(prd, tar, w, ws):
    """S0 = sum w |prd - tar| and S1 = sum w |tar| of every (b, c) plane (prd / tar as score_sums takes them: [B, C, H, W] or a channel
    block of a wider contiguous tensor, read in place) as slice partials in ws (l1_workspace); w [H] row weights"""
    (pp, pbs), (tp, tbs) = _plane_blocks("l1_sums", prd, tar)
    B, Cc, H, W = prd.shape
    _row_weights("l1_sums", w, H); _chk(ws, torch.float32, "l1 workspace")
    L.check(L.load().swv2_l1_sums(pp, pbs, tp, tbs, _p(w), B, Cc, H, W, _p(ws), ws.numel() * 4, _stream()), "swv2_l1_sums")


def l1_finalize(ws, B: int, Cc: int, H: int, W: int, chw=None, absolute: bool = False):
    """slice partials -> sums [B, C, 2] = (S0, S1); with chw [C] also (loss [1], coef [B, C] = d loss / d S0), else (None, None).  One
    launch; the results are views of one fresh buffer"""
    _chk(ws, torch.float32, "l1 workspace")
    if chw is not None and _chk(chw, torch.float32, "channel weights").numel() != Cc:
        raise L.Swv2Error(f"l1_finalize: {chw.numel()} channel weights for {Cc} channels")
    n = B * Cc
    buf = torch.empty(3 * n + 2, dtype=torch.float32, device=ws.device)
    sums = buf[:2 * n].view(B, Cc, 2)
    coef, loss = (buf[2 * n:3 * n].view(B, Cc), buf[3 * n:3 * n + 1]) if chw is not None else (None, None)
    L.check(L.load().swv2_l1_finalize(_p(ws), ws.numel() * 4, B, Cc, H, W, _p(chw), int(absolute), _p(sums), _p(loss), _p(coef), _stream()),
            "swv2_l1_finalize")
    return sums, loss, coef


def l1_grad(prd, tar, qw, coef, dprd):
    """dprd = coef[b, c] * qw[h] * sign(prd - tar); prd, tar, dprd contiguous fp32 [B, C, H, W]"""
    for t, what in ((prd, "prediction"), (tar, "target"), (dprd, "gradient"), (qw, "row weights"), (coef, "coef")):
        _chk(t, torch.float32, what)
    B, Cc, H, W = prd.shape
    if tar.shape != prd.shape or dprd.shape != prd.shape or coef.numel() != B * Cc or qw.numel() != H:
        raise L.Swv2Error(f"l1_grad: shapes {tuple(prd.shape)} / {tuple(tar.shape)} / {tuple(dprd.shape)}, coef {coef.numel()}, weights {qw.numel()}")
    L.check(L.load().swv2_l1_grad(_p(prd), _p(tar), _p(qw), _p(coef), _p(dprd), B * Cc, H, W, _stream()), "swv2_l1_grad")


def regrid_planes_ok(t: torch.Tensor, source: bool) -> bool:
    """what swv2_regrid reads (source: 16-byte vectors along the rows) or writes (element by element: any address, any width) in place: a
    CUDA fp32 [B, C, H, W] tensor or channel block of one"""
    return _planes_in_place(t, vec=bool(source))


def regrid(x, y, lat_start, lat_count, lat_w, lon_start, lon_count, lon_w):
    """y [B, C, Hd, Wd] = the banded operators applied to x [B, C, H, W] (each a tensor or channel block read / written in place):
    swv2_regrid with the tables of utils/regrid.py::band_tables on the device (int32 start and count [n], fp32 weights [n, K]).  The
    kernel trusts the tables' indices (include/swv2.h): build them with band_tables, as Regridder does."""
    (xp, xbs), (yp, ybs) = _plane_block("regrid", x), _plane_block("regrid", y, vec=False)
    if x.shape[:2] != y.shape[:2] or x.device != y.device:
        raise L.Swv2Error(f"regrid: source {tuple(x.shape)} on {x.device} / destination {tuple(y.shape)} on {y.device}: expected one B, C and device")
    B, Cc, H, W = x.shape
    Hd, Wd = y.shape[2:]
    for t, dt, n, what in ((lat_start, torch.int32, Hd, "lat_start"), (lat_count, torch.int32, Hd, "lat_count"), (lat_w, torch.float32, Hd, "lat_w"),
                           (lon_start, torch.int32, Wd, "lon_start"), (lon_count, torch.int32, Wd, "lon_count"), (lon_w, torch.float32, Wd, "lon_w")):
        if _chk(t, dt, what).shape[0] != n or t.dim() != (2 if dt == torch.float32 else 1) or t.device != x.device:
            raise L.Swv2Error(f"regrid: table {what} {tuple(t.shape)}, expected {n} rows on {x.device}")
    L.check(L.load().swv2_regrid(xp, xbs, yp, ybs, B, Cc, H, W, Hd, Wd,
                                 _p(lat_start), _p(lat_count), _p(lat_w), lat_w.shape[1], _p(lon_start), _p(lon_count), _p(lon_w), lon_w.shape[1],
                                 _stream()), "swv2_regrid")


def sht_power(table, X, keep_coeffs: bool = False, zero_coeffs: bool = False):
    """degree power [planes, lmax] of the spectral operand X [mmax, 2 planes, nlat] under table [mmax, lmax, nlat] (swv2_sht_power);
    with keep_coeffs also the coefficients [mmax, 2 planes, lmax] (l >= m written; the rest zeros with zero_coeffs, else whatever the
    allocation held) for sht_adjoint and sht_synth, else None"""
    _chk(table, torch.float32, "sht table"); _chk(X, torch.float32, "sht operand")
    if table.dim() != 3 or X.dim() != 3 or X.shape[0] != table.shape[0] or X.shape[2] != table.shape[2] or X.shape[1] % 2:
        raise L.Swv2Error(f"sht_power: table {tuple(table.shape)} [mmax, lmax, nlat] against operand {tuple(X.shape)} [mmax, 2 planes, nlat]")
    mmax, lmax, nlat = table.shape
    planes = X.shape[1] // 2
    lib = L.load()
    nb = lib.swv2_sht_ws_bytes(planes, lmax, mmax)
    ws = _scratch(nb, X.device, "sht_power")
    power = torch.empty(planes, lmax, dtype=torch.float32, device=X.device)
    coef = (torch.zeros if zero_coeffs else torch.empty)(mmax, 2 * planes, lmax, dtype=torch.float32, device=X.device) if keep_coeffs else None
    L.check(_timed("sht_power", lib.swv2_sht_power, _p(table), _p(X), _p(power), _p(coef), planes, nlat, lmax, mmax, _p(ws), nb, _stream()),
            "swv2_sht_power")
    return power, coef


def sht_repack(src, planes: int, nlat: int, mmax: int, scale: float, backward: bool = False):
    """rfft's layout F [planes, nlat, mmax, 2] -> the operand X [mmax, 2 planes, nlat] times scale; backward: the same map from X to F"""
    _chk(src, torch.float32, "sht repack source")
    if src.numel() != planes * nlat * mmax * 2:
        raise L.Swv2Error(f"sht_repack: {src.numel()} elements for planes {planes}, nlat {nlat}, mmax {mmax}")
    dst = torch.empty((planes, nlat, mmax, 2) if backward else (mmax, 2 * planes, nlat), dtype=torch.float32, device=src.device)
    L.check(_timed("sht_repack", L.load().swv2_sht_repack, _p(src), _p(dst), planes, nlat, mmax, float(scale), int(backward), _stream()),
            "swv2_sht_repack")
    return dst


def sht_adjoint(table, coef, gpower):
    """dX [mmax, 2 planes, nlat]: the gradient of sht_power's operand from gpower [planes, lmax] and the kept coefficients"""
    for t, what in ((table, "sht table"), (coef, "sht coefficients"), (gpower, "power gradient")):
        _chk(t, torch.float32, what)
    mmax, lmax, nlat = table.shape
    planes = coef.shape[1] // 2
    if tuple(coef.shape) != (mmax, 2 * planes, lmax) or tuple(gpower.shape) != (planes, lmax):
        raise L.Swv2Error(f"sht_adjoint: table {tuple(table.shape)}, coefficients {tuple(coef.shape)}, gradient {tuple(gpower.shape)}")
    dX = torch.empty(mmax, 2 * planes, nlat, dtype=torch.float32, device=coef.device)
    L.check(_timed("sht_adjoint", L.load().swv2_sht_adjoint, _p(table), _p(coef), _p(gpower), _p(dX), planes, nlat, lmax, mmax, _stream()),
            "swv2_sht_adjoint")
    return dX


def sht_cross_power(table, X, keep_coeffs: bool = False):
    """spectra [3, pairs, lmax] = (P_aa, P_bb, C_ab) of the operand X [mmax, 4 pairs, nlat] whose planes are interleaved as pairs a_0, b_0,
    a_1, b_1, ... (swv2_sht_cross_power); with keep_coeffs also the coefficients [mmax, 4 pairs, lmax] for sht_cross_adjoint, else None"""
    _chk(table, torch.float32, "sht table"); _chk(X, torch.float32, "sht operand")
    if table.dim() != 3 or X.dim() != 3 or X.shape[0] != table.shape[0] or X.shape[2] != table.shape[2] or X.shape[1] % 4:
        raise L.Swv2Error(f"sht_cross_power: table {tuple(table.shape)} [mmax, lmax, nlat] against operand {tuple(X.shape)} [mmax, 4 pairs, nlat]")
    mmax, lmax, nlat = table.shape
    pairs = X.shape[1] // 4
    lib = L.load()
    nb = lib.swv2_sht_cross_ws_bytes(pairs, lmax, mmax)
    ws = _scratch(nb, X.device, "sht_cross_power")
    spectra = torch.empty(3, pairs, lmax, dtype=torch.float32, device=X.device)
    coef = torch.empty(mmax, 4 * pairs, lmax, dtype=torch.float32, device=X.device) if keep_coeffs else None
    L.check(_timed("sht_cross_power", lib.swv2_sht_cross_power, _p(table), _p(X), _p(spectra), _p(coef), pairs, nlat, lmax, mmax, _p(ws), nb,
                   _stream()), "swv2_sht_cross_power")
    return spectra, coef


def sht_cross_adjoint(table, coef, gspectra):
    """dX [mmax, 4 pairs, nlat]: the gradient of sht_cross_power's operand from gspectra [3, pairs, lmax] and the kept coefficients"""
    for t, what in ((table, "sht table"), (coef, "sht coefficients"), (gspectra, "spectra gradient")):
        _chk(t, torch.float32, what)
    mmax, lmax, nlat = table.shape
    pairs = coef.shape[1] // 4
    if tuple(coef.shape) != (mmax, 4 * pairs, lmax) or tuple(gspectra.shape) != (3, pairs, lmax):
        raise L.Swv2Error(f"sht_cross_adjoint: table {tuple(table.shape)}, coefficients {tuple(coef.shape)}, gradient {tuple(gspectra.shape)}")
    dX = torch.empty(mmax, 4 * pairs, nlat, dtype=torch.float32, device=coef.device)
    L.check(_timed("sht_cross_adjoint", L.load().swv2_sht_cross_adjoint, _p(table), _p(coef), _p(gspectra), _p(dX), pairs, nlat, lmax, mmax,
                   _stream()), "swv2_sht_cross_adjoint")
    return dX


def sht_synth(table, rweights, coef, response=None, scales=(1.0, 1.0), *, nlon: int):
    """S [mmax, 2 planes, nlat] = rweights[k] sum_{l >= m} table[m, l, k] f_m h[plane, l] coef[m, n, l] (swv2_sht_synth): the synthesis from
    coefficients [mmax, 2 planes, lmax] back to the longitude transform of a field of nlon points per row.  response: None, [lmax] or
    [planes, lmax]; scales = (f_0, f_m for m >= 1)"""
    for t, what in ((table, "sht table"), (rweights, "inverse row weights"), (coef, "sht coefficients")):
        _chk(t, torch.float32, what)
    mmax, lmax, nlat = table.shape
    planes = coef.shape[1] // 2
    if tuple(coef.shape) != (mmax, 2 * planes, lmax) or tuple(rweights.shape) != (nlat,):
        raise L.Swv2Error(f"sht_synth: table {tuple(table.shape)}, coefficients {tuple(coef.shape)}, inverse weights {tuple(rweights.shape)}")
    stride = 0
    if response is not None:
        _chk(response, torch.float32, "degree response")
        if tuple(response.shape) not in ((lmax,), (planes, lmax)):
            raise L.Swv2Error(f"sht_synth: response {tuple(response.shape)} for {planes} planes of {lmax} degrees")
        stride = lmax if response.dim() == 2 else 0
    S = torch.empty(mmax, 2 * planes, nlat, dtype=torch.float32, device=coef.device)
    L.check(_timed("sht_synth", L.load().swv2_sht_synth, _p(table), _p(rweights), _p(coef), _p(response), stride, float(scales[0]), float(scales[1]),
                   _p(S), planes, nlat, lmax, mmax, int(nlon), _stream()), "swv2_sht_synth")
    return S


def ens_workspace(planes: int, H: int, W: int, M: int, device) -> torch.Tensor:
    """the caller's workspace of swv2_ens_sums / swv2_ens_finalize for `planes` = B * C planes and M members: allocate once, reuse"""
    return _plane_workspace("ens_workspace", L.load().swv2_ens_ws_bytes(planes, H, W, M), torch.float32, device,
                            f"planes {planes}, H {H}, W {W} must be positive and M = {M} within 2 .. {ENS_MAX_MEMBERS}")


def ens_members_ok(t: torch.Tensor) -> bool:
    """what swv2_ens_sums reads in place as the members: a CUDA fp32 [M, B, C, H, W] view (contiguous planes, W % 4 == 0, 2 <= M <= 64,
    member and batch strides multiples of 4) -- a channel block of a member-major [M * B, channels, H, W] tensor viewed that way"""
    return _planes_in_place(t, lead=2)


def ens_sums(ens, tar, w, ws):
    """the partial sums and rank counts of every (b, c) plane of the members ens [M, B, C, H, W] against tar [B, C, H, W] (both may be
    channel blocks of wider tensors, read in place) into ws (ens_workspace); w [H] row weights"""
    (ep, ems, ebs), (tp, tbs) = _plane_blocks("ens_sums", ens, tar, lead=2)
    M, B, Cc, H, W = ens.shape
    _row_weights("ens_sums", w, H); _chk(ws, torch.float32, "ensemble workspace")
    L.check(L.load().swv2_ens_sums(ep, ems, ebs, tp, tbs, _p(w), M, B, Cc, H, W, _p(ws), ws.numel() * 4, _stream()), "swv2_ens_sums")


def ens_finalize(ws, M: int, B: int, Cc: int, H: int, W: int, scale=None):
    """slice partials -> (sums [B, C, 4] = (S_mse, S_var, S_1, S_2), hist [B, C, M + 1] int32, ens_rmse, spread, crps, fair_crps [B, C] each,
    means [4, C]: their batch means, the first three x scale [C] if given), one launch; the float results are views of one fresh buffer"""
    _chk(ws, torch.float32, "ensemble workspace")
    if scale is not None and _chk(scale, torch.float32, "scale").numel() != Cc:
        raise L.Swv2Error(f"ens_finalize: scale of {scale.numel()} values for {Cc} channels")
    n = B * Cc
    buf = torch.empty(8 * n + 4 * Cc, dtype=torch.float32, device=ws.device)
    hist = torch.empty(B, Cc, M + 1, dtype=torch.int32, device=ws.device)
    sums = buf[:4 * n].view(B, Cc, 4)
    er, sp, cr, fc = (buf[(4 + k) * n:(5 + k) * n].view(B, Cc) for k in range(4))
    means = buf[8 * n:].view(4, Cc)
    L.check(L.load().swv2_ens_finalize(_p(ws), ws.numel() * 4, M, B, Cc, H, W, _p(scale), _p(sums), _p(hist), _p(er), _p(sp), _p(cr), _p(fc),
                                       _p(means), _stream()), "swv2_ens_finalize")
    return sums, hist, er, sp, cr, fc, means


def event_workspace(planes: int, H: int, W: int, K: int, device) -> torch.Tensor:
    """the caller's workspace of swv2_event_sums / swv2_event_finalize for `planes` = B * C planes and K thresholds: allocate once, reuse"""
    return _plane_workspace("event_workspace", L.load().swv2_event_ws_bytes(planes, H, W, K), torch.float32, device,
                            f"planes {planes}, H {H}, W {W} must be positive and K = {K} within 1 .. {EVENT_MAX_K}")


def ens_event_workspace(planes: int, H: int, W: int, M: int, K: int, device) -> torch.Tensor:
    """the caller's workspace of swv2_event_ens_sums / swv2_event_ens_finalize: allocate once, reuse"""
    return _plane_workspace("ens_event_workspace", L.load().swv2_event_ens_ws_bytes(planes, H, W, M, K), torch.float32, device,
                            f"planes {planes}, H {H}, W {W} must be positive, M = {M} within 2 .. {ENS_MAX_MEMBERS} and K = {K} within 1 .. "
                            f"{EVENT_MAX_K}")


def _event_operands(who, x_shape, thr, w, base):
    """checks of the operands both event kernels share -> (K, thr batch stride)"""
    B, Cc, H, W = x_shape
    _row_weights(who, w, H); _chk(thr, torch.float32, "thresholds")
    if thr.dim() != 3 or thr.shape[1] != Cc or thr.shape[0] not in (1, B) or not 1 <= thr.shape[2] <= EVENT_MAX_K:
        raise L.Swv2Error(f"{who}: thresholds {tuple(thr.shape)}, expected [1 or {B}, {Cc}, K <= {EVENT_MAX_K}]")
    if base is not None and (_chk(base, torch.float32, "base field").shape != (Cc, H, W)):
        raise L.Swv2Error(f"{who}: base field {tuple(base.shape)}, expected {(Cc, H, W)}")
    K = thr.shape[2]
    return K, (Cc * K if thr.shape[0] == B and B > 1 else 0)


def event_sums(prd, tar, thr, w, ws, base=None, below=False):
    """the contingency-table partial sums of every (b, c) plane of prd / tar (each [B, C, H, W] or a channel block of a wider tensor, read
    in place) into ws (event_workspace); thr [1 or B, C, K] contiguous, w [H] row weights, base [C, H, W] or None"""
    (pp, pbs), (tp, tbs) = _plane_blocks("event_sums", prd, tar)
    B, Cc, H, W = prd.shape
    K, thr_bs = _event_operands("event_sums", prd.shape, thr, w, base)
    _chk(ws, torch.float32, "event workspace")
    L.check(L.load().swv2_event_sums(pp, pbs, tp, tbs, _p(base), _p(thr), thr_bs, _p(w), K, int(bool(below)), B, Cc, H, W, _p(ws), ws.numel() * 4,
                                     _stream()), "swv2_event_sums")


def event_finalize(ws, K: int, B: int, Cc: int, H: int, W: int):
    """slice partials -> (table [B, C, K, 4] fp32, n_invalid [B, C] int32), one launch"""
    _chk(ws, torch.float32, "event workspace")
    table = torch.empty(B, Cc, K, 4, dtype=torch.float32, device=ws.device)
    ninv = torch.empty(B, Cc, dtype=torch.int32, device=ws.device)
    L.check(L.load().swv2_event_finalize(_p(ws), ws.numel() * 4, K, B, Cc, H, W, _p(table), _p(ninv), _stream()), "swv2_event_finalize")
    return table, ninv


def ens_event_sums(ens, tar, thr, w, ws, base=None, below=False):
    """the Brier partial sums and reliability counts of every (b, c) plane of the members ens [M, B, C, H, W] against tar [B, C, H, W] (both may
    be channel blocks of wider tensors, read in place) into ws (ens_event_workspace)"""
    (ep, ems, ebs), (tp, tbs) = _plane_blocks("ens_event_sums", ens, tar, lead=2)
    M, B, Cc, H, W = ens.shape
    K, thr_bs = _event_operands("ens_event_sums", tar.shape, thr, w, base)
    _chk(ws, torch.float32, "ensemble event workspace")
    L.check(L.load().swv2_event_ens_sums(ep, ems, ebs, tp, tbs, _p(base), _p(thr), thr_bs, _p(w), M, K, int(bool(below)), B, Cc, H, W, _p(ws),
                                         ws.numel() * 4, _stream()), "swv2_event_ens_sums")


def ens_event_finalize(ws, M: int, K: int, B: int, Cc: int, H: int, W: int):
    """slice partials -> (sums [B, C, K, 3] = (S_e, S_f, S_o), wv [B, C], hist [B, C, K, 2, M + 1] int32, n_invalid [B, C] int32), one launch"""
    _chk(ws, torch.float32, "ensemble event workspace")
    sums = torch.empty(B, Cc, K, 3, dtype=torch.float32, device=ws.device)
    wv = torch.empty(B, Cc, dtype=torch.float32, device=ws.device)
    hist = torch.empty(B, Cc, K, 2, M + 1, dtype=torch.int32, device=ws.device)
    ninv = torch.empty(B, Cc, dtype=torch.int32, device=ws.device)
    L.check(L.load().swv2_event_ens_finalize(_p(ws), ws.numel() * 4, M, K, B, Cc, H, W, _p(sums), _p(wv), _p(hist), _p(ninv), _stream()),
            "swv2_event_ens_finalize")
    return sums, wv, hist, ninv


def fss_band_rows(planes: int, H: int, K: int, r_max: int) -> int:
    """rows per band of swv2_fss_rows' box launch (host-only): one workgroup per (plane, threshold, band)"""
    return int(L.load().swv2_fss_band_rows(planes, H, K, r_max))


def fss_workspace(planes: int, H: int, W: int, K: int, S: int, device) -> torch.Tensor:
    """the caller's workspace of swv2_fss_rows for `planes` = B * C planes, K thresholds and S scales: allocate once, reuse; never zeroed"""
    return _plane_workspace("fss_workspace", L.load().swv2_fss_ws_bytes(planes, H, W, K, S), torch.int32, device,
                            f"planes {planes}, H {H}, W {W} must be positive and K = {K}, S = {S} within 1 .. {FSS_MAX_S}")


def fss_rows(prd, tar, thr, scales, ws, base=None, below=False):
    """the neighbourhood sums of every (b, c) plane of prd / tar (each [B, C, H, W] or a channel block of a wider tensor, read in place)
    -> (rows [B, C, K, S, H, 3] int64 = (sum_w (n_f - n_o)^2, sum_w n_f^2, sum_w n_o^2), n_invalid [B, C] int32); thr [1 or B, C, K]
    contiguous, scales: S strictly ascending half-widths in 0 .. 32 (host integers), ws: fss_workspace, base [C, H, W] or None"""
    (pp, pbs), (tp, tbs) = _plane_blocks("fss_rows", prd, tar)
    B, Cc, H, W = prd.shape
    _chk(thr, torch.float32, "thresholds")
    if thr.dim() != 3 or thr.shape[1] != Cc or thr.shape[0] not in (1, B) or not 1 <= thr.shape[2] <= EVENT_MAX_K:
        raise L.Swv2Error(f"fss_rows: thresholds {tuple(thr.shape)}, expected [1 or {B}, {Cc}, K <= {EVENT_MAX_K}]")
    if base is not None and (_chk(base, torch.float32, "base field").shape != (Cc, H, W)):
        raise L.Swv2Error(f"fss_rows: base field {tuple(base.shape)}, expected {(Cc, H, W)}")
    K, S = thr.shape[2], len(scales)
    thr_bs = Cc * K if thr.shape[0] == B and B > 1 else 0
    _chk(ws, torch.int32, "fss workspace")
    rows = torch.empty(B, Cc, K, S, H, 3, dtype=torch.int64, device=prd.device)
    ninv = torch.empty(B, Cc, dtype=torch.int32, device=prd.device)
    sc = (C.c_int * max(S, 1))(*[int(r) for r in scales])
    L.check(L.load().swv2_fss_rows(pp, pbs, tp, tbs, _p(base), _p(thr), thr_bs, sc, K, S, int(bool(below)), B, Cc, H, W, _p(ws), ws.numel() * 4,
                                   _p(rows), _p(ninv), _stream()), "swv2_fss_rows")
    return rows, ninv


def fss_ens_band_rows(planes: int, H: int, M: int, K: int, r_max: int) -> int:
    """rows per band of swv2_fss_ens_rows' box launch (host-only): the plan of swv2_fss_band_rows under 80 KiB of LDS for M members"""
    return int(L.load().swv2_fss_ens_band_rows(planes, H, M, K, r_max))


def fss_ens_workspace(planes: int, H: int, W: int, M: int, K: int, S: int, device) -> torch.Tensor:
    """the caller's workspace of swv2_fss_ens_rows for `planes` = B * C planes, M members, K thresholds and S scales: allocate once, reuse;
    never zeroed"""
    return _plane_workspace("fss_ens_workspace", L.load().swv2_fss_ens_ws_bytes(planes, H, W, M, K, S), torch.int32, device,
                            f"planes {planes}, H {H}, W {W} must be positive, M = {M} within 2 .. {ENS_MAX_MEMBERS} and K = {K}, S = {S} within "
                            f"1 .. {FSS_MAX_S}")


def fss_ens_rows(ens, tar, thr, scales, ws, base=None, below=False):
    """the neighbourhood sums of the members ens [M, B, C, H, W] (as ens_sums takes them: channel blocks of wider tensors are read in place)
    against tar [B, C, H, W] -> (rows [B, C, K, S, H, 3] int64 = (sum_w (N_f - M n_o)^2, sum_w N_f^2, sum_w n_o^2), n_invalid [B, C] int32);
    thr, scales, base, below: as fss_rows takes them, ws: fss_ens_workspace"""
    (ep, ems, ebs), (tp, tbs) = _plane_blocks("fss_ens_rows", ens, tar, lead=2)
    M, B, Cc, H, W = ens.shape
    _chk(thr, torch.float32, "thresholds")
    if thr.dim() != 3 or thr.shape[1] != Cc or thr.shape[0] not in (1, B) or not 1 <= thr.shape[2] <= EVENT_MAX_K:
        raise L.Swv2Error(f"fss_ens_rows: thresholds {tuple(thr.shape)}, expected [1 or {B}, {Cc}, K <= {EVENT_MAX_K}]")
    if base is not None and (_chk(base, torch.float32, "base field").shape != (Cc, H, W)):
        raise L.Swv2Error(f"fss_ens_rows: base field {tuple(base.shape)}, expected {(Cc, H, W)}")
    K, S = thr.shape[2], len(scales)
    thr_bs = Cc * K if thr.shape[0] == B and B > 1 else 0
    _chk(ws, torch.int32, "ensemble fss workspace")
    rows = torch.empty(B, Cc, K, S, H, 3, dtype=torch.int64, device=tar.device)
    ninv = torch.empty(B, Cc, dtype=torch.int32, device=tar.device)
    sc = (C.c_int * max(S, 1))(*[int(r) for r in scales])
    L.check(L.load().swv2_fss_ens_rows(ep, ems, ebs, tp, tbs, _p(base), _p(thr), thr_bs, sc, M, K, S, int(bool(below)), B, Cc, H, W, _p(ws),
                                       ws.numel() * 4, _p(rows), _p(ninv), _stream()), "swv2_fss_ens_rows")
    return rows, ninv


def quantile_workspace(planes: int, H: int, W: int, K: int, device) -> torch.Tensor:
    """the caller's workspace of swv2_plane_order_stats for `planes` = B * C planes and K ranks: allocate once, reuse; never zeroed"""
    return _plane_workspace("quantile_workspace", L.load().swv2_quantile_ws_bytes(planes, H, W, K), torch.int32, device)


def quantile_planes_ok(t: torch.Tensor) -> bool:
    """what swv2_plane_order_stats reads in place: a CUDA fp32 [B, C, H, W] tensor or channel block of one (contiguous planes,
    H * W % 4 == 0)"""
    return _planes_in_place(t, vec="plane")


def plane_order_stats(x, ranks, ws=None):
    """-> (values [K, B, C]: the element of rank ranks[k] of every plane of x in ascending order, NaNs last; nan_count [B, C] int32).
    x: [B, C, H, W] or a channel block of a wider tensor, read in place; ranks: [K] int32 on x's device, distinct, ascending, in
    [0, H * W), K <= QUANTILE_MAX_RANKS (the caller's promise: utils/weighted_acc_rmse.quantile_ranks builds them); ws: a
    quantile_workspace to reuse (allocated here otherwise)."""
    xp, xbs = _plane_block("plane_order_stats", x, vec="plane")
    B, Cc, H, W = x.shape
    _chk(ranks, torch.int32, "ranks")
    K = ranks.numel()
    if ranks.dim() != 1 or ranks.device != x.device:
        raise L.Swv2Error(f"plane_order_stats: ranks {tuple(ranks.shape)} on {ranks.device}, expected [K] on {x.device}")
    if ws is None:
        ws = quantile_workspace(B * Cc, H, W, K, x.device)
    _chk(ws, torch.int32, "quantile workspace")
    out = torch.empty(K, B, Cc, dtype=torch.float32, device=x.device)
    nan_count = torch.empty(B, Cc, dtype=torch.int32, device=x.device)
    L.check(L.load().swv2_plane_order_stats(xp, xbs, B, Cc, H, W, _p(ranks), K, _p(out), _p(nan_count),
                                            _p(ws), ws.numel() * 4, _stream()), "swv2_plane_order_stats")
    return out, nan_count


def stats_slices(Cc: int, H: int, W: int) -> int:
    """slices per channel of swv2_stats_accumulate's plan (host-only)"""
    return int(L.load().swv2_stats_slices(Cc, H, W))


def stats_workspace(Cc: int, H: int, W: int, device) -> torch.Tensor:
    """part [C, slices, 6] fp64 of swv2_stats_accumulate / swv2_stats_finalize; not zeroed: the first accumulate (first=True) stores"""
    return torch.empty(int(L.load().swv2_stats_ws_bytes(Cc, H, W)) // 8, dtype=torch.float64, device=device).view(Cc, -1, 6)


def stats_accumulate(slab, prev, pivot, tsum, part, first: bool, stream=None):
    """one time slab [C, H, W] fp32 into the running fp64 sums: tsum [C, H, W] += slab - pivot[c], part [C, slices, 6] += the slice sums of
    (x', x'^2, d, d^2, non-finite count, 0), d = slab - prev (prev None: no difference terms).  first: store instead of add."""
    _chk(slab, torch.float32, "stats slab"); _chk(pivot, torch.float64, "stats pivot")
    _chk(tsum, torch.float64, "stats tsum"); _chk(part, torch.float64, "stats workspace")
    if slab.dim() != 3 or tsum.shape != slab.shape or pivot.numel() != slab.shape[0]:
        raise L.Swv2Error(f"stats_accumulate: slab {tuple(slab.shape)}, tsum {tuple(tsum.shape)}, pivot {tuple(pivot.shape)}: expected "
                          "[C, H, W], [C, H, W], [C]")
    if prev is not None and _chk(prev, torch.float32, "stats prev").shape != slab.shape:
        raise L.Swv2Error(f"stats_accumulate: prev {tuple(prev.shape)}, slab {tuple(slab.shape)}")
    Cc, H, W = slab.shape
    L.check(L.load().swv2_stats_accumulate(_p(slab), _p(prev), _p(pivot), _p(tsum), _p(part), part.numel() * 8, Cc, H, W, int(bool(first)),
                                           stream if stream is not None else _stream()), "swv2_stats_accumulate")


def stats_finalize(part, tsum, pivot, T: int, stream=None):
    """-> (folded [C, 6] fp64: the slices of every channel added in a fixed order, time_means [C, H, W] fp32 = pivot + tsum / T)"""
    _chk(part, torch.float64, "stats workspace"); _chk(tsum, torch.float64, "stats tsum"); _chk(pivot, torch.float64, "stats pivot")
    if tsum.dim() != 3 or pivot.numel() != tsum.shape[0]:
        raise L.Swv2Error(f"stats_finalize: tsum {tuple(tsum.shape)}, pivot {tuple(pivot.shape)}: expected [C, H, W], [C]")
    Cc, H, W = tsum.shape
    folded = torch.empty(Cc, 6, dtype=torch.float64, device=tsum.device)
    time_means = torch.empty(Cc, H, W, dtype=torch.float32, device=tsum.device)
    L.check(L.load().swv2_stats_finalize(_p(part), part.numel() * 8, _p(tsum), _p(pivot), Cc, H, W, int(T), _p(folded), _p(time_means),
                                         stream if stream is not None else _stream()), "swv2_stats_finalize")
    return folded, time_means


def era5_select_normalize(raw, out, chan, mean, std, coff=0, stream=None):
    """raw [B, S, Craw, Hraw, Wraw] fp32 -> out[:, coff : coff + S*len(chan)] = (raw[:, s, chan] - mean) / std, cropped to out's H, W"""
    B, S, Craw, Hraw, Wraw = raw.shape
    _, Ct, H, W = out.shape
    _chk(raw, torch.float32, "era5 raw"); _chk(out, torch.float32, "era5 out")
    L.check(L.load().swv2_era5_select_normalize(_p(raw), _p(out), _p(chan), _p(mean), _p(std), B, S, chan.numel(), Craw, Hraw, Wraw,
                                                H, W, Ct, coff, stream if stream is not None else _stream()), "swv2_era5_select_normalize")


def era5_select_normalize_i16(raw, out, chan, mean, std, offset, scale, slab_row, coff=0, stream=None):
    """era5_select_normalize over int16-packed slabs (utils/packed.py): raw [B, S, Craw, Hraw, Wraw] int16, offset / scale [rows, Craw] fp32
    (every year file's parameters), slab_row [B, S] int32 (the row of each slab).  Bit for bit what era5_select_normalize gives on the
    unpacked slabs."""
    B, S, Craw, Hraw, Wraw = raw.shape
    _, Ct, H, W = out.shape
    _chk(raw, torch.int16, "era5 packed raw"); _chk(out, torch.float32, "era5 out")
    _chk(offset, torch.float32, "era5 pack offset"); _chk(scale, torch.float32, "era5 pack scale"); _chk(slab_row, torch.int32, "era5 slab_row")
    if offset.dim() != 2 or offset.shape[1] != Craw or scale.shape != offset.shape or slab_row.numel() != B * S:
        raise L.Swv2Error(f"era5_select_normalize_i16: offset {tuple(offset.shape)}, scale {tuple(scale.shape)}, slab_row {tuple(slab_row.shape)}: "
                          f"expected [rows, {Craw}] twice and [{B}, {S}]")
    L.check(L.load().swv2_era5_select_normalize_i16(_p(raw), _p(out), _p(chan), _p(mean), _p(std), _p(offset), _p(scale), _p(slab_row), B, S,
                                                    chan.numel(), Craw, Hraw, Wraw, H, W, Ct, coff,
                                                    stream if stream is not None else _stream()), "swv2_era5_select_normalize_i16")


def _pack_slab_args(who, i16, f32, offset, scale):
    _chk(i16, torch.int16, who + " int16 slab"); _chk(f32, torch.float32, who + " fp32 slab")
    _chk(offset, torch.float32, who + " offset"); _chk(scale, torch.float32, who + " scale")
    if f32.dim() != 3 or i16.shape != f32.shape or offset.numel() != f32.shape[0] or scale.numel() != f32.shape[0]:
        raise L.Swv2Error(f"{who}: int16 {tuple(i16.shape)}, fp32 {tuple(f32.shape)}, offset {tuple(offset.shape)}, scale {tuple(scale.shape)}: "
                          "expected [C, H, W] twice and [C] twice")
    return f32.shape


def era5_unpack_i16(raw, out, offset, scale, stream=None):
    """raw [C, H, W] int16 -> out [C, H, W] fp32 = raw * scale[c] + offset[c] (NaN for the code -32768), utils/packed.py::unpack_array"""
    Cc, H, W = _pack_slab_args("era5_unpack_i16", raw, out, offset, scale)
    L.check(L.load().swv2_era5_unpack_i16(_p(raw), _p(out), _p(offset), _p(scale), Cc, H, W,
                                          stream if stream is not None else _stream()), "swv2_era5_unpack_i16")


def era5_pack_i16(slab, out, offset, scale, stream=None):
    """slab [C, H, W] fp32 -> out [C, H, W] int16, utils/packed.py::pack_array"""
    Cc, H, W = _pack_slab_args("era5_pack_i16", out, slab, offset, scale)
    L.check(L.load().swv2_era5_pack_i16(_p(slab), _p(out), _p(offset), _p(scale), Cc, H, W,
                                        stream if stream is not None else _stream()), "swv2_era5_pack_i16")


def pack_range_workspace(Cc: int, H: int, W: int, device) -> torch.Tensor:
    """the slice partials of swv2_pack_range (bytes; not zeroed: every launch stores all of them)"""
    return _plane_workspace("pack_range_workspace", L.load().swv2_pack_range_ws_bytes(Cc, H, W), torch.uint8, device)


def pack_range(slab, rng, missing, ws, first: bool, stream=None):
    """slab [C, H, W] fp32 into the running rng [C, 2] fp32 (min, max of the finite values) and missing [C] int64 (the others);
    first: overwrite them"""
    _chk(slab, torch.float32, "pack_range slab"); _chk(rng, torch.float32, "pack_range range"); _chk(missing, torch.int64, "pack_range missing")
    _chk(ws, torch.uint8, "pack_range workspace")
    if slab.dim() != 3 or tuple(rng.shape) != (slab.shape[0], 2) or missing.numel() != slab.shape[0]:
        raise L.Swv2Error(f"pack_range: slab {tuple(slab.shape)}, range {tuple(rng.shape)}, missing {tuple(missing.shape)}: expected [C, H, W], "
                          "[C, 2], [C]")
    Cc, H, W = slab.shape
    L.check(L.load().swv2_pack_range(_p(slab), Cc, H, W, int(bool(first)), _p(rng), _p(missing), _p(ws), ws.numel(),
                                     stream if stream is not None else _stream()), "swv2_pack_range")


def era5_zenith(out, sun, coff, stream=None):
    """sun [B, nz, 3] fp32 = (sin dec, cos dec, hour angle at longitude 0) per time point (utils/data_loader_era5.sun_position)
    -> out[:, coff : coff + nz] = cos of the solar zenith angle"""
    B, Ct, H, W = out.shape
    _chk(sun, torch.float32, "era5_zenith sun")
    if sun.dim() != 3 or sun.shape[0] != B or sun.shape[2] != 3:
        raise L.Swv2Error(f"era5_zenith: sun must be [B, nz, 3], got {tuple(sun.shape)}")
    L.check(L.load().swv2_era5_zenith(_p(out), _p(sun), B, sun.shape[1], H, W, Ct, coff,
                                      stream if stream is not None else _stream()), "swv2_era5_zenith")


def era5_static(stat, out, coff, stream=None):
    """stat [Cs, H, W] fp32 -> out[:, coff : coff + Cs] (broadcast over the batch)"""
    B, Ct, H, W = out.shape
    L.check(L.load().swv2_era5_static(_p(stat), _p(out), B, stat.shape[0], H, W, Ct, coff,
                                      stream if stream is not None else _stream()), "swv2_era5_static")


def adam_step(p, g, m, v, lr, beta1, beta2, eps, step, grad_inv_scale=1.0):
    L.check(L.load().swv2_adam_step(_p(p), _p(g), _p(m), _p(v), p.numel(), lr, beta1, beta2, eps, step, grad_inv_scale,
                                    _stream()), "swv2_adam_step")


def mlp_fwd(x, w1, b1, w2, b2, gamma, beta, scale, rows_per_sample, eps=1e-5, keep_hpre=True, out=None):
    """Fused fc1 -> GELU -> fc2 -> LayerNorm -> drop-path -> +x.  Returns (y, hpre, a2, mean, rstd); keep_hpre=False: the
    pre-activation is not written (hpre = None; the backward's recompute mode rebuilds it from x).  out = (y, hpre, a2, mean, rstd)
    hands in the caller's own tensors (hpre = None there selects the mode that keeps none, whatever keep_hpre says)."""
    M, Cc = x.shape
    hid = w1.shape[0]
    _chk(x, torch.float32, "mlp x"); _chk(w1, BF16, "mlp w1"); _chk(w2, BF16, "mlp w2")
    dev = x.device
    if out is None:
        out = (torch.empty(M, Cc, dtype=torch.float32, device=dev), torch.empty(M, hid, dtype=BF16, device=dev) if keep_hpre else None,
               torch.empty(M, Cc, dtype=BF16, device=dev), torch.empty(M, device=dev), torch.empty(M, device=dev))
    y, hpre, a2, mean, rstd = out
    a = L.MlpArgs()
    a.x, a.w1, a.b1, a.w2, a.b2, a.gamma, a.beta, a.scale = (_p(t) for t in (x, w1, b1, w2, b2, gamma, beta, scale))
    a.hpre, a.a2, a.mean, a.rstd, a.y = (_p(t) for t in (hpre, a2, mean, rstd, y))
    a.M, a.C, a.hidden, a.rows_per_sample, a.eps = M, Cc, hid, rows_per_sample, eps
    L.check(_timed("mlp_fwd", L.load().swv2_mlp_fwd, C.byref(a), _stream()), "swv2_mlp_fwd")
    return y, hpre, a2, mean, rstd


def mlp_bwd(dy, a2, mean, rstd, gamma, scale, hpre, w2t, w1t, dgamma, dbeta, rows_per_sample, x=None, w1=None, b1=None, out=None, ws=None):
    """Fused LN backward -> dh = (da2 W2) * GELU'(hpre) -> dx = dy + dh W1.  Returns (dx, da2, dh); dgamma/dbeta accumulated.
    hpre=None: recompute mode -- the pre-activation is rebuilt from the forward's input x, fc1.weight w1 (bf16 [hid, C]), b1.
    out = (dx, da2, dh) and ws (fp32, swv2_mlp_bwd_ws_floats(M, C) floats) hand in the caller's own tensors."""
    M, Cc = dy.shape
    hid = w2t.shape[0]
    dev = dy.device
    if out is None:
        out = (torch.empty(M, Cc, dtype=torch.float32, device=dev), torch.empty(M, Cc, dtype=BF16, device=dev),
               torch.empty(M, hid, dtype=BF16, device=dev))
    if ws is None:
        ws = torch.empty(L.load().swv2_mlp_bwd_ws_floats(M, Cc), dtype=torch.float32, device=dev)
    dx, da2, dh = out
    a = L.MlpBwdArgs()
    a.dy, a.a2, a.mean, a.rstd, a.gamma, a.scale, a.hpre, a.w2t, a.w1t = (_p(t) for t in (dy, a2, mean, rstd, gamma, scale, hpre, w2t, w1t))
    a.da2, a.dh, a.dx, a.dgamma, a.dbeta, a.ws = (_p(t) for t in (da2, dh, dx, dgamma, dbeta, ws))
    a.M, a.C, a.hidden, a.rows_per_sample = M, Cc, hid, rows_per_sample
    a.x, a.w1, a.b1 = _p(x), _p(w1), _p(b1)
    L.check(_timed("mlp_bwd", L.load().swv2_mlp_bwd, C.byref(a), _stream()), "swv2_mlp_bwd")
    return dx, da2, dh


def proj_ln_fwd(oh, wp, bp, gamma, beta, scale, rowidx, x, Bw, Lp, heads, rows_per_sample, eps=1e-5, out=None):
    """Fused merge heads -> proj -> LayerNorm -> drop-path -> +x, scattered through the row table.  oh bf16 [Bw][heads][Lp][slot],
    wp bf16 [C][heads * slot] (prep_weight with the head-padding column map), x fp32 [rows][C] in destination order; scale / rowidx
    may be None.  Returns (y, a1, mean, rstd); out = (y, a1, mean, rstd) hands in the caller's own tensors (y rows that no table
    entry names are left as they were: a fresh y is uninitialised there)."""
    Cc, Mw = wp.shape[0], Bw * Lp
    _chk(oh, BF16, "proj_ln oh"); _chk(wp, BF16, "proj_ln wp"); _chk(x, torch.float32, "proj_ln x")
    dev = x.device
    if out is None:
        out = (torch.empty_like(x), torch.empty(Mw, Cc, dtype=BF16, device=dev), torch.empty(Mw, device=dev), torch.empty(Mw, device=dev))
    y, a1, mean, rstd = out
    a = L.ProjLnArgs()
    a.oh, a.wp, a.bp, a.gamma, a.beta, a.scale, a.rowidx, a.x = (_p(t) for t in (oh, wp, bp, gamma, beta, scale, rowidx, x))
    a.a1, a.mean, a.rstd, a.y = (_p(t) for t in (a1, mean, rstd, y))
    a.Bw, a.Lp, a.heads, a.C, a.rows_per_sample, a.eps = Bw, Lp, heads, Cc, rows_per_sample, eps
    L.check(_timed("proj_ln_fwd", L.load().swv2_proj_ln_fwd, C.byref(a), _stream()), "swv2_proj_ln_fwd")
    return y, a1, mean, rstd


def proj_ln_bwd(dy, a1, mean, rstd, gamma, scale, rowidx, wpt, dgamma, dbeta, Bw, Lp, heads, rows_per_sample, out=None, ws=None):
    """Fused LN backward (dy rows gathered through the row table) -> d(oh) = split_heads(da1 Wp).  wpt bf16 [heads * slot][C]
    (prep_weight, transpose, head-padding row map).  Returns (da1, doh); dgamma / dbeta accumulated.  out = (da1, doh) and ws
    (fp32, swv2_proj_ln_bwd_ws_floats(Bw * Lp, C) floats) hand in the caller's own tensors."""
    Cc, Mw = wpt.shape[1], Bw * Lp
    _chk(dy, torch.float32, "proj_ln dy"); _chk(a1, BF16, "proj_ln a1"); _chk(wpt, BF16, "proj_ln wpt")
    dev = dy.device
    if out is None:
        out = (torch.empty(Mw, Cc, dtype=BF16, device=dev), torch.empty(Bw, heads, Lp, wpt.shape[0] // max(heads, 1), dtype=BF16, device=dev))
    if ws is None:
        ws = torch.empty(L.load().swv2_proj_ln_bwd_ws_floats(Mw, Cc), dtype=torch.float32, device=dev)
    da1, doh = out
    a = L.ProjLnBwdArgs()
    a.dy, a.a1, a.mean, a.rstd, a.gamma, a.scale, a.rowidx, a.wpt = (_p(t) for t in (dy, a1, mean, rstd, gamma, scale, rowidx, wpt))
    a.da1, a.doh, a.dgamma, a.dbeta, a.ws = (_p(t) for t in (da1, doh, dgamma, dbeta, ws))
    a.Bw, a.Lp, a.heads, a.C, a.rows_per_sample = Bw, Lp, heads, Cc, rows_per_sample
    L.check(_timed("proj_ln_bwd", L.load().swv2_proj_ln_bwd, C.byref(a), _stream()), "swv2_proj_ln_bwd")
    return da1, doh


def cpb_fwd(w1, b1, w2, b2, keep, bias, wh, ww, heads, hidden, drop_p):
    L.check(L.load().swv2_cpb_fwd(_p(w1), _p(b1), _p(w2), _p(b2), _p(keep), _p(bias), wh, ww, heads, hidden, drop_p, _stream()),
            "swv2_cpb_fwd")


_SCRATCH = {}


def _scratch(nbytes: int, device, tag: str) -> torch.Tensor:
    """a cached uint8 workspace per (device, tag), grown on demand: kernels that only need scratch for the duration of their own
    launches on the current stream share it instead of a torch.empty per call in the training step"""
    key = (device.index if device.index is not None else torch.cuda.current_device(), tag, _stream())
    t = _SCRATCH.get(key)
    if t is None or t.numel() < nbytes:
        t = _SCRATCH[key] = torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=device)
    return t


def cpb_bwd(dbias, w1, b1, w2, keep, dw1, db1, dw2, db2, wh, ww, heads, hidden, drop_p, atomics=False):
    """d(meta MLP) accumulated into dw1 / db1 / dw2 / db2: partial rows in a scratch buffer + a fixed-order fold (default), or the float
    atomics of swv2_cpb_bwd (`atomics=True`)"""
    lib = L.load()
    if atomics:
        L.check(lib.swv2_cpb_bwd(_p(dbias), _p(w1), _p(b1), _p(w2), _p(keep), _p(dw1), _p(db1), _p(dw2), _p(db2), wh, ww,
                                 heads, hidden, drop_p, _stream()), "swv2_cpb_bwd")
        return
    nb = lib.swv2_cpb_bwd_ws_bytes(wh, ww, heads, hidden)
    ws = _scratch(nb, dbias.device, "cpb_bwd")
    L.check(lib.swv2_cpb_bwd_ws(_p(dbias), _p(w1), _p(b1), _p(w2), _p(keep), _p(dw1), _p(db1), _p(dw2), _p(db2), wh, ww,
                                heads, hidden, drop_p, _p(ws), nb, _stream()), "swv2_cpb_bwd_ws")


def cpb_multi_supported(heads: int, hidden: int, drop_p: float) -> bool:
    """shapes the one-launch-per-stage CPB kernels cover (swv2_cpb_fwd_multi / _bwd_multi: MFMA tiles of 16 heads x 64-unit waves; the
    keep words express Dropout(0.125))"""
    return 0 < heads <= 16 and hidden in (64, 128, 256, 384, 512) and abs(drop_p - 0.125) < 1e-6


def cpb_fwd_multi(ptab, nblk, keep_bits, bias_all, wh, ww, heads, hidden, drop_p):
    """bias_all [nblk][heads][L][L] from the blocks' meta MLPs (device pointer table ptab [nblk][4]); keep_bits int32 [nblk][L^2][hidden / 8]
    of random bits or None (eval)"""
    _chk(bias_all, torch.float32, "cpb_fwd_multi bias")
    if keep_bits is not None:
        _chk(keep_bits, torch.int32, "cpb_fwd_multi keep_bits")
    L.check(L.load().swv2_cpb_fwd_multi(_p(ptab), nblk, _p(keep_bits), _p(bias_all), wh, ww, heads, hidden, drop_p, _stream()),
            "swv2_cpb_fwd_multi")


def cpb_bwd_multi(dtables, nchunk, ptab, nblk, keep_bits, grads, wh, ww, heads, hidden, drop_p):
    """grads [nblk][3 hidden + heads hidden + heads] += d(meta MLP) of every block from dtables [nblk][nchunk][heads][L][L] (summed over nchunk)"""
    lib = L.load()
    _chk(dtables, torch.float32, "cpb_bwd_multi tables"); _chk(grads, torch.float32, "cpb_bwd_multi grads")
    nb = lib.swv2_cpb_bwd_multi_ws_bytes(nblk, wh, ww, heads, hidden)
    ws = _scratch(nb, grads.device, "cpb_bwd_multi")
    L.check(lib.swv2_cpb_bwd_multi(_p(dtables), nchunk, _p(ptab), nblk, _p(keep_bits), _p(grads), wh, ww, heads, hidden, drop_p,
                                   _p(ws), nb, _stream()), "swv2_cpb_bwd_multi")


def attn_pack_bias_multi(bias_all: torch.Tensor) -> torch.Tensor:
    """[ntab][heads][L][L] fp32 CPB tables -> [ntab][swv2_attn_pack_bias_bytes] uint8, one launch"""
    _chk(bias_all, torch.float32, "attn_pack_bias_multi")
    ntab, heads, Lw = bias_all.shape[0], bias_all.shape[1], bias_all.shape[2]
    nb = L.load().swv2_attn_pack_bias_bytes(heads, Lw)
    out = torch.empty(ntab, nb, dtype=torch.uint8, device=bias_all.device)
    L.check(L.load().swv2_attn_pack_bias_multi(_p(bias_all), ntab, heads, Lw, _p(out), _stream()), "swv2_attn_pack_bias_multi")
    return out


# ---- per-geometry index tables ------------------------------------------------------------------------------
class WindowPlan:
    """Index tables for one (batch, grid, window, shift, heads) geometry: the cyclic roll, the window partition, its
    inverse and the attention mask are all reduced to one int32 row table + one threshold."""

    def __init__(self, B, gh, gw, wh, ww, sh, sw, heads, head_dim, device):
        self.B, self.gh, self.gw, self.wh, self.ww, self.sh, self.sw = B, gh, gw, wh, ww, sh, sw
        self.heads, self.d = heads, head_dim
        self.L = wh * ww
        self.Lp, self.DP = attn_geometry(self.L, head_dim)
        self.nwh, self.nww = gh // wh, gw // ww
        self.nW = self.nwh * self.nww
        self.Bw = B * self.nW
        self.T = gh * gw
        if gh % wh or gw % ww:
            raise L.Swv2Error(f"window {wh}x{ww} does not divide the patch grid {gh}x{gw}")
        # swinv2_global.py:403-424 closed form: only a row shift produces a (non-zero) mask
        self.mask_thr = (wh - sh) * ww if sh > 0 else 0
        wi = torch.arange(self.nwh).view(-1, 1, 1, 1)
        wj = torch.arange(self.nww).view(1, -1, 1, 1)
        r = torch.arange(wh).view(1, 1, -1, 1)
        c = torch.arange(ww).view(1, 1, 1, -1)
        src = (((wi * wh + r + sh) % gh) * gw + (wj * ww + c + sw) % gw).reshape(self.nW, self.L)
        tab = torch.full((B, self.nW, self.Lp), -1, dtype=torch.int64)
        tab[:, :, :self.L] = src.unsqueeze(0) + (torch.arange(B) * self.T).view(B, 1, 1)
        self.rowidx = tab.reshape(-1).to(torch.int32).to(device)
        # head padding maps: padded feature (part*h + head)*DP + j -> part*C + head*d + j (or -1)
        Cc = heads * head_dim
        j = torch.arange(self.DP)
        hd = torch.arange(heads).view(-1, 1)
        one = torch.where(j.view(1, -1) < head_dim, hd * head_dim + j.view(1, -1), torch.full((1, 1), -1)).reshape(-1)
        self.proj_map = one.to(torch.int32).to(device)                          # [h*DP]
        three = torch.cat([torch.where(one >= 0, one + part * Cc, one) for part in range(3)])
        self.qkv_map = three.to(torch.int32).to(device)                         # [3*h*DP]


@functools.lru_cache(maxsize=64)
def window_plan(B, gh, gw, wh, ww, sh, sw, heads, head_dim, device_index) -> WindowPlan:
    return WindowPlan(B, gh, gw, wh, ww, sh, sw, heads, head_dim, torch.device("cuda", device_index))
