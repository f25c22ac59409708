"""Adam and LAMB on the HIP multi-tensor kernels.

Adam (reference train.py:176: `optim.Adam(model.parameters(), lr, betas=(0.9, 0.95))`,
stepped at train.py:330).

`HipAdam` is a drop-in `torch.optim.Adam`: same constructor, same `state_dict()` layout (`step`, `exp_avg`, `exp_avg_sq`
per parameter, so the reference's checkpoints restore into it and its checkpoints restore into torch's Adam).  `step()`
updates every fp32 CUDA parameter of a group with ONE `swv2_adam_multi` launch (torch's fused path: 5 launches of ~45 us
for the depth-12 model); options the kernel does not implement (amsgrad, weight decay, maximize, non-fp32 or CPU
parameters) take torch's own path for that group, so nothing is silently dropped.

`HipLamb` is apex's `FusedLAMB` (reference train.py:177-178: `optimizers.FusedLAMB(model.parameters(), lr, max_grad_norm=5.)`) on
`swv2_lamb_grad_norm` / `swv2_lamb_multi`: see the class.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from .. import _lib as L

_Item, _LambItem = L.AdamItem, L.LambItem      # the names these mirrors had while they were defined here (still imported by older callers)


def _dense(t: torch.Tensor) -> bool:
    """memory is one gap-free block (the kernel walks it linearly; p, grad, m, v must then only share the strides)"""
    return t.is_contiguous() or (t.dim() == 4 and t.is_contiguous(memory_format=torch.channels_last)) or \
        (t.dim() == 5 and t.is_contiguous(memory_format=torch.channels_last_3d))


def _kernel_ok(p, s, dev) -> bool:
    """the kernels walk raw memory: (p, grad, exp_avg, exp_avg_sq) must all be fp32 on `dev`, dense and laid out alike"""
    g = p.grad
    return (p.is_cuda and p.device == dev and p.dtype == torch.float32 and not g.is_sparse and g.dtype == torch.float32 and
            g.device == dev and _dense(p) and g.stride() == p.stride() and
            all(s[k].dtype == torch.float32 and s[k].device == dev and s[k].stride() == p.stride() for k in ("exp_avg", "exp_avg_sq")))


def chunk_pairs(numels, chunk):
    """(pairs, chunk0) of a multi-tensor launch: pairs = (item, chunk) for every chunk of `chunk` elements of every item, in order (one
    workgroup each); chunk0[i] = the index of item i's first pair"""
    pairs, chunk0 = [], []
    for i, n in enumerate(numels):
        chunk0.append(len(pairs))
        pairs += [(i, c) for c in range((n + chunk - 1) // chunk)]
    return pairs, chunk0


class _LaunchTable:
    """The device tables of a multi-tensor launch: the chunk pairs (static per parameter set) and the item rows of pointers, refreshed by
    `upload` whenever a pointer moved (gradient buffers may move between steps).  The optimizers hang their own bookkeeping on it."""

    def __init__(self, numels, chunk, item, dev):
        pairs, self.chunk0 = chunk_pairs(numels, chunk)
        self.n_items, self.n_chunks, self.words = len(numels), len(pairs), C.sizeof(item) // 8
        nbytes = C.sizeof(item) * self.n_items
        self.host = [torch.empty(nbytes, dtype=torch.uint8).pin_memory() for _ in range(2)]
        self.events, self.flip, self.rows = [None, None], 0, None
        self.dev = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        self.chunks = torch.tensor(pairs, dtype=torch.int32).to(dev)

    def upload(self, rows):
        """Two pinned staging buffers are used alternately, each guarded by an event recorded behind its H2D copy: the host may run
        several steps ahead of the GPU (no per-step sync in bench.py / train.py), so a staging buffer is rewritten only after the copy
        that last read it has executed (without the wait, step N's table could be overwritten with step N + 2's pointers
        before step N's copy ran)."""
        self.flip = 1 - self.flip
        host, ev = self.host[self.flip], self.events
        if ev[self.flip] is not None:
            ev[self.flip].synchronize()
        np.frombuffer(host.numpy(), dtype=np.int64).reshape(self.n_items, self.words)[:] = np.asarray(rows, dtype=np.int64)
        self.dev.copy_(host, non_blocking=True)
        e = torch.cuda.Event()
        e.record(torch.cuda.current_stream(self.dev.device))
        ev[self.flip] = e
        self.rows = rows


class HipAdam(torch.optim.Adam):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, **kw):
        kw.pop("fused", None)
        kw.pop("foreach", None)
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, **kw)
        self._tables = {}       # group index -> cached launch tables

    def _table(self, gi, plist):
        """the group's launch table; sizes are static per group, pointers are refreshed by `upload`"""
        key = tuple((p.data_ptr(), p.numel()) for p in plist)
        t = self._tables.get(gi)
        if t is None or t.key != key:
            t = self._tables[gi] = _LaunchTable([p.numel() for p in plist], L.load().swv2_adam_chunk(), L.AdamItem, plist[0].device)
            t.key, t.step = key, None
        return t

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._tables = {}

    # ---- step ----------------------------------------------------------------------------------------------
    @torch.no_grad()
    def step(self, closure=None, grad_inv_scale: float = 1.0):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        slow = []
        for gi, group in enumerate(self.param_groups):
            plist = [p for p in group["params"] if p.grad is not None]
            if (group["amsgrad"] or group["weight_decay"] != 0 or group["maximize"] or isinstance(group["lr"], torch.Tensor) or
                    not plist):
                slow.append(gi)
                continue
            states = []
            for p in plist:
                s = self.state[p]
                if len(s) == 0:
                    s["step"] = torch.tensor(0.0, dtype=torch.float32)
                    s["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    s["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                states.append(s)
            t = self._table(gi, plist)
            ptrs = tuple((p.data_ptr(), p.grad.data_ptr(), s["exp_avg"].data_ptr(), s["exp_avg_sq"].data_ptr(), p.numel())
                         for p, s in zip(plist, states))
            if ptrs != t.rows:
                # new tensors: anything the kernel cannot walk, or per-parameter step counters that disagree, keeps torch's exact path
                ok = all(_kernel_ok(p, s, plist[0].device) for p, s in zip(plist, states))
                if ok and t.step is None:           # new table (first step, new parameters, restored state)
                    steps = {int(s["step"]) for s in states}
                    ok = len(steps) == 1
                    if ok:
                        t.step, t.step_tensors = steps.pop(), [s["step"] for s in states]
                if not ok:
                    self._tables.pop(gi, None)
                    slow.append(gi)
                    continue
                t.upload(ptrs)
            t.step += 1
            step = t.step
            stream = torch.cuda.current_stream(plist[0].device).cuda_stream
            b1, b2 = group["betas"]
            L.check(L.load().swv2_adam_multi(t.dev.data_ptr(), t.chunks.data_ptr(), t.n_chunks, float(group["lr"]),
                                             float(b1), float(b2), float(group["eps"]), step, float(grad_inv_scale), stream),
                    "swv2_adam_multi")
            torch._foreach_add_(t.step_tensors, 1.0)      # state_dict() keeps torch's per-parameter `step` entries
            # the kernel wrote the parameters behind autograd's back: bump their version counters like an in-place torch op
            # would (anything keyed on `Tensor._version` -- e.g. cached casts of the weights -- must see the change)
            torch.autograd.graph.increment_version(plist)
        if slow:
            keep = self.param_groups
            try:
                self.param_groups = [keep[i] for i in slow]
                if grad_inv_scale != 1.0:           # torch's path knows no gradient scale: unscale these groups' gradients first
                    gs = [p.grad for g_ in self.param_groups for p in g_["params"] if p.grad is not None]
                    if gs:
                        torch._foreach_mul_(gs, float(grad_inv_scale))
                super().step()
            finally:
                self.param_groups = keep
        return loss


# ---------------------------------------------------------------------------------------------------------------
# LAMB
# ---------------------------------------------------------------------------------------------------------------
def _f32(x) -> float:
    """the fp32 value of a scalar, as a Python float: what the kernel receives (1 - beta2 formed from the DOUBLE 0.999 is off by 3e-5)"""
    return float(np.float32(x))


class HipLamb(torch.optim.Optimizer):
    """apex `FusedLAMB`: the same constructor, defaults and state layout (`state[p] = {exp_avg, exp_avg_sq}`, one step counter per group
    in `group['step']`, 1 on the first step), so its checkpoints restore here.  `amsgrad=True` raises, as in apex.

    One `step()`:
      1. G = sqrt(sum over the gradients of ALL groups of (g * grad_inv_scale)^2); c = G / max_grad_norm if G > max_grad_norm else 1
         (max_grad_norm is the constructor's value, not a group's); g^ = g * grad_inv_scale / c.
      2. per element, b3 = 1 - beta1 if grad_averaging else 1, bc_i = 1 - beta_i^step if bias_correction else 1:
         adam_w_mode:  m <- beta1 m + b3 g^, v <- beta2 v + (1 - beta2) g^^2, a = (m / bc1) / (sqrt(v / bc2) + eps), u = a + weight_decay p
         otherwise  :  g^ <- g^ + weight_decay p first, then m, v, a as above and u = a.
      3. per tensor, r = |p| / |u| if (use_nvlamb or weight_decay != 0) and |p| != 0 and |u| != 0 else 1, |p| before the update.
      4. p <- p - lr r u.
    Non-finite gradients are NOT skipped: they propagate into m, v, the norms and p as the arithmetic dictates (an inf in one gradient
    makes G inf and every g^ zero or NaN); guard the step from outside if the loss can overflow.

    fp32, dense parameters on one GPU take the HIP kernels: one gradient-norm launch per step over all groups and four launches per group,
    44 bytes moved per parameter, gradients only read (apex overwrites them with u; here u is recomputed from m, v and the old p), no
    read-back and no synchronisation (pointer tables are uploaded from two pinned buffers, as in `HipAdam`).  A group the kernels cannot take
    (CPU tensors, another dtype, non-dense layouts, sparse gradients) runs the same algorithm in torch ops, in float64 rounded once to the
    tensors' dtype; the norm G always spans both kinds of group.  After a step `kernel_norms()` returns what the kernels stored: G^2 and
    (|p|^2, |u|^2, r) per parameter, still on the device.
    """

    def __init__(self, params, lr=1e-3, bias_correction=True, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.01, amsgrad=False,
                 adam_w_mode=True, grad_averaging=True, set_grad_none=True, max_grad_norm=1.0, use_nvlamb=False):
        if amsgrad:
            raise RuntimeError("HipLamb does not support the AMSGrad variant.")
        defaults = dict(lr=lr, bias_correction=bias_correction, betas=betas, eps=eps, weight_decay=weight_decay,
                        grad_averaging=grad_averaging, max_grad_norm=max_grad_norm)
        super().__init__(params, defaults)
        self.adam_w_mode = 1 if adam_w_mode else 0
        self.set_grad_none = set_grad_none
        self.use_nvlamb = use_nvlamb
        self._table = None          # launch tables of the groups the kernels take
        self._torch_only = set()    # groups found unfit for the kernels (by index)

    def __getstate__(self):
        # (torch's Optimizer pickles defaults, state and param_groups only; the launch tables hold events and pinned buffers and stay behind)
        return dict(super().__getstate__(), adam_w_mode=self.adam_w_mode, set_grad_none=self.set_grad_none, use_nvlamb=self.use_nvlamb)

    def __setstate__(self, state):
        super().__setstate__(state)
        self._table, self._torch_only = None, set()

    def zero_grad(self, set_to_none=None):
        super().zero_grad(set_to_none=self.set_grad_none if set_to_none is None else set_to_none)

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._table, self._torch_only = None, set()

    def _tables_for(self, work, dev):
        """ONE launch table for the tensors of every group the kernels take (group = a range of its items and chunks) and the workspace"""
        sig = tuple((gi, tuple((p.data_ptr(), p.numel()) for p in pl)) for gi, _, pl in work)
        t = self._table
        if t is not None and t.sig == sig:
            return t
        lib = L.load()
        t = _LaunchTable([p.numel() for _, _, pl in work for p in pl], lib.swv2_lamb_chunk(), L.LambItem, dev)
        t.sig, t.params, t.ranges, i0 = sig, [p for _, _, pl in work for p in pl], {}, 0
        for gi, _, pl in work:
            i1 = i0 + len(pl)
            t.ranges[gi] = (i0, t.chunk0[i0], i1, t.chunk0[i1] if i1 < t.n_items else t.n_chunks)      # item_lo, chunk_lo, item_hi, chunk_hi
            i0 = i1
        t.ws_bytes = lib.swv2_lamb_ws_bytes(t.n_items, t.n_chunks)
        t.ws = torch.zeros(t.ws_bytes // 4, dtype=torch.float32, device=dev)
        self._table = t
        return t

    def kernel_norms(self):
        """(G^2, {parameter: float tensor (|p|^2, |u|^2, r)}) as the kernels of the last step stored them (device tensors, views of the
        workspace); None when no group took the kernels"""
        t = self._table
        if t is None:
            return None
        ws = t.ws
        return ws[L.LAMB_WS_GNORM2], {p: ws[L.lamb_ws_item(i):L.lamb_ws_item(i) + 3] for i, p in enumerate(t.params)}

    # ---- step ----------------------------------------------------------------------------------------------
    def _flags(self, group):
        return ((L.LAMB_ADAMW if self.adam_w_mode else 0) | (L.LAMB_BIAS_CORRECTION if group["bias_correction"] else 0) |
                (L.LAMB_GRAD_AVERAGING if group["grad_averaging"] else 0) | (L.LAMB_NVLAMB if self.use_nvlamb else 0))

    @torch.no_grad()
    def step(self, closure=None, grad_inv_scale: float = 1.0):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        inv = _f32(grad_inv_scale)
        max_norm = _f32(self.defaults["max_grad_norm"])
        groups = []
        for gi, group in enumerate(self.param_groups):
            group["step"] = group["step"] + 1 if "step" in group else 1
            plist = [p for p in group["params"] if p.grad is not None and p.numel() > 0]
            for p in plist:
                s = self.state[p]
                if len(s) == 0:
                    s["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    s["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            if plist:
                groups.append((gi, group, plist))
        # which groups the kernels take: the first CUDA parameter names the device; tensors are looked at again whenever a pointer moved
        dev = next((p.device for _, _, pl in groups for p in pl if p.is_cuda), None)
        while True:
            work = [w for w in groups if dev is not None and w[0] not in self._torch_only]
            if not work:
                self._table, t = None, None
                break
            t = self._tables_for(work, dev)
            rows = tuple((p.data_ptr(), p.grad.data_ptr(), self.state[p]["exp_avg"].data_ptr(), self.state[p]["exp_avg_sq"].data_ptr(),
                          p.numel(), c0) for p, c0 in zip(t.params, t.chunk0))
            if rows == t.rows:
                break
            bad = {gi for gi, _, pl in work if not all(_kernel_ok(p, self.state[p], dev) for p in pl)}
            if not bad:
                t.upload(rows)
                break
            self._torch_only |= bad
        slow = [w for w in groups if t is None or w[0] not in t.ranges]
        # the slow groups' share of G^2 (float64), handed to the kernels as a device float
        extra = None
        for _, _, pl in slow:
            for p in pl:
                g = p.grad.to_dense() if p.grad.is_sparse else p.grad
                e = (g.double() * inv).pow(2).sum()
                extra = e if extra is None else extra + e.to(extra.device)
        if t is not None:
            lib = L.load()
            stream = torch.cuda.current_stream(dev).cuda_stream
            extra_dev = extra.to(dev, torch.float32).reshape(1) if extra is not None else None
            ws = t.ws
            L.check(lib.swv2_lamb_grad_norm(t.dev.data_ptr(), t.chunks.data_ptr(), t.n_items, t.n_chunks, inv, ws.data_ptr(),
                                            t.ws_bytes, stream), "swv2_lamb_grad_norm")
            for gi, group, pl in work:
                i0, c0, i1, c1 = t.ranges[gi]
                b1, b2 = group["betas"]
                L.check(lib.swv2_lamb_multi(t.dev.data_ptr(), t.chunks.data_ptr(), t.n_items, t.n_chunks, i0, i1, c0, c1,
                                            float(group["lr"]), float(b1), float(b2), float(group["eps"]), float(group["weight_decay"]), inv,
                                            max_norm, int(group["step"]), self._flags(group),
                                            extra_dev.data_ptr() if extra_dev is not None else None, ws.data_ptr(), t.ws_bytes, stream),
                        "swv2_lamb_multi")
                # the kernel wrote the parameters behind autograd's back: bump their version counters like an in-place torch op would
                torch.autograd.graph.increment_version(pl)
            clip = ws[L.LAMB_WS_CLIP].double()             # the kernels' own c (spans both kinds of group)
        elif extra is not None:
            G = extra.sqrt()
            clip = torch.where(G > max_norm, G / max_norm, torch.ones_like(G))
        for _, group, pl in slow:
            self._torch_group(group, pl, clip, inv)
        return loss

    def _torch_group(self, group, plist, clip, inv, ratios=None):
        """the update of one group in torch ops: float64 arithmetic on the fp32 values of the scalars, rounded once into m, v and p.
        ratios: {parameter: r} taken in place of the tensors' own trust ratios (a test steps both paths from the same c and r)"""
        b1, b2 = (_f32(b) for b in group["betas"])
        b3 = 1.0 - b1 if group["grad_averaging"] else 1.0
        eps, lr, wd, step = _f32(group["eps"]), _f32(group["lr"]), _f32(group["weight_decay"]), int(group["step"])
        bc1 = _f32(1.0 - b1 ** step) if group["bias_correction"] else 1.0
        bc2 = _f32(1.0 - b2 ** step) if group["bias_correction"] else 1.0
        for p in plist:
            s = self.state[p]
            m, v = s["exp_avg"], s["exp_avg_sq"]
            g = p.grad.to_dense() if p.grad.is_sparse else p.grad
            p64 = p.double()
            gh = g.double() * inv / clip.to(p.device)
            if not self.adam_w_mode:
                gh = gh + wd * p64
            m.copy_(b1 * m.double() + b3 * gh)
            v.copy_(b2 * v.double() + (1.0 - b2) * gh * gh)
            u = (m.double() / bc1) / ((v.double() / bc2).sqrt() + eps)         # from the moments as stored, like the kernels' stage 2
            if self.adam_w_mode:
                u = u + wd * p64
            if ratios is not None:
                r = ratios[p]
            elif self.use_nvlamb or wd != 0:
                pn, un = p64.norm(), u.norm()
                r = torch.where((pn != 0) & (un != 0), pn / un, torch.ones_like(pn))
            else:
                r = 1.0
            p.copy_(p64 - lr * r * u)
