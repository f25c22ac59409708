"""Host (no GPU): the host half of the l2 loss entry points that stream planes, swv2_loss_ws_bytes / swv2_loss_sums / swv2_loss_grad
(csrc/loss_l2.hip): the workspace arithmetic, header and ctypes in step, and every refusal before a launch."""
import ctypes
import os
import re

from swin_v2_weather_amd import _lib as L
from tests import score_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_abi_version_sources_and_workspace_arithmetic():
    assert L.ABI_VERSION == 113 and "loss_l2.hip" in L.SOURCES
    lib = L.load()
    assert lib.swv2_version() == 113
    for (B, C, H, W) in ((1, 1, 1, 4), (2, 3, 5, 8), (1, 73, 720, 1440), (2, 73, 720, 1440), (1, 2100, 2, 4), (3, 5, 16, 32)):
        slices = lib.swv2_score_slices(B * C, H, W)
        assert lib.swv2_loss_ws_bytes(B * C, H, W) == B * C * slices * 8 == lib.swv2_l1_ws_bytes(B * C, H, W) and slices == R.plan_slices(B * C)
    for bad in ((0, 4, 4), (4, 0, 4), (4, 4, 0), (-1, 4, 4)):
        assert lib.swv2_loss_ws_bytes(*bad) == 0, bad


def test_header_and_ctypes_agree_on_the_l2_loss_entry_points():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "swv2.h")).read(), flags=re.S)
    kinds = {"int": ctypes.c_int, "long": ctypes.c_long, "size_t": ctypes.c_size_t}
    seen = []
    for ret, name, args in re.findall(r"\b(int|size_t)\s+(swv2_loss_[a-z_]+)\s*\(([^)]*)\)\s*;", txt):
        want = [ctypes.c_void_p if "*" in a else kinds[a.split()[0]] for a in (x.strip() for x in args.split(","))]
        res, argtypes = L.SYMBOLS[name]
        assert res is kinds[ret] and argtypes == want, name
        seen.append(name)
    assert sorted(seen) == ["swv2_loss_finalize", "swv2_loss_grad", "swv2_loss_part_reduce", "swv2_loss_resid_to_image", "swv2_loss_sums",
                            "swv2_loss_ws_bytes"]
    lib = L.load()
    assert all(hasattr(lib, n) for n in seen)


def test_every_refusal_returns_invalid_with_a_message_and_without_a_gpu():
    """Arguments are checked before anything is launched, so the pointers only have to be non-null here: a refused call touches nothing."""
    lib = L.load()
    P = 4096
    BC, H, W = 6, 8, 16
    ok = lib.swv2_loss_ws_bytes(BC, H, W)

    def sums(prd=P, tar=P, q=P, s=P, BC=BC, H=H, W=W, ws=P, wb=ok):
        return lib.swv2_loss_sums(prd, tar, q, s, BC, H, W, ws, wb, None)

    def grad(prd=P, tar=P, q=P, coef=P, d=P, BC=BC, H=H, W=W):
        return lib.swv2_loss_grad(prd, tar, q, coef, d, BC, H, W, None)
    for call, word in ((lambda: sums(prd=None), b"null"), (lambda: sums(tar=None), b"null"), (lambda: sums(q=None), b"null"),
                       (lambda: sums(s=None), b"null"), (lambda: sums(ws=None), b"null"), (lambda: sums(W=18), b"W % 4"),
                       (lambda: sums(W=0), b"shape"), (lambda: sums(BC=0), b"shape"), (lambda: sums(H=0), b"shape"),
                       (lambda: sums(prd=P + 4), b"aligned"), (lambda: sums(tar=P + 8), b"aligned"), (lambda: sums(ws=P + 4), b"aligned"),
                       (lambda: sums(s=P + 4), b"aligned"), (lambda: sums(wb=ok - 1), b"workspace"), (lambda: sums(wb=0), b"workspace"),
                       (lambda: sums(BC=1 << 20), b"shape"), (lambda: sums(H=1 << 15, W=1 << 15), b"shape"),
                       (lambda: grad(prd=None), b"bad argument"), (lambda: grad(tar=None), b"bad argument"), (lambda: grad(q=None), b"bad argument"),
                       (lambda: grad(coef=None), b"bad argument"), (lambda: grad(d=None), b"bad argument"), (lambda: grad(W=18), b"W % 4"),
                       (lambda: grad(BC=65536), b"too large"), (lambda: grad(H=1 << 15, W=1 << 15), b"too large"),
                       (lambda: grad(prd=P + 4), b"aligned"), (lambda: grad(tar=P + 8), b"aligned"), (lambda: grad(d=P + 4), b"aligned"),
                       (lambda: grad(H=0), b"bad argument"), (lambda: grad(BC=0), b"bad argument")):
        assert call() == -1
        assert word in lib.swv2_last_error() and b"loss_" in lib.swv2_last_error(), lib.swv2_last_error()
