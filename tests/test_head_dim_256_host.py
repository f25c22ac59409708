"""Host tests (no GPU) of the 256-channel attention heads: the geometry the C ABI reports, the model constructor at embed 2048 /
8 heads, the yaml entry that uses it, and the compiler's resource report of csrc/attn_d256.hip (cross-compiled for gfx950)."""
import ctypes
import os
import re
import subprocess

import pytest

from swin_v2_weather_amd import _lib as L
from swin_v2_weather_amd.networks import helpers, swinv2_global as N
from swin_v2_weather_amd.utils.YParams import YParams

CFG = os.path.join(os.path.dirname(L.__file__), "config", "swin.yaml")
E2048 = "swin_73var_geo_depth24_e2048_mlp2_chweight_invar"


def geometry(Lw, d):
    lp, dp = ctypes.c_int(), ctypes.c_int()
    rc = L.load().swv2_attn_geometry(Lw, d, ctypes.byref(lp), ctypes.byref(dp))
    return (lp.value, dp.value) if rc == 0 else rc


@pytest.mark.parametrize("Lw", [162, 170, 80, 65, 176])
def test_geometry_of_256_wide_heads(Lw):
    assert geometry(Lw, 256) == (176, 256)


@pytest.mark.parametrize("Lw,d", [(54, 256), (64, 256), (162, 192), (162, 160), (162, 260), (200, 256)])
def test_other_wide_geometries_stay_rejected(Lw, d):
    assert geometry(Lw, d) == -1


def _kw(**over):
    kw = dict(img_size=(72, 144), patch_size=4, depths=(1,), num_heads=(8,), in_chans=3, out_chans=3, embed_dim=2048,
              img_window_ratio=8, full_pos_embed=True, rel_pos=False)
    kw.update(over)
    return kw


def test_constructor_at_embed_2048_on_a_162_token_window():
    m = N.SwinTransformerV2Cr(**_kw())
    blk = m.stages[0].blocks[0] if hasattr(m, "stages") else next(b for b in m.modules() if isinstance(b, N.SwinTransformerV2CrBlock))
    assert blk.window_area == 162


def test_rel_pos_at_head_dim_256_is_rejected_at_construction():
    with pytest.raises(L.Swv2Error, match="rel_pos"):
        N.SwinTransformerV2Cr(**_kw(rel_pos=True))


def test_head_dim_256_on_a_54_token_window_names_the_window_range():
    with pytest.raises(L.Swv2Error, match="head_dim=256 needs a window of 65 - 176 tokens"):
        N.SwinTransformerV2Cr(**_kw(img_size=(48, 72)))


def test_yaml_entry_builds_through_get_model():
    p = YParams(CFG, E2048)
    assert p.embed_dim == 2048 and p.mlp_ratio == 2 and p.rel_pos is False
    p.update_params({"depth": 1, "n_in_channels": len(p.in_channels), "n_out_channels": len(p.out_channels)})
    m = helpers.get_model(p)
    blocks = [b for b in m.modules() if isinstance(b, N.SwinTransformerV2CrBlock)]
    assert len(blocks) == 1 and blocks[0].window_area == 162 and blocks[0].attn.num_heads == 8


def test_256_wide_attention_kernels_use_no_scratch(tmp_path):
    """0 bytes of scratch and 0 spilled VGPRs in every kernel of csrc/attn_d256.hip (compiler resource report, gfx950)."""
    src = os.path.join(L.CSRC, "attn_d256.hip")
    r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Rpass-analysis=kernel-resource-usage",
                        "-c", src, "-o", str(tmp_path / "d256.o")], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    seen, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            continue
        m = re.search(r"(ScratchSize \[bytes/lane\]|VGPRs Spill|LDS Size \[bytes/block\]): (\d+)", line)
        if m and name:
            seen.setdefault(name, {})[m.group(1)] = int(m.group(2))
    kern = {k: v for k, v in seen.items() if "d256_kernel" in k}
    assert len(kern) == 4, sorted(seen)                        # forward / backward x (L = 162, run-time L)
    for k, v in kern.items():
        assert v.get("ScratchSize [bytes/lane]") == 0 and v.get("VGPRs Spill") == 0, (k, v)
        assert v.get("LDS Size [bytes/block]", 1 << 30) <= 160 * 1024, (k, v)
