"""csrc/gemm_rw.hip retires its LDS-DMA stages with hand-counted `s_waitcnt vmcnt(N)`: a register spill is a VMEM operation the count
does not know about (a reload would be waited for too early or too late).  The compiler's own resource report must show 0 bytes of
scratch and 0 spilled VGPRs for every gemm_rw_kernel instantiation of that file (cross-compiled for gfx950, no GPU needed; the pattern
of test_dma_kernels_with_hand_counted_waits_use_no_scratch)."""
import os
import re
import subprocess

from swin_v2_weather_amd import _lib as L


def test_streaming_row_gemm_uses_no_scratch(tmp_path):
    assert "gemm_rw.hip" in L.SOURCES
    src = os.path.join(L.CSRC, "gemm_rw.hip")
    r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Rpass-analysis=kernel-resource-usage",
                        "-c", src, "-o", str(tmp_path / "gemm_rw.o")], capture_output=True, text=True, timeout=900)
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
    rw = {k: v for k, v in seen.items() if "gemm_rw_kernel" in k}
    assert len(rw) >= 1, sorted(seen)
    for k, v in rw.items():
        assert v.get("ScratchSize [bytes/lane]") == 0 and v.get("VGPRs Spill") == 0, (k, v)
