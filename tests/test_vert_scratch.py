"""The compiler's resource report of csrc/vert_ops.hip: the kernels of vertical interpolation use no scratch memory and no LDS (the
levels of a crossing are per-lane values; a register array indexed by one would go to scratch)."""
from __future__ import annotations

import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not installed")
def test_the_kernels_use_no_scratch_memory():
    r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "--cuda-device-only", "-c", "vert_ops.hip",
                        "-o", "/dev/null", "-Rpass-analysis=kernel-resource-usage"], cwd=ROOT / "skyrim_amd" / "csrc", capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    found, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            found[name] = {}
        for key in ("VGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "LDS Size [bytes/block]"):
            m = re.search(re.escape(key) + r": (\d+)", line)
            if m and name:
                found[name][key] = int(m.group(1))
    kernels = [k for k in found if "vert_kernel" in k]
    assert len(kernels) == 2 and len(found) == 2, list(found)                                         # the vector and the scalar path
    for k in kernels:
        print(k, found[k])
        assert found[k]["ScratchSize [bytes/lane]"] == 0 and found[k]["LDS Size [bytes/block]"] == 0, (k, found[k])
        assert found[k]["VGPRs"] <= 256 and found[k]["Occupancy [waves/SIMD]"] >= 2, (k, found[k])
