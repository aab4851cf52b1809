"""The compiler's resource report of the fused QKV + attention kernel (hipcc -Rpass-analysis=kernel-resource-usage, as in
test_pangu_scratch.py): the nine Q fragments of a (window, head) stay in registers through the rolled query loop -- four 9-element vectors
read with the register index, csrc/attention.hip, docs/experiments.md A8 -- so NOTHING of the kernel lives in scratch memory, which on this
chip leaves the L2 and comes back.  Every instantiation: <C, PL> = <192, 1>, <192, 2>, <384, 1>, each with one and with two output planes.
No GPU: a cross-compile for gfx950."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

CSRC = Path(__file__).resolve().parent.parent / "skyrim_amd" / "csrc"
KEYS = {"VGPRs": "vgprs", "VGPRs Spill": "vgpr_spill", "ScratchSize [bytes/lane]": "scratch", "Occupancy [waves/SIMD]": "occupancy"}
SHAPES = [f"QaShapeILi{c}ELi{pl}EEELi{npl}E" for c, pl in ((192, 1), (192, 2), (384, 1)) for npl in (1, 2)]

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not installed")


@pytest.fixture(scope="module")
def resources():
    """{mangled kernel name: {"vgprs", "vgpr_spill", "scratch", "occupancy"}} of attention.hip"""
    r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "--cuda-device-only", "-c", "attention.hip", "-o", "/dev/null",
                        "-Rpass-analysis=kernel-resource-usage"], cwd=CSRC, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    out, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            out[name] = {}
        for key, short in KEYS.items():
            m = re.search(r" " + re.escape(key) + r": (\d+)", line)
            if m and name:
                out[name][short] = int(m.group(1))
    return out


def test_every_instantiation_is_reported(resources):
    fused = [k for k in resources if "qkv_attention_kernel" in k]
    assert len(fused) == len(SHAPES) == 6, fused


@pytest.mark.parametrize("shape", SHAPES)
def test_fused_attention_kernel_uses_no_scratch(resources, shape):
    hits = [v for k, v in resources.items() if "qkv_attention_kernel" in k and shape in k]
    assert len(hits) == 1, (shape, [k for k in resources if "qkv_attention_kernel" in k])
    r = hits[0]
    assert set(r) == set(KEYS.values()), r
    assert r["scratch"] == 0 and r["vgpr_spill"] == 0, r
    assert r["occupancy"] == 2 and r["vgprs"] <= 256, r
