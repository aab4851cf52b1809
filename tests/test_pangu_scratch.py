"""The compiler's resource report of Pangu's block and attention kernels (hipcc -Rpass-analysis=kernel-resource-usage, the way
tools/kernel_resources.py reads it): scratch memory of these kernels leaves the L2 and comes back (profiles/r06_pangu_pmc.json: WRITE_SIZE
above the algorithm's bytes by exactly the scratch size x lanes x tiles), so the figures reached in docs/experiments.md A7 are pinned here.
No GPU: a cross-compile for gfx950."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

CSRC = Path(__file__).resolve().parent.parent / "skyrim_amd" / "csrc"
KEYS = {"VGPRs": "vgprs", "ScratchSize [bytes/lane]": "scratch", "Occupancy [waves/SIMD]": "occupancy"}

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not installed")


@pytest.fixture(scope="module")
def resources():
    """{mangled kernel name: {"vgprs", "scratch", "occupancy"}} of fused_block.hip and attention.hip"""
    out = {}
    for f in ("fused_block", "attention"):
        r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "--cuda-device-only", "-c", f"{f}.hip", "-o", "/dev/null",
                            "-Rpass-analysis=kernel-resource-usage"], cwd=CSRC, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        name = None
        for line in r.stderr.splitlines():
            m = re.search(r"Function Name: (\S+)", line)
            if m:
                name = m.group(1)
                out[name] = {}
            for key, short in KEYS.items():
                m = re.search(re.escape(key) + r": (\d+)", line)
                if m and name:
                    out[name][short] = int(m.group(1))
    return out


def _one(resources, *parts):
    hits = [v for k, v in resources.items() if all(p in k for p in parts)]
    assert len(hits) == 1, (parts, [k for k in resources if parts[0] in k])
    return hits[0]


# <C, FM, ONE>: the first two are what the default plan launches (12 x C = 384 with one-plane activations, 4 x C = 192 with two terms)
@pytest.mark.parametrize("shape", ["Li384ELi1ELb1E", "Li192ELi2ELb0E", "Li192ELi2ELb1E", "Li384ELi1ELb0E"])
def test_block_kernel_uses_no_scratch_at_two_waves_per_simd(resources, shape):
    r = _one(resources, "proj_mlp2_kernel", f"Blk2ShapeI{shape}")
    assert r["scratch"] == 0, r
    assert r["occupancy"] == 2 and r["vgprs"] <= 256, r


# <T, C, FM, NWAVES, WPE> of the three-term kernel (bf16x3, term_plan 0, the load-time guard's fall-back) and its scratch before it was
# put on the two-term kernel's ring and stages (docs/experiments.md, "Pangu block kernels on shared stages"): sharing code may not add to it
@pytest.mark.parametrize("shape, cap", [("IDF16bNS_10BlockShapeILi192ELi2ELi4ELi2E", 396), ("IDF16bNS_10BlockShapeILi384ELi1ELi8ELi2E", 396),
                                        ("IDF16_NS_10BlockShapeILi192ELi2ELi4ELi2E", 396), ("IDF16_NS_10BlockShapeILi384ELi1ELi8ELi2E", 444)])
def test_three_term_block_kernel_scratch_stays_at_or_below_its_figure(resources, shape, cap):
    r = _one(resources, "proj_mlp_kernel", shape)
    assert r["scratch"] <= cap, r
    assert r["occupancy"] == 2 and r["vgprs"] <= 256, r


# <C, PL>, output planes: what the default plan launches
@pytest.mark.parametrize("shape", ["QaShapeILi384ELi1EEELi1E", "QaShapeILi192ELi2EEELi2E"])
def test_attention_kernel_scratch_is_the_query_fragments_only(resources, shape):
    """144 bytes of qv[9] (indexed at run time by the rolled query loop) + 16 of alignment: no register spills on top"""
    r = _one(resources, "qkv_attention_kernel", shape)
    assert r["scratch"] <= 160, r
    assert r["occupancy"] == 2 and r["vgprs"] <= 256, r
