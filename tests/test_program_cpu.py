"""csrc/program.h, the host prelude the program-driven product libraries share, on its own: a stand-alone program that includes nothing
else is compiled by the host compiler (no offload) and checks ``grid_ok``, ``Slots``, ``blocks_for``, ``vec_ok`` and the two range tests
at their edges.  What each library refuses as a whole is the record of tests/test_{derive,thermo,vert,agg,nbr}_cpu.py."""
from __future__ import annotations

import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]

SOURCE = r"""
#include "program.h"
#include <cstdio>
#include <limits>
using namespace skprogram;

static int failed = 0;
#define CHECK(c) do { if (!(c)) { std::printf("line %d: %s\n", __LINE__, #c); ++failed; } } while (0)

int main() {
    const int MAXM = 64;
    const size_t ONE = 1;
    // grid_ok(M, max_members, member_align, C, H, W, D, member_stride, min_H, min_W)
    CHECK(grid_ok(2, MAXM, 16, 6, 5, 8, 3, 120));
    CHECK(grid_ok(1, MAXM, 4, 1, 1, 1, 1, 1) && grid_ok(MAXM, MAXM, 4, 1, 1, 1, 1, 1));
    CHECK(!grid_ok(0, MAXM, 4, 1, 1, 1, 1, 1) && !grid_ok(MAXM + 1, MAXM, 4, 1, 1, 1, 1, 1) && !grid_ok(-1, MAXM, 4, 1, 1, 1, 1, 1));
    CHECK(!grid_ok(2, MAXM, 8, 6, 5, 8, 3, 120) && !grid_ok(2, MAXM, 0, 6, 5, 8, 3, 120) && !grid_ok(2, MAXM, 32, 6, 5, 8, 3, 120));
    CHECK(!grid_ok(2, MAXM, 16, 0, 5, 8, 3, 120) && !grid_ok(2, MAXM, 16, 6, 0, 8, 3, 120) && !grid_ok(2, MAXM, 16, 6, 5, 0, 3, 120));
    CHECK(!grid_ok(2, MAXM, 16, 6, 5, 8, 0, 120));
    CHECK(grid_ok(1, MAXM, 4, 1, 32768, 32768, 1, ONE << 30));                  // H W = 2^30
    CHECK(!grid_ok(1, MAXM, 4, 1, 32769, 32768, 1, ONE << 31));                 // the first H W beyond it on these rows
    CHECK(!grid_ok(1, MAXM, 4, 2, 32768, 32768, 1, ONE << 30));                 // C = 2^30 / (H W) + 1
    CHECK(!grid_ok(1, MAXM, 4, 1, 32768, 32768, 2, ONE << 31));                 // D = 2^30 / (H W) + 1
    CHECK(grid_ok(1, MAXM, 4, 1 << 20, 32, 32, 1 << 20, ONE << 30));            // C H W = D H W = 2^30
    CHECK(!grid_ok(1, MAXM, 4, (1 << 20) + 1, 32, 32, 1, 1024) && !grid_ok(1, MAXM, 4, 1, 32, 32, (1 << 20) + 1, ONE << 31));
    CHECK(grid_ok(2, MAXM, 16, 6, 5, 8, 3, 121) && !grid_ok(2, MAXM, 16, 6, 5, 8, 3, 119));      // member_stride = D H W - 1
    CHECK(grid_ok(1, MAXM, 4, std::numeric_limits<int>::max() / 4, 2, 2, 1, 4) == false);        // C H W beyond 2^30, no overflow on the way
    CHECK(grid_ok(2, MAXM, 16, 6, 3, 4, 3, 36, 3, 4));                          // min_H, min_W (derive: 3 and 4)
    CHECK(!grid_ok(2, MAXM, 16, 6, 2, 4, 3, 24, 3, 4) && !grid_ok(2, MAXM, 16, 6, 3, 3, 3, 27, 3, 4));
    CHECK(grid_ok(2, MAXM, 16, 6, 2, 3, 3, 18));

    // Slots<N>::claim(s, D)
    Slots<4> s;
    CHECK(!s.claim(-2, 8) && !s.claim(8, 8) && s.n == 0);
    CHECK(s.claim(-1, 8) && s.claim(-1, 8) && s.n == 0);                        // "not computed" claims nothing, as often as it comes
    CHECK(s.claim(7, 8) && !s.claim(7, 8) && s.n == 1);
    CHECK(s.claim(0, 8) && s.claim(3, 8) && s.claim(5, 8) && s.n == 4);         // the capacity, exactly
    CHECK(!s.claim(0, 8) && !s.claim(5, 8) && s.claim(-1, 8) && s.n == 4);
    CHECK(!s.claim(1, 8) && s.n == 4);                                          // a full table refuses; it does not write past its end
    Slots<1> one;
    CHECK(!one.claim(1, 1) && one.claim(0, 1) && !one.claim(0, 1));

    // blocks_for(M, tiles)
    CHECK(blocks_for(1, 1) == 1 && blocks_for(1, 4) == 1 && blocks_for(1, 5) == 2 && blocks_for(3, 3) == 3);
    CHECK(blocks_for(64, 128) == 2048 && blocks_for(64, 128 - 1) == 2032 && blocks_for(1, 8188) == 2047);      // 8192 pairs in fours: 2048 groups
    CHECK(blocks_for(64, 129) == 2048 && blocks_for(64, 512) == 2048 && blocks_for(64, 0xffffffffu) == 2048);     // (64, 512): 8192 groups

    // vec_ok(member_align, n_mult4, member_stride, ptr...)
    const void *a16 = (const void*)4096, *a4 = (const void*)4100, *null = nullptr;
    CHECK(vec_ok(16, true, 120, a16) && vec_ok(16, true, 120, a16, null) && vec_ok(16, true, 120, a16, a16));
    CHECK(!vec_ok(4, true, 120, a16) && !vec_ok(16, false, 120, a16) && !vec_ok(16, true, 122, a16));
    CHECK(!vec_ok(16, true, 120, a4) && !vec_ok(16, true, 120, a16, a4) && !vec_ok(16, true, 120, a4, null));
    CHECK(vec_ok(16, true, 120, (const float*)a16, (const double*)a16));

    CHECK(channel_ok(0, 6) && channel_ok(5, 6) && !channel_ok(6, 6) && !channel_ok(-1, 6));
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    CHECK(pressure_ok(1e-3f) && pressure_ok(500.f) && pressure_ok(2000.f));
    CHECK(!pressure_ok(0.f) && !pressure_ok(-500.f) && !pressure_ok(9e-4f) && !pressure_ok(2000.5f) && !pressure_ok(inf) && !pressure_ok(-inf) && !pressure_ok(nan));
    if (!failed) std::printf("program.h ok\n");
    return failed ? 1 : 0;
}
"""


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not installed")
def test_the_header_stands_alone_and_holds_at_its_edges(tmp_path):
    src, exe = tmp_path / "program_check.cpp", tmp_path / "program_check"
    src.write_text(SOURCE)
    r = subprocess.run(["hipcc", "-x", "c++", "-std=c++17", "-Wall", "-Werror", f"-I{ROOT / 'skyrim_amd' / 'csrc'}", str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "program.h ok", r.stdout[-2000:] + r.stderr[-2000:]


def test_the_header_includes_nothing_of_hip():
    text = (ROOT / "skyrim_amd" / "csrc" / "program.h").read_text()
    includes = [line.split()[1] for line in text.splitlines() if line.startswith("#include")]
    assert includes == ["<cstddef>", "<cstdint>"] and "__device__" not in text and "__global__" not in text
