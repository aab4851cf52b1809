// What the program-driven product libraries (derive, thermo, vert, agg, nbr) share on the host: the refusals of the descriptor's head, the
// table of claimed output slots, and the launch geometry of the (member, tile) kernels.  Plain C++ with nothing of HIP in it: a host
// compiler takes it on its own (tests/test_program_cpu.py).  Each library's valid() keeps the checks only it has.
#pragma once
#include <cstddef>
#include <cstdint>

namespace skprogram {

// the head of a descriptor: M members of (C, H, W) into (M, D, H, W) with member_stride.  C H W and D H W stay within 2^30 elements, so
// that a 32-bit lane offset in bytes reaches every point of a member and of its output
inline bool grid_ok(int M, int max_members, int member_align, int C, int H, int W, int D, size_t member_stride, int min_H = 1, int min_W = 1) {
    if (M < 1 || M > max_members || (member_align != 4 && member_align != 16)) return false;
    if (C < 1 || H < min_H || W < min_W || D < 1) return false;
    const size_t lim = (size_t)1 << 30, HW = (size_t)H * (size_t)W;
    return HW <= lim && (size_t)C <= lim / HW && (size_t)D <= lim / HW && member_stride >= (size_t)D * HW;
}

// the output slots a program has claimed so far; N: the most it can name
template <int N>
struct Slots {
    int slot[N], n = 0;
    // false for a slot outside [-1, D) or claimed before; -1 (a result not computed) claims nothing
    bool claim(int s, int D) {
        if (s < -1 || s >= D) return false;
        if (s < 0) return true;
        for (int k = 0; k < n; ++k)
            if (slot[k] == s) return false;
        if (n == N) return false;
        slot[n++] = s;
        return true;
    }
};

// 256 CUs x 8 workgroups of four waves at the most; a wave walks the (member, tile) pairs with the grid's stride
inline unsigned blocks_for(int M, uint32_t tiles) {
    const size_t groups = ((size_t)M * tiles + 3) / 4;
    return (unsigned)(groups < 2048 ? groups : 2048);
}

// whether a lane may move four floats at once: the members, the planes `ptr` (a null one passes) and every member's output begin on 16
// bytes; n_mult4: the length the kernel cuts into lanes' shares (W or H W) is a multiple of 4
template <typename... P>
inline bool vec_ok(int member_align, bool n_mult4, size_t member_stride, const P*... ptr) {
    return member_align == 16 && n_mult4 && member_stride % 4 == 0 && (... && (((uintptr_t)ptr & 15) == 0));
}

inline bool channel_ok(int ch, int C) { return ch >= 0 && ch < C; }

// a pressure in hPa (a NaN or an infinity fails the comparisons)
inline bool pressure_ok(float p) { return p >= 1e-3f && p <= 2000.f; }

}  // namespace skprogram
