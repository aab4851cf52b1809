// Cyclone detection (include/skyrim_track.h): a prefilter over each member's msl band -- the 3 x 3 lexicographic minima, each value read
// from HBM once -- and one wave per survivor that walks the integer windows of the four criteria and reduces over its 64 lanes.  All
// geometry is host-made integer tables: no distance is computed here.  The only atomics are integer adds on the two counters.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "../../include/skyrim_track.h"
#include "fields.h"

namespace {

struct TrackArgs {
    int M, H, W, j0, Hb;
    int ch_msl, ch_u10, ch_v10, ch_u850, ch_v850, ch_zup, ch_zlo;
    int d_msl, d_vort, d_wind, d_core;
    float thr_msl, thr_vort, thr_wind, thr_core;
    uint32_t list_cap;
    int capacity;
};

// the workspace: one counter (16 bytes reserved), then the survivors as (member, idx) pairs
struct Survivor { int32_t member, idx; };

using namespace skfields;

// a member's address is its pointer (wave-uniform, scalar registers) plus one 32-bit per-lane offset (C H W <= 2^30)
__device__ __forceinline__ float load_f(const float* base, uint32_t elem) { return load_vec<1>(base, elem); }

// (pa, ia) strictly below (pb, ib) in the lexicographic order; false when either value is a NaN
__device__ __forceinline__ bool lex_below(float pa, int ia, float pb, int ib) { return pa < pb || (pa == pb && ia < ib); }

// kernel 1: one wave per (member, band row); lanes 1 .. 62 of a step own a point, lanes 0 and 63 hold the halo columns
__global__ void __launch_bounds__(256) track_prefilter_kernel(const TrackArgs a, const float* const* __restrict__ members,
                                                               uint32_t* __restrict__ n_surv, Survivor* __restrict__ list) {
    const int lane = threadIdx.x & 63;
    const int W = a.W;
    const uint32_t rows = (uint32_t)a.M * (uint32_t)a.Hb, nw = gridDim.x * 4u;
    for (uint32_t r = blockIdx.x * 4u + (threadIdx.x >> 6); r < rows; r += nw) {
        const int m = uniform((int)(r / (uint32_t)a.Hb));
        const int j = uniform(a.j0 + (int)(r - (uint32_t)m * (uint32_t)a.Hb));      // 1 <= j <= H - 2: checked by the caller
        const float* x = members[m];
        const uint32_t row_c = ((uint32_t)a.ch_msl * (uint32_t)a.H + (uint32_t)j) * (uint32_t)W;
        for (int base = 0; base < W; base += 62) {
            const int c = base + lane - 1;                        // -1 .. W + 61
            const int col = c < 0 ? W - 1 : (c >= W ? 0 : c);     // (c == W is column 0; beyond it the lane owns nothing)
            const float pn = load_f(x, row_c - W + col), pc = load_f(x, row_c + col), ps = load_f(x, row_c + W + col);
            const int ic = j * W + col;
            const int lw = lane > 0 ? lane - 1 : 0, le = lane < 63 ? lane + 1 : 63;
            const float wn = __shfl(pn, lw), wc = __shfl(pc, lw), wsv = __shfl(ps, lw);
            const float en = __shfl(pn, le), ec = __shfl(pc, le), es = __shfl(ps, le);
            const int iw = __shfl(ic, lw), ie = __shfl(ic, le);
            bool ok = lane >= 1 && lane <= 62 && c < W && pc <= a.thr_msl;
            ok = ok && lex_below(pc, ic, wn, iw - W) && lex_below(pc, ic, pn, ic - W) && lex_below(pc, ic, en, ie - W);
            ok = ok && lex_below(pc, ic, wc, iw) && lex_below(pc, ic, ec, ie);
            ok = ok && lex_below(pc, ic, wsv, iw + W) && lex_below(pc, ic, ps, ic + W) && lex_below(pc, ic, es, ie + W);
            if (ok) {
                const uint32_t slot = atomicAdd(n_surv, 1u);
                if (slot < a.list_cap) list[slot] = Survivor{m, ic};           // (always: two survivors are never neighbours)
            }
        }
    }
}

// the points of one window: the wave's lanes along the longitude, row after row; f(row, col)
template <class F>
__device__ __forceinline__ void for_window(const int32_t* __restrict__ h, int D, int jb, int j, int i, int W, int lane, F f) {
    const int32_t* hr = h + (size_t)jb * (size_t)(2 * D + 1);
    const int wmax = (W - 1) / 2;
    for (int dj = -D; dj <= D; ++dj) {
        int hw = uniform(hr[dj + D]);
        if (hw < 0) continue;
        hw = hw < wmax ? hw : wmax;
        for (int di = lane - hw; di <= hw; di += 64) {
            int col = i + di;
            col += col < 0 ? W : 0;
            col -= col >= W ? W : 0;
            f(j + dj, col);
        }
    }
}

// kernel 2: one wave per survivor.  CORE: the warm-core criterion is in use.
template <bool CORE>
__global__ void __launch_bounds__(256) track_eval_kernel(const TrackArgs a, const float* const* __restrict__ members,
                                                          const int32_t* __restrict__ h_msl, const int32_t* __restrict__ h_vort,
                                                          const int32_t* __restrict__ h_wind, const int32_t* __restrict__ h_core,
                                                          const float* __restrict__ rowc, const uint32_t* __restrict__ n_surv,
                                                          const Survivor* __restrict__ list, sktrack_record* __restrict__ records,
                                                          int32_t* __restrict__ count) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const int W = a.W;
    const uint32_t H = (uint32_t)a.H, Wu = (uint32_t)a.W;
    uint32_t total = *n_surv;
    total = total < a.list_cap ? total : a.list_cap;
    const uint32_t nw = gridDim.x * 4u;
    for (uint32_t s = blockIdx.x * 4u + (threadIdx.x >> 6); s < total; s += nw) {
        const int m = uniform(list[s].member), idx = uniform(list[s].idx);
        const int j = idx / W, i = idx - j * W, jb = j - a.j0;
        const float* x = members[m];
        const float pc = load_f(x, ((uint32_t)a.ch_msl * H + (uint32_t)j) * Wu + (uint32_t)i);

        // 1. the lexicographic minimum of the msl window, the centre left out; a NaN anywhere in the window fails
        float bp = __builtin_inff();
        int bi = 0x7fffffff;
        bool nan = false;
        for_window(h_msl, a.d_msl, jb, j, i, W, lane, [&](int row, int col) {
            const float p = load_f(x, ((uint32_t)a.ch_msl * H + (uint32_t)row) * Wu + (uint32_t)col);
            const int iq = row * W + col;
            nan = nan || p != p;
            if (iq != idx && lex_below(p, iq, bp, bi)) { bp = p; bi = iq; }
        });
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const float op = __shfl_xor(bp, off);
            const int oi = __shfl_xor(bi, off);
            if (lex_below(op, oi, bp, bi)) { bp = op; bi = oi; }
        }
        if (__any(nan) || !lex_below(pc, idx, bp, bi)) continue;

        // 2. cyclonic vorticity at 850 hPa
        float vort = -__builtin_inff();
        for_window(h_vort, a.d_vort, jb, j, i, W, lane, [&](int row, int col) {
            const int ce = col + 1 < W ? col + 1 : 0, cw = col > 0 ? col - 1 : W - 1;
            const uint32_t vrow = ((uint32_t)a.ch_v850 * H + (uint32_t)row) * Wu, urow = ((uint32_t)a.ch_u850 * H + (uint32_t)row) * Wu;
            const float ve = load_f(x, vrow + ce), vw = load_f(x, vrow + cw);
            const float un = load_f(x, urow + Wu + col), us = load_f(x, urow - Wu + col);       // rows row + 1 and row - 1
            const float4 rc = *(const float4*)(rowc + 4 * row);
            const float t1 = rc.x * (ve - vw), t2 = rc.y * un, t3 = rc.z * us;
            const float z = (t1 - (t2 - t3)) * rc.w;
            vort = z > vort ? z : vort;
        });
        vort = wave_max(vort);
        if (!(vort >= a.thr_vort)) continue;

        // 3. wind at 10 m
        float wind = -__builtin_inff();
        for_window(h_wind, a.d_wind, jb, j, i, W, lane, [&](int row, int col) {
            const float u = load_f(x, ((uint32_t)a.ch_u10 * H + (uint32_t)row) * Wu + (uint32_t)col);
            const float v = load_f(x, ((uint32_t)a.ch_v10 * H + (uint32_t)row) * Wu + (uint32_t)col);
            const float uu = u * u, vv = v * v;
            const float sp = sqrtf(uu + vv);
            wind = sp > wind ? sp : wind;
        });
        wind = wave_max(wind);
        if (!(wind >= a.thr_wind)) continue;

        // 4. warm core
        float core = 0.f;
        if (CORE) {
            const uint32_t cu = ((uint32_t)a.ch_zup * H + (uint32_t)j) * Wu + (uint32_t)i, cl = ((uint32_t)a.ch_zlo * H + (uint32_t)j) * Wu + (uint32_t)i;
            const float tc = load_f(x, cu) - load_f(x, cl);
            float dmax = -__builtin_inff();
            double sum = 0.0;
            int n = 0;
            for_window(h_core, a.d_core, jb, j, i, W, lane, [&](int row, int col) {
                const float tq = load_f(x, ((uint32_t)a.ch_zup * H + (uint32_t)row) * Wu + (uint32_t)col) -
                                 load_f(x, ((uint32_t)a.ch_zlo * H + (uint32_t)row) * Wu + (uint32_t)col);
                const float d = tq - tc;
                dmax = d > dmax ? d : dmax;
                sum += (double)d;
                ++n;
            });
            dmax = wave_max(dmax);
            sum = wave_sum(sum);
            n = wave_sum(n);
            core = (float)((double)dmax - sum / (double)n);
            if (!(core >= a.thr_core)) continue;
        }
        if (lane == 0) {
            const int slot = atomicAdd(count, 1);
            if (slot >= 0 && slot < a.capacity) records[slot] = sktrack_record{m, j, i, pc, vort, wind, core, 0};
        }
    }
}

size_t list_cap(int M, int Hb, int W) { return (size_t)M * (size_t)((Hb + 1) / 2) * (size_t)((W + 1) / 2); }

bool valid_shape(int M, int Hb, int W) { return M >= 1 && M <= SKTRACK_MAX_MEMBERS && Hb >= 1 && W >= 3; }

bool channel_ok(int ch, int C) { return ch >= 0 && ch < C; }

// every row a window of reach D touches, and the rows above and below it, are inside the grid whatever the table holds
bool reach_ok(int D, int j0, int j1, int H) { return D >= 0 && j0 - D >= 1 && j1 - 1 + D <= H - 2; }

}  // namespace

extern "C" int sktrack_abi_version(void) { return SKTRACK_ABI_VERSION; }

extern "C" size_t sktrack_workspace_bytes(int M, int Hb, int W) {
    if (!valid_shape(M, Hb, W)) return 0;
    return 16 + sizeof(Survivor) * list_cap(M, Hb, W);
}

extern "C" int sktrack_detect(const sktrack_desc* d, void* stream) {
    if (!d || !d->members || !d->rowc || !d->count || !d->workspace || d->C < 1 || d->H < 3 || d->j0 < 0 || d->j1 <= d->j0 || d->j1 > d->H)
        return SKTRACK_E_ARG;
    const int Hb = d->j1 - d->j0;
    if (!valid_shape(d->M, Hb, d->W)) return SKTRACK_E_ARG;
    if ((size_t)d->C * (size_t)d->H > (1ull << 30) / (size_t)d->W) return SKTRACK_E_ARG;               // 32-bit byte offsets in the kernels
    if (!channel_ok(d->ch_msl, d->C) || !channel_ok(d->ch_u10, d->C) || !channel_ok(d->ch_v10, d->C) || !channel_ok(d->ch_u850, d->C) ||
        !channel_ok(d->ch_v850, d->C))
        return SKTRACK_E_ARG;
    const bool core = d->ch_zup != -1 || d->ch_zlo != -1;
    if (core && (!channel_ok(d->ch_zup, d->C) || !channel_ok(d->ch_zlo, d->C) || !d->h_core || ((uintptr_t)d->h_core & 3))) return SKTRACK_E_ARG;
    if (!d->h_msl || !d->h_vort || !d->h_wind || (((uintptr_t)d->h_msl | (uintptr_t)d->h_vort | (uintptr_t)d->h_wind) & 3)) return SKTRACK_E_ARG;
    if (!reach_ok(d->d_msl, d->j0, d->j1, d->H) || !reach_ok(d->d_vort, d->j0, d->j1, d->H) || !reach_ok(d->d_wind, d->j0, d->j1, d->H) ||
        (core && !reach_ok(d->d_core, d->j0, d->j1, d->H)))
        return SKTRACK_E_ARG;
    if (d->capacity < 0 || (d->capacity > 0 && !d->records) || ((uintptr_t)d->records & 3) || ((uintptr_t)d->count & 3)) return SKTRACK_E_ARG;
    if (((uintptr_t)d->rowc & 15) || ((uintptr_t)d->workspace & 7) || d->workspace_bytes < sktrack_workspace_bytes(d->M, Hb, d->W))
        return SKTRACK_E_ARG;
    TrackArgs a = {};
    a.M = d->M; a.H = d->H; a.W = d->W; a.j0 = d->j0; a.Hb = Hb;
    a.ch_msl = d->ch_msl; a.ch_u10 = d->ch_u10; a.ch_v10 = d->ch_v10; a.ch_u850 = d->ch_u850; a.ch_v850 = d->ch_v850;
    a.ch_zup = d->ch_zup; a.ch_zlo = d->ch_zlo;
    a.d_msl = d->d_msl; a.d_vort = d->d_vort; a.d_wind = d->d_wind; a.d_core = core ? d->d_core : 0;
    a.thr_msl = d->thr_msl; a.thr_vort = d->thr_vort; a.thr_wind = d->thr_wind; a.thr_core = d->thr_core;
    a.list_cap = (uint32_t)list_cap(d->M, Hb, d->W);
    a.capacity = d->capacity;
    hipStream_t s = (hipStream_t)stream;
    uint32_t* n_surv = (uint32_t*)d->workspace;
    Survivor* list = (Survivor*)((char*)d->workspace + 16);
    if (hipMemsetAsync(n_surv, 0, 16, s) != hipSuccess || hipMemsetAsync(d->count, 0, sizeof(int32_t), s) != hipSuccess) return SKTRACK_E_HIP;
    // 256 CUs x 8 workgroups of four waves at the most; a wave walks the (member, row) pairs, then the survivors, with the grid's stride
    const size_t groups = ((size_t)d->M * Hb + 3) / 4;
    const unsigned blocks = (unsigned)(groups < 2048 ? groups : 2048);
    hipLaunchKernelGGL(track_prefilter_kernel, dim3(blocks), dim3(256), 0, s, a, d->members, n_surv, list);
    if (hipGetLastError() != hipSuccess) return SKTRACK_E_HIP;
    const size_t most = (a.list_cap + 3) / 4;
    const unsigned eblocks = (unsigned)(most < 2048 ? most : 2048);
    if (core)
        hipLaunchKernelGGL(track_eval_kernel<true>, dim3(eblocks), dim3(256), 0, s, a, d->members, d->h_msl, d->h_vort, d->h_wind, d->h_core,
                           d->rowc, n_surv, list, d->records, d->count);
    else
        hipLaunchKernelGGL(track_eval_kernel<false>, dim3(eblocks), dim3(256), 0, s, a, d->members, d->h_msl, d->h_vort, d->h_wind, d->h_wind,
                           d->rowc, n_surv, list, d->records, d->count);
    if (hipGetLastError() != hipSuccess) return SKTRACK_E_HIP;
    return 0;
}
