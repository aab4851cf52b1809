// Derived fields (include/skyrim_derive.h): one streaming kernel over (member, op, tile) -- wind speed, differences, column integrals,
// vorticity and divergence, each input plane read once -- and one wave per pole row for the polar-cap values.  Contraction to fma is off
// for the whole file (and on the build line): the header fixes the order of the fp32 operations.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "../../include/skyrim_derive.h"
#include "fields.h"
#include "program.h"

#pragma clang fp contract(off)

namespace {

constexpr int TILE = 512;        // points of a SPEED / DIFF / COLUMN tile
constexpr int BAND = 8;          // rows of a VORTDIV tile
constexpr int OWN = 62;          // lanes of a VORTDIV tile that own columns; lanes 0 and 63 hold the halo

struct OpArgs {
    int kind;
    int a, b;                    // SPEED, DIFF, VORTDIV: the two input channels; COLUMN: the first entry in `lev` and L
    int out[4];
    uint32_t tile0;              // the op's first tile in a member's list
};
struct Level { int q, u, v; float w; };
struct DeriveArgs {
    int M, H, W, n_ops;
    int edge_first, edge_last;
    uint32_t tiles;              // tiles of one member, all ops
    uint32_t strips;             // column strips of a VORTDIV tile row
    size_t member_stride;
    OpArgs op[SKDERIVE_MAX_OPS];
    Level lev[SKDERIVE_LEVELS_PER_LAUNCH];
};

using namespace skfields;
using namespace skprogram;

__device__ __forceinline__ float speed(float u, float v) {
    const float uu = u * u, vv = v * v;
    return sqrtf(uu + vv);
}

// SPEED, DIFF, COLUMN: TILE points of the planes, a lane VEC of them per step
template <int VEC>
__device__ __forceinline__ void pointwise_tile(const DeriveArgs& a, const OpArgs& op, const float* x, float* y, uint32_t tile, int lane) {
    const uint32_t n = (uint32_t)a.H * (uint32_t)a.W;
#pragma unroll 1
    for (int s = 0; s < TILE / (64 * VEC); ++s) {
        const uint32_t e = tile * TILE + (uint32_t)(s * 64 + lane) * VEC;     // (vector path: n is a multiple of 4, so e < n covers e + 3)
        if (e >= n) continue;
        if (op.kind == SKDERIVE_COLUMN) {
            const bool wind = op.out[0] >= 0 || op.out[1] >= 0 || op.out[2] >= 0;
            Pts<VEC> sw, su, sv;
#pragma unroll
            for (int i = 0; i < VEC; ++i) sw.v[i] = su.v[i] = sv.v[i] = 0.f;
            for (int k = 0; k < op.b; ++k) {
                const Level lv = a.lev[op.a + k];
                const Pts<VEC> q = load<VEC>(x, (uint32_t)lv.q * n + e);
                if (wind) {
                    const Pts<VEC> u = load<VEC>(x, (uint32_t)lv.u * n + e), v = load<VEC>(x, (uint32_t)lv.v * n + e);
#pragma unroll
                    for (int i = 0; i < VEC; ++i) {
                        const float t = lv.w * q.v[i], tu = t * u.v[i], tv = t * v.v[i];
                        sw.v[i] = k ? sw.v[i] + t : t;
                        su.v[i] = k ? su.v[i] + tu : tu;
                        sv.v[i] = k ? sv.v[i] + tv : tv;
                    }
                } else {
#pragma unroll
                    for (int i = 0; i < VEC; ++i) {
                        const float t = lv.w * q.v[i];
                        sw.v[i] = k ? sw.v[i] + t : t;
                    }
                }
            }
            if (op.out[0] >= 0) store<VEC>(y, (uint32_t)op.out[0] * n + e, su);
            if (op.out[1] >= 0) store<VEC>(y, (uint32_t)op.out[1] * n + e, sv);
            if (op.out[2] >= 0) {
                Pts<VEC> r;
#pragma unroll
                for (int i = 0; i < VEC; ++i) r.v[i] = speed(su.v[i], sv.v[i]);
                store<VEC>(y, (uint32_t)op.out[2] * n + e, r);
            }
            if (op.out[3] >= 0) store<VEC>(y, (uint32_t)op.out[3] * n + e, sw);
        } else {
            const Pts<VEC> p = load<VEC>(x, (uint32_t)op.a * n + e), q = load<VEC>(x, (uint32_t)op.b * n + e);
            Pts<VEC> r;
#pragma unroll
            for (int i = 0; i < VEC; ++i) r.v[i] = op.kind == SKDERIVE_SPEED ? speed(p.v[i], q.v[i]) : p.v[i] - q.v[i];
            store<VEC>(y, (uint32_t)op.out[0] * n + e, r);
        }
    }
}

// VORTDIV: BAND rows by OWN lanes of VEC columns; the rows slide through registers, east and west come from the neighbouring lanes
template <int VEC>
__device__ __forceinline__ void vortdiv_tile(const DeriveArgs& a, const OpArgs& op, const float* x, float* y, const float* __restrict__ rowc,
                                             uint32_t tile, int lane) {
    const int H = a.H, W = a.W;
    const int band = (int)(tile / a.strips), strip = (int)(tile - (uint32_t)band * a.strips);
    const int chunks = W / VEC;                                   // (vector path: W is a multiple of 4)
    const int c = strip * OWN + lane - 1;                         // -1 .. chunks + 61
    const bool owns = lane >= 1 && lane <= OWN && c < chunks;
    const uint32_t col = (uint32_t)(c < 0 ? chunks - 1 : (c >= chunks ? 0 : c)) * VEC;        // (c == chunks is column 0; beyond it the lane owns nothing)
    const uint32_t Hu = (uint32_t)H, Wu = (uint32_t)W;
    const uint32_t ub = (uint32_t)op.a * Hu, vb = (uint32_t)op.b * Hu;
    const int j0 = band * BAND, j1 = j0 + BAND < H ? j0 + BAND : H;
    const int js = j0 > 0 ? j0 - 1 : 0;
    Pts<VEC> us = load<VEC>(x, (ub + (uint32_t)js) * Wu + col), vs = load<VEC>(x, (vb + (uint32_t)js) * Wu + col);
    Pts<VEC> uc = load<VEC>(x, (ub + (uint32_t)j0) * Wu + col), vc = load<VEC>(x, (vb + (uint32_t)j0) * Wu + col);
    const int lw = lane > 0 ? lane - 1 : 0, le = lane < 63 ? lane + 1 : 63;
    for (int j = j0; j < j1; ++j) {
        const int jn = j + 1 < H ? j + 1 : H - 1;
        const Pts<VEC> un = load<VEC>(x, (ub + (uint32_t)jn) * Wu + col), vn = load<VEC>(x, (vb + (uint32_t)jn) * Wu + col);
        const float4 rc = *(const float4*)(rowc + 4 * j);
        const float uw0 = __shfl(uc.v[VEC - 1], lw), vw0 = __shfl(vc.v[VEC - 1], lw);
        const float ue0 = __shfl(uc.v[0], le), ve0 = __shfl(vc.v[0], le);
        const bool pole = (j == 0 && a.edge_first == SKDERIVE_EDGE_POLE) || (j == H - 1 && a.edge_last == SKDERIVE_EDGE_POLE);
        if (!pole) {                                              // (the pole rows are the second kernel's)
            Pts<VEC> vo, dv;
#pragma unroll
            for (int i = 0; i < VEC; ++i) {
                const float uw = i > 0 ? uc.v[i > 0 ? i - 1 : 0] : uw0, vw = i > 0 ? vc.v[i > 0 ? i - 1 : 0] : vw0;
                const float ue = i < VEC - 1 ? uc.v[i < VEC - 1 ? i + 1 : 0] : ue0, ve = i < VEC - 1 ? vc.v[i < VEC - 1 ? i + 1 : 0] : ve0;
                const float t1 = rc.x * (ve - vw), t2 = rc.y * un.v[i], t3 = rc.z * us.v[i];
                vo.v[i] = t1 - (t2 - t3);
                const float d1 = rc.x * (ue - uw), d2 = rc.y * vn.v[i], d3 = rc.z * vs.v[i];
                dv.v[i] = d1 + (d2 - d3);
            }
            if (owns) {
                if (op.out[0] >= 0) store<VEC>(y, ((uint32_t)op.out[0] * Hu + (uint32_t)j) * Wu + col, vo);
                if (op.out[1] >= 0) store<VEC>(y, ((uint32_t)op.out[1] * Hu + (uint32_t)j) * Wu + col, dv);
            }
        }
        us = uc; vs = vc; uc = un; vc = vn;
    }
}

template <int VEC>
__global__ void __launch_bounds__(256) derive_kernel(const DeriveArgs a, const float* const* __restrict__ members,
                                                     const float* __restrict__ rowc, float* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const uint32_t total = (uint32_t)a.M * a.tiles, nw = gridDim.x * 4u;
    for (uint32_t w = blockIdx.x * 4u + (threadIdx.x >> 6); w < total; w += nw) {
        const MemberTile mt = member_tile(w, a.tiles);
        int o = 0;
        for (int k = 1; k < a.n_ops; ++k) o += mt.t >= a.op[k].tile0 ? 1 : 0;
        o = uniform(o);
        const OpArgs& op = a.op[o];
        const float* x = members[mt.m];
        float* y = out + (size_t)mt.m * a.member_stride;
        if (op.kind == SKDERIVE_VORTDIV)
            vortdiv_tile<VEC>(a, op, x, y, rowc, mt.t - op.tile0, lane);
        else
            pointwise_tile<VEC>(a, op, x, y, mt.t - op.tile0, lane);
    }
}

// the pole rows of VORTDIV: one wave per (member, op, edge); float64 means of the neighbouring row in a fixed order
__global__ void __launch_bounds__(64) derive_pole_kernel(const DeriveArgs a, const float* const* __restrict__ members,
                                                         const float* __restrict__ rowc, float* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int edge = uniform((int)(blockIdx.x & 1u)), o = uniform((int)((blockIdx.x >> 1) % (uint32_t)a.n_ops));
    const int m = uniform((int)((blockIdx.x >> 1) / (uint32_t)a.n_ops));
    const OpArgs& op = a.op[o];
    if (op.kind != SKDERIVE_VORTDIV || (edge ? a.edge_last : a.edge_first) != SKDERIVE_EDGE_POLE) return;
    const uint32_t H = (uint32_t)a.H, W = (uint32_t)a.W;
    const uint32_t j = edge ? H - 1 : 0, r = edge ? H - 2 : 1;
    const float* x = members[m];
    float* y = out + (size_t)m * a.member_stride;
    double su = 0.0, sv = 0.0;
    for (uint32_t i = lane; i < W; i += 64) {
        su += (double)load<1>(x, ((uint32_t)op.a * H + r) * W + i).v[0];
        sv += (double)load<1>(x, ((uint32_t)op.b * H + r) * W + i).v[0];
    }
    su = wave_sum(su) / (double)W;
    sv = wave_sum(sv) / (double)W;
    Pts<1> vo, dv;
    vo.v[0] = (float)((double)rowc[4 * j] * su);
    dv.v[0] = (float)((double)rowc[4 * j + 1] * sv);
    for (uint32_t i = lane; i < W; i += 64) {
        if (op.out[0] >= 0) store<1>(y, ((uint32_t)op.out[0] * H + j) * W + i, vo);
        if (op.out[1] >= 0) store<1>(y, ((uint32_t)op.out[1] * H + j) * W + i, dv);
    }
}

int results_of(int kind) { return kind == SKDERIVE_COLUMN ? 4 : (kind == SKDERIVE_VORTDIV ? 2 : 1); }

// every refusal of skderive_run: nothing here touches the GPU
bool valid(const skderive_desc* d) {
    if (!d || !d->members || !d->out || ((uintptr_t)d->out & 3)) return false;
    if (!grid_ok(d->M, SKDERIVE_MAX_MEMBERS, d->member_align, d->C, d->H, d->W, d->D, d->member_stride, 3, 4)) return false;
    if (d->n_ops < 1 || d->n_ops > SKDERIVE_MAX_OPS) return false;
    Slots<4 * SKDERIVE_MAX_OPS> slots;
    bool vortdiv = false;
    for (int o = 0; o < d->n_ops; ++o) {
        const skderive_op& op = d->ops[o];
        if (op.kind < SKDERIVE_SPEED || op.kind > SKDERIVE_VORTDIV) return false;
        if (op.kind == SKDERIVE_COLUMN) {
            if (op.n_levels < 2 || op.n_levels > SKDERIVE_MAX_LEVELS) return false;
            for (int k = 0; k < op.n_levels; ++k)
                if (!channel_ok(op.in_a[k], d->C) || !channel_ok(op.in_b[k], d->C) || !channel_ok(op.in_c[k], d->C)) return false;
        } else if (!channel_ok(op.in_a[0], d->C) || !channel_ok(op.in_b[0], d->C)) {
            return false;
        }
        vortdiv = vortdiv || op.kind == SKDERIVE_VORTDIV;
        bool any = false;
        for (int r = 0; r < results_of(op.kind); ++r) {
            if (!slots.claim(op.out[r], d->D)) return false;
            any = any || op.out[r] >= 0;
        }
        if (!any) return false;
    }
    if (vortdiv) {
        if (!d->rowc || ((uintptr_t)d->rowc & 15)) return false;
        for (int e : {d->edge_first, d->edge_last})
            if (e != SKDERIVE_EDGE_ONESIDED && e != SKDERIVE_EDGE_POLE) return false;
    }
    return true;
}

}  // namespace

extern "C" int skderive_abi_version(void) { return SKDERIVE_ABI_VERSION; }

extern "C" int skderive_run(const skderive_desc* d, void* stream) {
    if (!valid(d)) return SKDERIVE_E_ARG;
    hipStream_t s = (hipStream_t)stream;
    const bool vec = vec_ok(d->member_align, d->W % 4 == 0, d->member_stride, d->out);
    const uint32_t HW = (uint32_t)d->H * (uint32_t)d->W;
    const uint32_t chunks = (uint32_t)d->W / (vec ? 4u : 1u);
    DeriveArgs a = {};
    a.M = d->M; a.H = d->H; a.W = d->W;
    a.edge_first = d->edge_first; a.edge_last = d->edge_last;
    a.strips = (chunks + OWN - 1) / OWN;
    a.member_stride = d->member_stride;
    bool poles = false;
    // whole ops per launch, as many as their column levels allow (in practice: all of them)
    for (int first = 0; first < d->n_ops;) {
        int n = 0, levels = 0;
        uint32_t tiles = 0;
        for (; first + n < d->n_ops; ++n) {
            const skderive_op& op = d->ops[first + n];
            OpArgs& k = a.op[n];
            k.kind = op.kind;
            k.tile0 = tiles;
            for (int r = 0; r < 4; ++r) k.out[r] = r < results_of(op.kind) ? op.out[r] : -1;
            if (op.kind == SKDERIVE_COLUMN) {
                if (levels + op.n_levels > SKDERIVE_LEVELS_PER_LAUNCH) break;
                k.a = levels; k.b = op.n_levels;
                for (int l = 0; l < op.n_levels; ++l) a.lev[levels++] = Level{op.in_a[l], op.in_b[l], op.in_c[l], op.weight[l]};
            } else {
                k.a = op.in_a[0]; k.b = op.in_b[0];
            }
            if (op.kind == SKDERIVE_VORTDIV) {
                tiles += a.strips * (uint32_t)((d->H + BAND - 1) / BAND);
                poles = poles || d->edge_first == SKDERIVE_EDGE_POLE || d->edge_last == SKDERIVE_EDGE_POLE;
            } else {
                tiles += (HW + TILE - 1) / TILE;
            }
        }
        a.n_ops = n;
        a.tiles = tiles;
        const unsigned blocks = blocks_for(d->M, tiles);
        if (vec)
            hipLaunchKernelGGL(derive_kernel<4>, dim3(blocks), dim3(256), 0, s, a, d->members, d->rowc, d->out);
        else
            hipLaunchKernelGGL(derive_kernel<1>, dim3(blocks), dim3(256), 0, s, a, d->members, d->rowc, d->out);
        if (hipGetLastError() != hipSuccess) return SKDERIVE_E_HIP;
        if (poles) {
            hipLaunchKernelGGL(derive_pole_kernel, dim3((unsigned)(2 * n * d->M)), dim3(64), 0, s, a, d->members, d->rowc, d->out);
            if (hipGetLastError() != hipSuccess) return SKDERIVE_E_HIP;
            poles = false;
        }
        first += n;
    }
    return 0;
}
