// Time-window aggregates (include/skyrim_agg.h): one streaming kernel over (member, group of ops that read one channel, tile) folds a
// lead time into the accumulator -- the input plane is read once per group, each slot is read (without FIRST) and written once.
// Contraction to fma is off for the whole file (and on the build line): the header fixes the order of the fp32 operations.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "../../include/skyrim_agg.h"
#include "fields.h"
#include "program.h"

#pragma clang fp contract(off)

namespace {

constexpr int TILE = 512;        // points of a tile

struct OpArgs {
    int kind, out, when, phase;
    float thr, scale;
};
struct GroupArgs {
    int in;                      // the input channel the group's ops share
    int first, count;            // its ops in `op`
};
struct AggArgs {
    int M, n_groups;
    uint32_t n;                  // H W
    uint32_t tiles_per_group;
    uint32_t tiles;              // tiles of one member, all groups
    float stamp;
    size_t member_stride;
    GroupArgs grp[SKAGG_MAX_OPS];
    OpArgs op[SKAGG_MAX_OPS];    // sorted by group
};

using namespace skfields;
using namespace skprogram;

// one op on the VEC points `x` of a lane; `e` is the lane's first point in a plane
template <int VEC>
__device__ __forceinline__ void fold(const AggArgs& a, const OpArgs& op, const Pts<VEC>& x, float* y, uint32_t e) {
    const bool first = (op.phase & SKAGG_FIRST) != 0, last = (op.phase & SKAGG_LAST) != 0;
    const uint32_t at = (uint32_t)op.out * a.n + e;
    Pts<VEC> old, r;
#pragma unroll
    for (int i = 0; i < VEC; ++i) old.v[i] = 0.f;
    if (!first) old = load<VEC>(y, at);
    if (op.kind == SKAGG_MAX || op.kind == SKAGG_MIN) {
        const bool stamped = op.when >= 0;
        const uint32_t wat = (uint32_t)(stamped ? op.when : 0) * a.n + e;
        Pts<VEC> w;
#pragma unroll
        for (int i = 0; i < VEC; ++i) w.v[i] = 0.f;
        if (stamped && !first) w = load<VEC>(y, wat);
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
            const float v = x.v[i];
            const bool nan = v != v;
            const bool beats = op.kind == SKAGG_MAX ? v > old.v[i] : v < old.v[i];
            const bool take = first || beats || nan;
            r.v[i] = take ? v : old.v[i];
            w.v[i] = take ? (nan ? v : a.stamp) : w.v[i];
        }
        store<VEC>(y, at, r);
        if (stamped) store<VEC>(y, wat, w);
    } else {
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
            const float v = x.v[i];
            const float b = op.kind == SKAGG_SUM ? v : ((v != v) ? v : (v > op.thr ? 1.0f : 0.0f));
            float s = first ? b : old.v[i] + b;
            if (last) s = s * op.scale;
            r.v[i] = s;
        }
        store<VEC>(y, at, r);
    }
}

template <int VEC>
__global__ void __launch_bounds__(256) agg_kernel(const AggArgs a, const float* const* __restrict__ members, float* acc) {
    const int lane = threadIdx.x & 63;
    const uint32_t total = (uint32_t)a.M * a.tiles, nw = gridDim.x * 4u;
    for (uint32_t w = blockIdx.x * 4u + (threadIdx.x >> 6); w < total; w += nw) {
        const MemberTile mt = member_tile(w, a.tiles);
        const int g = uniform((int)(mt.t / a.tiles_per_group));
        const uint32_t tile = mt.t - (uint32_t)g * a.tiles_per_group;
        const GroupArgs& G = a.grp[g];
        const float* x = members[mt.m];
        float* y = acc + (size_t)mt.m * a.member_stride;
#pragma unroll 1
        for (int s = 0; s < TILE / (64 * VEC); ++s) {
            const uint32_t e = tile * TILE + (uint32_t)(s * 64 + lane) * VEC;      // (vector path: n is a multiple of 4, so e < n covers e + 3)
            if (e >= a.n) continue;
            const Pts<VEC> p = load<VEC>(x, (uint32_t)G.in * a.n + e);              // the group's one read of the input plane
            for (int k = 0; k < G.count; ++k) fold<VEC>(a, a.op[G.first + k], p, y, e);
        }
    }
}

// every refusal of skagg_update: nothing here touches the GPU
bool valid(const skagg_desc* d) {
    if (!d || !d->members || ((uintptr_t)d->members & 7) || !d->acc || ((uintptr_t)d->acc & 3)) return false;
    if (!grid_ok(d->M, SKAGG_MAX_MEMBERS, d->member_align, d->C, d->H, d->W, d->D, d->member_stride)) return false;
    if (d->n_ops < 1 || d->n_ops > SKAGG_MAX_OPS) return false;
    Slots<2 * SKAGG_MAX_OPS> slots;
    for (int o = 0; o < d->n_ops; ++o) {
        const skagg_op& op = d->ops[o];
        if (op.kind < SKAGG_MAX || op.kind > SKAGG_COUNT_ABOVE) return false;
        if (op.phase < 0 || op.phase > (SKAGG_FIRST | SKAGG_LAST)) return false;
        if (op.in < 0 || op.in >= d->C || op.out < 0 || op.out >= d->D || op.when < -1 || op.when >= d->D) return false;
        if (op.when >= 0 && op.kind != SKAGG_MAX && op.kind != SKAGG_MIN) return false;
        if (!slots.claim(op.out, d->D) || !slots.claim(op.when, d->D)) return false;
    }
    return true;
}

}  // namespace

extern "C" int skagg_abi_version(void) { return SKAGG_ABI_VERSION; }

extern "C" int skagg_update(const skagg_desc* d, void* stream) {
    if (!valid(d)) return SKAGG_E_ARG;
    hipStream_t s = (hipStream_t)stream;
    const uint32_t HW = (uint32_t)d->H * (uint32_t)d->W;
    const bool vec = vec_ok(d->member_align, HW % 4 == 0, d->member_stride, d->acc);
    AggArgs a = {};
    a.M = d->M;
    a.n = HW;
    a.stamp = d->stamp;
    a.member_stride = d->member_stride;
    // the ops sorted into groups that read one channel, in the order the channels first appear
    int n = 0;
    for (int o = 0; o < d->n_ops; ++o) {
        bool seen = false;
        for (int p = 0; p < o; ++p) seen = seen || d->ops[p].in == d->ops[o].in;
        if (seen) continue;
        GroupArgs& G = a.grp[a.n_groups++];
        G.in = d->ops[o].in;
        G.first = n;
        for (int p = o; p < d->n_ops; ++p) {
            const skagg_op& op = d->ops[p];
            if (op.in != G.in) continue;
            const bool extreme = op.kind == SKAGG_MAX || op.kind == SKAGG_MIN;
            a.op[n++] = OpArgs{op.kind, op.out, extreme ? op.when : -1, op.phase, op.thr, op.scale};
        }
        G.count = n - G.first;
    }
    a.tiles_per_group = (HW + TILE - 1) / TILE;
    a.tiles = a.tiles_per_group * (uint32_t)a.n_groups;
    const unsigned blocks = blocks_for(d->M, a.tiles);
    if (vec)
        hipLaunchKernelGGL(agg_kernel<4>, dim3(blocks), dim3(256), 0, s, a, d->members, d->acc);
    else
        hipLaunchKernelGGL(agg_kernel<1>, dim3(blocks), dim3(256), 0, s, a, d->members, d->acc);
    if (hipGetLastError() != hipSuccess) return SKAGG_E_HIP;
    return 0;
}
