// Vertical interpolation (include/skyrim_vert.h): one kernel over (member, op, tile).  A tile's columns scan the op's coordinate planes
// once, top down, and keep per target the layer of the first crossing and its fraction; the fields are then read at the two levels of
// that layer only, the plane a lane reads chosen by compare-and-select over the wave-uniform level loop.  Contraction to fma is off for
// the whole file (and on the build line): the header fixes the order of the fp32 operations, and exp and log are those of thermo_math.h.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "../../include/skyrim_vert.h"
#include "fields.h"
#include "program.h"
#include "thermo_math.h"

#pragma clang fp contract(off)

namespace {

constexpr int TILE = 512;                    // points of a tile
constexpr int ML = SKVERT_MAX_LEVELS, MT = SKVERT_MAX_TARGETS;
constexpr int POOL_FIELDS = 16, POOL_CHAN = 448, POOL_LEVELS = 48;      // what one launch's argument block holds, all ops together

struct FieldArgs {
    int kind, a0, b0;                        // the first entries of in_a and in_b in `chan`
    int node_a, node_b;
    float gh;
    int out[MT];
};
struct OpArgs {
    int coord, L, T, F, outside, mask;
    int c0, z0;                              // the first entries of in_c and in_z in `chan`
    int lev0, field0;                        // the first entries in `lnp` / `ex` and in `field`
    int two_pass;                            // more than one result: the non-finite test spans them and runs first
    uint32_t tile0;                          // the op's first tile in a member's list
    float target[MT];
};
struct VertArgs {
    int M, H, W, n_ops;
    uint32_t tiles;                          // tiles of one member, all ops
    size_t member_stride;
    OpArgs op[SKVERT_MAX_OPS];
    FieldArgs field[POOL_FIELDS];
    int chan[POOL_CHAN];
    float lnp[POOL_LEVELS], ex[POOL_LEVELS];
};

using namespace skfields;
using namespace skprogram;
using namespace skthermo_math;

constexpr float KAPPA = 0.2854f;

// the packed search state of a (column, target): kl | ku << 8 | (nearest level + 1) << 16 | found << 24
constexpr int NEAR_MASK = 0x00ff0000, FOUND = 0x01000000;
// where a result comes from
constexpr int NONE = 0, LAYER = 1, NODE_LAYER = 2, LEVEL = 3, NODE = 4;

__device__ __forceinline__ float nanf32() { return float_of(0x7fc00000u); }
__device__ __forceinline__ float speed(float u, float v) {
    const float uu = u * u, vv = v * v;
    return sqrtf(uu + vv);
}
__device__ __forceinline__ bool crosses(float p, float q) { return ((p >= 0.f && q <= 0.f) || (p <= 0.f && q >= 0.f)) && p != q; }

// what the search leaves behind for the columns of a lane
template <int VEC> struct Found {
    float frac[VEC][MT], bestd[VEC][MT];
    int lev[VEC][MT];
    float cu[VEC], zsv[VEC];                 // the coordinate of the lowest unmasked level, the surface
    int klast[VEC];                          // that level
    bool have[VEC], bad[VEC];
};

// the fields of one op at the columns of a lane.  STORE = false: only the non-finite test of what the results read
template <int VEC, bool STORE>
__device__ __forceinline__ void field_pass(const VertArgs& a, const OpArgs& op, const float* x, float* y, uint32_t n, uint32_t e, Found<VEC>& s) {
    const bool agl = op.coord == SKVERT_Z_AGL;
#pragma unroll 1
    for (int f = 0; f < op.F; ++f) {
        const FieldArgs& fa = a.field[op.field0 + f];
        bool wanted = false;
#pragma unroll
        for (int t = 0; t < MT; ++t) wanted = wanted || (t < op.T && fa.out[t] >= 0);
        if (!wanted) continue;
        const bool node = fa.node_a != SKVERT_NODE_NONE;
        Pts<VEC> na, nb;
#pragma unroll
        for (int i = 0; i < VEC; ++i) na.v[i] = nb.v[i] = 0.f;
        if (node) {
            if (fa.node_a >= 0) na = load<VEC>(x, (uint32_t)fa.node_a * n + e);
            if (fa.kind == SKVERT_SPEED && fa.node_b >= 0) nb = load<VEC>(x, (uint32_t)fa.node_b * n + e);
#pragma unroll
            for (int i = 0; i < VEC; ++i) {
                na.v[i] = fa.node_a == SKVERT_NODE_ZS ? s.zsv[i] : na.v[i];
                nb.v[i] = fa.node_b == SKVERT_NODE_ZS ? s.zsv[i] : nb.v[i];
                s.bad[i] = s.bad[i] || !finite(na.v[i]) || !finite(nb.v[i]);
            }
        }
#pragma unroll
        for (int t = 0; t < MT; ++t) {
            if (t >= op.T || fa.out[t] < 0) continue;
            int kL[VEC], kU[VEC], mode[VEC];
            float fr[VEC];
            bool lbad[VEC];
#pragma unroll
            for (int i = 0; i < VEC; ++i) {
                const int lv = s.lev[i][t];
                const bool found = (lv & FOUND) != 0;
                mode[i] = found ? LAYER : NONE;
                kL[i] = lv & 0xff;
                kU[i] = (lv >> 8) & 0xff;
                fr[i] = s.frac[i][t];
                lbad[i] = false;
                const float tau = agl ? s.zsv[i] + op.target[t] : op.target[t];
                const float p = (s.zsv[i] + fa.gh) - tau, q = s.cu[i] - tau;
                const bool free = node && !found && s.have[i];
                if (free && crosses(p, q)) {
                    mode[i] = NODE_LAYER;
                    fr[i] = p / (p - q);
                    kU[i] = s.klast[i];
                }
                if (mode[i] == NONE && op.outside == SKVERT_NEAREST && s.have[i]) {
                    const float d = p < 0.f ? -p : p;
                    mode[i] = node && d <= s.bestd[i][t] ? NODE : LEVEL;
                    kL[i] = ((lv & NEAR_MASK) >> 16) - 1;
                }
            }
            float res[VEC];
            if (fa.kind == SKVERT_PRESSURE) {
                float lL[VEC], lU[VEC];
#pragma unroll
                for (int i = 0; i < VEC; ++i) lL[i] = lU[i] = 0.f;
#pragma unroll 1
                for (int k = 0; k < op.L; ++k) {
                    const float lk = a.lnp[op.lev0 + k];
#pragma unroll
                    for (int i = 0; i < VEC; ++i) {
                        lL[i] = kL[i] == k ? lk : lL[i];
                        lU[i] = kU[i] == k ? lk : lU[i];
                    }
                }
#pragma unroll
                for (int i = 0; i < VEC; ++i) res[i] = mode[i] == LAYER ? sk_exp(lL[i] + (lU[i] - lL[i]) * fr[i]) : sk_exp(lL[i]);
            } else {
                float val[2][VEC];
#pragma unroll
                for (int c = 0; c < 2; ++c) {
                    if (c == 1 && fa.kind != SKVERT_SPEED) continue;
                    const int base = c ? fa.b0 : fa.a0;
                    uint32_t oL[VEC], oU[VEC];
                    float xL[VEC], xU[VEC];
#pragma unroll
                    for (int i = 0; i < VEC; ++i) {
                        oL[i] = oU[i] = (uint32_t)a.chan[base] * n;
                        xL[i] = xU[i] = 1.f;
                    }
#pragma unroll 1
                    for (int k = 0; k < op.L; ++k) {
                        const uint32_t ch = (uint32_t)a.chan[base + k] * n;
                        const float exk = a.ex[op.lev0 + k];
#pragma unroll
                        for (int i = 0; i < VEC; ++i) {
                            oL[i] = kL[i] == k ? ch : oL[i];
                            oU[i] = kU[i] == k ? ch : oU[i];
                            xL[i] = kL[i] == k ? exk : xL[i];
                            xU[i] = kU[i] == k ? exk : xU[i];
                        }
                    }
#pragma unroll
                    for (int i = 0; i < VEC; ++i) {
                        float vl = load<1>(x, oL[i] + e + (uint32_t)i).v[0], vu = load<1>(x, oU[i] + e + (uint32_t)i).v[0];
                        const bool layer = mode[i] == LAYER || mode[i] == NODE_LAYER;
                        const bool from_node = mode[i] == NODE_LAYER || mode[i] == NODE;
                        lbad[i] = lbad[i] || ((mode[i] == LAYER || mode[i] == LEVEL) && !finite(vl)) || (layer && !finite(vu));
                        if (fa.kind == SKVERT_THETA_F) {
                            vl = vl * xL[i];
                            vu = vu * xU[i];
                        }
                        const float lower = from_node ? (c ? nb.v[i] : na.v[i]) : vl;
                        val[c][i] = layer ? lower + (vu - lower) * fr[i] : lower;
                    }
                }
#pragma unroll
                for (int i = 0; i < VEC; ++i) res[i] = fa.kind == SKVERT_SPEED ? speed(val[0][i], val[1][i]) : val[0][i];
            }
            if constexpr (STORE) {
                Pts<VEC> r;
#pragma unroll
                for (int i = 0; i < VEC; ++i) r.v[i] = s.bad[i] || lbad[i] || mode[i] == NONE ? nanf32() : res[i];
                store<VEC>(y, (uint32_t)fa.out[t] * n + e, r);
            } else {
#pragma unroll
                for (int i = 0; i < VEC; ++i) s.bad[i] = s.bad[i] || lbad[i];
            }
        }
    }
}

template <int VEC>
__device__ __forceinline__ void vert_tile(const VertArgs& a, const OpArgs& op, const float* x, const float* zs, float* y, uint32_t tile,
                                          int lane) {
    const uint32_t n = (uint32_t)a.H * (uint32_t)a.W;
    const bool agl = op.coord == SKVERT_Z_AGL;
    const bool own_z = op.coord == SKVERT_Z || agl;                               // the coordinate planes are the z planes
    const bool masked = zs != nullptr && (op.coord != SKVERT_P || op.mask != 0);
    const bool z_planes = masked && !own_z;
#pragma unroll 1
    for (int st = 0; st < TILE / (64 * VEC); ++st) {
        const uint32_t e = tile * TILE + (uint32_t)(st * 64 + lane) * VEC;        // (vector path: n is a multiple of 4, so e < n covers e + 3)
        if (e >= n) continue;
        Found<VEC> s;
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
            s.cu[i] = s.zsv[i] = 0.f;
            s.klast[i] = 0;
            s.have[i] = s.bad[i] = false;
#pragma unroll
            for (int t = 0; t < MT; ++t) {
                s.frac[i][t] = s.bestd[i][t] = 0.f;
                s.lev[i][t] = 0;
            }
        }
        if (masked || agl) {
            const Pts<VEC> v = load<VEC>(zs, e);
#pragma unroll
            for (int i = 0; i < VEC; ++i) {
                s.zsv[i] = v.v[i];
                s.bad[i] = !finite(v.v[i]);
            }
        }
#pragma unroll 1
        for (int k = op.L - 1; k >= 0; --k) {
            Pts<VEC> c, z;
            if (op.coord == SKVERT_P) {
#pragma unroll
                for (int i = 0; i < VEC; ++i) c.v[i] = a.lnp[op.lev0 + k];
            } else {
                c = load<VEC>(x, (uint32_t)a.chan[op.c0 + k] * n + e);
                const float exk = op.coord == SKVERT_THETA ? a.ex[op.lev0 + k] : 1.f;
#pragma unroll
                for (int i = 0; i < VEC; ++i) {
                    s.bad[i] = s.bad[i] || !finite(c.v[i]);
                    c.v[i] = op.coord == SKVERT_THETA ? c.v[i] * exk : c.v[i];
                }
            }
            z = c;
            if (z_planes) {
                z = load<VEC>(x, (uint32_t)a.chan[op.z0 + k] * n + e);
#pragma unroll
                for (int i = 0; i < VEC; ++i) s.bad[i] = s.bad[i] || !finite(z.v[i]);
            }
#pragma unroll
            for (int i = 0; i < VEC; ++i) {
                const bool ok = masked ? !(z.v[i] < s.zsv[i]) : true;
                const int hit_lev = FOUND | k | (s.klast[i] << 8);
#pragma unroll
                for (int t = 0; t < MT; ++t) {
                    if (t >= op.T) continue;
                    const float tau = agl ? s.zsv[i] + op.target[t] : op.target[t];
                    const float p = c.v[i] - tau, q = s.cu[i] - tau;
                    int lv = s.lev[i][t];
                    const bool hit = ok && s.have[i] && !(lv & FOUND) && crosses(p, q);
                    s.frac[i][t] = hit ? p / (p - q) : s.frac[i][t];
                    lv = hit ? (lv & NEAR_MASK) | hit_lev : lv;
                    const float d = p < 0.f ? -p : p;
                    const bool near = ok && (!(lv & NEAR_MASK) || d <= s.bestd[i][t]);
                    s.bestd[i][t] = near ? d : s.bestd[i][t];
                    s.lev[i][t] = near ? (lv & ~NEAR_MASK) | ((k + 1) << 16) : lv;
                }
                s.cu[i] = ok ? c.v[i] : s.cu[i];
                s.klast[i] = ok ? k : s.klast[i];
                s.have[i] = s.have[i] || ok;
            }
        }
        if (op.two_pass) field_pass<VEC, false>(a, op, x, y, n, e, s);
        field_pass<VEC, true>(a, op, x, y, n, e, s);
    }
}

template <int VEC>
__global__ void __launch_bounds__(256) vert_kernel(const VertArgs a, const float* const* __restrict__ members, const float* __restrict__ zs,
                                                   float* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const uint32_t total = (uint32_t)a.M * a.tiles, nw = gridDim.x * 4u;
    for (uint32_t w = blockIdx.x * 4u + (threadIdx.x >> 6); w < total; w += nw) {
        const MemberTile mt = member_tile(w, a.tiles);
        int o = 0;
        for (int k = 1; k < a.n_ops; ++k) o += mt.t >= a.op[k].tile0 ? 1 : 0;
        o = uniform(o);
        const OpArgs& op = a.op[o];
        vert_tile<VEC>(a, op, members[mt.m], zs, out + (size_t)mt.m * a.member_stride, mt.t - op.tile0, lane);
    }
}

// every refusal of skvert_run: nothing here touches the GPU
bool valid(const skvert_desc* d) {
    if (!d || !d->members || !d->out || ((uintptr_t)d->out & 3) || ((uintptr_t)d->zs & 3)) return false;
    if (!grid_ok(d->M, SKVERT_MAX_MEMBERS, d->member_align, d->C, d->H, d->W, d->D, d->member_stride)) return false;
    if (d->n_ops < 1 || d->n_ops > SKVERT_MAX_OPS) return false;
    const size_t HW = (size_t)d->H * (size_t)d->W;
    if ((size_t)d->M * (size_t)d->n_ops * (HW / TILE + 1) > ((size_t)1 << 31)) return false;        // (member, tile) pairs are counted in 32 bits
    Slots<SKVERT_MAX_OPS * SKVERT_MAX_FIELDS * SKVERT_MAX_TARGETS> slots;
    for (int o = 0; o < d->n_ops; ++o) {
        const skvert_op& op = d->ops[o];
        if (op.coord < SKVERT_P || op.coord > SKVERT_T) return false;
        if (op.n_levels < 2 || op.n_levels > SKVERT_MAX_LEVELS) return false;
        if (op.n_targets < 1 || op.n_targets > SKVERT_MAX_TARGETS || op.n_fields < 1 || op.n_fields > SKVERT_MAX_FIELDS) return false;
        if (op.outside != SKVERT_NAN && op.outside != SKVERT_NEAREST) return false;
        const bool p_kind = op.coord == SKVERT_P, agl = op.coord == SKVERT_Z_AGL;
        if (p_kind && op.mask != 0 && op.mask != 1) return false;
        if ((agl || (p_kind && op.mask == 1)) && !d->zs) return false;
        const bool z_planes = p_kind ? op.mask == 1 : (d->zs && (op.coord == SKVERT_THETA || op.coord == SKVERT_T));
        for (int k = 0; k < op.n_levels; ++k) {
            if (!pressure_ok(op.p[k]) || (k > 0 && !(op.p[k] < op.p[k - 1]))) return false;
            if (!p_kind && !channel_ok(op.in_c[k], d->C)) return false;
            if (z_planes && !channel_ok(op.in_z[k], d->C)) return false;
        }
        for (int t = 0; t < op.n_targets; ++t)
            if (!finite(op.target[t])) return false;
        bool any = false;
        for (int f = 0; f < op.n_fields; ++f) {
            const skvert_field& fd = op.fields[f];
            if (fd.kind < SKVERT_PLAIN || fd.kind > SKVERT_PRESSURE) return false;
            const bool speed_kind = fd.kind == SKVERT_SPEED;
            for (int k = 0; k < op.n_levels; ++k) {
                if (fd.kind != SKVERT_PRESSURE && !channel_ok(fd.in_a[k], d->C)) return false;
                if (speed_kind && !channel_ok(fd.in_b[k], d->C)) return false;
            }
            const bool may_node = agl && (fd.kind == SKVERT_PLAIN || speed_kind);
            if (fd.node_a != SKVERT_NODE_NONE) {
                if (!may_node || !(fd.node_a == SKVERT_NODE_ZS || channel_ok(fd.node_a, d->C))) return false;
                if (speed_kind && !(fd.node_b == SKVERT_NODE_ZS || channel_ok(fd.node_b, d->C))) return false;
                if (!finite(fd.gh) || fd.gh < 0.f) return false;
            }
            if ((!speed_kind || fd.node_a == SKVERT_NODE_NONE) && fd.node_b != SKVERT_NODE_NONE) return false;
            for (int t = 0; t < op.n_targets; ++t) {
                if (!slots.claim(fd.out[t], d->D)) return false;
                any = any || fd.out[t] >= 0;
            }
        }
        if (!any) return false;
    }
    return true;
}

// the entries of `chan` an op takes
int chans_of(const skvert_op& op, bool z_planes) {
    int n = (op.coord == SKVERT_P ? 0 : op.n_levels) + (z_planes ? op.n_levels : 0);
    for (int f = 0; f < op.n_fields; ++f)
        n += op.fields[f].kind == SKVERT_PRESSURE ? 0 : (op.fields[f].kind == SKVERT_SPEED ? 2 : 1) * op.n_levels;
    return n;
}

}  // namespace

extern "C" int skvert_abi_version(void) { return SKVERT_ABI_VERSION; }

extern "C" int skvert_run(const skvert_desc* d, void* stream) {
    if (!valid(d)) return SKVERT_E_ARG;
    hipStream_t s = (hipStream_t)stream;
    const uint32_t HW = (uint32_t)d->H * (uint32_t)d->W;
    const bool vec = vec_ok(d->member_align, HW % 4 == 0, d->member_stride, d->out, d->zs);
    static_assert(sizeof(VertArgs) <= 4096, "the launch arguments fit the kernel-argument segment");
    static_assert(POOL_FIELDS >= SKVERT_MAX_FIELDS && POOL_LEVELS >= ML && POOL_CHAN >= (2 + 2 * SKVERT_MAX_FIELDS) * ML, "one op always fits a launch");
    const float LN1000 = sk_log(1000.f);
    VertArgs a = {};
    a.M = d->M; a.H = d->H; a.W = d->W;
    a.member_stride = d->member_stride;
    // whole ops per launch, as many as the pools of the argument block hold
    for (int first = 0; first < d->n_ops;) {
        int n = 0, fields = 0, chans = 0, levels = 0;
        uint32_t tiles = 0;
        for (; first + n < d->n_ops; ++n) {
            const skvert_op& op = d->ops[first + n];
            const bool z_planes = op.coord == SKVERT_P ? op.mask == 1 : (d->zs && (op.coord == SKVERT_THETA || op.coord == SKVERT_T));
            if (fields + op.n_fields > POOL_FIELDS || chans + chans_of(op, z_planes) > POOL_CHAN || levels + op.n_levels > POOL_LEVELS) break;
            OpArgs& k = a.op[n];
            k = OpArgs{};
            k.coord = op.coord; k.L = op.n_levels; k.T = op.n_targets; k.F = op.n_fields; k.outside = op.outside;
            k.mask = op.coord == SKVERT_P ? op.mask : 0;
            k.tile0 = tiles;
            k.lev0 = levels; k.field0 = fields;
            for (int l = 0; l < op.n_levels; ++l) {
                const float lnp = sk_log(op.p[l]);
                a.lnp[levels] = lnp;
                a.ex[levels++] = sk_exp(KAPPA * (LN1000 - lnp));
            }
            for (int t = 0; t < op.n_targets; ++t) k.target[t] = op.target[t];
            k.c0 = chans;
            if (op.coord != SKVERT_P)
                for (int l = 0; l < op.n_levels; ++l) a.chan[chans++] = op.in_c[l];
            k.z0 = chans;
            if (z_planes)
                for (int l = 0; l < op.n_levels; ++l) a.chan[chans++] = op.in_z[l];
            int results = 0;
            for (int f = 0; f < op.n_fields; ++f) {
                const skvert_field& fd = op.fields[f];
                FieldArgs& g = a.field[fields++];
                g = FieldArgs{};
                g.kind = fd.kind; g.node_a = fd.node_a; g.node_b = fd.kind == SKVERT_SPEED ? fd.node_b : SKVERT_NODE_NONE; g.gh = fd.gh;
                for (int t = 0; t < MT; ++t) {
                    g.out[t] = t < op.n_targets ? fd.out[t] : -1;
                    results += g.out[t] >= 0 ? 1 : 0;
                }
                g.a0 = g.b0 = chans;
                if (fd.kind != SKVERT_PRESSURE)
                    for (int l = 0; l < op.n_levels; ++l) a.chan[chans++] = fd.in_a[l];
                if (fd.kind == SKVERT_SPEED) {
                    g.b0 = chans;
                    for (int l = 0; l < op.n_levels; ++l) a.chan[chans++] = fd.in_b[l];
                }
            }
            k.two_pass = results > 1 ? 1 : 0;
            tiles += (HW + TILE - 1) / TILE;
        }
        a.n_ops = n;
        a.tiles = tiles;
        const unsigned blocks = blocks_for(d->M, tiles);
        if (vec)
            hipLaunchKernelGGL(vert_kernel<4>, dim3(blocks), dim3(256), 0, s, a, d->members, d->zs, d->out);
        else
            hipLaunchKernelGGL(vert_kernel<1>, dim3(blocks), dim3(256), 0, s, a, d->members, d->zs, d->out);
        if (hipGetLastError() != hipSuccess) return SKVERT_E_HIP;
        first += n;
    }
    return 0;
}
