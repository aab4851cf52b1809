// Column thermodynamics (include/skyrim_thermo.h): one kernel over (member, op, tile) -- the pointwise moisture conversions and
// indices, the 0 C level, and the parcel ascent with its levels unrolled and their virtual temperatures in registers.  Contraction to fma
// is off for the whole file (and on the build line): the header fixes the order of the fp32 operations, and exp and log are those of
// thermo_math.h, not the device library's.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "../../include/skyrim_thermo.h"
#include "fields.h"
#include "program.h"
#include "thermo_math.h"

#pragma clang fp contract(off)

namespace {

constexpr int TILE = 512;        // points of a MOIST / INDEX / FREEZE tile
constexpr int PTILE = 64;        // columns of a PARCEL tile: one per lane
constexpr int ML = SKTHERMO_MAX_LEVELS;
constexpr int NSUB = SKTHERMO_NSUB;

struct OpArgs {
    int kind, moist, source;
    int a, b;                    // MOIST: t, m; INDEX, FREEZE, PARCEL: the first entry in `lev` and L
    int ktop, k500;              // PARCEL
    int out[4];
    uint32_t tile0;              // the op's first tile in a member's list
    float p, p_src_min;          // MOIST: the level; PARCEL: the candidates' lowest pressure
};
struct Level { int t, m, z; float p; };
// the host constants of the ascent over one set of pressure levels (every PARCEL op of a launch has the same)
struct ParcelTab {
    float lq[ML], ex[ML];                    // per level
    float npp[ML - 1][NSUB], nlq[ML - 1][NSUB], nex[ML - 1][NSUB], h[ML - 1];
};
struct ThermoArgs {
    int M, H, W, n_ops;
    uint32_t tiles;              // tiles of one member, all ops
    size_t member_stride;
    OpArgs op[SKTHERMO_MAX_OPS];
    Level lev[SKTHERMO_LEVELS_PER_LAUNCH];
    ParcelTab tab;
};

using namespace skfields;
using namespace skprogram;
using namespace skthermo_math;

constexpr float EPS = 0.622f, ONE_M_EPS = 0.378f, KAPPA = 0.2854f, RD = 287.04f, T0C = 273.15f, E_MIN = 1e-10f;

__host__ __device__ __forceinline__ float ln1000() { return sk_log(1000.f); }
__device__ __forceinline__ float nanf32() { return float_of(0x7fc00000u); }

__device__ __forceinline__ float es_of(float T) { return 6.112f * sk_exp((17.67f * (T - T0C)) / (T - 29.65f)); }
__device__ __forceinline__ float vapour(int moist, float m, float T, float p) {
    const float e = moist == SKTHERMO_Q ? (m * p) / (EPS + ONE_M_EPS * m) : (m / 100.f) * es_of(T);
    return e < E_MIN ? E_MIN : e;
}
__device__ __forceinline__ float mixr(float e, float p) {
    const float h = 0.5f * p;
    e = e > h ? h : e;
    return (EPS * e) / (p - e);
}
__device__ __forceinline__ float tvirt(float T, float w) { return (T * (1.f + w / EPS)) / (1.f + w); }
__device__ __forceinline__ float dewpoint(float e) {
    const float le = sk_log(e / 6.112f);
    return (243.5f * le) / (17.67f - le) + T0C;
}
__device__ __forceinline__ float tlcl(float T, float td) { return 1.f / (1.f / (td - 56.f) + sk_log(T / td) / 800.f) + 56.f; }
__device__ __forceinline__ float thetae(float T, float TL, float lq, float w) {
    const float a = sk_exp((KAPPA * (1.f - 0.28f * w)) * lq);
    const float b = sk_exp(((3.376f / TL - 0.00254f) * (w * 1000.f)) * (1.f + 0.81f * w));
    return (T * a) * b;
}
__device__ __forceinline__ float thetae_sat(float T, float pp, float lq) { return thetae(T, T, lq, mixr(es_of(T), pp)); }

__device__ __forceinline__ bool any_lane(bool c) { return __builtin_amdgcn_ballot_w64(c) != 0; }

// MOIST, INDEX, FREEZE: TILE points of the planes, a lane VEC of them per step
template <int VEC>
__device__ __forceinline__ void pointwise_tile(const ThermoArgs& a, const OpArgs& op, const float* x, const float* zs, float* y,
                                               uint32_t tile, int lane) {
    const uint32_t n = (uint32_t)a.H * (uint32_t)a.W;
#pragma unroll 1
    for (int s = 0; s < TILE / (64 * VEC); ++s) {
        const uint32_t e = tile * TILE + (uint32_t)(s * 64 + lane) * VEC;     // (vector path: n is a multiple of 4, so e < n covers e + 3)
        if (e >= n) continue;
        if (op.kind == SKTHERMO_MOIST) {
            const bool wet = op.out[0] >= 0 || op.out[1] >= 0 || op.out[2] >= 0;
            const float lq = ln1000() - sk_log(op.p);
            const Pts<VEC> t = load<VEC>(x, (uint32_t)op.a * n + e);
            Pts<VEC> th;
            bool bad[VEC];
#pragma unroll
            for (int i = 0; i < VEC; ++i) {
                bad[i] = !finite(t.v[i]);
                th.v[i] = t.v[i] * sk_exp(KAPPA * lq);
            }
            if (wet) {
                const Pts<VEC> m = load<VEC>(x, (uint32_t)op.b * n + e);
                Pts<VEC> td, other, the;
#pragma unroll
                for (int i = 0; i < VEC; ++i) {
                    bad[i] = bad[i] || !finite(m.v[i]);
                    const float ev = vapour(op.moist, m.v[i], t.v[i], op.p);
                    const float d = dewpoint(ev);
                    const float o = op.moist == SKTHERMO_Q ? (100.f * ev) / es_of(t.v[i]) : (EPS * ev) / (op.p - ONE_M_EPS * ev);
                    const float q = thetae(t.v[i], tlcl(t.v[i], d), lq, mixr(ev, op.p));
                    td.v[i] = bad[i] ? nanf32() : d;
                    other.v[i] = bad[i] ? nanf32() : o;
                    the.v[i] = bad[i] ? nanf32() : q;
                }
                if (op.out[0] >= 0) store<VEC>(y, (uint32_t)op.out[0] * n + e, td);
                if (op.out[1] >= 0) store<VEC>(y, (uint32_t)op.out[1] * n + e, other);
                if (op.out[2] >= 0) store<VEC>(y, (uint32_t)op.out[2] * n + e, the);
            }
            if (op.out[3] >= 0) {
#pragma unroll
                for (int i = 0; i < VEC; ++i) th.v[i] = bad[i] ? nanf32() : th.v[i];
                store<VEC>(y, (uint32_t)op.out[3] * n + e, th);
            }
        } else if (op.kind == SKTHERMO_INDEX) {
            const Level l0 = a.lev[op.a], l1 = a.lev[op.a + 1], l2 = a.lev[op.a + 2];
            const Pts<VEC> t850 = load<VEC>(x, (uint32_t)l0.t * n + e), t700 = load<VEC>(x, (uint32_t)l1.t * n + e);
            const Pts<VEC> t500 = load<VEC>(x, (uint32_t)l2.t * n + e);
            const Pts<VEC> m850 = load<VEC>(x, (uint32_t)l0.m * n + e), m700 = load<VEC>(x, (uint32_t)l1.m * n + e);
            Pts<VEC> kx, tt;
#pragma unroll
            for (int i = 0; i < VEC; ++i) {
                const bool bad = !(finite(t850.v[i]) && finite(t700.v[i]) && finite(t500.v[i]) && finite(m850.v[i]) && finite(m700.v[i]));
                const float td850 = dewpoint(vapour(op.moist, m850.v[i], t850.v[i], 850.f));
                const float td700 = dewpoint(vapour(op.moist, m700.v[i], t700.v[i], 700.f));
                const float k = ((t850.v[i] - t500.v[i]) + (td850 - T0C)) - (t700.v[i] - td700);
                const float u = (t850.v[i] - t500.v[i]) + (td850 - t500.v[i]);
                kx.v[i] = bad ? nanf32() : k;
                tt.v[i] = bad ? nanf32() : u;
            }
            if (op.out[0] >= 0) store<VEC>(y, (uint32_t)op.out[0] * n + e, kx);
            if (op.out[1] >= 0) store<VEC>(y, (uint32_t)op.out[1] * n + e, tt);
        } else {                                                               // FREEZE
            Pts<VEC> res, tu, zu, zsv;
            bool bad[VEC], found[VEC], have[VEC];
#pragma unroll
            for (int i = 0; i < VEC; ++i) {
                res.v[i] = tu.v[i] = zu.v[i] = zsv.v[i] = 0.f;
                bad[i] = found[i] = have[i] = false;
            }
            if (zs) {
                zsv = load<VEC>(zs, e);
#pragma unroll
                for (int i = 0; i < VEC; ++i) bad[i] = !finite(zsv.v[i]);
            }
            for (int k = op.b - 1; k >= 0; --k) {
                const Level lv = a.lev[op.a + k];
                const Pts<VEC> t = load<VEC>(x, (uint32_t)lv.t * n + e), z = load<VEC>(x, (uint32_t)lv.z * n + e);
#pragma unroll
                for (int i = 0; i < VEC; ++i) {
                    bad[i] = bad[i] || !finite(t.v[i]) || !finite(z.v[i]);
                    const bool ok = zs ? !(z.v[i] < zsv.v[i]) : true;
                    const float p = t.v[i] - T0C, q = tu.v[i] - T0C;
                    const bool cross = ((p >= 0.f && q <= 0.f) || (p <= 0.f && q >= 0.f)) && p != q;
                    const bool hit = ok && have[i] && !found[i] && cross;
                    const float zc = z.v[i] + (zu.v[i] - z.v[i]) * (p / (p - q));
                    res.v[i] = hit ? zc : res.v[i];
                    found[i] = found[i] || hit;
                    res.v[i] = ok && !found[i] ? z.v[i] : res.v[i];
                    tu.v[i] = ok ? t.v[i] : tu.v[i];
                    zu.v[i] = ok ? z.v[i] : zu.v[i];
                    have[i] = have[i] || ok;
                }
            }
#pragma unroll
            for (int i = 0; i < VEC; ++i) res.v[i] = bad[i] || !have[i] ? nanf32() : res.v[i];
            store<VEC>(y, (uint32_t)op.out[0] * n + e, res);
        }
    }
}

// PARCEL: PTILE columns, one per lane.  Pass 1 reads the levels once, keeps tv_k in registers and picks the source; pass 2 is the ascent
__device__ __forceinline__ void parcel_tile(const ThermoArgs& a, const OpArgs& op, const float* x, const float* zs, float* y, uint32_t tile,
                                            int lane) {
    const uint32_t n = (uint32_t)a.H * (uint32_t)a.W;
    const uint32_t e0 = tile * PTILE + (uint32_t)lane;
    const bool owns = e0 < n;
    const uint32_t e = owns ? e0 : n - 1;                         // (a lane past the end works on the last column and stores nothing)
    const int L = op.b;
    float tv[ML];
    float t500 = 0.f, zsv = 0.f;
    bool bad = false;
    uint32_t masked = 0;
    int src = -1;
    float best = 0.f, T0 = 0.f, es0 = 0.f, w0 = 0.f, lq_s = 0.f, ex_s = 1.f, p_s = 0.f;
    if (zs) {
        zsv = load<1>(zs, e).v[0];
        bad = !finite(zsv);
    }
#pragma unroll
    for (int k = 0; k < ML; ++k) {
        tv[k] = 0.f;
        if (k < L) {
            const Level lv = a.lev[op.a + k];
            const float t = load<1>(x, (uint32_t)lv.t * n + e).v[0], m = load<1>(x, (uint32_t)lv.m * n + e).v[0];
            bad = bad || !finite(t) || !finite(m);
            bool ok = true;
            if (zs) {
                const float z = load<1>(x, (uint32_t)lv.z * n + e).v[0];
                bad = bad || !finite(z);
                ok = !(z < zsv);
                masked |= ok ? 0u : 1u << k;
            }
            const float ev = vapour(op.moist, m, t, lv.p), w = mixr(ev, lv.p);
            tv[k] = tvirt(t, w);
            t500 = k == op.k500 ? t : t500;
            bool take;
            if (op.source == SKTHERMO_SRC_MAX_THETAE && lv.p >= op.p_src_min) {
                const float th = thetae(t, tlcl(t, dewpoint(ev)), a.tab.lq[k], w);
                take = ok && (src < 0 || th > best);
                best = take ? th : best;
            } else {
                take = ok && src < 0;
            }
            src = take ? k : src;
            T0 = take ? t : T0;
            es0 = take ? ev : es0;
            w0 = take ? w : w0;
            lq_s = take ? a.tab.lq[k] : lq_s;
            ex_s = take ? a.tab.ex[k] : ex_s;
            p_s = take ? lv.p : p_s;
        }
    }
    const float TL = tlcl(T0, dewpoint(es0));
    const float the = thetae(T0, TL, lq_s, w0);
    const float th0 = T0 / ex_s;
    const float lq_lcl = lq_s - sk_log(TL / T0) / KAPPA;
    float tot = 0.f, prevB = 0.f, Tprev = T0;
    bool stopped = false;
    float li = op.k500 >= 0 && src == op.k500 ? 0.f : nanf32();
    if (op.out[0] >= 0 || op.out[1] >= 0) {
#pragma unroll
        for (int k = 0; k < ML - 1; ++k) {
            if (k < op.ktop) {
                const bool run = src <= k, up = (masked >> (k + 1)) & 1u;
                const bool act = run && !stopped && !up;
                stopped = stopped || (run && up);
                if (any_lane(act && src >= 0)) {
                    float exprev = a.tab.ex[k];
#pragma unroll 1
                    for (int s = 0; s < NSUB; ++s) {
                        const float pp = a.tab.npp[k][s], lq = a.tab.nlq[k][s], ex = a.tab.nex[k][s];
                        const float tenv = tv[k] + ((float)(s + 1) / (float)NSUB) * (tv[k + 1] - tv[k]);
                        const float Tdry = th0 * ex;
                        const bool sat = lq > lq_lcl;
                        float Ta = Tprev, Tb = (Tprev / exprev) * ex;
                        if (any_lane(sat && act)) {
                            float Fa = thetae_sat(Ta, pp, lq) - the;
#pragma unroll 1
                            for (int it = 0; it < SKTHERMO_NITER; ++it) {
                                const float Fb = thetae_sat(Tb, pp, lq) - the;
                                const float d = Fb - Fa;
                                const float step = d != 0.f ? (Fb * (Tb - Ta)) / (d != 0.f ? d : 1.f) : 0.f;
                                Ta = Tb;
                                Fa = Fb;
                                Tb = Tb - step;
                            }
                        }
                        const float T = sat ? Tb : Tdry;
                        const float wp = sat ? mixr(es_of(T), pp) : w0;
                        float B = tvirt(T, wp) - tenv;
                        B = B > 0.f ? B : 0.f;
                        tot = act ? tot + (0.5f * (B + prevB)) * a.tab.h[k] : tot;
                        prevB = act ? B : prevB;
                        Tprev = act ? T : Tprev;
                        exprev = ex;
                    }
                    if (k + 1 == op.k500) li = act ? t500 - Tprev : li;
                }
            }
        }
    }
    if (!owns) return;
    const bool none = bad || src < 0;
    Pts<1> r;
    if (op.out[0] >= 0) {
        r.v[0] = none ? nanf32() : RD * tot;
        store<1>(y, (uint32_t)op.out[0] * n + e, r);
    }
    if (op.out[1] >= 0) {
        r.v[0] = none ? nanf32() : li;
        store<1>(y, (uint32_t)op.out[1] * n + e, r);
    }
    if (op.out[2] >= 0) {
        r.v[0] = none ? nanf32() : p_s;
        store<1>(y, (uint32_t)op.out[2] * n + e, r);
    }
}

template <int VEC>
__global__ void __launch_bounds__(256) thermo_kernel(const ThermoArgs a, const float* const* __restrict__ members,
                                                     const float* __restrict__ zs, float* __restrict__ out) {
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
        if (op.kind == SKTHERMO_PARCEL)
            parcel_tile(a, op, x, zs, y, mt.t - op.tile0, lane);
        else
            pointwise_tile<VEC>(a, op, x, zs, y, mt.t - op.tile0, lane);
    }
}

int results_of(int kind) { return kind == SKTHERMO_MOIST ? 4 : (kind == SKTHERMO_INDEX ? 2 : (kind == SKTHERMO_FREEZE ? 1 : 3)); }

// every refusal of skthermo_run: nothing here touches the GPU
bool valid(const skthermo_desc* d) {
    if (!d || !d->members || !d->out || ((uintptr_t)d->out & 3) || ((uintptr_t)d->zs & 3)) return false;
    if (!grid_ok(d->M, SKTHERMO_MAX_MEMBERS, d->member_align, d->C, d->H, d->W, d->D, d->member_stride)) return false;
    if (d->n_ops < 1 || d->n_ops > SKTHERMO_MAX_OPS) return false;
    const size_t HW = (size_t)d->H * (size_t)d->W;
    if ((size_t)d->M * (size_t)d->n_ops * (HW / PTILE + 1) > ((size_t)1 << 31)) return false;      // (member, tile) pairs are counted in 32 bits
    Slots<4 * SKTHERMO_MAX_OPS> slots;
    for (int o = 0; o < d->n_ops; ++o) {
        const skthermo_op& op = d->ops[o];
        if (op.kind < SKTHERMO_MOIST || op.kind > SKTHERMO_PARCEL) return false;
        if (op.kind != SKTHERMO_FREEZE && op.moisture != SKTHERMO_Q && op.moisture != SKTHERMO_R) return false;
        if (op.kind == SKTHERMO_MOIST) {
            const bool wet = op.out[0] >= 0 || op.out[1] >= 0 || op.out[2] >= 0;
            if (!channel_ok(op.in_t[0], d->C) || (wet && !channel_ok(op.in_m[0], d->C)) || !pressure_ok(op.p[0])) return false;
        } else if (op.kind == SKTHERMO_INDEX) {
            for (int k = 0; k < 3; ++k)
                if (!channel_ok(op.in_t[k], d->C) || (k < 2 && !channel_ok(op.in_m[k], d->C))) return false;
        } else {
            const bool parcel = op.kind == SKTHERMO_PARCEL;
            if (op.n_levels < 2 || op.n_levels > SKTHERMO_MAX_LEVELS) return false;
            for (int k = 0; k < op.n_levels; ++k) {
                if (!channel_ok(op.in_t[k], d->C)) return false;
                if (parcel && !channel_ok(op.in_m[k], d->C)) return false;
                if ((!parcel || d->zs) && !channel_ok(op.in_z[k], d->C)) return false;
                if (parcel && (!pressure_ok(op.p[k]) || (k > 0 && !(op.p[k] < op.p[k - 1])))) return false;
            }
            if (parcel) {
                if (op.source != SKTHERMO_SRC_LOWEST && op.source != SKTHERMO_SRC_MAX_THETAE) return false;
                if (!pressure_ok(op.p_top) || op.p_top > op.p[0]) return false;
                if (op.source == SKTHERMO_SRC_MAX_THETAE && !pressure_ok(op.p_src_min)) return false;
                if (op.out[1] >= 0) {                              // li: a 500-hPa level that the ascent reaches
                    bool has = false;
                    for (int k = 0; k < op.n_levels; ++k) has = has || op.p[k] == 500.f;
                    if (!has || op.p_top > 500.f) return false;
                }
            }
        }
        bool any = false;
        for (int r = 0; r < results_of(op.kind); ++r) {
            if (!slots.claim(op.out[r], d->D)) return false;
            any = any || op.out[r] >= 0;
        }
        if (!any) return false;
    }
    return true;
}

int levels_of(const skthermo_op& op) {
    return op.kind == SKTHERMO_MOIST ? 0 : (op.kind == SKTHERMO_INDEX ? 3 : op.n_levels);
}

void fill_tab(ParcelTab& tab, const skthermo_op& op) {
    const float LN1000 = ln1000();
    float lnp[ML];
    for (int k = 0; k < op.n_levels; ++k) {
        lnp[k] = sk_log(op.p[k]);
        tab.lq[k] = LN1000 - lnp[k];
        tab.ex[k] = sk_exp(KAPPA * (lnp[k] - LN1000));
    }
    for (int k = 0; k + 1 < op.n_levels; ++k) {
        tab.h[k] = (lnp[k] - lnp[k + 1]) / (float)NSUB;
        for (int s = 1; s <= NSUB; ++s) {
            const float lp = lnp[k] + ((float)s / (float)NSUB) * (lnp[k + 1] - lnp[k]);
            tab.npp[k][s - 1] = sk_exp(lp);
            tab.nlq[k][s - 1] = LN1000 - lp;
            tab.nex[k][s - 1] = sk_exp(KAPPA * (lp - LN1000));
        }
    }
}

bool same_levels(const skthermo_op& p, const skthermo_op& q) {
    if (p.n_levels != q.n_levels) return false;
    for (int k = 0; k < p.n_levels; ++k)
        if (p.p[k] != q.p[k]) return false;
    return true;
}

}  // namespace

extern "C" int skthermo_abi_version(void) { return SKTHERMO_ABI_VERSION; }

extern "C" int skthermo_run(const skthermo_desc* d, void* stream) {
    if (!valid(d)) return SKTHERMO_E_ARG;
    hipStream_t s = (hipStream_t)stream;
    const uint32_t HW = (uint32_t)d->H * (uint32_t)d->W;
    const bool vec = vec_ok(d->member_align, HW % 4 == 0, d->member_stride, d->out, d->zs);
    static_assert(sizeof(ThermoArgs) <= 4096, "the launch arguments fit the kernel-argument segment");
    ThermoArgs a = {};
    a.M = d->M; a.H = d->H; a.W = d->W;
    a.member_stride = d->member_stride;
    // whole ops per launch, as many as the level pool and the one table of ascent constants allow (in practice: all of them)
    for (int first = 0; first < d->n_ops;) {
        int n = 0, levels = 0;
        uint32_t tiles = 0;
        const skthermo_op* parcel = nullptr;
        for (; first + n < d->n_ops; ++n) {
            const skthermo_op& op = d->ops[first + n];
            if (levels + levels_of(op) > SKTHERMO_LEVELS_PER_LAUNCH) break;
            if (op.kind == SKTHERMO_PARCEL && parcel && !same_levels(*parcel, op)) break;
            OpArgs& k = a.op[n];
            k = OpArgs{};
            k.kind = op.kind; k.moist = op.moisture; k.source = op.source;
            k.tile0 = tiles;
            k.k500 = -1;
            for (int r = 0; r < 4; ++r) k.out[r] = r < results_of(op.kind) ? op.out[r] : -1;
            if (op.kind == SKTHERMO_MOIST) {
                k.a = op.in_t[0]; k.b = op.in_m[0]; k.p = op.p[0];
            } else {
                k.a = levels; k.b = levels_of(op);
                for (int l = 0; l < k.b; ++l) a.lev[levels++] = Level{op.in_t[l], op.in_m[l], op.in_z[l], op.p[l]};
            }
            if (op.kind == SKTHERMO_PARCEL) {
                if (!parcel) {
                    parcel = &op;
                    fill_tab(a.tab, op);
                }
                k.p_src_min = op.p_src_min;
                for (int l = 0; l < op.n_levels; ++l) {
                    if (op.p[l] >= op.p_top) k.ktop = l;
                    if (op.p[l] == 500.f) k.k500 = l;
                }
                tiles += (HW + PTILE - 1) / PTILE;
            } else {
                tiles += (HW + TILE - 1) / TILE;
            }
        }
        a.n_ops = n;
        a.tiles = tiles;
        const unsigned blocks = blocks_for(d->M, tiles);
        if (vec)
            hipLaunchKernelGGL(thermo_kernel<4>, dim3(blocks), dim3(256), 0, s, a, d->members, d->zs, d->out);
        else
            hipLaunchKernelGGL(thermo_kernel<1>, dim3(blocks), dim3(256), 0, s, a, d->members, d->zs, d->out);
        if (hipGetLastError() != hipSuccess) return SKTHERMO_E_HIP;
        first += n;
    }
    return 0;
}
