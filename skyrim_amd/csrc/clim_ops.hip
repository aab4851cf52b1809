// Climate-relative extremes (include/skyrim_clim.h): two kernels.  extremes_kernel: a lane owns one point (or four) of one listed field,
// holds the M member values in registers and streams the Q climate planes past them, one unrolled compare-and-add pass per plane.
// quantiles_kernel: a workgroup sorts the N samples of a tile of points in LDS and writes the Q planes of the climate.  Contraction to
// fma is off for the whole file (and on the build line): the header fixes every rounding; the two fmaf of the SOT quantile are its own.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include "../../include/skyrim_clim.h"
#include "fields.h"

#pragma clang fp contract(off)

namespace {

using namespace skfields;

constexpr int LANES = 256;
constexpr int LDS_FLOATS = 32768;        // 128 KiB of columns per workgroup
constexpr int SORT_LANES = 1024;         // of the workgroup that sorts them: one workgroup per CU, so all 16 waves a workgroup may hold
constexpr int MAX_TILE = 256;            // points of a tile at most

__device__ __forceinline__ float quiet_nan() { return __uint_as_float(0x7FC00000u); }
__device__ __forceinline__ bool not_finite(float v) { return !(fabsf(v) < __builtin_inff()); }

// ---- members against a climate ---------------------------------------------------------------------------------------------------------- //
struct ExArgs {
    const float* const* members;
    const float* clim;
    float *efi, *sot, *prob;
    int M, Q, nf, n_sot, n_prob;
    uint32_t HW, items;
    uint32_t plane[SKCLIM_MAX_FIELDS];       // first element of the f-th listed channel's plane
    float p[SKCLIM_MAX_LEVELS], A[SKCLIM_MAX_LEVELS], B[SKCLIM_MAX_LEVELS], rdp[SKCLIM_MAX_LEVELS];
    float floor[SKCLIM_MAX_FIELDS];
    int sq_lo[SKCLIM_MAX_SOT], sq_hi[SKCLIM_MAX_SOT], s_ref[SKCLIM_MAX_SOT], s_base[SKCLIM_MAX_SOT];
    float sq_frac[SKCLIM_MAX_SOT];
    int pk[SKCLIM_MAX_PROB], pbelow[SKCLIM_MAX_PROB];
};

// MB: the member-count bucket (M <= MB; every loop over members is unrolled over MB with the slot a compile-time constant, so the values
// stay in registers); V: points per lane; SORT: a SOT is asked for.  Every index into the tables of `a` is wave-uniform (scalar loads)
template <int MB, int V, bool SORT>
__global__ void __launch_bounds__(LANES) extremes_kernel(const ExArgs a) {
    const uint32_t item = blockIdx.x * LANES + threadIdx.x;
    if (item >= a.items) return;                                            // (no barrier below)
    const int f = blockIdx.y, M = a.M, Q = a.Q;
    const uint32_t j = item * V, HW = a.HW;
    const float fM = (float)M, inf = __builtin_inff();
    float x[MB][V];
    bool bad[V];
#pragma unroll
    for (int e = 0; e < V; ++e) bad[e] = false;
    const uint32_t at = 4u * (a.plane[f] + j);
#pragma unroll
    for (int m = 0; m < MB; ++m) {
        if (m < M) {
            load_to<V>(a.members[m], at, x[m]);
#pragma unroll
            for (int e = 0; e < V; ++e) {
                x[m][e] = x[m][e] + 0.0f;                                   // -0 is +0
                bad[e] = bad[e] || not_finite(x[m][e]);
            }
        } else {
#pragma unroll
            for (int e = 0; e < V; ++e) x[m][e] = inf;                      // an empty slot: never <= or < a finite level, last in the order
        }
    }
    const float* cl = a.clim + (size_t)f * (size_t)Q * HW;
    const bool counting = a.efi != nullptr || a.n_prob > 0;
    const float flo = a.floor[f];
    float cur[V], nxt[V], Fprev[V], num[V], den[V], pr[SKCLIM_MAX_PROB][V], cref[SKCLIM_MAX_SOT][V], cbase[SKCLIM_MAX_SOT][V];
    bool act[V];
#pragma unroll
    for (int e = 0; e < V; ++e) {
        Fprev[e] = 0.f; num[e] = 0.f; den[e] = 0.f; act[e] = false;
#pragma unroll
        for (int t = 0; t < SKCLIM_MAX_PROB; ++t) pr[t][e] = 0.f;
#pragma unroll
        for (int s = 0; s < SKCLIM_MAX_SOT; ++s) { cref[s][e] = 0.f; cbase[s][e] = 0.f; }
    }
    load_to<V>(cl, 4u * j, cur);
    for (int i = 0; i < Q; ++i) {
        const int in = i + 1 < Q ? i + 1 : i;
        load_to<V>(cl + (size_t)in * HW, 4u * j, nxt);                      // the next plane's load is in flight while this one is counted
        int cnt[V];
#pragma unroll
        for (int e = 0; e < V; ++e) {
            cur[e] = cur[e] + 0.0f;
            bad[e] = bad[e] || not_finite(cur[e]);
            cnt[e] = 0;
        }
        if (counting) {
#pragma unroll
            for (int m = 0; m < MB; ++m) {
#pragma unroll
                for (int e = 0; e < V; ++e) cnt[e] += x[m][e] <= cur[e] ? 1 : 0;
            }
#pragma unroll
            for (int e = 0; e < V; ++e) {
                const float F = (float)cnt[e] / fM;
                if (i > 0) {                                                // interval i - 1
                    const float b = (F - Fprev[e]) * a.rdp[i - 1];
                    const float a0 = Fprev[e] - b * a.p[i - 1];
                    const float t = (a.B[i - 1] - a0 * a.A[i - 1]) - b * a.B[i - 1];
                    const bool on = cur[e] > flo;
                    num[e] = on ? num[e] + t : num[e];
                    den[e] = on ? den[e] + a.B[i - 1] : den[e];
                    act[e] = act[e] || on;
                }
                Fprev[e] = F;
            }
#pragma unroll
            for (int t = 0; t < SKCLIM_MAX_PROB; ++t) {
                if (t < a.n_prob && a.pk[t] == i) {
                    if (a.pbelow[t]) {
#pragma unroll
                        for (int e = 0; e < V; ++e) {
                            int n = 0;
#pragma unroll
                            for (int m = 0; m < MB; ++m) n += x[m][e] < cur[e] ? 1 : 0;
                            pr[t][e] = (float)n / fM;
                        }
                    } else {
#pragma unroll
                        for (int e = 0; e < V; ++e) pr[t][e] = (float)(M - cnt[e]) / fM;      // finite values: x > c is not (x <= c)
                    }
                }
            }
        }
        if (SORT) {
#pragma unroll
            for (int s = 0; s < SKCLIM_MAX_SOT; ++s) {
                if (s < a.n_sot) {
                    const bool r = a.s_ref[s] == i, b = a.s_base[s] == i;
#pragma unroll
                    for (int e = 0; e < V; ++e) {
                        cref[s][e] = r ? cur[e] : cref[s][e];
                        cbase[s][e] = b ? cur[e] : cbase[s][e];
                    }
                }
            }
        }
#pragma unroll
        for (int e = 0; e < V; ++e) cur[e] = nxt[e];
    }
    const float qnan = quiet_nan();
    Pts<V> o;
    if (a.efi) {
#pragma unroll
        for (int e = 0; e < V; ++e) {
            const float r = fminf(fmaxf(num[e] / den[e], -1.f), 1.f);
            o.v[e] = bad[e] ? qnan : (act[e] ? r : 0.f);
        }
        store<V>(a.efi + (size_t)f * HW, j, o);
    }
#pragma unroll
    for (int t = 0; t < SKCLIM_MAX_PROB; ++t) {
        if (t < a.n_prob) {
#pragma unroll
            for (int e = 0; e < V; ++e) o.v[e] = bad[e] ? qnan : pr[t][e];
            store<V>(a.prob + ((size_t)t * a.nf + f) * HW, j, o);
        }
    }
    if (SORT) {
        // ascending order in place: the bitonic network of ens_ops.hip over MB slots, every index a compile-time constant
#pragma unroll
        for (int k = 2; k <= MB; k <<= 1) {
#pragma unroll
            for (int s = k >> 1; s > 0; s >>= 1) {
#pragma unroll
                for (int p = 0; p < MB; ++p) {
                    const int q = p ^ s;
                    if (q > p) {
                        const bool up = (p & k) == 0;
#pragma unroll
                        for (int e = 0; e < V; ++e) {
                            const float lo = fminf(x[p][e], x[q][e]), hi = fmaxf(x[p][e], x[q][e]);
                            x[p][e] = up ? lo : hi;
                            x[q][e] = up ? hi : lo;
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int s = 0; s < SKCLIM_MAX_SOT; ++s) {
            if (s < a.n_sot) {
#pragma unroll
                for (int e = 0; e < V; ++e) {
                    float lo = x[0][e], hi = x[0][e];
#pragma unroll
                    for (int m = 1; m < MB; ++m) {
                        lo = m == a.sq_lo[s] ? x[m][e] : lo;
                        hi = m == a.sq_hi[s] ? x[m][e] : hi;
                    }
                    // skens_stats' quantile: the difference carried exactly (two-sum), then the header's two fused operations
                    const float nl = -lo, d = hi + nl, bb = d - hi, err = (hi - (d - bb)) + (nl - bb);
                    const float qf = fmaf(a.sq_frac[s], err, fmaf(a.sq_frac[s], d, lo));
                    const float dn = cref[s][e] - cbase[s][e];
                    const float r = (qf - cref[s][e]) / dn;
                    o.v[e] = (bad[e] || cref[s][e] == cbase[s][e]) ? qnan : r;
                }
                store<V>(a.sot + ((size_t)s * a.nf + f) * HW, j, o);
            }
        }
    }
}

template <int MB, int V>
void launch_extremes(const ExArgs& a, hipStream_t s) {
    const dim3 grid((a.items + LANES - 1) / LANES, (unsigned)a.nf);
    if (a.n_sot > 0)
        hipLaunchKernelGGL((extremes_kernel<MB, V, true>), grid, dim3(LANES), 0, s, a);
    else
        hipLaunchKernelGGL((extremes_kernel<MB, V, false>), grid, dim3(LANES), 0, s, a);
}

bool channels_ok(const int32_t* ch, int nf, int C) {
    if (nf < 1 || nf > SKCLIM_MAX_FIELDS) return false;
    for (int k = 0; k < nf; ++k)
        if (ch[k] < 0 || ch[k] >= C) return false;
    return true;
}

// C H W <= 2^30 and nf Q H W <= 2^30
bool sizes_ok(int C, int H, int W, int nf, int Q) {
    if (C < 1 || H < 1 || W < 1) return false;
    const size_t lim = (size_t)1 << 30, HW = (size_t)H * (size_t)W;
    return HW <= lim && (size_t)C <= lim / HW && (size_t)nf * (size_t)Q <= lim / HW;
}

// every refusal of skclim_extremes: nothing here touches the GPU
bool valid(const skclim_extremes_desc* d) {
    if (!d || !d->members || ((uintptr_t)d->members & 7) || !d->clim || ((uintptr_t)d->clim & 3)) return false;
    if (d->M < 1 || d->M > SKCLIM_MAX_MEMBERS || (d->member_align != 4 && d->member_align != 16)) return false;
    if (d->Q < 2 || d->Q > SKCLIM_MAX_LEVELS || !channels_ok(d->channels, d->nf, d->C) || !sizes_ok(d->C, d->H, d->W, d->nf, d->Q)) return false;
    if (d->n_sot < 0 || d->n_sot > SKCLIM_MAX_SOT || d->n_prob < 0 || d->n_prob > SKCLIM_MAX_PROB) return false;
    if ((d->n_sot > 0) != (d->sot != nullptr) || (d->n_prob > 0) != (d->prob != nullptr)) return false;
    if (!d->efi && !d->sot && !d->prob) return false;
    if (((uintptr_t)d->efi | (uintptr_t)d->sot | (uintptr_t)d->prob) & 3) return false;
    for (int i = 0; i < d->Q; ++i) {
        if (!(d->p[i] >= 0.f && d->p[i] <= 1.f) || (i > 0 && !(d->p[i] > d->p[i - 1]))) return false;
        if (i + 1 < d->Q) {
            const float t[3] = {d->A[i], d->B[i], d->rdp[i]};
            for (float v : t)
                if (!(v > 0.f) || !std::isfinite(v)) return false;
        }
    }
    for (int k = 0; k < d->nf; ++k)
        if (std::isnan(d->floor[k])) return false;
    for (int s = 0; s < d->n_sot; ++s) {
        const skclim_sot& r = d->sot_req[s];
        if (r.q_index < 0 || r.q_index >= d->M || !(r.q_frac >= 0.f && r.q_frac < 1.f)) return false;
        if (r.k_ref < 0 || r.k_ref >= d->Q || r.k_base < 0 || r.k_base >= d->Q) return false;
    }
    for (int t = 0; t < d->n_prob; ++t)
        if (d->prob_req[t].k < 0 || d->prob_req[t].k >= d->Q) return false;
    return true;
}

// ---- a climate from samples ------------------------------------------------------------------------------------------------------------- //
struct QArgs {
    const float* const* samples;
    float* clim;
    int N, NP, logT, Q;
    uint32_t HW;
    uint32_t plane[SKCLIM_MAX_FIELDS];
    int q_lo[SKCLIM_MAX_LEVELS], q_hi[SKCLIM_MAX_LEVELS];
    float q_frac[SKCLIM_MAX_LEVELS];
};

// one workgroup of SORT_LANES lanes = T = 2^logT consecutive points of one listed field; col[n * T + t] is sample n of point t (NP T <= LDS_FLOATS)
__global__ void __launch_bounds__(SORT_LANES) quantiles_kernel(const QArgs a) {
    __shared__ float col[LDS_FLOATS];
    __shared__ int poisoned[MAX_TILE];
    const uint32_t tid = threadIdx.x, logT = (uint32_t)a.logT, T = 1u << logT, f = blockIdx.y;
    const uint32_t p0 = blockIdx.x << logT, HW = a.HW, N = (uint32_t)a.N, NP = (uint32_t)a.NP;
    const float inf = __builtin_inff();
    if (tid < MAX_TILE) poisoned[tid] = 0;
    __syncthreads();
    const uint32_t total = NP << logT;
    for (uint32_t e = tid; e < total; e += SORT_LANES) {
        const uint32_t n = e >> logT, t = e & (T - 1);
        float v = inf;                                                      // beyond N: last in the order
        if (n < N) {
            v = 0.f;                                                        // a point beyond the grid: sorted, never written
            if (p0 + t < HW) {
                v = load_vec<1>(a.samples[n], a.plane[f] + p0 + t) + 0.0f;  // -0 is +0
                if (not_finite(v)) poisoned[t] = 1;                         // (every writer stores the same value)
            }
        }
        col[e] = v;
    }
    __syncthreads();
    // the bitonic network over NP, for all T columns at once: pair `pi` of a stage and point t per lane, t fastest
    const uint32_t half = total >> 1;
    for (uint32_t k = 2; k <= NP; k <<= 1) {
        for (uint32_t s = k >> 1; s > 0; s >>= 1) {
            for (uint32_t e = tid; e < half; e += SORT_LANES) {
                const uint32_t pi = e >> logT, t = e & (T - 1);
                const uint32_t lo_n = ((pi & ~(s - 1)) << 1) | (pi & (s - 1)), hi_n = lo_n | s;       // a zero bit put in at s
                const bool up = (lo_n & k) == 0;
                const uint32_t il = (lo_n << logT) + t, ih = (hi_n << logT) + t;
                const float u = col[il], w = col[ih];
                const float lo = fminf(u, w), hi = fmaxf(u, w);
                col[il] = up ? lo : hi;
                col[ih] = up ? hi : lo;
            }
            __syncthreads();
        }
    }
    // the Q planes, spread over the waves: a unit is (level i, run of 64 points), so the level is wave-uniform (scalar loads of its table)
    // and a tile of 16 points still keeps all 16 waves storing
    const uint32_t lane = tid & 63u, wave = (uint32_t)uniform((int)(tid >> 6));
    const uint32_t logC = logT > 6 ? logT - 6 : 0, units = (uint32_t)a.Q << logC;
    float* out = a.clim + (size_t)f * (size_t)a.Q * HW;
    for (uint32_t u = wave; u < units; u += SORT_LANES / 64) {
        const uint32_t i = u >> logC, t = ((u & ((1u << logC) - 1)) << 6) + lane;
        if (t < T && p0 + t < HW) {
            const float lo = col[((uint32_t)a.q_lo[i] << logT) + t], hi = col[((uint32_t)a.q_hi[i] << logT) + t];
            const float r = fminf(lo + a.q_frac[i] * (hi - lo), hi);
            store_vec<1>(out + (size_t)i * HW, p0 + t, poisoned[t] != 0 ? quiet_nan() : r);
        }
    }
}

int pow2_at_least(int n) {
    int p = 1;
    while (p < n) p <<= 1;
    return p;
}

int log_tile(int N) {
    const int t = LDS_FLOATS / pow2_at_least(N);
    int l = 0;
    while ((2 << l) <= (t < MAX_TILE ? t : MAX_TILE)) ++l;
    return l;
}

bool valid(const skclim_quantiles_desc* d) {
    if (!d || !d->samples || ((uintptr_t)d->samples & 7) || !d->clim || ((uintptr_t)d->clim & 3)) return false;
    if (d->N < 1 || d->N > SKCLIM_MAX_SAMPLES || d->Q < 1 || d->Q > SKCLIM_MAX_LEVELS) return false;
    if (!channels_ok(d->channels, d->nf, d->C) || !sizes_ok(d->C, d->H, d->W, d->nf, d->Q)) return false;
    for (int i = 0; i < d->Q; ++i)
        if (d->q_index[i] < 0 || d->q_index[i] >= d->N || !(d->q_frac[i] >= 0.f && d->q_frac[i] < 1.f)) return false;
    return true;
}

}  // namespace

extern "C" int skclim_abi_version(void) { return SKCLIM_ABI_VERSION; }

extern "C" int skclim_tile_points(int N) { return N < 1 || N > SKCLIM_MAX_SAMPLES ? 0 : 1 << log_tile(N); }

extern "C" int skclim_extremes_check(const skclim_extremes_desc* d) { return valid(d) ? 0 : SKCLIM_E_ARG; }

extern "C" int skclim_quantiles_check(const skclim_quantiles_desc* d) { return valid(d) ? 0 : SKCLIM_E_ARG; }

extern "C" int skclim_extremes(const skclim_extremes_desc* d, void* stream) {
    if (!valid(d)) return SKCLIM_E_ARG;
    ExArgs a = {};
    a.members = d->members; a.clim = d->clim; a.efi = d->efi; a.sot = d->sot; a.prob = d->prob;
    a.M = d->M; a.Q = d->Q; a.nf = d->nf; a.n_sot = d->n_sot; a.n_prob = d->n_prob;
    a.HW = (uint32_t)d->H * (uint32_t)d->W;
    for (int k = 0; k < d->nf; ++k) {
        a.plane[k] = (uint32_t)d->channels[k] * a.HW;
        a.floor[k] = d->floor[k];
    }
    for (int i = 0; i < d->Q; ++i) {
        a.p[i] = d->p[i];
        if (i + 1 < d->Q) { a.A[i] = d->A[i]; a.B[i] = d->B[i]; a.rdp[i] = d->rdp[i]; }
    }
    for (int s = 0; s < d->n_sot; ++s) {
        const skclim_sot& r = d->sot_req[s];
        a.sq_lo[s] = r.q_index;
        a.sq_hi[s] = r.q_index + 1 < d->M ? r.q_index + 1 : d->M - 1;
        a.sq_frac[s] = r.q_frac; a.s_ref[s] = r.k_ref; a.s_base[s] = r.k_base;
    }
    for (int t = 0; t < d->n_prob; ++t) { a.pk[t] = d->prob_req[t].k; a.pbelow[t] = d->prob_req[t].below != 0; }
    const uintptr_t ptrs = (uintptr_t)d->clim | (uintptr_t)d->efi | (uintptr_t)d->sot | (uintptr_t)d->prob;
    const bool vec = d->member_align == 16 && a.HW % 4 == 0 && (ptrs & 15) == 0 && d->M <= 16;
    a.items = vec ? a.HW / 4 : a.HW;
    hipStream_t s = (hipStream_t)stream;
    if (d->M <= 8) { if (vec) launch_extremes<8, 4>(a, s); else launch_extremes<8, 1>(a, s); }
    else if (d->M <= 16) { if (vec) launch_extremes<16, 4>(a, s); else launch_extremes<16, 1>(a, s); }
    else if (d->M <= 32) launch_extremes<32, 1>(a, s);
    else launch_extremes<64, 1>(a, s);
    return hipGetLastError() == hipSuccess ? 0 : SKCLIM_E_HIP;
}

extern "C" int skclim_quantiles(const skclim_quantiles_desc* d, void* stream) {
    if (!valid(d)) return SKCLIM_E_ARG;
    QArgs a = {};
    a.samples = d->samples; a.clim = d->clim; a.N = d->N; a.NP = pow2_at_least(d->N); a.logT = log_tile(d->N); a.Q = d->Q;
    a.HW = (uint32_t)d->H * (uint32_t)d->W;
    for (int k = 0; k < d->nf; ++k) a.plane[k] = (uint32_t)d->channels[k] * a.HW;
    for (int i = 0; i < d->Q; ++i) {
        a.q_lo[i] = d->q_index[i];
        a.q_hi[i] = d->q_index[i] + 1 < d->N ? d->q_index[i] + 1 : d->N - 1;
        a.q_frac[i] = d->q_frac[i];
    }
    const uint32_t T = 1u << a.logT;
    const dim3 grid((a.HW + T - 1) / T, (unsigned)d->nf);
    hipLaunchKernelGGL(quantiles_kernel, grid, dim3(SORT_LANES), 0, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? 0 : SKCLIM_E_HIP;
}
