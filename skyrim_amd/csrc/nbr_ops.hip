// Neighbourhood fields (include/skyrim_nbr.h): one kernel, a workgroup per (member, op, centre row).  It streams the source rows of the
// disc through LDS in ascending order, builds per source row a doubling table (MAX, MIN) or inclusive prefixes (FRAC_ABOVE, MEAN), and
// folds the periodic range of each of its columns into accumulators in registers; every output is written once.
// Contraction to fma is off for the whole file (and on the build line): the header fixes the order of the float64 operations.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "../../include/skyrim_nbr.h"
#include "fields.h"
#include "program.h"

#pragma clang fp contract(off)

namespace {

constexpr int THREADS = 256;
constexpr int Q = SKNBR_MAX_W / THREADS;      // columns of a lane: i = lane + THREADS q
static_assert(SKNBR_MAX_W % THREADS == 0, "a lane owns a whole number of columns");

struct OpArgs {
    int kind, in, out, radius;
    float thr;
};
struct NbrArgs {
    int M, H, W, n_ops;
    size_t member_stride;
    int reach[SKNBR_MAX_RADII];
    const int32_t* half[SKNBR_MAX_RADII];
    OpArgs op[SKNBR_MAX_OPS];
};

using namespace skfields;

// the NaN-propagating extreme: exact selection, infinities as numbers
template <bool IS_MAX>
__device__ __forceinline__ float ext(float a, float b) {
    if (a != a) return a;
    if (b != b) return b;
    return IS_MAX ? (b > a ? b : a) : (b < a ? b : a);
}

__device__ __forceinline__ bool finite(float v) { return __builtin_fabsf(v) <= 3.402823466e+38f; }

// the sum over the periodic columns c - n ... c + n (2 n + 1 < W) of a row from its inclusive prefixes P: two or three reads
template <typename T>
__device__ __forceinline__ T range(const T* P, int c, int n, int W) {
    const int lo = c - n, hi = c + n;
    if (lo < 0) return P[hi] + (P[W - 1] - P[lo + W - 1]);
    if (hi >= W) return (P[W - 1] - P[lo - 1]) + P[hi - W];
    return lo > 0 ? P[hi] - P[lo - 1] : P[hi];
}

// inclusive scan over the 64 lanes of a wave, lane order
template <typename T>
__device__ __forceinline__ T wave_scan(T v, int lane) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const T o = __shfl_up(v, off);
        if (lane >= off) v = o + v;
    }
    return v;
}

// what stands before the lane's chunk: the totals of the waves before, in order, then of the lanes before in this wave.  `wt`: THREADS / 64
// entries in LDS.  Holds two barriers' worth of traffic: every lane must call it
template <typename T>
__device__ __forceinline__ T before(T total, T* wt) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const T incl = wave_scan(total, lane);
    T excl = __shfl_up(incl, 1);
    if (lane == 0) excl = T(0);
    __syncthreads();                                 // (the readers of wt's last use are done)
    if (lane == 63) wt[wave] = incl;
    __syncthreads();
    T off = T(0);
    for (int w = 0; w < wave; ++w) off = off + wt[w];
    return off + excl;
}

__global__ void __launch_bounds__(THREADS) nbr_kernel(const NbrArgs a, const float* const* __restrict__ members, const double* __restrict__ weights,
                                                      float* out) {
    __shared__ float rowA[SKNBR_MAX_W], rowB[SKNBR_MAX_W];
    __shared__ double preD[SKNBR_MAX_W];
    __shared__ int preI[SKNBR_MAX_W], preJ[SKNBR_MAX_W];
    __shared__ double wtD[THREADS / 64];
    __shared__ int wtI[THREADS / 64], wtJ[THREADS / 64];

    const int tid = threadIdx.x, H = a.H, W = a.W;
    const uint32_t unit = blockIdx.x;
    const int j = (int)(unit % (uint32_t)H);
    const int o = (int)((unit / (uint32_t)H) % (uint32_t)a.n_ops);
    const int m = (int)(unit / ((uint32_t)H * (uint32_t)a.n_ops));
    const OpArgs& op = a.op[o];
    const int kind = op.kind, reach = a.reach[op.radius];
    const int32_t* half = a.half[op.radius] + (size_t)j * (size_t)(2 * reach + 1) + reach;
    const float* x = members[m];
    const uint32_t plane = (uint32_t)op.in * (uint32_t)H * (uint32_t)W;
    const bool extreme = kind == SKNBR_MAX || kind == SKNBR_MIN;
    const int chunk = (W + THREADS - 1) / THREADS;   // the consecutive values a lane sums when a prefix is made

    float acc[Q];                                     // MAX, MIN
    int cnt[Q], bad[Q];                               // FRAC_ABOVE: points above; FRAC_ABOVE, MEAN: non-finite points
    double num[Q];                                    // MEAN
    double den = 0.0;
    int N = 0;
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        acc[q] = kind == SKNBR_MAX ? -__builtin_inff() : __builtin_inff();
        cnt[q] = 0;
        bad[q] = 0;
        num[q] = 0.0;
    }

    // the source rows the table does not mark empty, in ascending order; the next one is fetched into registers while this one is worked on
    auto next_row = [&](int d) {                     // (everything that decides it is the same in all lanes: the barriers are safe)
        for (; d <= reach; ++d) {
            const int r = j + d;
            if (r >= 0 && r < H && uniform(half[d]) >= 0) break;
        }
        return d;
    };
    float pre[Q];
    auto fetch = [&](int d) {
        const uint32_t row = plane + (uint32_t)(j + d) * (uint32_t)W;
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            const int c = tid + THREADS * q;
            pre[q] = c < W ? load_vec<1>(x, row + (uint32_t)c) : 0.f;
        }
    };
    int d = next_row(-reach);
    if (d <= reach) fetch(d);
    while (d <= reach) {
        const int r = j + d;
        int n = uniform(half[d]);
        n = n > W / 2 ? W / 2 : n;
        const bool full = 2 * n + 1 >= W;
        const int L = full ? W : 2 * n + 1;
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            const int c = tid + THREADS * q;
            if (c < W) rowA[c] = pre[q];
        }
        const int d_next = next_row(d + 1);
        if (d_next <= reach) fetch(d_next);
        __syncthreads();
        if (extreme) {
            int k = 31 - __builtin_clz((unsigned)L);                     // floor(log2 L)
            if (full && (1 << k) < W) ++k;                               // a whole row: 2^k >= W periodic points hold every point
            float *cur = rowA, *nxt = rowB;
            for (int s = 0; s < k; ++s) {                                // (1 << s) < W at every level made
                const int step = 1 << s;
#pragma unroll
                for (int q = 0; q < Q; ++q) {
                    const int c = tid + THREADS * q;
                    if (c < W) {
                        int e = c + step;
                        e = e >= W ? e - W : e;
                        nxt[c] = kind == SKNBR_MAX ? ext<true>(cur[c], cur[e]) : ext<false>(cur[c], cur[e]);
                    }
                }
                __syncthreads();
                float* t = cur;
                cur = nxt;
                nxt = t;
            }
#pragma unroll
            for (int q = 0; q < Q; ++q) {
                const int c = tid + THREADS * q;
                if (c < W) {
                    float v;
                    if (full) {
                        v = cur[c];
                    } else {
                        int i1 = c - n, i2 = c + n - (1 << k) + 1;
                        i1 = i1 < 0 ? i1 + W : i1;
                        i2 = i2 < 0 ? i2 + W : (i2 >= W ? i2 - W : i2);
                        v = kind == SKNBR_MAX ? ext<true>(cur[i1], cur[i2]) : ext<false>(cur[i1], cur[i2]);
                    }
                    acc[q] = kind == SKNBR_MAX ? ext<true>(acc[q], v) : ext<false>(acc[q], v);
                }
            }
        } else {
            // the lane's chunk of consecutive values, summed in order; then what stands before the chunk; then the prefixes
            const int c0 = tid * chunk, c1 = (c0 + chunk) < W ? (c0 + chunk) : W;
            const bool mean = kind == SKNBR_MEAN;
            double sd = 0.0;
            int si = 0, sj = 0;
            for (int c = c0; c < c1; ++c) {
                const float v = rowA[c];
                if (mean) {
                    const bool ok = finite(v);
                    sd = sd + (ok ? (double)v : 0.0);
                    sj += ok ? 0 : 1;
                } else {
                    si += v > op.thr ? 1 : 0;
                    sj += v != v ? 1 : 0;
                }
            }
            double bd = 0.0;
            int bi = 0;
            if (mean)
                bd = before<double>(sd, wtD);
            else
                bi = before<int>(si, wtI);
            int bj = before<int>(sj, wtJ);
            for (int c = c0; c < c1; ++c) {
                const float v = rowA[c];
                if (mean) {
                    const bool ok = finite(v);
                    bd = bd + (ok ? (double)v : 0.0);
                    bj += ok ? 0 : 1;
                    preD[c] = bd;
                } else {
                    bi += v > op.thr ? 1 : 0;
                    bj += v != v ? 1 : 0;
                    preI[c] = bi;
                }
                preJ[c] = bj;
            }
            __syncthreads();
            const double w = mean ? weights[r] : 0.0;
            den = den + w * (double)L;
            N += L;
#pragma unroll
            for (int q = 0; q < Q; ++q) {
                const int c = tid + THREADS * q;
                if (c < W) {
                    bad[q] += full ? preJ[W - 1] : range<int>(preJ, c, n, W);
                    if (mean) {
                        const double s = full ? preD[W - 1] : range<double>(preD, c, n, W);
                        num[q] = num[q] + w * s;
                    } else {
                        cnt[q] += full ? preI[W - 1] : range<int>(preI, c, n, W);
                    }
                }
            }
        }
        __syncthreads();                             // the next source row overwrites the buffers
        d = d_next;
    }

    const float qnan = __int_as_float(0x7fc00000);
    float* y = out + (size_t)m * a.member_stride;
    const uint32_t at = ((uint32_t)op.out * (uint32_t)H + (uint32_t)j) * (uint32_t)W;
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        const int c = tid + THREADS * q;
        if (c < W) {
            float v;
            if (extreme)
                v = acc[q] != acc[q] ? qnan : acc[q];
            else if (bad[q] > 0)
                v = qnan;
            else if (kind == SKNBR_MEAN)
                v = (float)(num[q] / den);
            else
                v = (float)((double)cnt[q] / (double)N);
            store_vec<1>(y, at + (uint32_t)c, v);
        }
    }
}

// every refusal of sknbr_run: nothing here touches the GPU
bool valid(const sknbr_desc* d) {
    if (!d || !d->members || ((uintptr_t)d->members & 7) || !d->out || ((uintptr_t)d->out & 3)) return false;
    if (!d->weights || ((uintptr_t)d->weights & 7)) return false;
    if (!skprogram::grid_ok(d->M, SKNBR_MAX_MEMBERS, d->member_align, d->C, d->H, d->W, d->D, d->member_stride) || d->W > SKNBR_MAX_W) return false;
    if (d->n_radii < 1 || d->n_radii > SKNBR_MAX_RADII) return false;
    for (int r = 0; r < d->n_radii; ++r) {
        const sknbr_radius& R = d->radii[r];
        if (R.reach < 0 || R.reach > SKNBR_MAX_REACH || !R.half || ((uintptr_t)R.half & 3)) return false;
    }
    if (d->n_ops < 1 || d->n_ops > SKNBR_MAX_OPS) return false;
    skprogram::Slots<SKNBR_MAX_OPS> slots;
    for (int o = 0; o < d->n_ops; ++o) {
        const sknbr_op& op = d->ops[o];
        if (op.kind < SKNBR_MAX || op.kind > SKNBR_FRAC_ABOVE) return false;
        if (op.in < 0 || op.in >= d->C || op.out < 0 || op.out >= d->D || op.radius < 0 || op.radius >= d->n_radii) return false;
        if (op.kind == SKNBR_FRAC_ABOVE && op.thr != op.thr) return false;
        if (!slots.claim(op.out, d->D)) return false;
    }
    // one workgroup per (member, op, centre row): what a grid holds
    if ((size_t)d->M * (size_t)d->n_ops * (size_t)d->H > 0x7fffffffu) return false;
    return true;
}

}  // namespace

extern "C" int sknbr_abi_version(void) { return SKNBR_ABI_VERSION; }

extern "C" int sknbr_check(const sknbr_desc* d) { return valid(d) ? 0 : SKNBR_E_ARG; }

extern "C" int sknbr_run(const sknbr_desc* d, void* stream) {
    if (!valid(d)) return SKNBR_E_ARG;
    NbrArgs a = {};
    a.M = d->M;
    a.H = d->H;
    a.W = d->W;
    a.n_ops = d->n_ops;
    a.member_stride = d->member_stride;
    for (int r = 0; r < d->n_radii; ++r) {
        a.reach[r] = d->radii[r].reach;
        a.half[r] = d->radii[r].half;
    }
    for (int o = 0; o < d->n_ops; ++o) a.op[o] = OpArgs{d->ops[o].kind, d->ops[o].in, d->ops[o].out, d->ops[o].radius, d->ops[o].thr};
    const size_t units = (size_t)d->M * (size_t)d->n_ops * (size_t)d->H;
    hipLaunchKernelGGL(nbr_kernel, dim3((unsigned)units), dim3(THREADS), 0, (hipStream_t)stream, a, d->members, d->weights, d->out);
    if (hipGetLastError() != hipSuccess) return SKNBR_E_HIP;
    return 0;
}
