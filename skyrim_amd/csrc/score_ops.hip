// Forecast verification (include/skyrim_score.h): the scores of M member states against a truth state in ONE pass over the members --
// every member value and every truth value is read from HBM once -- and a small second kernel that weights and sums the latitude rows.
// Stage 1 is a wave per latitude row: fp32 inside a point's term, float64 from the lane's accumulator on, no floating-point atomics.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "../../include/skyrim_score.h"
#include "fields.h"

namespace {

using namespace skfields;

struct ScoreArgs {
    int M, H, W, c0, nc, flags;
};

// the pointers of a launch are kernel parameters of their own, each __restrict__: only then does the compiler know that the stores to
// `partial` and `counts` cannot change the member table, and reads the M member pointers with scalar loads into scalar registers
struct ScorePtrs {
    const float* const* members;
    const float* truth;
    const float* clim;
    double* partial;       // [nc][H][SKSCORE_PARTIALS]
    int32_t* counts;       // [nc][H][M + 1]
};

// slots of a row partial
enum { P_BIAS, P_MAE, P_MSE, P_VAR, P_ABS, P_PAIR, P_FA, P_FF, P_AA };
static_assert(P_AA + 1 == SKSCORE_PARTIALS, "row partial layout");

// MB: the member-count bucket (M <= MB; every loop over members is unrolled over MB with the member index a compile-time constant, so the
// values stay in registers: a register array indexed at run time would live in scratch); V: consecutive points per lane; SORT: the pair
// term of the fair CRPS is wanted (M > 1).  The flags are wave-uniform branches.
template <int MB, int V, bool SORT>
__global__ void __launch_bounds__(256) score_rows_kernel(const ScoreArgs a, const float* const* __restrict__ members,
                                                          const float* __restrict__ truth, const float* __restrict__ clim,
                                                          double* __restrict__ partial, int32_t* __restrict__ counts) {
    __shared__ int hist[4][SKSCORE_MAX_MEMBERS + 1];                  // rank counts of the row each wave is on
    const int M = a.M, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float fm = (float)M, fm1 = (float)(M > 1 ? M - 1 : 1);
    const bool det = a.flags & SKSCORE_DET, var = MB > 1 && (a.flags & SKSCORE_VAR), crps = a.flags & SKSCORE_CRPS;
    const bool acc = a.flags & SKSCORE_ACC, rank = a.flags & SKSCORE_RANK;
    const uint32_t H = (uint32_t)a.H, W = (uint32_t)a.W, rows = (uint32_t)a.nc * H, groups = (rows + 3) / 4, items = W / V;
    if (rank) {
        for (int r = lane; r <= M; r += 64) hist[wave][r] = 0;
        __syncthreads();
    }
    for (uint32_t g = blockIdx.x; g < groups; g += gridDim.x) {       // the same trip count for the four waves: barriers below
        const uint32_t row = 4 * g + wave;
        const bool live = row < rows;
        double s[SKSCORE_PARTIALS];
#pragma unroll
        for (int k = 0; k < SKSCORE_PARTIALS; ++k) s[k] = 0.0;
        if (live) {
            const uint32_t cc = row / H, j = row - cc * H;
            // 32-bit byte offsets (C * H * W <= 2^30: checked by the caller): a member's address is its pointer, wave-uniform in scalar
            // registers, plus ONE per-lane offset shared by the members, the truth and the climatology
            const uint32_t base = 4u * ((((uint32_t)a.c0 + cc) * H + j) * W);
            for (uint32_t t = lane; t < items; t += 64) {
                const uint32_t off = base + 4u * V * t;
                float x[MB][V], y[V], c[V];
                load_to<V>(truth, off, y);
                if (acc) load_to<V>(clim, off, c);
                load_to<V>(members[0], off, x[0]);
#pragma unroll
                for (int m = 1; m < MB; ++m) {
                    if (m < M) {
                        load_to<V>(members[m], off, x[m]);
                    } else {
#pragma unroll
                        for (int e = 0; e < V; ++e) x[m][e] = x[0][e];      // a member that is not there: no term below counts it
                    }
                }
#pragma unroll
                for (int e = 0; e < V; ++e) {
                    const float yy = y[e];
                    // every section forms the e_m = x_m - y it needs itself, the later ones from a copy of y the compiler cannot identify
                    // with it: values kept from one section for the next would be MB more live registers next to the member values
                    float se = 0.f;
                    if (det || acc) {
#pragma unroll
                        for (int m = 0; m < MB; ++m) se += m < M ? x[m][e] - yy : 0.f;
                    }
                    const float eb = MB == 1 ? se : se / fm;
                    if (MB >= 32) __builtin_amdgcn_sched_barrier(0);        // (the big buckets: no section starts under the one before it,
                                                                            // which would hold both sections' temporaries in registers)
                    if (det) {
                        s[P_BIAS] += (double)eb;
                        s[P_MAE] += (double)fabsf(eb);
                        s[P_MSE] += (double)(eb * eb);
                    }
                    if (acc) {
                        const float an = yy - c[e], f = eb + an;
                        s[P_FA] += (double)(f * an);
                        s[P_FF] += (double)(f * f);
                        s[P_AA] += (double)(an * an + (eb - eb));           // (eb - eb: 0, or NaN where a member is not finite)
                    }
                    if (rank) {
                        int r = 0;
#pragma unroll
                        for (int m = 0; m < MB; ++m) r += (m < M && x[m][e] < yy) ? 1 : 0;
                        atomicAdd(&hist[wave][r], 1);
                    }
                    if (var) {
                        float sd = 0.f;
#pragma unroll
                        for (int m = 1; m < MB; ++m) sd += m < M ? x[m][e] - x[0][e] : 0.f;
                        const float db = sd / fm;
                        // the deviations are formed a second time from a copy of x_0 the compiler cannot identify with it: kept from the
                        // first loop they would be MB more live registers next to the member values the sort still needs
                        float x0 = x[0][e];
                        asm volatile("" : "+v"(x0));
                        float ss = 0.f;
#pragma unroll
                        for (int m = 0; m < MB; ++m) {
                            const float dv = (x[m][e] - x0) - db;
                            ss += m < M ? dv * dv : 0.f;
                        }
                        s[P_VAR] += (double)(ss / fm1 + (yy - yy));         // (yy - yy: a non-finite truth reaches this slot too)
                    }
                    if (MB >= 32) __builtin_amdgcn_sched_barrier(0);
                    if (crps) {
                        float y2 = yy, sa = 0.f;
                        asm volatile("" : "+v"(y2));
#pragma unroll
                        for (int m = 0; m < MB; ++m) sa += m < M ? fabsf(x[m][e] - y2) : 0.f;
                        const float A = MB == 1 ? sa : sa / fm;
                        s[P_ABS] += (double)A;
                        if (SORT) {
                            // ascending order in place, LAST (nothing below needs the member order): a bitonic network over MB slots,
                            // +inf where there is no member, every index a compile-time constant
#pragma unroll
                            for (int m = 1; m < MB; ++m)
                                if (m >= M) x[m][e] = __builtin_inff();
#pragma unroll
                            for (int k = 2; k <= MB; k <<= 1) {
#pragma unroll
                                for (int st = k >> 1; st > 0; st >>= 1) {
#pragma unroll
                                    for (int p = 0; p < MB; ++p) {
                                        const int q = p ^ st;
                                        if (q > p) {
                                            const bool up = (p & k) == 0;
                                            const float lo = fminf(x[p][e], x[q][e]), hi = fmaxf(x[p][e], x[q][e]);
                                            x[p][e] = up ? lo : hi;
                                            x[q][e] = up ? hi : lo;
                                        }
                                    }
                                }
                            }
                            // gap i lies between (i + 1)(M - 1 - i) pairs: small integers, exact in fp32.  They are formed here, from a
                            // copy of M - 1 the compiler cannot see through: as loop invariants they would be hoisted into MB - 1 registers
                            // that stay live across the whole row
                            if (MB >= 32) __builtin_amdgcn_sched_barrier(0);
                            float top = fm1;
                            asm volatile("" : "+v"(top));
                            float sb = 0.f;
#pragma unroll
                            for (int i = 0; i + 1 < MB; ++i) {
                                const float pairs = (float)(i + 1) * (top - (float)i);
                                sb += i + 1 < M ? pairs * (x[i + 1][e] - x[i][e]) : 0.f;
                            }
                            s[P_PAIR] += (double)(sb / (fm * fm1) + (A - A));   // (A - A: fminf / fmaxf drop a NaN member, this does not)
                        }
                    }
                }
            }
        }
        if (det) {
            const double b = wave_sum(s[P_BIAS]), ab = wave_sum(s[P_MAE]), sq = wave_sum(s[P_MSE]);
            if (live && lane == 0) {
                double* p = partial + (size_t)row * SKSCORE_PARTIALS;
                p[P_BIAS] = b; p[P_MAE] = ab; p[P_MSE] = sq;
            }
        }
        if (a.flags & SKSCORE_VAR) {                                            // (M = 1: the zeros)
            const double v = wave_sum(s[P_VAR]);
            if (live && lane == 0) partial[(size_t)row * SKSCORE_PARTIALS + P_VAR] = v;
        }
        if (crps) {
            const double sa = wave_sum(s[P_ABS]), sb = wave_sum(s[P_PAIR]);
            if (live && lane == 0) {
                double* p = partial + (size_t)row * SKSCORE_PARTIALS;
                p[P_ABS] = sa; p[P_PAIR] = sb;
            }
        }
        if (acc) {
            const double fa = wave_sum(s[P_FA]), ff = wave_sum(s[P_FF]), aa = wave_sum(s[P_AA]);
            if (live && lane == 0) {
                double* p = partial + (size_t)row * SKSCORE_PARTIALS;
                p[P_FA] = fa; p[P_FF] = ff; p[P_AA] = aa;
            }
        }
        if (rank) {
            __syncthreads();
            for (int r = lane; r <= M; r += 64) {
                if (live) counts[(size_t)row * (M + 1) + r] = hist[wave][r];
                hist[wave][r] = 0;
            }
            __syncthreads();
        }
    }
}

// sum over the 256 threads in a fixed order; every thread returns the total
__device__ __forceinline__ double block_sum(double v, double* red) {
    const int t = threadIdx.x;
    __syncthreads();
    red[t] = v;
    __syncthreads();
#pragma unroll
    for (int n = 128; n > 0; n >>= 1) {
        if (t < n) red[t] += red[t + n];
        __syncthreads();
    }
    return red[0];
}

// stage 2: one workgroup per channel; thread t takes the rows t, t + 256, ... in ascending order
__global__ void __launch_bounds__(256) score_reduce_kernel(const double* __restrict__ partial, const double* __restrict__ w,
                                                           double* __restrict__ out, int H, int W, int flags) {
    __shared__ double red[256];
    const int cc = blockIdx.x, t = threadIdx.x;
    double sw = 0.0;
    for (int j = t; j < H; j += 256) sw += w[j];
    const double denom = (double)W * block_sum(sw, red);
    double res[SKSCORE_PARTIALS];
#pragma unroll
    for (int k = 0; k < SKSCORE_PARTIALS; ++k) {
        const int need = k <= P_MSE ? SKSCORE_DET : k == P_VAR ? SKSCORE_VAR : k <= P_PAIR ? SKSCORE_CRPS : SKSCORE_ACC;
        res[k] = 0.0;
        if (flags & need) {
            double acc = 0.0;
            for (int j = t; j < H; j += 256) acc += w[j] * partial[((size_t)cc * H + j) * SKSCORE_PARTIALS + k];
            res[k] = block_sum(acc, red) / denom;
        }
    }
    if (t == 0) {
        double* o = out + (size_t)cc * SKSCORE_SLOTS;
        if (flags & SKSCORE_DET) { o[SKSCORE_BIAS] = res[P_BIAS]; o[SKSCORE_MAE] = res[P_MAE]; o[SKSCORE_MSE] = res[P_MSE]; }
        if (flags & SKSCORE_VAR) o[SKSCORE_VARIANCE] = res[P_VAR];
        if (flags & SKSCORE_CRPS) { o[SKSCORE_ABS] = res[P_ABS]; o[SKSCORE_PAIR] = res[P_PAIR]; o[SKSCORE_CRPS_FAIR] = res[P_ABS] - res[P_PAIR]; }
        if (flags & SKSCORE_ACC) { o[SKSCORE_FA] = res[P_FA]; o[SKSCORE_FF] = res[P_FF]; o[SKSCORE_AA] = res[P_AA]; }
    }
}

template <int MB, int V>
void launch_rows(const ScoreArgs& a, const ScorePtrs& p, bool sort, hipStream_t s) {
    // 256 CUs x 8 workgroups of four waves; a workgroup walks the groups of four rows with the grid's stride (csrc/io_ops.hip)
    const size_t groups = ((size_t)a.nc * a.H + 3) / 4;
    const unsigned blocks = (unsigned)(groups < 2048 ? groups : 2048);
    if (MB > 1 && sort)
        hipLaunchKernelGGL((score_rows_kernel<MB, V, (MB > 1)>), dim3(blocks), dim3(256), 0, s, a, p.members, p.truth, p.clim, p.partial, p.counts);
    else
        hipLaunchKernelGGL((score_rows_kernel<MB, V, false>), dim3(blocks), dim3(256), 0, s, a, p.members, p.truth, p.clim, p.partial, p.counts);
}

// points per lane of a bucket: the member values of a lane's points are live together (MB x V registers), so the width falls with the bucket
constexpr int bucket_width(int MB) { return MB <= 8 ? 4 : MB <= 16 ? 2 : 1; }

template <int MB>
void launch_bucket(const ScoreArgs& a, const ScorePtrs& p, bool sort, bool aligned, hipStream_t s) {
    constexpr int V = bucket_width(MB);
    if (V > 1 && aligned && a.W % V == 0)                  // every row then starts on a vector boundary
        launch_rows<MB, V>(a, p, sort, s);
    else
        launch_rows<MB, 1>(a, p, sort, s);
}

bool valid_shape(int C, int H, int M, int flags) {
    return C >= 1 && H >= 1 && M >= 1 && M <= SKSCORE_MAX_MEMBERS && flags != 0 && (flags & ~SKSCORE_ALL_FLAGS) == 0;
}

}  // namespace

extern "C" int skscore_abi_version(void) { return SKSCORE_ABI_VERSION; }

extern "C" size_t skscore_workspace_bytes(int C, int H, int M, int flags) {
    if (!valid_shape(C, H, M, flags)) return 0;
    return (size_t)C * (size_t)H * SKSCORE_PARTIALS * sizeof(double);
}

extern "C" int skscore_run(const skscore_desc* d, void* stream) {
    if (!d || !d->members || !d->truth || !d->lat_weight || d->W < 1 || !valid_shape(d->C, d->H, d->M, d->flags)) return SKSCORE_E_ARG;
    if (d->member_align != 4 && d->member_align != 16) return SKSCORE_E_ARG;
    if (((uintptr_t)d->truth & 3) || ((uintptr_t)d->lat_weight & 7)) return SKSCORE_E_ARG;
    const bool acc = d->flags & SKSCORE_ACC, rank = d->flags & SKSCORE_RANK, sums = d->flags & ~SKSCORE_RANK;
    if (acc && (!d->clim || ((uintptr_t)d->clim & 3))) return SKSCORE_E_ARG;
    if (rank && (!d->counts || ((uintptr_t)d->counts & 3))) return SKSCORE_E_ARG;
    if (sums && (!d->out || ((uintptr_t)d->out & 7))) return SKSCORE_E_ARG;
    if (d->c0 < 0 || d->nc < 0 || d->c0 > d->C || d->nc > d->C - d->c0) return SKSCORE_E_ARG;
    if ((size_t)d->C * (size_t)d->H > (1ull << 30) / (size_t)d->W) return SKSCORE_E_ARG;            // 32-bit byte offsets in the kernel
    if (!d->workspace || ((uintptr_t)d->workspace & 7) || d->workspace_bytes < skscore_workspace_bytes(d->C, d->H, d->M, d->flags))
        return SKSCORE_E_ARG;
    if (d->nc == 0) return 0;
    ScoreArgs a = {};
    const ScorePtrs p = {d->members, d->truth, acc ? d->clim : nullptr, (double*)d->workspace, d->counts};
    a.M = d->M; a.H = d->H; a.W = d->W; a.c0 = d->c0; a.nc = d->nc; a.flags = d->flags;
    const bool sort = (d->flags & SKSCORE_CRPS) && d->M > 1;
    const bool aligned = d->member_align == 16 && ((uintptr_t)d->truth & 15) == 0 && (!acc || ((uintptr_t)d->clim & 15) == 0);
    hipStream_t s = (hipStream_t)stream;
    if (d->M == 1) launch_bucket<1>(a, p, false, aligned, s);
    else if (d->M <= 8) launch_bucket<8>(a, p, sort, aligned, s);
    else if (d->M <= 16) launch_bucket<16>(a, p, sort, aligned, s);
    else if (d->M <= 32) launch_bucket<32>(a, p, sort, aligned, s);
    else launch_bucket<64>(a, p, sort, aligned, s);
    if (hipGetLastError() != hipSuccess) return SKSCORE_E_HIP;
    if (sums) {
        hipLaunchKernelGGL(score_reduce_kernel, dim3((unsigned)d->nc), dim3(256), 0, s, (const double*)d->workspace, d->lat_weight, d->out,
                           d->H, d->W, d->flags);
        if (hipGetLastError() != hipSuccess) return SKSCORE_E_HIP;
    }
    return 0;
}
