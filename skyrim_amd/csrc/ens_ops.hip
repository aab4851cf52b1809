// Ensemble helpers (include/skyrim_ens.h): perturbed members from a counter-based generator, and the statistics of M member states in
// ONE pass -- every member value of a point is read from HBM once and held in registers for the centred sum, the second pass over the
// deviations and the order statistics.  Both kernels are HBM-bound grid-stride loops (csrc/io_ops.hip: the launch shape).
#include <hip/hip_runtime.h>
#include <cstdint>
#include "../../include/skyrim_ens.h"
#include "philox.h"

namespace {

using skrng::u32x4;
using skrng::philox4x32_10;
using skrng::normal_pair;      // csrc/philox.h: the generator and its normals, shared with noise_ops.hip

// one lane = one group of 4 consecutive elements (one Philox block); blockIdx.y = member of the batch
__global__ void __launch_bounds__(256) perturb_kernel(const float* __restrict__ x0, const float* __restrict__ std, float* __restrict__ out,
                                                      uint32_t n, uint32_t chan_stride, uint32_t C, float scale, uint32_t seed,
                                                      uint32_t member_first, int vec) {
    const uint32_t member = member_first + blockIdx.y;
    float* __restrict__ dst = out + (size_t)blockIdx.y * n;
    const uint32_t groups = (uint32_t)(((uint64_t)n + 3) / 4);
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t g = blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += stride) {
        const uint32_t i0 = 4 * g;
        const bool full = vec && n - i0 >= 4;
        float x[4];
        if (full) {
            const float4 v = *(const float4*)(x0 + i0);
            x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) x[e] = i0 + e < n ? x0[i0 + e] : 0.f;
        }
        if (member != 0) {                                   // (uniform in the block) member 0 is the control: a bit copy
            const u32x4 r = philox4x32_10(g, 0, 0, 0, seed, member);
            float z[4];
            normal_pair(r.x, r.y, z[0], z[1]);
            normal_pair(r.z, r.w, z[2], z[3]);
            uint32_t rem = i0 % chan_stride, c = (i0 / chan_stride) % C;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (i0 + e < n) x[e] = x[e] + (scale * std[c]) * z[e];
                if (++rem == chan_stride) { rem = 0; c = c + 1 == C ? 0 : c + 1; }
            }
        }
        if (full) {
            *(float4*)(dst + i0) = make_float4(x[0], x[1], x[2], x[3]);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (i0 + e < n) dst[i0 + e] = x[e];
        }
    }
}

// ---- statistics ------------------------------------------------------------------------------------------------------------------ //
struct StatsArgs {
    const float* const* members;
    int M;
    size_t offset;         // first element of the range in the members
    size_t n;              // length of the whole range: the stride of exceed[k] / quant[q]
    size_t j0, items;      // this launch: range-relative start, number of V-element items
    float *mean, *spread, *mn, *mx, *exceed, *quant;
    int n_thr;
    float thr[SKENS_MAX_THRESHOLDS];
    int n_quant;
    int q_lo[SKENS_MAX_QUANTILES], q_hi[SKENS_MAX_QUANTILES];
    float q_frac[SKENS_MAX_QUANTILES];
    int out_vec;           // the outputs of an item may be written with one V-wide store
};

template <int V> struct Vec;
template <> struct Vec<1> { typedef float type; };
template <> struct Vec<2> { typedef float2 type; };
template <> struct Vec<4> { typedef float4 type; };

template <int V> __device__ __forceinline__ void load_vec(const float* base, uint32_t byte_off, float* x) {
    const typename Vec<V>::type v = *(const typename Vec<V>::type*)((const char*)base + byte_off);
    const float* f = (const float*)&v;
#pragma unroll
    for (int e = 0; e < V; ++e) x[e] = f[e];
}

template <int V> __device__ __forceinline__ void store_vec(float* p, const float* x, int vec) {
    if (vec) {
        typename Vec<V>::type v;
        float* f = (float*)&v;
#pragma unroll
        for (int e = 0; e < V; ++e) f[e] = x[e];
        *(typename Vec<V>::type*)p = v;
    } else {
#pragma unroll
        for (int e = 0; e < V; ++e) p[e] = x[e];
    }
}

// MB: the member-count bucket (M <= MB; every loop over members is unrolled over MB with the member index a compile-time constant, so the
// values stay in registers: a register array indexed at run time would live in scratch); V: elements per lane; QUANT: order statistics wanted
template <int MB, int V, bool QUANT>
__global__ void __launch_bounds__(256) stats_kernel(const StatsArgs a) {
    const int M = a.M;
    const float fm = (float)M;
    // 32-bit indices (the range ends below 2^30 elements: checked by the caller): a member's address is its pointer, wave-uniform in scalar
    // registers, plus ONE per-lane byte offset shared by all members -- not M 64-bit per-lane addresses
    const uint32_t stride = gridDim.x * blockDim.x, items = (uint32_t)a.items;
    for (uint32_t t = blockIdx.x * blockDim.x + threadIdx.x; t < items; t += stride) {
        const uint32_t j = (uint32_t)a.j0 + t * V;
        const uint32_t i = 4u * ((uint32_t)a.offset + j);
        float x[MB][V];
        load_vec<V>(a.members[0], i, x[0]);
#pragma unroll
        for (int m = 1; m < MB; ++m) {
            if (m < M) {
                load_vec<V>(a.members[m], i, x[m]);
            } else {
#pragma unroll
                for (int e = 0; e < V; ++e) x[m][e] = x[0][e];          // a member that is not there: deviation 0, never min or max
            }
        }
        float mean[V], spread[V], mn[V], mx[V], ex[SKENS_MAX_THRESHOLDS][V];
#pragma unroll
        for (int e = 0; e < V; ++e) {
            const float x0 = x[0][e];
            // comparisons first, on the values themselves; after them only the deviations are needed (unless the order statistics follow), so
            // the registers of x can be taken over by d instead of both staying live
            float lo = x0, hi = x0;
#pragma unroll
            for (int m = 0; m < MB; ++m) {
                lo = fminf(lo, x[m][e]);
                hi = fmaxf(hi, x[m][e]);
            }
            mn[e] = lo;
            mx[e] = hi;
#pragma unroll
            for (int k = 0; k < SKENS_MAX_THRESHOLDS; ++k) {
                int cnt = 0;
                if (k < a.n_thr) {
#pragma unroll
                    for (int m = 0; m < MB; ++m) cnt += (m < M && x[m][e] > a.thr[k]) ? 1 : 0;
                }
                ex[k][e] = (float)cnt / fm;
            }
            float d[MB], sum = 0.f;
#pragma unroll
            for (int m = 0; m < MB; ++m) {
                d[m] = x[m][e] - x0;                                     // (0 for m >= M)
                sum += d[m];
            }
            const float c = sum / fm;
            float ss = 0.f;
#pragma unroll
            for (int m = 0; m < MB; ++m) {
                const float r = d[m] - c;
                ss += m < M ? r * r : 0.f;
            }
            mean[e] = x0 + c;
            spread[e] = sqrtf(ss / fm);
        }
        if (a.mean) store_vec<V>(a.mean + j, mean, a.out_vec);
        if (a.spread) store_vec<V>(a.spread + j, spread, a.out_vec);
        if (a.mn) store_vec<V>(a.mn + j, mn, a.out_vec);
        if (a.mx) store_vec<V>(a.mx + j, mx, a.out_vec);
#pragma unroll
        for (int k = 0; k < SKENS_MAX_THRESHOLDS; ++k)
            if (k < a.n_thr) store_vec<V>(a.exceed + (size_t)k * a.n + j, ex[k], a.out_vec);
        if (QUANT) {
            // ascending order in place: a bitonic network over MB slots (+inf where there is no member), every index a compile-time constant
#pragma unroll
            for (int m = 1; m < MB; ++m)
                if (m >= M) {
#pragma unroll
                    for (int e = 0; e < V; ++e) x[m][e] = __builtin_inff();
                }
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
            for (int qn = 0; qn < SKENS_MAX_QUANTILES; ++qn) {
                if (qn < a.n_quant) {
                    float res[V];
#pragma unroll
                    for (int e = 0; e < V; ++e) {
                        float lo = x[0][e], hi = x[0][e];
#pragma unroll
                        for (int m = 1; m < MB; ++m) {
                            lo = m == a.q_lo[qn] ? x[m][e] : lo;
                            hi = m == a.q_hi[qn] ? x[m][e] : hi;
                        }
                        // lo + frac * (hi - lo) with the difference carried exactly (two-sum), so neighbours of opposite sign cost nothing
                        const float nl = -lo, d = hi + nl, bb = d - hi, err = (hi - (d - bb)) + (nl - bb);
                        res[e] = fmaf(a.q_frac[qn], err, fmaf(a.q_frac[qn], d, lo));
                    }
                    store_vec<V>(a.quant + (size_t)qn * a.n + j, res, a.out_vec);
                }
            }
        }
    }
}

template <int MB, int V>
void launch_bucket(const StatsArgs& a, bool quant, hipStream_t s) {
    // 256 CUs x 8 workgroups of 256 lanes; every lane walks the range with the grid's stride (csrc/io_ops.hip)
    const size_t want = (a.items + 255) / 256;
    const unsigned blocks = (unsigned)(want < 2048 ? want : 2048);
    if (quant)
        hipLaunchKernelGGL((stats_kernel<MB, V, true>), dim3(blocks), dim3(256), 0, s, a);
    else
        hipLaunchKernelGGL((stats_kernel<MB, V, false>), dim3(blocks), dim3(256), 0, s, a);
}

// per-lane vector width of a bucket: the compiler keeps values and deviations live together (about 2 x MB x V registers), so the width falls
// with the bucket and every instantiation without order statistics runs 3 to 8
// waves per SIMD with no scratch (docs/experiments.md has the register table)
constexpr int bucket_width(int MB) { return MB <= 8 ? 4 : MB <= 16 ? 2 : 1; }

template <int MB>
void launch_range(StatsArgs a, bool quant, bool in_vec, bool out_aligned, hipStream_t s) {
    constexpr int V = bucket_width(MB);
    const size_t n = a.n;
    size_t head = 0, body = 0;
    if (V > 1 && in_vec) {
        head = (V - a.offset % V) % V;
        if (head > n) head = n;
        body = (n - head) / V;
    }
    a.out_vec = 0;
    if (head) {
        a.j0 = 0; a.items = head;
        launch_bucket<MB, 1>(a, quant, s);
    }
    if (body) {
        a.j0 = head; a.items = body;
        a.out_vec = out_aligned && head % V == 0 && n % V == 0;
        launch_bucket<MB, V>(a, quant, s);
        a.out_vec = 0;
    }
    const size_t done = head + body * V;
    if (done < n) {
        a.j0 = done; a.items = n - done;
        launch_bucket<MB, 1>(a, quant, s);
    }
}

}  // namespace

extern "C" int skens_abi_version(void) { return SKENS_ABI_VERSION; }

extern "C" int skens_perturb(const float* x0, const float* std, float* out, size_t n, size_t chan_stride, int C, float scale, uint32_t seed,
                             uint32_t member_first, int n_members, void* stream) {
    if (!x0 || !std || !out || (((uintptr_t)x0 | (uintptr_t)std | (uintptr_t)out) & 3)) return SKENS_E_ARG;
    if (n == 0 || n > 0xFFFFFFF0ull || chan_stride == 0 || C < 1 || n_members < 1 || n_members > 65535) return SKENS_E_ARG;
    if (n % chan_stride || (n / chan_stride) % (size_t)C) return SKENS_E_ARG;       // n = L * C * chan_stride
    const int vec = (((uintptr_t)x0 | (uintptr_t)out) & 15) == 0 && (n_members == 1 || n % 4 == 0);
    const size_t want = ((n + 3) / 4 + 255) / 256;
    const unsigned blocks = (unsigned)(want < 2048 ? want : 2048);
    hipLaunchKernelGGL(perturb_kernel, dim3(blocks, (unsigned)n_members), dim3(256), 0, (hipStream_t)stream, x0, std, out, (uint32_t)n,
                       (uint32_t)chan_stride, (uint32_t)C, scale, seed, member_first, vec);
    return hipGetLastError() == hipSuccess ? 0 : SKENS_E_HIP;
}

extern "C" int skens_stats(const skens_stats_desc* d, void* stream) {
    if (!d || !d->members || d->M < 1 || d->M > SKENS_MAX_MEMBERS) return SKENS_E_ARG;
    if (d->member_align != 4 && d->member_align != 16) return SKENS_E_ARG;
    if (d->n_thr < 0 || d->n_thr > SKENS_MAX_THRESHOLDS || d->n_quant < 0 || d->n_quant > SKENS_MAX_QUANTILES) return SKENS_E_ARG;
    if ((d->n_thr > 0) != (d->exceed != nullptr) || (d->n_quant > 0) != (d->quant != nullptr)) return SKENS_E_ARG;
    if (!d->mean && !d->spread && !d->min && !d->max && !d->exceed && !d->quant) return SKENS_E_ARG;
    const uintptr_t outs = (uintptr_t)d->mean | (uintptr_t)d->spread | (uintptr_t)d->min | (uintptr_t)d->max | (uintptr_t)d->exceed | (uintptr_t)d->quant;
    if (outs & 3) return SKENS_E_ARG;
    StatsArgs a = {};
    for (int q = 0; q < d->n_quant; ++q) {
        if (d->q_index[q] < 0 || d->q_index[q] >= d->M || !(d->q_frac[q] >= 0.f && d->q_frac[q] < 1.f)) return SKENS_E_ARG;
        a.q_lo[q] = d->q_index[q];
        a.q_hi[q] = d->q_index[q] + 1 < d->M ? d->q_index[q] + 1 : d->M - 1;
        a.q_frac[q] = d->q_frac[q];
    }
    if (d->n == 0) return 0;
    if (d->offset > (1ull << 30) || d->n > (1ull << 30) - d->offset) return SKENS_E_ARG;       // 32-bit byte offsets in the kernel
    a.members = d->members; a.M = d->M; a.offset = d->offset; a.n = d->n;
    a.mean = d->mean; a.spread = d->spread; a.mn = d->min; a.mx = d->max; a.exceed = d->exceed; a.quant = d->quant;
    a.n_thr = d->n_thr; a.n_quant = d->n_quant;
    for (int k = 0; k < d->n_thr; ++k) a.thr[k] = d->thr[k];
    const bool quant = d->n_quant > 0, in_vec = d->member_align == 16, out_aligned = (outs & 15) == 0;
    hipStream_t s = (hipStream_t)stream;
    if (d->M <= 8) launch_range<8>(a, quant, in_vec, out_aligned, s);
    else if (d->M <= 16) launch_range<16>(a, quant, in_vec, out_aligned, s);
    else if (d->M <= 32) launch_range<32>(a, quant, in_vec, out_aligned, s);
    else launch_range<64>(a, quant, in_vec, out_aligned, s);
    return hipGetLastError() == hipSuccess ? 0 : SKENS_E_HIP;
}
