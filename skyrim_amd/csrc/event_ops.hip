// Event verification (include/skyrim_event.h): for threshold events "x > thr", the per-row joint counts of (observed, members above) in
// ONE pass over the members of all event channels, and the neighbourhood sums of the fractions skill score from the uint8 planes that
// pass leaves behind.  Integers only: comparisons, integer adds in LDS, int64 squares.  No floating-point arithmetic, no float atomics.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "../../include/skyrim_event.h"
#include "fields.h"

namespace {

using namespace skfields;

constexpr int MAXT = SKEVENT_MAX_THRESHOLDS, MAXM = SKEVENT_MAX_MEMBERS;
constexpr int CHUNK = 8;                    // member loads in flight per lane (x V floats each)

struct CountArgs {
    int M, H, W, n_events, planes;          // planes: also store k and o as uint8 (a neighbourhood pass follows)
    int channel[SKEVENT_MAX_CHANNELS];
    int n_thr[SKEVENT_MAX_CHANNELS];
    float thr[SKEVENT_MAX_CHANNELS][MAXT];
};

struct ScaleArgs {
    int M, H, W, n_scales;
    int n_thr[SKEVENT_MAX_CHANNELS];
    int hy[SKEVENT_MAX_SCALES];
};


__device__ __forceinline__ int lanes_with(bool p) { return __popcll(__ballot(p)); }      // wave-uniform

// One workgroup owns one (event channel, latitude row) at a time and walks them with the grid's stride.  The members are read in chunks
// of CHUNK loads per lane (a member index past M - 1 reads member M - 1 again, from cache, and is not counted): nothing but the counts
// k[t] stays live across the chunks, so one instantiation serves every member count of score_ops.hip's buckets.
template <int V>
__global__ void __launch_bounds__(256) event_count_kernel(const CountArgs a, const float* const* __restrict__ members,
                                                          const float* __restrict__ truth, int32_t* __restrict__ counts,
                                                          uint8_t* __restrict__ planes) {
    __shared__ int hist[MAXT][2][MAXM + 1];
    const int M = a.M, tid = threadIdx.x, lane = tid & 63;
    const uint32_t H = (uint32_t)a.H, W = (uint32_t)a.W, units = (uint32_t)a.n_events * H, items = W / V;
    const size_t hw = (size_t)H * W;
    for (int r = tid; r < MAXT * 2 * (MAXM + 1); r += 256) (&hist[0][0][0])[r] = 0;
    __syncthreads();
    for (uint32_t unit = blockIdx.x; unit < units; unit += gridDim.x) {
        const uint32_t e = unit / H, j = unit - e * H;
        const int nt = a.n_thr[e];
        float thr[MAXT];
#pragma unroll
        for (int t = 0; t < MAXT; ++t) thr[t] = a.thr[e][t];
        // 32-bit byte offsets (C * H * W <= 2^30: checked by the caller), shared by the members and the truth
        const uint32_t base = 4u * (((uint32_t)a.channel[e] * H + j) * W);
        int corner[MAXT][4];                                            // wave-uniform: (o, k) = (0, 0), (1, 0), (0, M), (1, M)
#pragma unroll
        for (int t = 0; t < MAXT; ++t)
#pragma unroll
            for (int q = 0; q < 4; ++q) corner[t][q] = 0;
        for (uint32_t it0 = 0; it0 < items; it0 += 256) {              // the same trip count for every lane: ballots below
            const uint32_t it = it0 + tid;
            const bool valid = it < items;
            const uint32_t off = base + 4u * V * (valid ? it : 0u);
            int k[MAXT][V];
#pragma unroll
            for (int t = 0; t < MAXT; ++t)
#pragma unroll
                for (int v = 0; v < V; ++v) k[t][v] = 0;
            float y[V];
            load_to<V>(truth, off, y);
            for (int m0 = 0; m0 < M; m0 += CHUNK) {
                float x[CHUNK][V];
#pragma unroll
                for (int u = 0; u < CHUNK; ++u) load_to<V>(members[min(m0 + u, M - 1)], off, x[u]);
#pragma unroll
                for (int u = 0; u < CHUNK; ++u) {
                    const bool on = m0 + u < M;
#pragma unroll
                    for (int t = 0; t < MAXT; ++t) {
                        if (t < nt) {
#pragma unroll
                            for (int v = 0; v < V; ++v) k[t][v] += (on && x[u][v] > thr[t]) ? 1 : 0;
                        }
                    }
                }
            }
#pragma unroll
            for (int t = 0; t < MAXT; ++t) {
                if (t < nt) {
                    uint32_t kp = 0, op = 0;
#pragma unroll
                    for (int v = 0; v < V; ++v) {
                        const int kk = k[t][v], o = y[v] > thr[t] ? 1 : 0;
                        const bool none = valid && kk == 0, all = valid && kk == M;
                        corner[t][0] += lanes_with(none && !o);
                        corner[t][1] += lanes_with(none && o);
                        corner[t][2] += lanes_with(all && !o);
                        corner[t][3] += lanes_with(all && o);
                        if (valid && kk != 0 && kk != M) atomicAdd(&hist[t][o][kk], 1);
                        kp |= (uint32_t)kk << (8 * v);
                        op |= (uint32_t)o << (8 * v);
                    }
                    if (a.planes && valid) {
                        uint8_t* pk = planes + ((size_t)(e * MAXT + t) * 2) * hw + (size_t)j * W + (size_t)V * it;
                        if constexpr (V == 4) {                         // (W % 4 == 0 and a 16-byte aligned workspace: aligned words)
                            *(uint32_t*)pk = kp;
                            *(uint32_t*)(pk + hw) = op;
                        } else {
                            pk[0] = (uint8_t)kp;
                            pk[hw] = (uint8_t)op;
                        }
                    }
                }
            }
        }
        if (lane == 0) {
#pragma unroll
            for (int t = 0; t < MAXT; ++t) {
                if (t < nt) {
                    atomicAdd(&hist[t][0][0], corner[t][0]);
                    atomicAdd(&hist[t][1][0], corner[t][1]);
                    atomicAdd(&hist[t][0][M], corner[t][2]);
                    atomicAdd(&hist[t][1][M], corner[t][3]);
                }
            }
        }
        __syncthreads();
        const int bins = 2 * (M + 1);
        for (int r = tid; r < nt * bins; r += 256) {
            const int t = r / bins, b = r - t * bins, o = b / (M + 1), kk = b - o * (M + 1);
            counts[(((size_t)e * MAXT + t) * H + j) * bins + b] = hist[t][o][kk];
            hist[t][o][kk] = 0;
        }
        __syncthreads();
    }
}

__device__ __forceinline__ int wave_scan(int v, int lane) {             // inclusive, over the 64 lanes
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int n = __shfl_up(v, d);
        if (lane >= d) v += n;
    }
    return v;
}

// One workgroup per (e, t, scale, output row).  Dynamic LDS: 16 int64 of reduction scratch, 8 int32 of scan scratch, then the two
// int32 arrays [W] (k and o): column sums over the row window, turned in place into inclusive prefix sums.
constexpr int SCALE_LDS_HEAD = 16 * 8 + 8 * 4 + 96;                     // the arrays start at a multiple of 256 bytes
__global__ void __launch_bounds__(256) event_scale_kernel(const ScaleArgs a, const uint8_t* __restrict__ planes,
                                                          const int32_t* __restrict__ hx, long long* __restrict__ sums) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    long long* red = (long long*)smem;                                  // [4][3]
    int* wtot = (int*)(smem + 16 * 8);                                  // [4][2]
    const int W = a.W, H = a.H, M = a.M;
    int* pf = (int*)(smem + SCALE_LDS_HEAD);
    int* po = pf + W;
    const int j = blockIdx.x, s = blockIdx.y, et = blockIdx.z, e = et / MAXT, t = et - e * MAXT;
    if (t >= a.n_thr[e]) return;                                        // (the whole workgroup: before any barrier)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int hy = a.hy[s];                                             // (0 <= hy <= H: the caller's clamp)
    const int r0 = max(j - hy, 0), r1 = min(j + hy, H - 1);
    const int h = min(max(hx[(size_t)s * H + j], 0), (W - 1) / 2);     // a table entry beyond the clamp cannot lap the circle
    const size_t hw = (size_t)H * W;
    const uint8_t* pk = planes + (size_t)et * 2 * hw;
    for (int i = tid; i < W; i += 256) {
        int sf = 0, so = 0;
        for (int r = r0; r <= r1; ++r) {
            sf += pk[(size_t)r * W + i];
            so += pk[hw + (size_t)r * W + i];
        }
        pf[i] = sf;
        po[i] = so;
    }
    __syncthreads();
    // prefix scan: thread t owns the columns [t L, (t + 1) L)
    const int L = (W + 255) / 256, c0 = min(tid * L, W), c1 = min(c0 + L, W);
    int tf = 0, to = 0;
    for (int i = c0; i < c1; ++i) { tf += pf[i]; to += po[i]; }
    const int inf = wave_scan(tf, lane), ino = wave_scan(to, lane);
    if (lane == 63) { wtot[2 * wave] = inf; wtot[2 * wave + 1] = ino; }
    __syncthreads();
    int bf = inf - tf, bo = ino - to;                                   // exclusive over the threads before this one
    for (int w = 0; w < wave; ++w) { bf += wtot[2 * w]; bo += wtot[2 * w + 1]; }
    for (int i = c0; i < c1; ++i) {
        bf += pf[i]; pf[i] = bf;
        bo += po[i]; po[i] = bo;
    }
    __syncthreads();
    const int totf = pf[W - 1], toto = po[W - 1];
    long long q0 = 0, q1 = 0, q2 = 0;
    for (int i = tid; i < W; i += 256) {
        const int lo = i - h, hi = i + h;                               // 2 h + 1 <= W: at most one end leaves [0, W)
        int sf, so;
        if (lo < 0) {                                                   // columns lo + W .. W - 1 and 0 .. hi
            sf = pf[hi] + totf - pf[lo + W - 1];
            so = po[hi] + toto - po[lo + W - 1];
        } else if (hi >= W) {                                           // columns lo .. W - 1 and 0 .. hi - W
            sf = pf[hi - W] + totf - (lo > 0 ? pf[lo - 1] : 0);
            so = po[hi - W] + toto - (lo > 0 ? po[lo - 1] : 0);
        } else {
            sf = pf[hi] - (lo > 0 ? pf[lo - 1] : 0);
            so = po[hi] - (lo > 0 ? po[lo - 1] : 0);
        }
        const long long f = sf, g = (long long)M * so, d = f - g;
        q0 += d * d;
        q1 += f * f;
        q2 += g * g;
    }
    q0 = wave_sum(q0); q1 = wave_sum(q1); q2 = wave_sum(q2);
    if (lane == 0) { red[3 * wave] = q0; red[3 * wave + 1] = q1; red[3 * wave + 2] = q2; }
    __syncthreads();
    if (tid < 3) {
        long long* out = sums + (((size_t)et * a.n_scales + s) * H + j) * 3;
        out[tid] = red[tid] + red[3 + tid] + red[6 + tid] + red[9 + tid];
    }
}

bool valid_shape(int n_events, int H, int W, int n_scales) {
    return n_events >= 0 && n_events <= SKEVENT_MAX_CHANNELS && H >= 1 && W >= 1 && n_scales >= 0 && n_scales <= SKEVENT_MAX_SCALES &&
           (n_scales == 0 || W <= SKEVENT_MAX_WIDTH);
}

}  // namespace

extern "C" int skevent_abi_version(void) { return SKEVENT_ABI_VERSION; }

extern "C" size_t skevent_workspace_bytes(int n_events, int H, int W, int n_scales) {
    if (!valid_shape(n_events, H, W, n_scales) || n_scales == 0) return 0;
    return (size_t)n_events * MAXT * 2 * (size_t)H * (size_t)W;
}

extern "C" int skevent_run(const skevent_desc* d, void* stream) {
    if (!d || !d->members || !d->truth || !d->counts || d->C < 1 || d->M < 1 || d->M > SKEVENT_MAX_MEMBERS) return SKEVENT_E_ARG;
    if (!valid_shape(d->n_events, d->H, d->W, d->n_scales)) return SKEVENT_E_ARG;
    if (d->member_align != 4 && d->member_align != 16) return SKEVENT_E_ARG;
    if (((uintptr_t)d->truth & 3) || ((uintptr_t)d->counts & 3)) return SKEVENT_E_ARG;
    if ((size_t)d->C * (size_t)d->H > (1ull << 30) / (size_t)d->W) return SKEVENT_E_ARG;            // 32-bit byte offsets in the kernel
    CountArgs a = {};
    ScaleArgs sa = {};
    for (int e = 0; e < d->n_events; ++e) {
        if (d->channel[e] < 0 || d->channel[e] >= d->C || d->n_thr[e] < 1 || d->n_thr[e] > MAXT) return SKEVENT_E_ARG;
        a.channel[e] = d->channel[e];
        a.n_thr[e] = sa.n_thr[e] = d->n_thr[e];
        for (int t = 0; t < d->n_thr[e]; ++t) {
            if (d->thr[e][t] != d->thr[e][t]) return SKEVENT_E_ARG;                                  // a NaN threshold
            a.thr[e][t] = d->thr[e][t];
        }
    }
    const int S = d->n_scales;
    if (S > 0) {
        if (!d->hx || ((uintptr_t)d->hx & 3) || !d->sums || ((uintptr_t)d->sums & 7)) return SKEVENT_E_ARG;
        if (!d->workspace || ((uintptr_t)d->workspace & 15) || d->workspace_bytes < skevent_workspace_bytes(d->n_events, d->H, d->W, S))
            return SKEVENT_E_ARG;
        int hy_max = 0;
        for (int s = 0; s < S; ++s) {
            if (d->hy[s] < 0) return SKEVENT_E_ARG;
            hy_max = d->hy[s] > hy_max ? d->hy[s] : hy_max;
            sa.hy[s] = d->hy[s] < d->H ? d->hy[s] : d->H;                                            // (the same window: rows end at the grid)
        }
        // W (M (2 hy_max + 1) W)^2 < 2^63: the largest window sum fits an int32, the row sums of its squares an int64
        const unsigned __int128 n = (unsigned __int128)d->M * (2ull * (unsigned)hy_max + 1) * (unsigned)d->W;
        if (n >= ((unsigned __int128)1 << 31) || (unsigned __int128)d->W * n * n >= ((unsigned __int128)1 << 63)) return SKEVENT_E_ARG;
    }
    if (d->n_events == 0) return 0;
    a.M = sa.M = d->M; a.H = sa.H = d->H; a.W = sa.W = d->W; a.n_events = d->n_events; a.planes = S > 0; sa.n_scales = S;
    hipStream_t st = (hipStream_t)stream;
    // 256 CUs x 8 workgroups; a workgroup walks the (event, row) units with the grid's stride
    const size_t units = (size_t)d->n_events * d->H;
    const unsigned blocks = (unsigned)(units < 2048 ? units : 2048);
    uint8_t* planes = S > 0 ? (uint8_t*)d->workspace : nullptr;
    if (d->member_align == 16 && ((uintptr_t)d->truth & 15) == 0 && d->W % 4 == 0)                   // every row starts on a vector boundary
        hipLaunchKernelGGL(event_count_kernel<4>, dim3(blocks), dim3(256), 0, st, a, d->members, d->truth, d->counts, planes);
    else
        hipLaunchKernelGGL(event_count_kernel<1>, dim3(blocks), dim3(256), 0, st, a, d->members, d->truth, d->counts, planes);
    if (hipGetLastError() != hipSuccess) return SKEVENT_E_HIP;
    if (S > 0) {
        const size_t lds = SCALE_LDS_HEAD + 2 * (size_t)d->W * sizeof(int);
        if (lds > 65536 && hipFuncSetAttribute(reinterpret_cast<const void*>(event_scale_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                               (int)lds) != hipSuccess)
            return SKEVENT_E_HIP;
        hipLaunchKernelGGL(event_scale_kernel, dim3((unsigned)d->H, (unsigned)S, (unsigned)d->n_events * MAXT), dim3(256), lds, st, sa,
                           (const uint8_t*)planes, d->hx, (long long*)d->sums);
        if (hipGetLastError() != hipSuccess) return SKEVENT_E_HIP;
    }
    return 0;
}
