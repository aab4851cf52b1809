// Regridding (include/skyrim_regrid.h): one streaming kernel over (member, channel, output row).  A workgroup sums the row taps of its
// output row column by column into an LDS strip (every global load coalesced), then a lane per output column takes its column taps from
// the strip.  Contraction to fma is off for the whole file (and on the build line): the header fixes the order of the fp32 operations.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include "../../include/skyrim_regrid.h"
#include "fields.h"

#pragma clang fp contract(off)

namespace {

constexpr int LANES = 256;       // of a workgroup
constexpr int TAPS = SKREGRID_MAX_TAPS;

struct Table { const int32_t* start; const int32_t* count; const float* weight; };
struct RegridArgs {
    int M, H, W, Ho, Wo, nc;
    Table rows, cols;
    size_t member_stride;
    int32_t channels[SKREGRID_MAX_CHANNELS];
};

using namespace skfields;

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

template <int VEC>
__device__ __forceinline__ void add_tap(Pts<VEC>& acc, float w, const Pts<VEC>& p) {
#pragma unroll
    for (int i = 0; i < VEC; ++i) {
        const float t = w * p.v[i];
        acc.v[i] = acc.v[i] + t;
    }
}

template <int VEC>
__global__ void __launch_bounds__(LANES) regrid_kernel(const RegridArgs a, const float* const* __restrict__ members, float* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) float strip[];          // v: W floats
    const uint32_t H = (uint32_t)a.H, W = (uint32_t)a.W, Ho = (uint32_t)a.Ho, Wo = (uint32_t)a.Wo;
    const uint64_t total = (uint64_t)a.M * (uint64_t)a.nc * Ho;
    for (uint64_t w = blockIdx.x; w < total; w += gridDim.x) {             // member, channel and row are uniform over the workgroup
        const uint32_t mk = (uint32_t)(w / Ho), J = (uint32_t)(w - (uint64_t)mk * Ho);
        const uint32_t m = mk / (uint32_t)a.nc, k = mk - m * (uint32_t)a.nc;
        const uint32_t row0 = (uint32_t)a.channels[k] * H;                 // first row of the channel's plane
        const float* x = members[m];
        // the vertical pass: no access depends on the table beyond these clamps
        const int rs = clampi(a.rows.start[J], 0, (int)H - 1), rn = clampi(a.rows.count[J], 1, TAPS);
        const float* rw = a.rows.weight + (size_t)J * TAPS;
        for (uint32_t i = threadIdx.x * VEC; i < W; i += LANES * VEC) {    // (vector path: W is a multiple of 4, so i < W covers i + 3)
            const Pts<VEC> p0 = load<VEC>(x, (row0 + (uint32_t)rs) * W + i);
            const float w0 = rw[0];
            Pts<VEC> acc;
#pragma unroll
            for (int e = 0; e < VEC; ++e) acc.v[e] = w0 * p0.v[e];
            int t = 1;
            for (; t + 4 <= rn; t += 4) {                                  // four rows in flight, summed in tap order
                const uint32_t r0 = min((uint32_t)(rs + t), H - 1), r1 = min((uint32_t)(rs + t + 1), H - 1);
                const uint32_t r2 = min((uint32_t)(rs + t + 2), H - 1), r3 = min((uint32_t)(rs + t + 3), H - 1);
                const Pts<VEC> q0 = load<VEC>(x, (row0 + r0) * W + i), q1 = load<VEC>(x, (row0 + r1) * W + i);
                const Pts<VEC> q2 = load<VEC>(x, (row0 + r2) * W + i), q3 = load<VEC>(x, (row0 + r3) * W + i);
                add_tap<VEC>(acc, rw[t], q0);
                add_tap<VEC>(acc, rw[t + 1], q1);
                add_tap<VEC>(acc, rw[t + 2], q2);
                add_tap<VEC>(acc, rw[t + 3], q3);
            }
            for (; t < rn; ++t) {
                const uint32_t r = min((uint32_t)(rs + t), H - 1);
                add_tap<VEC>(acc, rw[t], load<VEC>(x, (row0 + r) * W + i));
            }
            if constexpr (VEC == 4)
                *(f32x4*)(strip + i) = f32x4{acc.v[0], acc.v[1], acc.v[2], acc.v[3]};
            else
                strip[i] = acc.v[0];
        }
        __syncthreads();
        // the horizontal pass: a lane per output column, its weights four at a time
        float* y = out + (size_t)m * a.member_stride + ((size_t)k * Ho + J) * Wo;
        for (uint32_t I = threadIdx.x; I < Wo; I += LANES) {
            const int cn = clampi(a.cols.count[I], 1, TAPS);
            uint32_t c = (uint32_t)clampi(a.cols.start[I], 0, (int)W - 1);
            const f32x4* cw = (const f32x4*)(a.cols.weight + (size_t)I * TAPS);
            float acc = 0.f;
            auto tap = [&](float wt, bool first) {
                const float t = wt * strip[c];
                acc = first ? t : acc + t;
                c = c + 1 == W ? 0 : c + 1;
            };
            for (int g = 0; 4 * g < cn; ++g) {
                const f32x4 wv = cw[g];
                tap(wv.x, g == 0);
                if (4 * g + 1 < cn) tap(wv.y, false);
                if (4 * g + 2 < cn) tap(wv.z, false);
                if (4 * g + 3 < cn) tap(wv.w, false);
            }
            y[I] = acc;
        }
        __syncthreads();                                                   // the next row overwrites the strip
    }
}

bool table_ok(const skregrid_table& t) {
    return t.start && t.count && t.weight && !(((uintptr_t)t.start | (uintptr_t)t.count | (uintptr_t)t.weight) & 15);
}

// every refusal of skregrid_run: nothing here touches the GPU
bool valid(const skregrid_desc* d) {
    if (!d || !d->members || ((uintptr_t)d->members & 7) || !d->out || ((uintptr_t)d->out & 3)) return false;
    if (d->M < 1 || d->M > SKREGRID_MAX_MEMBERS || (d->member_align != 4 && d->member_align != 16)) return false;
    if (d->C < 1 || d->H < 2 || d->W < 4 || d->W > SKREGRID_MAX_W || d->Ho < 1 || d->Wo < 1) return false;
    if (d->nc < 1 || d->nc > SKREGRID_MAX_CHANNELS) return false;
    const size_t lim = (size_t)1 << 30, HW = (size_t)d->H * (size_t)d->W, HWo = (size_t)d->Ho * (size_t)d->Wo;
    if (HW > lim || (size_t)d->C > lim / HW || HWo > lim || (size_t)d->nc > lim / HWo) return false;
    if (d->member_stride < (size_t)d->nc * HWo) return false;
    for (int k = 0; k < d->nc; ++k)
        if (d->channels[k] < 0 || d->channels[k] >= d->C) return false;
    return table_ok(d->rows) && table_ok(d->cols);
}

}  // namespace

extern "C" int skregrid_abi_version(void) { return SKREGRID_ABI_VERSION; }

extern "C" int skregrid_validate(const int32_t* start, const int32_t* count, const float* weight, int n_out, int n_src, int periodic) {
    if (!start || !count || !weight || n_out < 1 || n_src < 1) return SKREGRID_E_ARG;
    for (int o = 0; o < n_out; ++o) {
        const int s = start[o], n = count[o];
        if (s < 0 || s >= n_src || n < 1 || n > SKREGRID_MAX_TAPS || n > n_src) return SKREGRID_E_ARG;
        if (!periodic && s + n > n_src) return SKREGRID_E_ARG;
        for (int t = 0; t < n; ++t) {
            const float w = weight[(size_t)o * SKREGRID_MAX_TAPS + t];
            if (!std::isfinite(w) || w == 0.f) return SKREGRID_E_ARG;
        }
    }
    return 0;
}

extern "C" int skregrid_run(const skregrid_desc* d, void* stream) {
    if (!valid(d)) return SKREGRID_E_ARG;
    hipStream_t s = (hipStream_t)stream;
    RegridArgs a = {};
    a.M = d->M; a.H = d->H; a.W = d->W; a.Ho = d->Ho; a.Wo = d->Wo; a.nc = d->nc;
    a.rows = Table{d->rows.start, d->rows.count, d->rows.weight};
    a.cols = Table{d->cols.start, d->cols.count, d->cols.weight};
    a.member_stride = d->member_stride;
    for (int k = 0; k < d->nc; ++k) a.channels[k] = d->channels[k];
    // 256 CUs x 8 workgroups of four waves at the most; a workgroup walks the (member, channel, row) triples with the grid's stride
    const uint64_t total = (uint64_t)d->M * (uint64_t)d->nc * (uint64_t)d->Ho;
    const unsigned blocks = (unsigned)(total < 2048 ? total : 2048);
    const size_t lds = ((size_t)d->W + 3) / 4 * 16;
    if (d->member_align == 16 && d->W % 4 == 0)
        hipLaunchKernelGGL(regrid_kernel<4>, dim3(blocks), dim3(LANES), lds, s, a, d->members, d->out);
    else
        hipLaunchKernelGGL(regrid_kernel<1>, dim3(blocks), dim3(LANES), lds, s, a, d->members, d->out);
    return hipGetLastError() == hipSuccess ? 0 : SKREGRID_E_HIP;
}
