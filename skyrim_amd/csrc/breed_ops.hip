// The two device passes of a breeding cycle (include/skyrim_breed.h).
//   norms_kernel<VEC>  a one-wave workgroup walks tiles of 256 points of one row of one channel: a lane keeps its four y_0 values while it
//                      walks the member table (wave-uniform pointers, eight members' loads in flight) and adds w_j times the four exact
//                      squares to the lane's float64 accumulator of that member in LDS; lane m then sums member m's 64 accumulators
//   fold_kernel        sums the workgroups' partials of an entry in ascending order
//   apply_kernel<VEC>  out_m = x_0 + f[m][c] (y_m - y_0) for all members: x_0 and y_0 stay in registers across the members
// VEC: four floats per load and store (every pointer 16-byte aligned, rows / planes a multiple of four); the scalar path gives the same
// bits.  Contraction to fma is off for the whole file (and on the build line): the header fixes every rounding.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "../../include/skyrim_breed.h"
#include "fields.h"

#pragma clang fp contract(off)

namespace {

constexpr int WAVE = 64;
constexpr int TILE = SKBREED_TILE;
constexpr int STAGE = SKBREED_STAGE;
constexpr int PITCH = WAVE + 1;            // doubles of an accumulator row: lane m's final walk over a[m][.] is free of bank conflicts
constexpr int APPLY_LANES = 256;
constexpr int APPLY_POINTS = 4 * APPLY_LANES;
constexpr int FOLD_LANES = 256;

static_assert(TILE == 4 * WAVE, "a lane owns four points of a tile");
static_assert(SKBREED_MAX_MEMBERS <= WAVE, "lane m sums member m's accumulators");

struct NormsArgs {
    int M, C, W;
    int tiles_per_row, tiles, G;           // per channel
    uint32_t HW;
};

struct ApplyArgs {
    int M, C;
    uint32_t HW;
};

using namespace skfields;

// the lane's four points of a tile: elements e.x .. e.w of the state.  VEC: one 16-byte load at e.x (the four are consecutive)
template <bool VEC>
__device__ __forceinline__ f32x4 gather(const float* base, const uint32_t (&e)[4]) {
    if (VEC) return load_vec<4>(base, e[0]);
    f32x4 v;
    v.x = load_vec<1>(base, e[0]);
    v.y = load_vec<1>(base, e[1]);
    v.z = load_vec<1>(base, e[2]);
    v.w = load_vec<1>(base, e[3]);
    return v;
}

template <bool VEC>
__global__ void __launch_bounds__(WAVE) norms_kernel(const NormsArgs a, const float* __restrict__ y0, const float* const* __restrict__ members,
                                                      const double* __restrict__ lat_weight, double* __restrict__ partial) {
    extern __shared__ double acc[];                                        // [M][PITCH]
    const int lane = threadIdx.x;
    const int c = blockIdx.y;
    for (int m = 0; m < a.M; ++m) acc[m * PITCH + lane] = 0.0;
    const uint32_t plane = (uint32_t)c * a.HW;
    for (int t = blockIdx.x; t < a.tiles; t += a.G) {
        const int j = t / a.tiles_per_row, q = t - j * a.tiles_per_row;
        const int i0 = q * TILE + 4 * lane;                                // the lane's first column
        const uint32_t row = plane + (uint32_t)j * (uint32_t)a.W;
        uint32_t e[4];
        bool live[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            live[k] = i0 + k < a.W;
            // a point past the row's end reads the row's last point (VEC: its last four) and counts as d = 0
            e[k] = row + (uint32_t)(live[k] ? i0 + k : (VEC ? a.W - 4 + k : a.W - 1));
        }
        const f32x4 c0 = gather<VEC>(y0, e);
        const double w = lat_weight[j];
        for (int m0 = 0; m0 < a.M; m0 += STAGE) {
            f32x4 v[STAGE];
#pragma unroll
            for (int g = 0; g < STAGE; ++g)                                // all loads of the group before the first use
                v[g] = gather<VEC>(members[min(m0 + g, a.M - 1)], e);      // (past the last member: that member again, not used)
#pragma unroll
            for (int g = 0; g < STAGE; ++g) {
                if (m0 + g < a.M) {                                        // wave-uniform
                    const float d0 = v[g].x - c0.x, d1 = v[g].y - c0.y, d2 = v[g].z - c0.z, d3 = v[g].w - c0.w;
                    const double s0 = live[0] ? (double)d0 : 0.0, s1 = live[1] ? (double)d1 : 0.0;
                    const double s2 = live[2] ? (double)d2 : 0.0, s3 = live[3] ? (double)d3 : 0.0;
                    const double p = ((s0 * s0 + s1 * s1) + s2 * s2) + s3 * s3;
                    double* slot = acc + (m0 + g) * PITCH + lane;
                    *slot = *slot + w * p;
                }
            }
        }
    }
    __syncthreads();
    if (lane < a.M) {
        const double* rowp = acc + lane * PITCH;
        double s = rowp[0];
        for (int l = 1; l < WAVE; ++l) s = s + rowp[l];
        partial[((size_t)blockIdx.x * (size_t)a.C + (size_t)c) * (size_t)a.M + lane] = s;
    }
}

// S[m][c] = the G partials [g][c][m] in ascending g
__global__ void __launch_bounds__(FOLD_LANES) fold_kernel(int M, int C, int G, const double* __restrict__ partial, double* __restrict__ S) {
    const int idx = blockIdx.x * FOLD_LANES + threadIdx.x;                 // = c M + m
    if (idx >= M * C) return;
    const size_t step = (size_t)M * (size_t)C;
    double s = partial[idx];
    for (int g = 1; g < G; ++g) s = s + partial[(size_t)g * step + idx];
    const int c = idx / M, m = idx - c * M;
    S[(size_t)m * C + c] = s;
}

template <bool VEC>
__global__ void __launch_bounds__(APPLY_LANES) apply_kernel(const ApplyArgs a, const float* __restrict__ x0, const float* __restrict__ y0,
                                                             const float* const* __restrict__ members, float* const* __restrict__ out,
                                                             const float* __restrict__ f) {
    const int c = blockIdx.y;
    const uint32_t first = blockIdx.x * APPLY_POINTS;                      // of this workgroup, inside the channel's plane
    uint32_t e[4];
    bool live[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        // VEC: four consecutive points (H W % 4 == 0: all live or none); otherwise points a workgroup's width apart, coalesced per load
        const uint32_t p = VEC ? first + 4 * threadIdx.x + k : first + k * APPLY_LANES + threadIdx.x;
        live[k] = p < a.HW;
        e[k] = (uint32_t)c * a.HW + (live[k] ? p : (VEC ? a.HW - 4 + k : a.HW - 1));      // past the end: a valid address, never stored
    }
    const f32x4 xa = gather<VEC>(x0, e), ya = gather<VEC>(y0, e);
    for (int m0 = 0; m0 < a.M; m0 += STAGE) {
        f32x4 v[STAGE];
#pragma unroll
        for (int g = 0; g < STAGE; ++g) v[g] = gather<VEC>(members[min(m0 + g, a.M - 1)], e);      // all loads of the group before the first use
#pragma unroll
        for (int g = 0; g < STAGE; ++g) {
            if (m0 + g < a.M) {                                            // wave-uniform
                const float fm = f[(m0 + g) * a.C + c];
                float* o = out[m0 + g];
                const bool copy = fm == 0.f;
                f32x4 r;
                r.x = copy ? xa.x : xa.x + fm * (v[g].x - ya.x);
                r.y = copy ? xa.y : xa.y + fm * (v[g].y - ya.y);
                r.z = copy ? xa.z : xa.z + fm * (v[g].z - ya.z);
                r.w = copy ? xa.w : xa.w + fm * (v[g].w - ya.w);
                if (VEC) {
                    if (live[0]) store_vec<4>(o, e[0], r);
                } else {
                    if (live[0]) store_vec<1>(o, e[0], r.x);
                    if (live[1]) store_vec<1>(o, e[1], r.y);
                    if (live[2]) store_vec<1>(o, e[2], r.z);
                    if (live[3]) store_vec<1>(o, e[3], r.w);
                }
            }
        }
    }
}

struct Plan {
    int tiles_per_row, tiles, G;
    size_t bytes;
};

bool sizes_ok(int M, int C, int H, int W) {
    if (M < 1 || M > SKBREED_MAX_MEMBERS || C < 1 || C > SKBREED_MAX_CHANNELS || H < 1 || W < 1) return false;
    const size_t lim = (size_t)1 << 30, HW = (size_t)H * (size_t)W;
    return HW <= lim && (size_t)C <= lim / HW;
}

// the part of the refusals that the queries share with skbreed_norms
bool plan(int M, int C, int H, int W, Plan* p) {
    if (!sizes_ok(M, C, H, W)) return false;
    const size_t tpr = ((size_t)W + TILE - 1) / TILE, tiles = tpr * (size_t)H;
    size_t G = (4096 + (size_t)C - 1) / (size_t)C;
    if (G > SKBREED_MAX_GROUPS) G = SKBREED_MAX_GROUPS;
    if (G > tiles) G = tiles;
    p->tiles_per_row = (int)tpr;
    p->tiles = (int)tiles;
    p->G = (int)G;
    p->bytes = G * (size_t)C * (size_t)M * sizeof(double);
    return true;
}

// NULL and 4-byte alignment of a host copy of a pointer table; *vec is cleared unless every pointer is 16-byte aligned
bool table_ok(const float* const* dev, const float* const* host, int M, bool* vec) {
    if (!dev || ((uintptr_t)dev & 7) || !host) return false;
    for (int m = 0; m < M; ++m) {
        if (!host[m] || ((uintptr_t)host[m] & 3)) return false;
        if ((uintptr_t)host[m] & 15) *vec = false;
    }
    return true;
}

bool state_ok(const float* p, bool* vec) {
    if (!p || ((uintptr_t)p & 3)) return false;
    if ((uintptr_t)p & 15) *vec = false;
    return true;
}

bool overlap(const void* a, const void* b, size_t bytes) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + bytes && y < x + bytes;
}

// every refusal of skbreed_norms: nothing here touches the GPU
bool valid(const skbreed_norms_desc* d, Plan* p, bool* vec) {
    if (!d || !plan(d->M, d->C, d->H, d->W, p)) return false;
    *vec = d->W % 4 == 0;
    if (!state_ok(d->y0, vec) || !table_ok(d->members, d->members_host, d->M, vec)) return false;
    if (!d->lat_weight || ((uintptr_t)d->lat_weight & 7) || !d->S || ((uintptr_t)d->S & 7)) return false;
    if (!d->workspace || ((uintptr_t)d->workspace & 7) || d->workspace_bytes < p->bytes) return false;
    return true;
}

// every refusal of skbreed_apply
bool valid(const skbreed_apply_desc* d, bool* vec) {
    if (!d || !sizes_ok(d->M, d->C, d->H, d->W)) return false;
    *vec = ((size_t)d->H * (size_t)d->W) % 4 == 0;
    if (!state_ok(d->x0, vec) || !state_ok(d->y0, vec) || !table_ok(d->members, d->members_host, d->M, vec)) return false;
    if (!table_ok((const float* const*)d->out, (const float* const*)d->out_host, d->M, vec)) return false;
    if (!d->f || ((uintptr_t)d->f & 3)) return false;
    const size_t bytes = (size_t)d->C * (size_t)d->H * (size_t)d->W * sizeof(float);
    for (int m = 0; m < d->M; ++m) {
        const float* o = d->out_host[m];
        if (overlap(o, d->x0, bytes) || overlap(o, d->y0, bytes)) return false;
        for (int k = 0; k < d->M; ++k) {
            if (k != m && (overlap(o, d->members_host[k], bytes) || overlap(o, d->out_host[k], bytes))) return false;
        }
        if (o != d->members_host[m] && overlap(o, d->members_host[m], bytes)) return false;      // in place, or apart
    }
    return true;
}

}  // namespace

extern "C" int skbreed_abi_version(void) { return SKBREED_ABI_VERSION; }

extern "C" int skbreed_groups(int C, int H, int W) {
    Plan p;
    return plan(1, C, H, W, &p) ? p.G : 0;
}

extern "C" size_t skbreed_workspace_bytes(int M, int C, int H, int W) {
    Plan p;
    return plan(M, C, H, W, &p) ? p.bytes : 0;
}

extern "C" int skbreed_norms(const skbreed_norms_desc* d, void* stream) {
    Plan p;
    bool vec;
    if (!valid(d, &p, &vec)) return SKBREED_E_ARG;
    hipStream_t s = (hipStream_t)stream;
    NormsArgs a = {};
    a.M = d->M; a.C = d->C; a.W = d->W; a.tiles_per_row = p.tiles_per_row; a.tiles = p.tiles; a.G = p.G;
    a.HW = (uint32_t)d->H * (uint32_t)d->W;
    double* partial = (double*)d->workspace;
    const dim3 grid((unsigned)p.G, (unsigned)d->C);
    const size_t lds = (size_t)d->M * PITCH * sizeof(double);
    if (vec)
        hipLaunchKernelGGL(norms_kernel<true>, grid, dim3(WAVE), lds, s, a, d->y0, d->members, d->lat_weight, partial);
    else
        hipLaunchKernelGGL(norms_kernel<false>, grid, dim3(WAVE), lds, s, a, d->y0, d->members, d->lat_weight, partial);
    if (hipGetLastError() != hipSuccess) return SKBREED_E_HIP;
    const int entries = d->M * d->C;
    hipLaunchKernelGGL(fold_kernel, dim3((unsigned)((entries + FOLD_LANES - 1) / FOLD_LANES)), dim3(FOLD_LANES), 0, s, d->M, d->C, p.G, partial, d->S);
    return hipGetLastError() == hipSuccess ? 0 : SKBREED_E_HIP;
}

extern "C" int skbreed_apply(const skbreed_apply_desc* d, void* stream) {
    bool vec;
    if (!valid(d, &vec)) return SKBREED_E_ARG;
    hipStream_t s = (hipStream_t)stream;
    ApplyArgs a = {};
    a.M = d->M; a.C = d->C; a.HW = (uint32_t)d->H * (uint32_t)d->W;
    const dim3 grid((a.HW + APPLY_POINTS - 1) / APPLY_POINTS, (unsigned)d->C);
    if (vec)
        hipLaunchKernelGGL(apply_kernel<true>, grid, dim3(APPLY_LANES), 0, s, a, d->x0, d->y0, d->members, d->out, d->f);
    else
        hipLaunchKernelGGL(apply_kernel<false>, grid, dim3(APPLY_LANES), 0, s, a, d->x0, d->y0, d->members, d->out, d->f);
    return hipGetLastError() == hipSuccess ? 0 : SKBREED_E_HIP;
}
