// Ensemble scenarios (include/skyrim_gram.h): the member Gram matrix on the fp32-input MFMA and the member-combination stream.
//   gram_kernel<NBLK>  a workgroup walks tiles of 256 region points of one row: its four waves stage the differences to member 0 through
//                      LDS as [member][point], each wave multiplies its quarter of the tile (one fp32 chain of at most 64 points) and folds
//                      the block, times the row's weight, into float64 accumulators that live across the workgroup's tiles
//   reduce_kernel      sums the workgroups' partials of an entry in a fixed two-level order and mirrors the upper triangle
//   combine_kernel<K>  K linear combinations of the members per point, the loads of eight members in flight
// (gram_kernel keeps sixteen members' loads in flight: a tile is a serial chain of load rounds, and fewer rounds are what shortens it)
// Contraction to fma is off for the whole file (and on the build line): the header fixes the order of the fp32 operations of the
// combination, and a float64 accumulation is a product and a sum.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "../../include/skyrim_gram.h"
#include "fields.h"

#pragma clang fp contract(off)

namespace {

constexpr int LANES = 256;                 // of a workgroup: four waves
constexpr int TILE = SKGRAM_TILE;
constexpr int PITCH = TILE + 1;            // words of an LDS row: member m at point p lies in bank (m + p) mod 32
constexpr int GROUP = 8;                   // members whose loads are in flight together in combine_kernel
constexpr int STAGE = 16;                  // ... and in gram_kernel's staging
constexpr int RCHUNK = 32;                 // partials one thread of reduce_kernel sums
constexpr int RENTRY = 16;                 // entries of a reduce_kernel workgroup
constexpr int BLOCK = 32 * 32;             // entries of one accumulator block

static_assert(TILE == LANES, "a lane stages one point of a tile");
static_assert(SKGRAM_CHAIN * 4 == TILE, "a wave's chain is a quarter tile");
static_assert(SKGRAM_MAX_MEMBERS == 64, "two operand halves of 32 members");
static_assert(RENTRY * (SKGRAM_GROUPS / RCHUNK) == LANES && SKGRAM_GROUPS % RCHUNK == 0, "a reduce workgroup is entries x chunks");

struct GramArgs {
    int M, Mp;                             // members; columns with the truth
    int W, j0, i0, ni;
    int tiles_per_row, tiles, G;           // per channel
    uint32_t plane[SKGRAM_MAX_CHANNELS];   // first element of the cc-th listed channel's plane
};

struct CombineArgs {
    int M, nc;
    uint32_t HW;
    uint32_t plane[SKGRAM_MAX_CHANNELS];
};

using namespace skfields;
typedef float f32x16 __attribute__((ext_vector_type(16)));

// acc += (double)c * w, entry by entry (a product and a sum, each rounded)
__device__ __forceinline__ void fold(double (&acc)[16], const f32x16& c, double w) {
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = acc[r] + (double)c[r] * w;
}

// the four waves' blocks added in the order 0, 1, 2, 3 through `red` (3 x BLOCK doubles) and stored by wave 0 as [row][col]
__device__ __forceinline__ void store_block(double (&acc)[16], double* red, double* dst, int wave, int lane) {
    if (wave > 0) {
#pragma unroll
        for (int r = 0; r < 16; ++r) red[(wave - 1) * BLOCK + r * 64 + lane] = acc[r];
    }
    __syncthreads();
    if (wave == 0) {
        const int col = lane & 31, half = lane >> 5;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            double s = acc[r];
            s = s + red[0 * BLOCK + r * 64 + lane];
            s = s + red[1 * BLOCK + r * 64 + lane];
            s = s + red[2 * BLOCK + r * 64 + lane];
            const int row = (r & 3) + 8 * (r >> 2) + 4 * half;             // the C/D map of the 32x32 MFMA
            dst[row * 32 + col] = s;
        }
    }
    __syncthreads();
}

template <int NBLK>
__global__ void __launch_bounds__(LANES) gram_kernel(const GramArgs a, const float* const* __restrict__ members, const float* __restrict__ truth,
                                                     const double* __restrict__ lat_weight, double* __restrict__ partial) {
    constexpr int ROWS = NBLK == 1 ? 32 : 64;
    __shared__ float lds[ROWS * PITCH];
    static_assert(sizeof(float) * ROWS * PITCH >= sizeof(double) * 3 * BLOCK, "the wave reduction reuses the tile's LDS");
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int pt = threadIdx.x;                                            // the point of the tile this lane stages
    const int mem = lane & 31, half = lane >> 5;                           // the operand this lane feeds
    const bool lo_ok = mem < a.Mp, hi_ok = 32 + mem < a.Mp;                // lanes of padding members feed 0
    const uint32_t plane = a.plane[blockIdx.y];
    const float* x0p = members[0];
    double d0[16] = {}, d1[16] = {}, d2[16] = {};
    for (int t = blockIdx.x; t < a.tiles; t += a.G) {
        const int r = t / a.tiles_per_row, q = t - r * a.tiles_per_row;
        const int j = a.j0 + r;
        const int n = min(TILE, a.ni - q * TILE);                          // points of this tile
        const bool live = pt < n;
        int col = a.i0 + q * TILE + pt;                                    // (i0 < W and q TILE + pt < ni <= W for a live lane)
        col = col >= a.W ? col - a.W : col;
        const uint32_t off = plane + (uint32_t)j * (uint32_t)a.W + (uint32_t)(live ? col : 0);
        const float x0 = live ? load_vec<1>(x0p, off) : 0.f;
        lds[pt] = x0 - x0;                                                 // d_0: exactly 0, not finite when x_0 is not
        for (int m0 = 1; m0 < a.Mp; m0 += STAGE) {
            float v[STAGE];
#pragma unroll
            for (int g = 0; g < STAGE; ++g) {                              // all loads of the group before the first use
                const int m = min(m0 + g, a.Mp - 1);                       // (past the last column: that column again, not stored)
                const float* x = m < a.M ? members[m] : truth;             // wave-uniform
                v[g] = live ? load_vec<1>(x, off) : x0;
            }
#pragma unroll
            for (int g = 0; g < STAGE; ++g)
                if (m0 + g < a.Mp) lds[(m0 + g) * PITCH + pt] = v[g] - x0; // a point past the tile's end: 0
        }
        __syncthreads();
        const int cnt = min(n - SKGRAM_CHAIN * wave, SKGRAM_CHAIN);        // this wave's points of the tile
        const int pairs = cnt > 0 ? (cnt + 1) >> 1 : 0;                    // (an odd end pairs with a stored 0)
        if (pairs > 0) {
            f32x16 c0 = {}, c1 = {}, c2 = {};
            const float* lo = lds + mem * PITCH + SKGRAM_CHAIN * wave + half;
            const float* hi = lo + 32 * PITCH;
            for (int p = 0; p < pairs; ++p) {
                const float va = lo[2 * p];
                const float fa = lo_ok ? va : 0.f;
                c0 = __builtin_amdgcn_mfma_f32_32x32x2f32(fa, fa, c0, 0, 0, 0);
                if (NBLK == 3) {
                    const float vb = hi[2 * p];
                    const float fb = hi_ok ? vb : 0.f;
                    c1 = __builtin_amdgcn_mfma_f32_32x32x2f32(fa, fb, c1, 0, 0, 0);     // rows: members 0..31, columns: members 32..63
                    c2 = __builtin_amdgcn_mfma_f32_32x32x2f32(fb, fb, c2, 0, 0, 0);
                }
            }
            const double w = lat_weight[j];
            fold(d0, c0, w);
            if (NBLK == 3) {
                fold(d1, c1, w);
                fold(d2, c2, w);
            }
        }
        __syncthreads();                                                   // before the next tile overwrites the LDS
    }
    double* red = reinterpret_cast<double*>(lds);
    double* dst = partial + ((size_t)blockIdx.y * (size_t)a.G + blockIdx.x) * (size_t)(NBLK * BLOCK);
    store_block(d0, red, dst, wave, lane);
    if (NBLK == 3) {
        store_block(d1, red, dst + BLOCK, wave, lane);
        store_block(d2, red, dst + 2 * BLOCK, wave, lane);
    }
}

// entry (m, n) of a channel is the sum of the G partials' entry (min, max): bitwise symmetric.  A workgroup takes RENTRY neighbouring
// entries; thread (chunk c, entry) sums the partials g = RCHUNK c .. RCHUNK c + RCHUNK - 1 in ascending order, eight loads in flight, and
// the chunk sums are added in ascending c.  The order depends on G alone.
__global__ void __launch_bounds__(LANES) reduce_kernel(int Mp, int G, int nblk, size_t out_stride, const double* __restrict__ partial,
                                                       double* __restrict__ out) {
    __shared__ double part[SKGRAM_GROUPS / RCHUNK][RENTRY];
    const double* src = partial + (size_t)blockIdx.y * (size_t)G * (size_t)(nblk * BLOCK);
    const int le = threadIdx.x % RENTRY, chunk = threadIdx.x / RENTRY;
    const int e = min((int)blockIdx.x * RENTRY + le, Mp * Mp - 1);         // (past the last entry: that entry again, not stored)
    const int m = e / Mp, n = e - m * Mp;
    const int r = min(m, n), c = max(m, n);
    const int idx = ((r >> 5) + (c >> 5)) * BLOCK + (r & 31) * 32 + (c & 31);           // blocks (lo, lo), (lo, hi), (hi, hi)
    const size_t step = (size_t)(nblk * BLOCK);
    const int g0 = chunk * RCHUNK, g1 = min(g0 + RCHUNK, G);
    double s = 0.0;
    for (int g = g0; g < g1; g += 8) {
        double v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = src[(size_t)min(g + k, g1 - 1) * step + idx];
#pragma unroll
        for (int k = 0; k < 8; ++k)
            if (g + k < g1) s = (g + k == g0) ? v[k] : s + v[k];
    }
    part[chunk][le] = s;
    __syncthreads();
    if (chunk == 0 && (int)blockIdx.x * RENTRY + le < Mp * Mp) {
        double t = part[0][le];
        const int chunks = (G + RCHUNK - 1) / RCHUNK;
        for (int k = 1; k < chunks; ++k) t = t + part[k][le];
        out[(size_t)blockIdx.y * out_stride + e] = t;
    }
}

template <int K>
__global__ void __launch_bounds__(LANES) combine_kernel(const CombineArgs a, const float* const* __restrict__ members, const float* __restrict__ coef,
                                                        const float* __restrict__ b, float* __restrict__ out) {
    const uint32_t p = blockIdx.x * LANES + threadIdx.x;
    if (p >= a.HW) return;                                                 // (no barrier below)
    const uint32_t off = a.plane[blockIdx.y] + p;                          // member and channel are uniform
    const float x0 = load_vec<1>(members[0], off);
    float acc[K];
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] = b[k] * x0;
    for (int m0 = 1; m0 < a.M; m0 += GROUP) {
        float v[GROUP];
#pragma unroll
        for (int g = 0; g < GROUP; ++g) v[g] = load_vec<1>(members[min(m0 + g, a.M - 1)], off);      // all loads of the group before the first use
#pragma unroll
        for (int g = 0; g < GROUP; ++g) {
            if (m0 + g < a.M) {
                const float d = v[g] - x0;
#pragma unroll
                for (int k = 0; k < K; ++k) acc[k] = acc[k] + coef[k * a.M + m0 + g] * d;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < K; ++k) out[((size_t)k * (size_t)a.nc + blockIdx.y) * (size_t)a.HW + p] = acc[k];      // coalesced over p
}

struct Plan {
    int Mp, nblk, tiles_per_row, tiles, G;
    size_t bytes;
};

// the part of the refusals that skgram_workspace_bytes shares with skgram_run
bool plan(int Mp, int nc, int nj, int ni, Plan* p) {
    if (Mp < 2 || Mp > SKGRAM_MAX_MEMBERS || nc < 1 || nc > SKGRAM_MAX_CHANNELS || nj < 1 || ni < 1) return false;
    const size_t tpr = ((size_t)ni + TILE - 1) / TILE, tiles = tpr * (size_t)nj;
    if (tiles > ((size_t)1 << 21)) return false;
    p->Mp = Mp;
    p->nblk = Mp <= 32 ? 1 : 3;
    p->tiles_per_row = (int)tpr;
    p->tiles = (int)tiles;
    p->G = (int)(tiles < SKGRAM_GROUPS ? tiles : SKGRAM_GROUPS);
    p->bytes = (size_t)nc * (size_t)p->G * (size_t)(p->nblk * BLOCK) * sizeof(double);
    return true;
}

bool states_ok(const float* const* members, int M, int C, int H, int W, int nc, const int32_t* channels) {
    if (!members || ((uintptr_t)members & 7) || M < 2 || M > SKGRAM_MAX_MEMBERS) return false;
    if (C < 1 || H < 1 || W < 1 || nc < 1 || nc > SKGRAM_MAX_CHANNELS) return false;
    const size_t lim = (size_t)1 << 30, HW = (size_t)H * (size_t)W;
    if (HW > lim || (size_t)C > lim / HW) return false;
    for (int k = 0; k < nc; ++k)
        if (channels[k] < 0 || channels[k] >= C) return false;
    return true;
}

// every refusal of skgram_run: nothing here touches the GPU
bool valid(const skgram_desc* d, Plan* p) {
    if (!d || !states_ok(d->members, d->M, d->C, d->H, d->W, d->nc, d->channels)) return false;
    if (d->truth && ((uintptr_t)d->truth & 3)) return false;
    if (d->j0 < 0 || d->nj < 1 || d->nj > d->H || d->j0 > d->H - d->nj) return false;
    if (d->i0 < 0 || d->i0 >= d->W || d->ni < 1 || d->ni > d->W) return false;
    if (!d->lat_weight || ((uintptr_t)d->lat_weight & 7) || !d->out || ((uintptr_t)d->out & 7)) return false;
    if (!plan(d->M + (d->truth ? 1 : 0), d->nc, d->nj, d->ni, p)) return false;
    if (d->out_stride < (size_t)(p->Mp * p->Mp)) return false;
    if (!d->workspace || ((uintptr_t)d->workspace & 7) || d->workspace_bytes < p->bytes) return false;
    return true;
}

bool valid(const skgram_combine_desc* d) {
    if (!d || !states_ok(d->members, d->M, d->C, d->H, d->W, d->nc, d->channels)) return false;
    if (d->K < 1 || d->K > SKGRAM_MAX_OUT) return false;
    if (!d->coef || ((uintptr_t)d->coef & 3) || !d->b || ((uintptr_t)d->b & 3) || !d->out || ((uintptr_t)d->out & 3)) return false;
    const size_t lim = (size_t)1 << 30, HW = (size_t)d->H * (size_t)d->W;
    if ((size_t)d->K * (size_t)d->nc > lim / HW) return false;
    return true;
}

template <int K>
void launch_combine(const CombineArgs& a, const skgram_combine_desc* d, hipStream_t s) {
    const dim3 grid((a.HW + LANES - 1) / LANES, (unsigned)d->nc);
    hipLaunchKernelGGL(combine_kernel<K>, grid, dim3(LANES), 0, s, a, d->members, d->coef, d->b, d->out);
}

}  // namespace

extern "C" int skgram_abi_version(void) { return SKGRAM_ABI_VERSION; }

extern "C" size_t skgram_workspace_bytes(int Mp, int nc, int nj, int ni) {
    Plan p;
    return plan(Mp, nc, nj, ni, &p) ? p.bytes : 0;
}

extern "C" int skgram_run(const skgram_desc* d, void* stream) {
    Plan p;
    if (!valid(d, &p)) return SKGRAM_E_ARG;
    hipStream_t s = (hipStream_t)stream;
    GramArgs a = {};
    a.M = d->M; a.Mp = p.Mp; a.W = d->W; a.j0 = d->j0; a.i0 = d->i0; a.ni = d->ni;
    a.tiles_per_row = p.tiles_per_row; a.tiles = p.tiles; a.G = p.G;
    for (int k = 0; k < d->nc; ++k) a.plane[k] = (uint32_t)d->channels[k] * (uint32_t)d->H * (uint32_t)d->W;
    double* partial = (double*)d->workspace;
    const dim3 grid((unsigned)p.G, (unsigned)d->nc);
    if (p.nblk == 1)
        hipLaunchKernelGGL(gram_kernel<1>, grid, dim3(LANES), 0, s, a, d->members, d->truth, d->lat_weight, partial);
    else
        hipLaunchKernelGGL(gram_kernel<3>, grid, dim3(LANES), 0, s, a, d->members, d->truth, d->lat_weight, partial);
    if (hipGetLastError() != hipSuccess) return SKGRAM_E_HIP;
    const dim3 rgrid((unsigned)((p.Mp * p.Mp + RENTRY - 1) / RENTRY), (unsigned)d->nc);
    hipLaunchKernelGGL(reduce_kernel, rgrid, dim3(LANES), 0, s, p.Mp, p.G, p.nblk, d->out_stride, partial, d->out);
    return hipGetLastError() == hipSuccess ? 0 : SKGRAM_E_HIP;
}

extern "C" int skgram_combine(const skgram_combine_desc* d, void* stream) {
    if (!valid(d)) return SKGRAM_E_ARG;
    hipStream_t s = (hipStream_t)stream;
    CombineArgs a = {};
    a.M = d->M; a.nc = d->nc; a.HW = (uint32_t)d->H * (uint32_t)d->W;
    for (int k = 0; k < d->nc; ++k) a.plane[k] = (uint32_t)d->channels[k] * a.HW;
    switch (d->K) {
        case 1: launch_combine<1>(a, d, s); break;
        case 2: launch_combine<2>(a, d, s); break;
        case 3: launch_combine<3>(a, d, s); break;
        case 4: launch_combine<4>(a, d, s); break;
        case 5: launch_combine<5>(a, d, s); break;
        case 6: launch_combine<6>(a, d, s); break;
        case 7: launch_combine<7>(a, d, s); break;
        default: launch_combine<8>(a, d, s); break;
    }
    return hipGetLastError() == hipSuccess ? 0 : SKGRAM_E_HIP;
}
