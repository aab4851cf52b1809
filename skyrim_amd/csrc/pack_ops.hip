// Packed member archives (include/skyrim_pack.h): four streaming kernels.  range_partials: a workgroup reduces a tile of a plane to one
// (lo, hi, n_bad); range_table: a wave reduces the partials of a plane and writes its record.  quantize_kernel: a lane turns 8 values
// into 16 bytes of big-endian codes; unpack_kernel is its mirror.  Member, channel and tile of a unit come from the block index, so the
// member pointer, the plane offset and the table record are scalar loads.  Contraction to fma is off for the whole file (and on the build
// line): the header fixes every rounding.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include "../../include/skyrim_pack.h"
#include "fields.h"

#pragma clang fp contract(off)

namespace {

using namespace skfields;

constexpr int LANES = 256;
constexpr uint32_t RANGE_TILE = SKPACK_RANGE_TILE;   // values per unit of range_partials: 16 float4 per lane
constexpr uint32_t CODE_TILE = 8192;                 // values per unit of quantize_kernel and unpack_kernel: 4 groups of 8 per lane
constexpr uint32_t MAX_BLOCKS = 2048;                // 256 CUs x 8 workgroups; the units beyond are taken grid-stride

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

struct Planes {
    uint32_t first[SKPACK_MAX_CHANNELS];             // first element of the k-th listed channel's plane in a member state
};

__device__ __forceinline__ bool finite(float v) { return fabsf(v) < __builtin_inff(); }

// ---- the range of a plane --------------------------------------------------------------------------------------------------------------- //
struct Range {
    float lo, hi;
    int bad;
    __device__ __forceinline__ void take(float v) {
        const bool f = finite(v);
        lo = (f && v < lo) ? v : lo;
        hi = (f && v > hi) ? v : hi;
        bad += f ? 0 : 1;
    }
    __device__ __forceinline__ void join(float l, float h, int b) {
        lo = l < lo ? l : lo;
        hi = h > hi ? h : hi;
        bad += b;
    }
    __device__ __forceinline__ void over_wave() {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) join(__shfl_xor(lo, off), __shfl_xor(hi, off), __shfl_xor(bad, off));
    }
};

// unit u = (plane, tile), plane = m nc + k: values [tile RANGE_TILE, ...) of listed channel k of member m -> plo[u], phi[u], pbad[u]
__global__ void __launch_bounds__(LANES) range_partials(const float* const* __restrict__ members, const Planes planes, uint32_t nc, uint32_t HW,
                                                        uint32_t tiles, uint32_t units, float* __restrict__ plo, float* __restrict__ phi,
                                                        int32_t* __restrict__ pbad) {
    __shared__ float s_lo[LANES / 64], s_hi[LANES / 64];
    __shared__ int s_bad[LANES / 64];
    const uint32_t tid = threadIdx.x;
    for (uint32_t u = blockIdx.x; u < units; u += gridDim.x) {
        const uint32_t plane = u / tiles, t = u - plane * tiles, m = plane / nc, k = plane - m * nc;
        const float* base = members[m];
        const uint32_t first = planes.first[k] + t * RANGE_TILE;
        const uint32_t n = HW - t * RANGE_TILE < RANGE_TILE ? HW - t * RANGE_TILE : RANGE_TILE;
        // the values before the first 16-byte aligned address, the aligned body as float4, the values behind it
        uint32_t head = (uint32_t)(0u - ((uint32_t)((uintptr_t)base >> 2) + first)) & 3u;
        head = head < n ? head : n;
        const uint32_t nv = (n - head) >> 2, tail = head + 4u * nv;
        Range r = {__builtin_inff(), -__builtin_inff(), 0};
        if (tid < head) r.take(load_vec<1>(base, first + tid));
#pragma unroll 4
        for (uint32_t g = tid; g < nv; g += LANES) {
            const f32x4 v = load_vec<4>(base, first + head + 4u * g);
            r.take(v[0]); r.take(v[1]); r.take(v[2]); r.take(v[3]);
        }
        if (tid < n - tail) r.take(load_vec<1>(base, first + tail + tid));
        r.over_wave();
        if ((tid & 63u) == 0) { s_lo[tid >> 6] = r.lo; s_hi[tid >> 6] = r.hi; s_bad[tid >> 6] = r.bad; }
        __syncthreads();
        if (tid == 0) {
#pragma unroll
            for (int w = 1; w < LANES / 64; ++w) r.join(s_lo[w], s_hi[w], s_bad[w]);
            plo[u] = r.lo; phi[u] = r.hi; pbad[u] = r.bad;
        }
        __syncthreads();                                                    // the next unit writes the same LDS words
    }
}

// one wave per plane: its `tiles` partials -> its record
__global__ void __launch_bounds__(64) range_table(const float* plo, const float* phi, const int32_t* pbad, uint32_t tiles, skpack_entry* table) {
    const uint32_t plane = blockIdx.x, lane = threadIdx.x;
    Range r = {__builtin_inff(), -__builtin_inff(), 0};
    for (uint32_t t = lane; t < tiles; t += 64) r.join(plo[plane * tiles + t], phi[plane * tiles + t], pbad[plane * tiles + t]);
    r.over_wave();
    if (lane != 0) return;
    skpack_entry e;
    e.n_bad = r.bad; e.pad = 0;
    if (!(r.lo <= r.hi)) {                                                  // no finite value
        e.lo = 0.f; e.hi = 0.f; e.offset = 0.0; e.scale = 1.0; e.inv = 1.0;
    } else {
        e.lo = r.lo + 0.0f; e.hi = r.hi + 0.0f;                             // -0 is +0
        const double lo = (double)e.lo, hi = (double)e.hi, d = hi - lo;
        e.offset = 0.5 * lo + 0.5 * hi;
        e.scale = d == 0.0 ? 1.0 : d / 65534.0;
        e.inv = d == 0.0 ? 1.0 : 65534.0 / d;
    }
    table[plane] = e;
}

// ---- codes ------------------------------------------------------------------------------------------------------------------------------ //
// the big-endian code of x as the 16 bits a little-endian store puts into memory
__device__ __forceinline__ uint32_t code_of(float x, double offset, double inv) {
    double q = rint(((double)x - offset) * inv);
    q = q < -32767.0 ? -32767.0 : q;
    q = q > 32767.0 ? 32767.0 : q;
    const int c = finite(x) ? (int)q : SKPACK_FILL;
    return (((uint32_t)c & 0xFFu) << 8) | (((uint32_t)c >> 8) & 0xFFu);
}

__device__ __forceinline__ float value_of(uint32_t be16, double scale, double offset) {
    const int c = (int)(int16_t)(uint16_t)(((be16 & 0xFFu) << 8) | ((be16 >> 8) & 0xFFu));
    const float v = (float)((double)c * scale + offset);
    return c == SKPACK_FILL ? __uint_as_float(0x7FC00000u) : v;
}

__device__ __forceinline__ void store_u16(void* base, uint32_t byte_off, uint32_t v) {
    *(SK_GLOBAL uint16_t*)((SK_GLOBAL char*)base + byte_off) = (uint16_t)v;
}
__device__ __forceinline__ uint32_t load_u16(const void* base, uint32_t byte_off) {
    return *(const SK_GLOBAL uint16_t*)((const SK_GLOBAL char*)base + byte_off);
}

// unit u = (m, k, tile): values [tile CODE_TILE, ...) of listed channel k of member m -> codes [k HW + tile CODE_TILE, ...) of member m's image
__global__ void __launch_bounds__(LANES) quantize_kernel(const float* const* __restrict__ members, const Planes planes, uint32_t nc, uint32_t HW,
                                                         uint32_t tiles, uint32_t units, const skpack_entry* __restrict__ table,
                                                         char* __restrict__ out, size_t stride) {
    const uint32_t tid = threadIdx.x;
    for (uint32_t u = blockIdx.x; u < units; u += gridDim.x) {
        const uint32_t plane = u / tiles, t = u - plane * tiles, m = plane / nc, k = plane - m * nc;
        const float* base = members[m];
        const double offset = table[plane].offset, inv = table[plane].inv;
        char* img = out + (size_t)m * stride;
        const uint32_t in0 = planes.first[k] + t * CODE_TILE, out0 = k * HW + t * CODE_TILE;       // elements; codes of the image
        const uint32_t n = HW - t * CODE_TILE < CODE_TILE ? HW - t * CODE_TILE : CODE_TILE;
        // the codes before the first 16-byte aligned address of the image, the aligned body in groups of 8, the codes behind it
        uint32_t head = (uint32_t)(0u - ((uint32_t)((uintptr_t)img >> 1) + out0)) & 7u;
        head = head < n ? head : n;
        const uint32_t ng = (n - head) >> 3, tail = head + 8u * ng;
        if (tid < head) store_u16(img, 2u * (out0 + tid), code_of(load_vec<1>(base, in0 + tid), offset, inv));
        const bool wide = (((uint32_t)((uintptr_t)base >> 2) + in0 + head) & 3u) == 0;              // the body's reads are 16-byte aligned
        for (uint32_t g = tid; g < ng; g += LANES) {
            const uint32_t e = head + 8u * g;
            float x[8];
            if (wide) {
                const f32x4 a = load_vec<4>(base, in0 + e), b = load_vec<4>(base, in0 + e + 4u);
                x[0] = a[0]; x[1] = a[1]; x[2] = a[2]; x[3] = a[3]; x[4] = b[0]; x[5] = b[1]; x[6] = b[2]; x[7] = b[3];
            } else {
#pragma unroll
                for (int j = 0; j < 8; ++j) x[j] = load_vec<1>(base, in0 + e + (uint32_t)j);
            }
            u32x4 w;
#pragma unroll
            for (int j = 0; j < 4; ++j) w[j] = code_of(x[2 * j], offset, inv) | (code_of(x[2 * j + 1], offset, inv) << 16);
            *(SK_GLOBAL u32x4*)((SK_GLOBAL char*)img + 2u * (out0 + e)) = w;
        }
        if (tid < n - tail) store_u16(img, 2u * (out0 + tail + tid), code_of(load_vec<1>(base, in0 + tail + tid), offset, inv));
    }
}

// unit u = (k, tile): codes [k HW + tile CODE_TILE, ...) of the image -> the same elements of out
__global__ void __launch_bounds__(LANES) unpack_kernel(const char* __restrict__ codes, const skpack_entry* __restrict__ table, uint32_t HW,
                                                       uint32_t tiles, uint32_t units, float* __restrict__ out) {
    const uint32_t tid = threadIdx.x;
    for (uint32_t u = blockIdx.x; u < units; u += gridDim.x) {
        const uint32_t k = u / tiles, t = u - k * tiles;
        const double scale = table[k].scale, offset = table[k].offset;
        const uint32_t at = k * HW + t * CODE_TILE;
        const uint32_t n = HW - t * CODE_TILE < CODE_TILE ? HW - t * CODE_TILE : CODE_TILE;
        uint32_t head = (uint32_t)(0u - ((uint32_t)((uintptr_t)codes >> 1) + at)) & 7u;             // codes before the first 16-byte aligned one
        head = head < n ? head : n;
        const uint32_t ng = (n - head) >> 3, tail = head + 8u * ng;
        if (tid < head) store_vec<1>(out, at + tid, value_of(load_u16(codes, 2u * (at + tid)), scale, offset));
        const bool wide = (((uint32_t)((uintptr_t)out >> 2) + at + head) & 3u) == 0;                // the body's writes are 16-byte aligned
        for (uint32_t g = tid; g < ng; g += LANES) {
            const uint32_t e = at + head + 8u * g;
            const u32x4 w = *(const SK_GLOBAL u32x4*)((const SK_GLOBAL char*)codes + 2u * e);
            float x[8];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                x[2 * j] = value_of(w[j] & 0xFFFFu, scale, offset);
                x[2 * j + 1] = value_of(w[j] >> 16, scale, offset);
            }
            if (wide) {
                store_vec<4>(out, e, f32x4{x[0], x[1], x[2], x[3]});
                store_vec<4>(out, e + 4u, f32x4{x[4], x[5], x[6], x[7]});
            } else {
#pragma unroll
                for (int j = 0; j < 8; ++j) store_vec<1>(out, e + (uint32_t)j, x[j]);
            }
        }
        if (tid < n - tail) store_vec<1>(out, at + tail + tid, value_of(load_u16(codes, 2u * (at + tail + tid)), scale, offset));
    }
}

// ---- the argument checks: nothing here touches the GPU ---------------------------------------------------------------------------------- //
// H W <= 2^30, C H W <= 2^30, nc H W <= 2^30
bool sizes_ok(int C, int H, int W, int nc) {
    if (C < 1 || H < 1 || W < 1 || nc < 1 || nc > SKPACK_MAX_CHANNELS) return false;
    const size_t lim = (size_t)1 << 30, HW = (size_t)H * (size_t)W;
    return HW <= lim && (size_t)C <= lim / HW && (size_t)nc <= lim / HW;
}

uint32_t tiles_of(size_t HW, uint32_t tile) { return (uint32_t)((HW + tile - 1) / tile); }

// what skpack_range and skpack_quantize share
bool valid_common(const skpack_desc* d) {
    if (!d || !d->members || ((uintptr_t)d->members & 7) || !d->table || ((uintptr_t)d->table & 7)) return false;
    if (d->M < 1 || d->M > SKPACK_MAX_MEMBERS || !sizes_ok(d->C, d->H, d->W, d->nc)) return false;
    for (int k = 0; k < d->nc; ++k)
        if (d->channels[k] < 0 || d->channels[k] >= d->C) return false;
    return true;
}

bool valid_range(const skpack_desc* d) {
    if (!valid_common(d)) return false;
    if (!d->workspace || ((uintptr_t)d->workspace & 3)) return false;
    return d->workspace_bytes >= skpack_workspace_bytes(d->M, d->nc, d->H, d->W);
}

bool valid_quantize(const skpack_desc* d) {
    if (!valid_common(d)) return false;
    if (!d->out || ((uintptr_t)d->out & 1) || (d->member_stride_bytes & 1)) return false;
    return d->member_stride_bytes >= 2 * (size_t)d->nc * (size_t)d->H * (size_t)d->W;
}

bool valid(const skpack_unpack_desc* d) {
    if (!d || !d->codes || ((uintptr_t)d->codes & 1) || !d->table || ((uintptr_t)d->table & 7) || !d->out || ((uintptr_t)d->out & 3)) return false;
    return sizes_ok(1, d->H, d->W, d->nc);
}

Planes planes_of(const skpack_desc* d) {
    Planes p = {};
    for (int k = 0; k < d->nc; ++k) p.first[k] = (uint32_t)d->channels[k] * (uint32_t)d->H * (uint32_t)d->W;
    return p;
}

uint32_t blocks_for(uint32_t units) { return units < MAX_BLOCKS ? units : MAX_BLOCKS; }

}  // namespace

extern "C" int skpack_abi_version(void) { return SKPACK_ABI_VERSION; }

extern "C" size_t skpack_workspace_bytes(int M, int nc, int H, int W) {
    if (M < 1 || M > SKPACK_MAX_MEMBERS || !sizes_ok(1, H, W, nc)) return 0;
    return (size_t)12 * (size_t)M * (size_t)nc * tiles_of((size_t)H * (size_t)W, RANGE_TILE);
}

extern "C" int skpack_range_check(const skpack_desc* d) { return valid_range(d) ? 0 : SKPACK_E_ARG; }
extern "C" int skpack_quantize_check(const skpack_desc* d) { return valid_quantize(d) ? 0 : SKPACK_E_ARG; }
extern "C" int skpack_unpack_check(const skpack_unpack_desc* d) { return valid(d) ? 0 : SKPACK_E_ARG; }

extern "C" int skpack_range(const skpack_desc* d, void* stream) {
    if (!valid_range(d)) return SKPACK_E_ARG;
    const uint32_t HW = (uint32_t)d->H * (uint32_t)d->W, tiles = tiles_of(HW, RANGE_TILE), np = (uint32_t)d->M * (uint32_t)d->nc;
    const uint32_t units = np * tiles;                                      // <= 2^10 2^8 2^16
    float* plo = (float*)d->workspace;
    float* phi = plo + units;
    int32_t* pbad = (int32_t*)(phi + units);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(range_partials, dim3(blocks_for(units)), dim3(LANES), 0, s, d->members, planes_of(d), (uint32_t)d->nc, HW, tiles, units,
                       plo, phi, pbad);
    hipLaunchKernelGGL(range_table, dim3(np), dim3(64), 0, s, plo, phi, pbad, tiles, d->table);
    return hipGetLastError() == hipSuccess ? 0 : SKPACK_E_HIP;
}

extern "C" int skpack_quantize(const skpack_desc* d, void* stream) {
    if (!valid_quantize(d)) return SKPACK_E_ARG;
    const uint32_t HW = (uint32_t)d->H * (uint32_t)d->W, tiles = tiles_of(HW, CODE_TILE);
    const uint32_t units = (uint32_t)d->M * (uint32_t)d->nc * tiles;        // <= 2^10 2^8 2^17 < 2^32 (H W <= 2^30)
    hipLaunchKernelGGL(quantize_kernel, dim3(blocks_for(units)), dim3(LANES), 0, (hipStream_t)stream, d->members, planes_of(d), (uint32_t)d->nc,
                       HW, tiles, units, (const skpack_entry*)d->table, (char*)d->out, d->member_stride_bytes);
    return hipGetLastError() == hipSuccess ? 0 : SKPACK_E_HIP;
}

extern "C" int skpack_unpack(const skpack_unpack_desc* d, void* stream) {
    if (!valid(d)) return SKPACK_E_ARG;
    const uint32_t HW = (uint32_t)d->H * (uint32_t)d->W, tiles = tiles_of(HW, CODE_TILE), units = (uint32_t)d->nc * tiles;
    hipLaunchKernelGGL(unpack_kernel, dim3(blocks_for(units)), dim3(LANES), 0, (hipStream_t)stream, (const char*)d->codes, d->table, HW, tiles,
                       units, d->out);
    return hipGetLastError() == hipSuccess ? 0 : SKPACK_E_HIP;
}
