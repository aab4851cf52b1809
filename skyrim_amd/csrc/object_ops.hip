// Weather objects (include/skyrim_object.h): connected-component labelling by union-find on parent indices -- a tile in LDS, then the
// tile borders in global memory, then a flatten pass -- the numbering of the qualifying roots in raster order, integer attribute sums
// and the probability gather.  The only atomics are integer min / max / add; a stream's kernel boundaries are the only barriers
// between workgroups.
#include <hip/hip_runtime.h>
#include <climits>
#include <cmath>
#include <cstdint>
#include "../../include/skyrim_object.h"
#include "fields.h"

namespace {

using namespace skfields;

constexpr int TH = 16, TW = 64, TILE = TH * TW;   // a tile row is one wave: 256-byte loads and stores
constexpr int CHUNK = 1024;                        // points per workgroup of the numbering passes
constexpr int MAX_CAPACITY = 1 << 20;

struct ObjArgs {
    int M, P, H, W, periodic, min_pixels, capacity, tiles_x;
    uint32_t N, nchunks;                           // N = H W
    skobj_plane planes[SKOBJ_MAX_PLANES];
};

typedef unsigned long long u64;

// ---- union-find on an array of parent + 1 (0: background).  Invariant: 1 <= L[x] <= x + 1 for a foreground x, L[x] == x + 1 at a root,
// and L[x] only ever decreases (atomicMin).  Reads that race with an atomicMin go through a relaxed atomic load: an older value is still a
// point of the same component at or below x, which is all the walks need.
__device__ __forceinline__ int parent_of(const int* L, int x) { return __hip_atomic_load(L + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - 1; }

__device__ __forceinline__ int find_root(const int* L, int x) {
    // terminates: the walk goes on only to a strictly lower index n, 0 <= n < x, so after at most x steps it stands on a root
    for (;;) {
        const int n = parent_of(L, x);
        if ((unsigned)n >= (unsigned)x) return x;
        x = n;
    }
}

__device__ __forceinline__ void unite(int* L, int a, int b) {
    // terminates: a pass ends the loop when the two roots are equal or when the atomicMin found the higher root `a` still a root and
    // hung it below `b`.  It retries only when the atomicMin returned old < a + 1 -- another atomicMin had already lowered L[a] -- and
    // then goes on from old - 1 < a (the link a -> old - 1 that the minimum may have replaced by a -> b is restored by joining old - 1
    // to b).  The higher of the two indices strictly decreases from retry to retry and is never negative.
    for (;;) {
        a = find_root(L, a);
        b = find_root(L, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(L + a, b + 1);
        if (old >= a + 1 || old <= 0) return;
        a = old - 1;
    }
}

__device__ __forceinline__ bool in_mask(float v, const skobj_plane& pl) { return pl.direction > 0 ? v >= pl.threshold : v <= pl.threshold; }

// kernel 1: one workgroup labels one tile in LDS and writes every point's parent (the tile's root of its component) as a global index.
// The raster order inside the tile is the raster order of the plane, so the tile's smallest index is the smallest global one.
__global__ void __launch_bounds__(256) obj_tile_kernel(const ObjArgs a, const float* const* __restrict__ members, int32_t* __restrict__ labels) {
    __shared__ int lab[TILE];
    const int mp = blockIdx.y, m = mp / a.P, p = mp - m * a.P;
    const skobj_plane pl = a.planes[p];
    const int ty = blockIdx.x / a.tiles_x, tx = blockIdx.x - ty * a.tiles_x;
    const int j0 = ty * TH, i0 = tx * TW;
    const float* x = members[m];
    const uint32_t chan = (uint32_t)pl.channel * a.N;
    const bool eight = pl.connectivity == 8;
    bool fg[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int t = threadIdx.x + 256 * e, j = j0 + (t >> 6), i = i0 + (t & 63);
        bool f = false;
        if (j < a.H && i < a.W) f = in_mask(load_vec<1>(x, chan + (uint32_t)j * (uint32_t)a.W + (uint32_t)i), pl);
        fg[e] = f;
        lab[t] = f ? t + 1 : 0;
    }
    __syncthreads();
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int t = threadIdx.x + 256 * e, lj = t >> 6, li = t & 63;
        if (!fg[e]) continue;
        if (li > 0 && lab[t - 1] != 0) unite(lab, t, t - 1);
        if (lj > 0) {
            if (lab[t - TW] != 0) unite(lab, t, t - TW);
            if (eight && li > 0 && lab[t - TW - 1] != 0) unite(lab, t, t - TW - 1);
            if (eight && li < TW - 1 && lab[t - TW + 1] != 0) unite(lab, t, t - TW + 1);
        }
    }
    __syncthreads();
    int32_t* L = labels + (size_t)mp * a.N;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int t = threadIdx.x + 256 * e, j = j0 + (t >> 6), i = i0 + (t & 63);
        if (j >= a.H || i >= a.W) continue;
        int out = 0;
        if (fg[e]) {
            const int r = find_root(lab, t);
            out = (j0 + (r >> 6)) * a.W + i0 + (r & 63) + 1;
        }
        L[j * a.W + i] = out;
    }
}

// kernel 2: the points of a tile's first row and first and last column join their W, NW, N and NE neighbours where those lie in another
// tile or across the wrap column (every adjacent pair has exactly one point for which the other is one of these four)
__global__ void __launch_bounds__(128) obj_border_kernel(const ObjArgs a, int32_t* __restrict__ labels) {
    const int mp = blockIdx.y, p = mp % a.P;
    const int ty = blockIdx.x / a.tiles_x, tx = blockIdx.x - ty * a.tiles_x;
    const int j0 = ty * TH, i0 = tx * TW, H = a.H, W = a.W;
    const int last = W - 1 - i0 < TW - 1 ? W - 1 - i0 : TW - 1;          // the tile's last column inside the grid
    const int t = threadIdx.x;
    int lj, li;
    if (t < TW) { lj = 0; li = t; }
    else if (t < TW + TH - 1) { lj = t - TW + 1; li = 0; }
    else if (t < TW + 2 * (TH - 1) && last > 0) { lj = t - TW - TH + 2; li = last; }
    else return;
    const int j = j0 + lj, i = i0 + li;
    if (j >= H || i >= W) return;
    int32_t* L = labels + (size_t)mp * a.N;
    const int q = j * W + i;
    if (L[q] == 0) return;
    const bool eight = a.planes[p].connectivity == 8;
    int iw = i - 1, ie = i + 1;                                         // -1: no such column
    if (iw < 0) iw = a.periodic ? W - 1 : -1;
    if (ie >= W) ie = a.periodic ? 0 : -1;
    if (li == 0 && iw >= 0 && L[j * W + iw] != 0) unite(L, q, j * W + iw);
    if (j > 0) {
        const int up = (j - 1) * W;
        if (lj == 0 && L[up + i] != 0) unite(L, q, up + i);
        if (eight && (lj == 0 || li == 0) && iw >= 0 && L[up + iw] != 0) unite(L, q, up + iw);
        if (eight && (lj == 0 || li == last) && ie >= 0 && L[up + ie] != 0) unite(L, q, up + ie);
    }
}

// kernel 3: every label becomes its root's, and the roots count their points.  No union runs any more: the labels this kernel writes
// are roots' and leave every walk where it would have ended
__global__ void __launch_bounds__(256) obj_flatten_kernel(const ObjArgs a, int32_t* __restrict__ labels, int32_t* __restrict__ cnt) {
    const int mp = blockIdx.y;
    const uint32_t q = blockIdx.x * 256u + threadIdx.x;
    int32_t* L = labels + (size_t)mp * a.N;
    int32_t* c = cnt + (size_t)mp * a.N;
    const bool on = q < a.N && L[q] != 0;
    int r = 0;
    if (on) {
        r = find_root(L, (int)q);
        L[q] = r + 1;
    }
    const int common = wave_common(r, on);
    if (common >= 0) {
        const u64 act = __ballot(on);
        if ((threadIdx.x & 63) == __ffsll((long long)act) - 1) atomicAdd(c + common, __popcll(act));
    } else if (on) {
        atomicAdd(c + r, 1);
    }
}

__device__ __forceinline__ bool qualifies(const ObjArgs& a, const int32_t* L, const int32_t* c, uint32_t q) {
    return q < a.N && L[q] == (int32_t)q + 1 && c[q] >= a.min_pixels;
}

// kernel 4: the qualifying roots of each chunk of 1024 points
__global__ void __launch_bounds__(256) obj_chunk_kernel(const ObjArgs a, const int32_t* __restrict__ labels, const int32_t* __restrict__ cnt,
                                                        int32_t* __restrict__ sums) {
    __shared__ int part[4];
    const int mp = blockIdx.y;
    const int32_t* L = labels + (size_t)mp * a.N;
    const int32_t* c = cnt + (size_t)mp * a.N;
    const uint32_t q0 = blockIdx.x * (uint32_t)CHUNK + threadIdx.x * 4u;
    int n = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) n += qualifies(a, L, c, q0 + e) ? 1 : 0;
    n = wave_sum(n);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) sums[(size_t)mp * a.nchunks + blockIdx.x] = part[0] + part[1] + part[2] + part[3];
}

// kernel 5: one wave per plane turns the chunk counts into exclusive offsets; the total is n_found
__global__ void __launch_bounds__(64) obj_scan_kernel(const ObjArgs a, int32_t* __restrict__ sums, int32_t* __restrict__ n_found) {
    const int mp = blockIdx.x, lane = threadIdx.x;
    int32_t* s = sums + (size_t)mp * a.nchunks;
    int carry = 0;
    for (uint32_t base = 0; base < a.nchunks; base += 64) {
        const uint32_t k = base + lane;
        const int v = k < a.nchunks ? s[k] : 0;
        int incl = v;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int o = __shfl_up(incl, off);
            if (lane >= off) incl += o;
        }
        if (k < a.nchunks) s[k] = carry + incl - v;
        carry += __shfl(incl, 63);
    }
    if (lane == 0) n_found[mp] = carry;
}

// kernel 6: the qualifying roots take their numbers, in raster order; the count of every other root becomes 0
__global__ void __launch_bounds__(256) obj_number_kernel(const ObjArgs a, const int32_t* __restrict__ labels, int32_t* __restrict__ cnt,
                                                         const int32_t* __restrict__ sums) {
    __shared__ int part[4];
    const int mp = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int32_t* L = labels + (size_t)mp * a.N;
    int32_t* c = cnt + (size_t)mp * a.N;
    const uint32_t q0 = blockIdx.x * (uint32_t)CHUNK + threadIdx.x * 4u;
    bool f[4];
    int n = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        f[e] = qualifies(a, L, c, q0 + e);
        n += f[e] ? 1 : 0;
    }
    int incl = n;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int o = __shfl_up(incl, off);
        if (lane >= off) incl += o;
    }
    if (lane == 63) part[wave] = incl;
    __syncthreads();
    int number = sums[(size_t)mp * a.nchunks + blockIdx.x] + incl - n;
    for (int w = 0; w < wave; ++w) number += part[w];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const uint32_t q = q0 + e;
        if (q < a.N && L[q] == (int32_t)q + 1) c[q] = f[e] ? ++number : 0;
    }
}

// kernel 7: the id plane
__global__ void __launch_bounds__(256) obj_id_kernel(const ObjArgs a, const int32_t* __restrict__ labels, const int32_t* __restrict__ cnt,
                                                     int32_t* __restrict__ ids) {
    const int mp = blockIdx.y;
    const uint32_t q = blockIdx.x * 256u + threadIdx.x;
    if (q >= a.N) return;
    const int l = labels[(size_t)mp * a.N + q];
    int id = 0;
    if (l > 0 && (uint32_t)l <= a.N) id = cnt[(size_t)mp * a.N + (uint32_t)(l - 1)];
    ids[(size_t)mp * a.N + q] = id >= 1 && id <= a.capacity ? id : 0;
}

// ---- attributes ------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int kept(const ObjArgs& a, const int32_t* n_found, int mp) {
    const int n = n_found[mp];
    return n < 0 ? 0 : (n < a.capacity ? n : a.capacity);
}

__global__ void __launch_bounds__(256) obj_init_kernel(const ObjArgs a, const int32_t* __restrict__ n_found, skobj_record* __restrict__ records) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    const int mp = (int)(t / (uint32_t)a.capacity), k = (int)(t - (uint32_t)mp * (uint32_t)a.capacity);
    if (mp >= a.M * a.P || k >= kept(a, n_found, mp)) return;
    skobj_record r = {};
    r.member = mp / a.P;
    r.plane = mp - r.member * a.P;
    r.id = k + 1;
    r.jmin = INT_MAX;
    r.jmax = -1;
    records[(size_t)mp * a.capacity + k] = r;           // (ext_value / ext_index hold the 64-bit key, 0, until obj_finish_kernel)
}

struct Sums {
    long long s[11];      // area, sx, sy, sz, sxx, sxy, sxz, syy, syz, szz, sum_v
    int n, sat;
    u64 key;
};

__device__ __forceinline__ long long rn(double v) { return (long long)__builtin_rint(v); }

__device__ __forceinline__ void add_to(skobj_record* r, const Sums& s, int j) {
    u64* dst = (u64*)&r->area;
#pragma unroll
    for (int k = 0; k < 11; ++k) atomicAdd(dst + k, (u64)s.s[k]);
    atomicAdd(&r->n_pixels, s.n);
    if (s.sat) atomicAdd(&r->saturated, s.sat);
    atomicMin(&r->jmin, j);
    atomicMax(&r->jmax, j);
    atomicMax((u64*)&r->ext_value, s.key);
}

__device__ __forceinline__ u64 wave_max_u64(u64 v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const u64 o = __shfl_xor(v, off);
        v = o > v ? o : v;
    }
    return v;
}

// one wave per (plane, row).  The lanes keep their sums in registers while the wave's points share one id (the inside of a large object,
// where 64 lanes would otherwise queue on one record) and reduce over the wave before one lane's atomics; a step whose points belong to
// several objects adds lane by lane.  All sums are integers: neither path changes a bit.
__global__ void __launch_bounds__(256) obj_sum_kernel(const ObjArgs a, const float* const* __restrict__ members, const int32_t* __restrict__ ids,
                                                      const double* __restrict__ rowt, const double* __restrict__ colt,
                                                      skobj_record* __restrict__ records) {
    const int lane = threadIdx.x & 63, H = a.H, W = a.W;
    const uint32_t w = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (w >= (uint32_t)(a.M * a.P) * (uint32_t)H) return;             // (a whole wave leaves)
    const int mp = uniform((int)(w / (uint32_t)H)), j = uniform((int)(w - (uint32_t)mp * (uint32_t)H));
    const int m = mp / a.P, p = mp - m * a.P;
    const skobj_plane pl = a.planes[p];
    const float* x = members[m];
    const uint32_t row = (uint32_t)pl.channel * a.N + (uint32_t)j * (uint32_t)W;
    const int32_t* I = ids + (size_t)mp * a.N + (size_t)j * W;
    skobj_record* rec = records + (size_t)mp * a.capacity;
    const double R1 = rowt[H + j], R3 = rowt[3 * H + j], R4 = rowt[4 * H + j];
    const long long area = rn(rowt[j]), sz = rn(rowt[2 * H + j]), szz = rn(rowt[5 * H + j]);
    const double A = (double)area * (1.0 / 4096.0), inv = 1.0 / (double)pl.value_scale;       // (a power of two: the product is the quotient)
    Sums acc = {};
    int cur = 0;                                                       // the id the lanes' sums belong to; 0: none
    auto flush = [&]() {
        Sums t;
#pragma unroll
        for (int k = 0; k < 11; ++k) t.s[k] = wave_sum(acc.s[k]);
        t.n = wave_sum(acc.n);
        t.sat = wave_sum(acc.sat);
        t.key = wave_max_u64(acc.key);
        if (lane == 0) add_to(rec + (cur - 1), t, j);
        acc = Sums{};
        cur = 0;
    };
    for (int i0 = 0; i0 < W; i0 += 64) {
        const int i = i0 + lane;
        int id = i < W ? I[i] : 0;
        if (id < 0 || id > a.capacity) id = 0;
        const bool on = id > 0;
        if (__ballot(on) == 0) continue;
        const int common = wave_common(id, on);
        if (cur != 0 && common != cur) flush();
        Sums c = {};
        if (on) {
            const float v = load_vec<1>(x, row + (uint32_t)i);
            const double C0 = colt[i], C1 = colt[W + i], C2 = colt[2 * W + i], C3 = colt[3 * W + i], C4 = colt[4 * W + i];
            c.s[0] = area;         c.s[1] = rn(R1 * C0);  c.s[2] = rn(R1 * C1);  c.s[3] = sz;
            c.s[4] = rn(R3 * C2);  c.s[5] = rn(R3 * C3);  c.s[6] = rn(R4 * C0);
            c.s[7] = rn(R3 * C4);  c.s[8] = rn(R4 * C1);  c.s[9] = szz;
            double s = (double)v * inv;
            const bool sat = s > SKOBJ_CLAMP || s < -SKOBJ_CLAMP;
            s = s > SKOBJ_CLAMP ? SKOBJ_CLAMP : (s < -SKOBJ_CLAMP ? -SKOBJ_CLAMP : s);
            c.s[10] = rn(s * A);
            c.n = 1;
            c.sat = sat ? 1 : 0;
            const uint32_t k = __float_as_uint(v);
            uint32_t o = k ^ ((k >> 31) ? 0xffffffffu : 0x80000000u);
            if (pl.direction < 0) o = ~o;
            c.key = ((u64)o << 32) | (u64)(0xffffffffu - (uint32_t)(j * W + i));
        }
        if (common > 0) {
#pragma unroll
            for (int k = 0; k < 11; ++k) acc.s[k] += c.s[k];
            acc.n += c.n;
            acc.sat += c.sat;
            acc.key = c.key > acc.key ? c.key : acc.key;
            cur = common;
        } else if (on) {
            add_to(rec + (id - 1), c, j);
        }
    }
    if (cur != 0) flush();
}

__global__ void __launch_bounds__(256) obj_finish_kernel(const ObjArgs a, const int32_t* __restrict__ n_found, const int32_t* __restrict__ labels,
                                                         skobj_record* __restrict__ records) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    const int mp = (int)(t / (uint32_t)a.capacity), k = (int)(t - (uint32_t)mp * (uint32_t)a.capacity);
    if (mp >= a.M * a.P || k >= kept(a, n_found, mp)) return;
    skobj_record* r = records + (size_t)mp * a.capacity + k;
    const u64 key = *(const u64*)&r->ext_value;
    uint32_t o = (uint32_t)(key >> 32);
    const uint32_t q = 0xffffffffu - (uint32_t)key;
    if (a.planes[mp % a.P].direction < 0) o = ~o;
    r->ext_value = __uint_as_float((o >> 31) ? o ^ 0x80000000u : ~o);
    r->ext_index = (int32_t)q;
    r->root = q < a.N ? labels[(size_t)mp * a.N + q] - 1 : -1;
}

// ---- probability -----------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) obj_probability_kernel(const ObjArgs a, const int32_t* __restrict__ ids, const uint8_t* __restrict__ keep,
                                                              int32_t* __restrict__ counts) {
    const int p = blockIdx.y;
    const uint32_t q = blockIdx.x * 256u + threadIdx.x;
    if (q >= a.N) return;
    int n = 0;
    for (int m = 0; m < a.M; ++m) {
        const size_t mp = (size_t)m * a.P + p;
        int id = ids[mp * a.N + q];
        if (id < 0 || id > a.capacity) id = 0;
        n += keep[mp * (size_t)(a.capacity + 1) + id];
    }
    counts[(size_t)p * a.N + q] = n;
}

// ---- the host side ---------------------------------------------------------------------------------------------------------------------
bool valid_shape(int M, int P, int H, int W) {
    return M >= 1 && M <= SKOBJ_MAX_MEMBERS && P >= 1 && P <= SKOBJ_MAX_PLANES && H >= 1 && W >= 1 && (size_t)H <= (1ull << 30) / (size_t)W;
}

size_t chunks_of(int H, int W) { return ((size_t)H * W + CHUNK - 1) / CHUNK; }

bool aligned(const void* p, uintptr_t mask) { return p && !((uintptr_t)p & mask); }

// what every call needs
bool common_ok(const skobj_desc* d) {
    return d && valid_shape(d->M, d->P, d->H, d->W) && d->capacity >= 1 && d->capacity <= MAX_CAPACITY && aligned(d->ids, 3);
}

// what the calls that read the members need
bool planes_ok(const skobj_desc* d) {
    if (!aligned(d->members, 7) || d->C < 1 || (size_t)d->C * (size_t)d->H > (1ull << 30) / (size_t)d->W) return false;
    for (int p = 0; p < d->P; ++p) {
        const skobj_plane& pl = d->planes[p];
        if (pl.channel < 0 || pl.channel >= d->C || (pl.direction != 1 && pl.direction != -1) || (pl.connectivity != 4 && pl.connectivity != 8))
            return false;
        int e = 0;
        if (!(pl.value_scale > 0) || pl.value_scale > 3e38f || frexpf(pl.value_scale, &e) != 0.5f) return false;       // a power of two
        if (pl.threshold != pl.threshold) return false;
    }
    return true;
}

ObjArgs args_of(const skobj_desc* d) {
    ObjArgs a = {};
    a.M = d->M; a.P = d->P; a.H = d->H; a.W = d->W;
    a.periodic = d->periodic ? 1 : 0;
    a.min_pixels = d->min_pixels;
    a.capacity = d->capacity;
    a.tiles_x = (d->W + TW - 1) / TW;
    a.N = (uint32_t)d->H * (uint32_t)d->W;
    a.nchunks = (uint32_t)chunks_of(d->H, d->W);
    for (int p = 0; p < d->P; ++p) a.planes[p] = d->planes[p];
    return a;
}

#define LAUNCHED() \
    if (hipGetLastError() != hipSuccess) return SKOBJ_E_HIP

}  // namespace

extern "C" int skobj_abi_version(void) { return SKOBJ_ABI_VERSION; }

extern "C" size_t skobj_workspace_bytes(int M, int P, int H, int W) {
    if (!valid_shape(M, P, H, W)) return 0;
    const size_t ints = (size_t)M * P * ((size_t)H * W + chunks_of(H, W));
    return (4 * ints + 7) & ~(size_t)7;
}

extern "C" int skobj_label(const skobj_desc* d, void* stream) {
    if (!common_ok(d) || !planes_ok(d) || d->min_pixels < 1) return SKOBJ_E_ARG;
    if (!aligned(d->labels, 3) || !aligned(d->n_found, 3) || !aligned(d->workspace, 7) ||
        d->workspace_bytes < skobj_workspace_bytes(d->M, d->P, d->H, d->W))
        return SKOBJ_E_ARG;
    const ObjArgs a = args_of(d);
    hipStream_t s = (hipStream_t)stream;
    const unsigned MP = (unsigned)(d->M * d->P);
    int32_t* cnt = (int32_t*)d->workspace;
    int32_t* sums = cnt + (size_t)MP * a.N;
    if (hipMemsetAsync(cnt, 0, sizeof(int32_t) * (size_t)MP * a.N, s) != hipSuccess) return SKOBJ_E_HIP;
    const unsigned tiles = (unsigned)a.tiles_x * (unsigned)((d->H + TH - 1) / TH), points = (a.N + 255u) / 256u;
    hipLaunchKernelGGL(obj_tile_kernel, dim3(tiles, MP), dim3(256), 0, s, a, d->members, d->labels);
    LAUNCHED();
    hipLaunchKernelGGL(obj_border_kernel, dim3(tiles, MP), dim3(128), 0, s, a, d->labels);
    LAUNCHED();
    hipLaunchKernelGGL(obj_flatten_kernel, dim3(points, MP), dim3(256), 0, s, a, d->labels, cnt);
    LAUNCHED();
    hipLaunchKernelGGL(obj_chunk_kernel, dim3(a.nchunks, MP), dim3(256), 0, s, a, d->labels, cnt, sums);
    LAUNCHED();
    hipLaunchKernelGGL(obj_scan_kernel, dim3(MP), dim3(64), 0, s, a, sums, d->n_found);
    LAUNCHED();
    hipLaunchKernelGGL(obj_number_kernel, dim3(a.nchunks, MP), dim3(256), 0, s, a, d->labels, cnt, sums);
    LAUNCHED();
    hipLaunchKernelGGL(obj_id_kernel, dim3(points, MP), dim3(256), 0, s, a, d->labels, cnt, d->ids);
    LAUNCHED();
    return 0;
}

extern "C" int skobj_attributes(const skobj_desc* d, void* stream) {
    if (!common_ok(d) || !planes_ok(d)) return SKOBJ_E_ARG;
    if (!aligned(d->labels, 3) || !aligned(d->n_found, 3) || !aligned(d->row_tables, 7) || !aligned(d->col_tables, 7) || !aligned(d->records, 7))
        return SKOBJ_E_ARG;
    const ObjArgs a = args_of(d);
    hipStream_t s = (hipStream_t)stream;
    const unsigned MP = (unsigned)(d->M * d->P);
    const unsigned slots = (unsigned)(((size_t)MP * d->capacity + 255) / 256), rows = (unsigned)(((size_t)MP * d->H + 3) / 4);
    hipLaunchKernelGGL(obj_init_kernel, dim3(slots), dim3(256), 0, s, a, d->n_found, d->records);
    LAUNCHED();
    hipLaunchKernelGGL(obj_sum_kernel, dim3(rows), dim3(256), 0, s, a, d->members, d->ids, d->row_tables, d->col_tables, d->records);
    LAUNCHED();
    hipLaunchKernelGGL(obj_finish_kernel, dim3(slots), dim3(256), 0, s, a, d->n_found, d->labels, d->records);
    LAUNCHED();
    return 0;
}

extern "C" int skobj_probability(const skobj_desc* d, void* stream) {
    if (!common_ok(d) || !d->keep || !aligned(d->counts, 3)) return SKOBJ_E_ARG;
    const ObjArgs a = args_of(d);
    hipLaunchKernelGGL(obj_probability_kernel, dim3((a.N + 255u) / 256u, (unsigned)d->P), dim3(256), 0, (hipStream_t)stream, a, d->ids, d->keep,
                       d->counts);
    LAUNCHED();
    return 0;
}
