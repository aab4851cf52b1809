// What the product kernels (score, event, track, derive, thermo, regrid, agg, point, gram, breed, spec, object) share on the device: how a lane reads and
// writes the points of a member state, the wave reductions, and the walk of the (member, tile) kernels (derive, thermo, vert, agg):
// `member_tile` gives the pair of a wave index.  Everything is __device__ __forceinline__ and leaves no call behind.
// (ens_ops.hip is not among them: its load goes through a generic pointer.)
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

// A pointer read from the member table is a generic pointer to the compiler (flat loads from 64-bit per-lane addresses); it is a global one,
// and said to be: the load then takes the pointer from scalar registers and the 32-bit lane offset as it is.
#define SK_GLOBAL __attribute__((address_space(1)))

namespace skfields {

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

template <int V> struct Vec;
template <> struct Vec<1> { typedef float type; };
template <> struct Vec<2> { typedef f32x2 type; };
template <> struct Vec<4> { typedef f32x4 type; };

// V consecutive floats at a wave-uniform pointer plus one 32-bit per-lane offset (the callers keep C H W <= 2^30, so the byte offset
// fits): V = 1 gives a float, V = 2 and 4 the vector.  The offset counts elements; score_ops.hip and event_ops.hip, which carry byte
// offsets through their loops, use the _bytes form under it
template <int V>
__device__ __forceinline__ typename Vec<V>::type load_vec_bytes(const float* base, uint32_t byte_off) {
    return *(const SK_GLOBAL typename Vec<V>::type*)((const SK_GLOBAL char*)base + byte_off);
}
template <int V>
__device__ __forceinline__ typename Vec<V>::type load_vec(const float* base, uint32_t elem) {
    return load_vec_bytes<V>(base, 4u * elem);
}

template <int V>
__device__ __forceinline__ void store_vec(float* base, uint32_t elem, typename Vec<V>::type v) {
    *(SK_GLOBAL typename Vec<V>::type*)((SK_GLOBAL char*)base + 4u * elem) = v;
}

// VEC consecutive points of a lane, as an array the kernels index
template <int VEC> struct Pts { float v[VEC]; };

// the same load into the V floats at x (a row of a register array), at a byte offset
template <int V>
__device__ __forceinline__ void load_to(const float* base, uint32_t byte_off, float* x) {
    const typename Vec<V>::type t = load_vec_bytes<V>(base, byte_off);
    if constexpr (V == 1) {
        x[0] = t;
    } else {
#pragma unroll
        for (int e = 0; e < V; ++e) x[e] = t[e];
    }
}

template <int VEC>
__device__ __forceinline__ Pts<VEC> load(const float* base, uint32_t elem) {
    Pts<VEC> r;
    load_to<VEC>(base, 4u * elem, r.v);
    return r;
}

template <int VEC>
__device__ __forceinline__ void store(float* base, uint32_t elem, const Pts<VEC>& p) {
    static_assert(VEC == 1 || VEC == 4, "a lane stores one point or four");
    if constexpr (VEC == 4)
        store_vec<4>(base, elem, f32x4{p.v[0], p.v[1], p.v[2], p.v[3]});
    else
        store_vec<1>(base, elem, p.v[0]);
}

// a value the compiler is told is the same in every lane: it goes to a scalar register
__device__ __forceinline__ int uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }

// the (member, tile) pair of the wave index w, when every member has `tiles` tiles; both are the same in every lane
struct MemberTile { int m; uint32_t t; };
__device__ __forceinline__ MemberTile member_tile(uint32_t w, uint32_t tiles) {
    const int m = uniform((int)(w / tiles));
    return {m, (uint32_t)uniform((int)(w - (uint32_t)m * tiles))};
}

// butterflies over the 64 lanes: every lane ends with the same bits
template <typename T>
__device__ __forceinline__ T wave_sum_of(T s) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    return s;
}
__device__ __forceinline__ double wave_sum(double s) { return wave_sum_of(s); }
__device__ __forceinline__ long long wave_sum(long long s) { return wave_sum_of(s); }
__device__ __forceinline__ int wave_sum(int s) { return wave_sum_of(s); }

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float o = __shfl_xor(v, off);
        v = o > v ? o : v;
    }
    return v;
}

// the key (>= 0) that every lane with `on` holds, or -1 when they hold different keys or no lane is on: with a common key the wave
// reduces over its lanes and ONE lane issues the atomic, where 64 lanes would otherwise queue on one address.  Every lane must call it
__device__ __forceinline__ int wave_common(int key, bool on) {
    const unsigned long long act = __ballot(on);
    if (act == 0) return -1;
    const int first = __shfl(key, __ffsll((long long)act) - 1);
    return __ballot(on && key != first) == 0 ? uniform(first) : -1;
}

}  // namespace skfields
