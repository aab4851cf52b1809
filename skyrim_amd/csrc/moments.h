// Mean and M2 = sum (x - mean)^2 of one channel x[0, HW) by one workgroup, reading x once (the instance norm of SFNO and its statistics).
// Each thread folds its values -- float4 batches, or single values when HW is not a multiple of 4 -- into a (count, mean, M2) triple
// with Chan's pairwise update; the triples of the threads merge the same way, through the lanes of a wave and then across waves.  Unlike
// the one-pass  E[(x - p)^2] - E[x - p]^2  this does not cancel however far single elements lie from the rest: shifted by one element p,
// that form loses (|mean - p| / sigma)^2 ulps, 1e-3 of rstd with an outlier of ~300 sigma at p.  The values are still shifted by a pivot
// p first, which keeps a large common offset (1e4 +- 1) out of the sums; what p costs is the mean's precision, ~|mean - p| / 2^24, so p
// is the median of the first, middle and last element: no single element can move it.  Counts are floats: exact up to 2^24 per channel.
#pragma once
#include <hip/hip_runtime.h>

namespace skp {

struct Moments { float n, mean, m2; };

__device__ __forceinline__ void moments_merge(Moments& a, const Moments& b) {
    const float n = a.n + b.n;
    const float f = b.n > 0.f ? b.n * __builtin_amdgcn_rcpf(n) : 0.f;       // weight of b in the merged mean
    const float d = b.mean - a.mean;
    a.mean += d * f;
    a.m2 += b.m2 + d * d * a.n * f;
    a.n = n;
}

// (HW, mean, M2) of xc[0, HW), the same in every thread of the workgroup; blockDim.x a multiple of 64, at most 1024.
__device__ __forceinline__ Moments block_moments(const float* __restrict__ xc, long long HW) {
    __shared__ Moments red[16];
    const float p0 = xc[0], p1 = xc[HW / 2], p2 = xc[HW - 1];
    const float pv = fmaxf(fminf(p0, p1), fminf(fmaxf(p0, p1), p2));          // median of three
    Moments t{0.f, 0.f, 0.f};
    if ((HW & 3) == 0) {
        for (long long i = threadIdx.x; i < HW / 4; i += blockDim.x) {
            const float4 v = reinterpret_cast<const float4*>(xc)[i];
            const float a = v.x - pv, b = v.y - pv, c = v.z - pv, d = v.w - pv;
            const float bm = ((a + b) + (c + d)) * 0.25f;
            const float ea = a - bm, eb = b - bm, ec = c - bm, ed = d - bm;
            moments_merge(t, Moments{4.f, bm, (ea * ea + eb * eb) + (ec * ec + ed * ed)});
        }
    } else {
        for (long long i = threadIdx.x; i < HW; i += blockDim.x) moments_merge(t, Moments{1.f, xc[i] - pv, 0.f});
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) moments_merge(t, Moments{__shfl_xor(t.n, o), __shfl_xor(t.mean, o), __shfl_xor(t.m2, o)});
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();                                // a previous call's readers of red[] are done (more than one call per kernel)
    if (lane == 0) red[wave] = t;
    __syncthreads();
    Moments s = red[0];
    for (int w = 1; w < (int)(blockDim.x >> 6); ++w) moments_merge(s, red[w]);
    s.mean += pv;
    return s;
}

}  // namespace skp
