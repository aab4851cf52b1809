// LayerNorm of one row by one wavefront, the row in registers: NVEC float4 per lane (C <= 256 NVEC, C % 4 == 0).  Two passes: sum ->
// mean, centred squares -> rstd, each per lane over its float4 in order and then a butterfly over the 64 lanes.
#pragma once
#include <hip/hip_runtime.h>

namespace skp {

// src(c): float4 c < C / 4 of the row.  gamma / beta / res / out: the row's own pointers; res (added after the affine) may be null and
// may alias out.
template <int NVEC, class SRC>
__device__ __forceinline__ void row_layer_norm(const SRC& src, const float* gamma, const float* beta, const float* res, float* out, int C, float eps) {
    const int lane = threadIdx.x & 63, C4 = C >> 2;
    float4 v[NVEC];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < NVEC; ++i) {
        const int c = lane + 64 * i;
        v[i] = c < C4 ? src(c) : make_float4(0.f, 0.f, 0.f, 0.f);
        s += (v[i].x + v[i].y) + (v[i].z + v[i].w);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    const float mean = s / (float)C;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < NVEC; ++i) {
        if (lane + 64 * i < C4) {
            const float a = v[i].x - mean, b = v[i].y - mean, c = v[i].z - mean, d = v[i].w - mean;
            q += (a * a + b * b) + (c * c + d * d);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) q += __shfl_xor(q, o);
    const float rstd = rsqrtf(q / (float)C + eps);
#pragma unroll
    for (int i = 0; i < NVEC; ++i) {
        const int c = lane + 64 * i;
        if (c < C4) {
            const float4 gm = reinterpret_cast<const float4*>(gamma)[c], bt = reinterpret_cast<const float4*>(beta)[c];
            float4 y = make_float4((v[i].x - mean) * rstd * gm.x + bt.x, (v[i].y - mean) * rstd * gm.y + bt.y,
                                   (v[i].z - mean) * rstd * gm.z + bt.z, (v[i].w - mean) * rstd * gm.w + bt.w);
            if (res) {
                const float4 t = reinterpret_cast<const float4*>(res)[c];
                y.x += t.x; y.y += t.y; y.z += t.z; y.w += t.w;
            }
            reinterpret_cast<float4*>(out)[c] = y;
        }
    }
}

// the plain row source
struct RowContig {
    const float4* p;
    __device__ __forceinline__ float4 operator()(int c) const { return p[c]; }
};

}  // namespace skp
