// Spherical (spatially correlated) perturbations, include/skyrim_noise.h: the random spherical-harmonic coefficients of a member's fields
// in the layout the synthesis GEMM reads, and the fused multiply-add that puts the synthesised field on the initial condition.  The synthesis
// between the two is sksfno_gemm_run, twice (skyrim_amd/noise.py).  Both kernels are grid-stride loops (csrc/io_ops.hip: the launch shape).
#include <hip/hip_runtime.h>
#include <cstdint>
#include "../../include/skyrim_noise.h"
#include "philox.h"

namespace {

using skrng::u32x4;
using skrng::philox4x32_10;
using skrng::normal_pair;

// one lane = one (l, order pair, field): ONE Philox block gives the orders 2p (n0, n1) and 2p + 1 (n2, n3).  Lanes run along the field index,
// the fastest index of the output, so each of the four stores of a wave is one contiguous run.  blockIdx.y = member of the batch.
__global__ void __launch_bounds__(256) coeffs_kernel(float* __restrict__ out, const float* __restrict__ sigma, uint32_t lmax, uint32_t F,
                                                     uint32_t f_first, uint32_t seed, uint32_t member_first) {
    const uint32_t member = member_first + blockIdx.y;
    const uint32_t pairs = (lmax + 1) / 2, items = lmax * pairs * F;
    float* __restrict__ dst = out + (size_t)blockIdx.y * lmax * lmax * 2 * F;
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t t = blockIdx.x * blockDim.x + threadIdx.x; t < items; t += stride) {
        const uint32_t lp = t / F, f = t - lp * F;
        const uint32_t l = lp / pairs, p = lp - l * pairs;
        const uint32_t m0 = 2 * p, m1 = m0 + 1;
        float v[4] = {0.f, 0.f, 0.f, 0.f};                    // (re, im) of order m0, (re, im) of order m1
        if (l > 0 && m0 <= l) {                               // degree 0 carries no variance; orders above the degree do not exist
            const u32x4 r = philox4x32_10(l, p, f_first + f, 1u, seed, member);
            float n[4];
            normal_pair(r.x, r.y, n[0], n[1]);
            normal_pair(r.z, r.w, n[2], n[3]);
            const float s = sigma[l], h = s * 0.70710678f;
            if (m0 == 0) {
                v[0] = s * n[0];                              // the zonal coefficient is real
            } else {
                v[0] = h * n[0];
                v[1] = h * n[1];
            }
            if (m1 <= l) {
                v[2] = h * n[2];
                v[3] = h * n[3];
            }
        }
        float* q = dst + ((size_t)(l * lmax + m0) * 2) * F + f;
        q[0] = v[0];
        q[F] = v[1];
        if (m1 < lmax) {                                      // (odd lmax: the last pair's second order is outside the table)
            q[2 * (size_t)F] = v[2];
            q[3 * (size_t)F] = v[3];
        }
    }
}

// one lane = 4 consecutive elements of the flat (L, C, H, W) state: out = fma(g[c], y, x0)
__global__ void __launch_bounds__(256) apply_kernel(const float* __restrict__ x0, const float* __restrict__ y, const float* __restrict__ g,
                                                    float* __restrict__ out, uint32_t n, uint32_t chan_stride, uint32_t C, int vec) {
    const uint32_t groups = (uint32_t)(((uint64_t)n + 3) / 4);
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < groups; k += stride) {
        const uint32_t i0 = 4 * k;
        const bool full = vec && n - i0 >= 4;
        float x[4], z[4];
        if (full) {
            const float4 a = *(const float4*)(x0 + i0), b = *(const float4*)(y + i0);
            x[0] = a.x; x[1] = a.y; x[2] = a.z; x[3] = a.w;
            z[0] = b.x; z[1] = b.y; z[2] = b.z; z[3] = b.w;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                x[e] = i0 + e < n ? x0[i0 + e] : 0.f;
                z[e] = i0 + e < n ? y[i0 + e] : 0.f;
            }
        }
        uint32_t rem = i0 % chan_stride, c = (i0 / chan_stride) % C;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float gc = g[c];
            x[e] = gc == 0.f ? x[e] : fmaf(gc, z[e], x[e]);      // an unperturbed channel is a bit copy, whatever y holds
            if (++rem == chan_stride) { rem = 0; c = c + 1 == C ? 0 : c + 1; }
        }
        if (full) {
            *(float4*)(out + i0) = make_float4(x[0], x[1], x[2], x[3]);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (i0 + e < n) out[i0 + e] = x[e];
        }
    }
}

}  // namespace

extern "C" int sknoise_abi_version(void) { return SKNOISE_ABI_VERSION; }

extern "C" int sknoise_coeffs(float* out, const float* sigma, int lmax, int F, uint32_t f_first, uint32_t seed, uint32_t member_first,
                              int n_members, void* stream) {
    if (!out || !sigma || (((uintptr_t)out | (uintptr_t)sigma) & 3)) return SKNOISE_E_ARG;
    if (lmax < 1 || lmax > SKNOISE_MAX_LMAX || F < 1 || n_members < 1 || n_members > 65535) return SKNOISE_E_ARG;
    const uint64_t items = (uint64_t)lmax * (uint64_t)((lmax + 1) / 2) * (uint64_t)F;
    if (items > 0xFFFFFF00ull || (uint64_t)f_first + (uint64_t)F > 0x100000000ull) return SKNOISE_E_ARG;      // 32-bit item and field indices
    const uint64_t want = (items + 255) / 256;
    const unsigned blocks = (unsigned)(want < 2048 ? want : 2048);
    hipLaunchKernelGGL(coeffs_kernel, dim3(blocks, (unsigned)n_members), dim3(256), 0, (hipStream_t)stream, out, sigma, (uint32_t)lmax,
                       (uint32_t)F, f_first, seed, member_first);
    return hipGetLastError() == hipSuccess ? 0 : SKNOISE_E_HIP;
}

extern "C" int sknoise_apply(const float* x0, const float* y, const float* g, float* out, size_t n, size_t chan_stride, int C, void* stream) {
    if (!x0 || !y || !g || !out || (((uintptr_t)x0 | (uintptr_t)y | (uintptr_t)g | (uintptr_t)out) & 3)) return SKNOISE_E_ARG;
    if (n == 0 || n > 0xFFFFFFF0ull || chan_stride == 0 || C < 1) return SKNOISE_E_ARG;
    if (n % chan_stride || (n / chan_stride) % (size_t)C) return SKNOISE_E_ARG;       // n = L * C * chan_stride
    const int vec = (((uintptr_t)x0 | (uintptr_t)y | (uintptr_t)out) & 15) == 0;
    const size_t want = ((n + 3) / 4 + 255) / 256;
    const unsigned blocks = (unsigned)(want < 2048 ? want : 2048);
    hipLaunchKernelGGL(apply_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, x0, y, g, out, (uint32_t)n, (uint32_t)chan_stride,
                       (uint32_t)C, vec);
    return hipGetLastError() == hipSuccess ? 0 : SKNOISE_E_HIP;
}
