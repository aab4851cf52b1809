// Per-step stochastic perturbations, include/skyrim_stoch.h: the spherical-harmonic coefficients of draw number `draw` (noise_ops.hip's
// coefficients with another Philox counter word), their autoregressive step in place, and the fused step that puts the SPPT multiplier and
// the additive field on one member's model step.  The synthesis between them is sksfno_gemm_run, twice (skyrim_amd/noise.py).  All three
// kernels are grid-stride loops (csrc/io_ops.hip: the launch shape).
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include "../../include/skyrim_stoch.h"
// The generator and the coefficient arithmetic must be compiled exactly as libskyrim_noise.so compiles them -- the compiler's default
// contraction, no -ffp-contract=off on this file -- because draw 0 has to give sknoise_coeffs' bits: with contraction off, two additions inside
// the inlined logf / cosf / sinf are no longer fused and a few coefficients change in their last bit (a pragma around philox.h does not bring
// them back).  The roundings the header fixes come after `fresh4`, under `#pragma clang fp contract(off)`, and are of shapes no contraction
// applies to anyway: a product or a difference that feeds an fmaf or an fmaxf, never an addition.
#include "philox.h"

namespace {

using skrng::u32x4;
using skrng::philox4x32_10;
using skrng::normal_pair;

// the four values of one (l, order pair p, field): (re, im) of order 2p, (re, im) of order 2p + 1 -- coeffs_kernel of noise_ops.hip with
// the counter word 1 + draw
__device__ __forceinline__ void fresh4(const float* __restrict__ sigma, uint32_t l, uint32_t p, uint32_t field, uint32_t word, uint32_t seed,
                                       uint32_t member, float v[4]) {
    const uint32_t m0 = 2 * p, m1 = m0 + 1;
    v[0] = v[1] = v[2] = v[3] = 0.f;
    if (l > 0 && m0 <= l) {                                   // degree 0 carries no variance; orders above the degree do not exist
        const u32x4 r = philox4x32_10(l, p, field, word, seed, member);
        float n[4];
        normal_pair(r.x, r.y, n[0], n[1]);
        normal_pair(r.z, r.w, n[2], n[3]);
        const float s = sigma[l], h = s * 0.70710678f;
        if (m0 == 0) {
            v[0] = s * n[0];                                  // the zonal coefficient is real
        } else {
            v[0] = h * n[0];
            v[1] = h * n[1];
        }
        if (m1 <= l) {
            v[2] = h * n[2];
            v[3] = h * n[3];
        }
    }
}

#pragma clang fp contract(off)

// one lane = one (l, order pair, field): ONE Philox block gives the orders 2p and 2p + 1.  Lanes run along the field index, the fastest
// index of the state, so each of the four loads and stores of a wave is one contiguous run.  blockIdx.y = member of the batch.
// EVOLVE: p = fma(phi, p, psi * fresh) in place; otherwise p = fresh.
template <bool EVOLVE>
__global__ void __launch_bounds__(256) coeffs_kernel(float* __restrict__ out, const float* __restrict__ sigma, uint32_t lmax, uint32_t F,
                                                     uint32_t f_first, uint32_t seed, uint32_t member_first, uint32_t word, float phi,
                                                     float psi) {
    const uint32_t member = member_first + blockIdx.y;
    const uint32_t pairs = (lmax + 1) / 2, items = lmax * pairs * F;
    float* __restrict__ dst = out + (size_t)blockIdx.y * lmax * lmax * 2 * F;
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t t = blockIdx.x * blockDim.x + threadIdx.x; t < items; t += stride) {
        const uint32_t lp = t / F, f = t - lp * F;
        const uint32_t l = lp / pairs, p = lp - l * pairs;
        const bool second = 2 * p + 1 < lmax;                 // (odd lmax: the last pair's second order is outside the table)
        float* q = dst + ((size_t)(l * lmax + 2 * p) * 2) * F + f;
        float old[4] = {0.f, 0.f, 0.f, 0.f};
        if (EVOLVE) {                                         // the loads go out before the Philox rounds and wait behind them
            old[0] = q[0];
            old[1] = q[F];
            if (second) {
                old[2] = q[2 * (size_t)F];
                old[3] = q[3 * (size_t)F];
            }
        }
        float v[4];
        fresh4(sigma, l, p, f_first + f, word, seed, member, v);
        if (EVOLVE) {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = fmaf(phi, old[e], psi * v[e]);
        }
        q[0] = v[0];
        q[F] = v[1];
        if (second) {
            q[2 * (size_t)F] = v[2];
            q[3 * (size_t)F] = v[3];
        }
    }
}

// one element of skstoch_apply
template <bool SPPT, bool ADD>
__device__ __forceinline__ float perturbed(float xp, float xn, float r, float y, float gs, float ga, float lim) {
    float t = xn;
    if (SPPT) {
        const float d = xn - xp;
        const float w = fminf(fmaxf(gs * r, -lim), lim);
        t = gs == 0.f ? xn : fmaf(w, d, xn);                  // an unperturbed channel is a bit copy, whatever r holds
    }
    if (ADD) t = ga == 0.f ? t : fmaf(ga, y, t);
    return t;
}

// one lane = 4 consecutive elements of the flat (L, C, H, W) state.  vec bit 0: xp, xn, y and out are 16-byte aligned; bit 1: r is.
template <bool SPPT, bool ADD>
__global__ void __launch_bounds__(256) apply_kernel(const float* __restrict__ xp, const float* xn, const float* __restrict__ r,
                                                    const float* __restrict__ y, const float* __restrict__ gs, const float* __restrict__ ga,
                                                    float lim, float* out, uint32_t n, uint32_t chan_stride, uint32_t C, int vec) {
    const uint32_t groups = (uint32_t)(((uint64_t)n + 3) / 4);
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < groups; k += stride) {
        const uint32_t i0 = 4 * k;
        const bool full = (vec & 1) && n - i0 >= 4;
        uint32_t rem = i0 % chan_stride, c = (i0 / chan_stride) % C;
        float a[4] = {0.f, 0.f, 0.f, 0.f}, b[4], z[4] = {0.f, 0.f, 0.f, 0.f}, s[4] = {0.f, 0.f, 0.f, 0.f};
        if (full) {
            const float4 vb = *(const float4*)(xn + i0);
            b[0] = vb.x; b[1] = vb.y; b[2] = vb.z; b[3] = vb.w;
            if (SPPT) {
                const float4 va = *(const float4*)(xp + i0);
                a[0] = va.x; a[1] = va.y; a[2] = va.z; a[3] = va.w;
            }
            if (ADD) {
                const float4 vz = *(const float4*)(y + i0);
                z[0] = vz.x; z[1] = vz.y; z[2] = vz.z; z[3] = vz.w;
            }
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const bool in = i0 + e < n;
                b[e] = in ? xn[i0 + e] : 0.f;
                if (SPPT) a[e] = in ? xp[i0 + e] : 0.f;
                if (ADD) z[e] = in ? y[i0 + e] : 0.f;
            }
        }
        if (SPPT) {                                           // the plane index of the group's elements; the plane may end inside the group
            if ((vec & 2) && (rem & 3) == 0 && chan_stride - rem >= 4) {
                const float4 vs = *(const float4*)(r + rem);
                s[0] = vs.x; s[1] = vs.y; s[2] = vs.z; s[3] = vs.w;
            } else {
                uint32_t q = rem;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    s[e] = r[q];                              // q < chan_stride always: in bounds also past the end of the state
                    if (++q == chan_stride) q = 0;
                }
            }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            b[e] = perturbed<SPPT, ADD>(a[e], b[e], s[e], z[e], SPPT ? gs[c] : 0.f, ADD ? ga[c] : 0.f, lim);
            if (++rem == chan_stride) { rem = 0; c = c + 1 == C ? 0 : c + 1; }
        }
        if (full) {
            *(float4*)(out + i0) = make_float4(b[0], b[1], b[2], b[3]);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (i0 + e < n) out[i0 + e] = b[e];
        }
    }
}

int coeffs_args(const float* out, const float* sigma, int lmax, int F, uint32_t f_first, int n_members, uint32_t draw, unsigned* blocks) {
    if (!out || !sigma || (((uintptr_t)out | (uintptr_t)sigma) & 3)) return SKSTOCH_E_ARG;
    if (lmax < 1 || lmax > SKSTOCH_MAX_LMAX || F < 1 || n_members < 1 || n_members > 65535) return SKSTOCH_E_ARG;
    if (draw > SKSTOCH_MAX_DRAW) return SKSTOCH_E_ARG;                                                          // 1 + draw would wrap to white noise's word
    const uint64_t items = (uint64_t)lmax * (uint64_t)((lmax + 1) / 2) * (uint64_t)F;
    if (items > 0xFFFFFF00ull || (uint64_t)f_first + (uint64_t)F > 0x100000000ull) return SKSTOCH_E_ARG;      // 32-bit item and field indices
    const uint64_t want = (items + 255) / 256;
    *blocks = (unsigned)(want < 2048 ? want : 2048);
    return 0;
}

}  // namespace

extern "C" int skstoch_abi_version(void) { return SKSTOCH_ABI_VERSION; }

extern "C" int skstoch_coeffs(float* out, const float* sigma, int lmax, int F, uint32_t f_first, uint32_t seed, uint32_t member_first,
                              int n_members, uint32_t draw, void* stream) {
    unsigned blocks = 0;
    if (coeffs_args(out, sigma, lmax, F, f_first, n_members, draw, &blocks)) return SKSTOCH_E_ARG;
    hipLaunchKernelGGL(coeffs_kernel<false>, dim3(blocks, (unsigned)n_members), dim3(256), 0, (hipStream_t)stream, out, sigma, (uint32_t)lmax,
                       (uint32_t)F, f_first, seed, member_first, 1u + draw, 0.f, 0.f);
    return hipGetLastError() == hipSuccess ? 0 : SKSTOCH_E_HIP;
}

extern "C" int skstoch_evolve(float* p, const float* sigma, int lmax, int F, uint32_t f_first, uint32_t seed, uint32_t member_first,
                              int n_members, uint32_t draw, float phi, float psi, void* stream) {
    unsigned blocks = 0;
    if (coeffs_args(p, sigma, lmax, F, f_first, n_members, draw, &blocks)) return SKSTOCH_E_ARG;
    if (!std::isfinite(phi) || !std::isfinite(psi)) return SKSTOCH_E_ARG;
    hipLaunchKernelGGL(coeffs_kernel<true>, dim3(blocks, (unsigned)n_members), dim3(256), 0, (hipStream_t)stream, p, sigma, (uint32_t)lmax,
                       (uint32_t)F, f_first, seed, member_first, 1u + draw, phi, psi);
    return hipGetLastError() == hipSuccess ? 0 : SKSTOCH_E_HIP;
}

extern "C" int skstoch_apply(const float* xp, const float* xn, const float* r, const float* y, const float* gs, const float* ga, float lim,
                             float* out, size_t n, size_t chan_stride, int C, void* stream) {
    const bool sppt = r && gs, add = y && ga;
    if ((r == nullptr) != (gs == nullptr) || (y == nullptr) != (ga == nullptr) || (!sppt && !add)) return SKSTOCH_E_ARG;
    if (!xn || !out || (sppt && !xp) || out == xp) return SKSTOCH_E_ARG;
    if ((((uintptr_t)xp | (uintptr_t)xn | (uintptr_t)r | (uintptr_t)y | (uintptr_t)gs | (uintptr_t)ga | (uintptr_t)out) & 3)) return SKSTOCH_E_ARG;
    if (!(lim > 0.f && lim <= 1.f)) return SKSTOCH_E_ARG;
    if (n == 0 || n > 0xFFFFFFF0ull || chan_stride == 0 || C < 1) return SKSTOCH_E_ARG;
    if (n % chan_stride || (n / chan_stride) % (size_t)C) return SKSTOCH_E_ARG;       // n = L * C * chan_stride
    const uintptr_t streams = (uintptr_t)xn | (uintptr_t)out | (sppt ? (uintptr_t)xp : 0) | (add ? (uintptr_t)y : 0);
    const int vec = ((streams & 15) == 0 ? 1 : 0) | (sppt && ((uintptr_t)r & 15) == 0 ? 2 : 0);
    const size_t want = ((n + 3) / 4 + 255) / 256;
    const dim3 grid((unsigned)(want < 2048 ? want : 2048)), block(256);
    hipStream_t s = (hipStream_t)stream;
    const uint32_t n32 = (uint32_t)n, cs = (uint32_t)chan_stride, c32 = (uint32_t)C;
    if (sppt && add)
        hipLaunchKernelGGL((apply_kernel<true, true>), grid, block, 0, s, xp, xn, r, y, gs, ga, lim, out, n32, cs, c32, vec);
    else if (sppt)
        hipLaunchKernelGGL((apply_kernel<true, false>), grid, block, 0, s, xp, xn, r, y, gs, ga, lim, out, n32, cs, c32, vec);
    else
        hipLaunchKernelGGL((apply_kernel<false, true>), grid, block, 0, s, xp, xn, r, y, gs, ga, lim, out, n32, cs, c32, vec);
    return hipGetLastError() == hipSuccess ? 0 : SKSTOCH_E_HIP;
}
