// The counter-based generator of the ensemble kernels (include/skyrim_ens.h, include/skyrim_noise.h): Philox4x32-10 and the mapping of its
// words to standard normals.  One definition, so that white noise (ens_ops.hip) and spherical coefficients (noise_ops.hip) share every bit.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace skrng {

// ---- Philox4x32-10 (Salmon et al., SC11; constants of Random123) ---------------------------------------------------------------- //
struct u32x4 { uint32_t x, y, z, w; };

__device__ __forceinline__ u32x4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return {c0, c1, c2, c3};
}

// U(r) = ((r >> 8) + 0.5) * 2^-24 has 25 significant bits once r >> 8 reaches 2^23: rounded to fp32 the upper half of the uniforms would lose
// its half (and 1 - 2^-25 would become 1).  Neither use needs U itself, so it is never rounded: with k = r >> 8,
//   ln U       = logf((k + 0.5) 2^-24)                        k <  2^23   (24 bits: exact argument)
//              = log1pf(-((2^24 - 1 - k) + 0.5) 2^-24)        k >= 2^23   (1 - U, again 24 bits)
//   cos / sin of 2 pi U = of 2 pi (U - 1) for k >= 2^23       (U - 1 = ((k - 2^24) + 0.5) 2^-24: 24 bits)
__device__ __forceinline__ float log_unit(uint32_t r) {
    const uint32_t k = r >> 8;
    const float lo = logf(((float)k + 0.5f) * 5.9604644775390625e-8f);
    const float hi = log1pf(-(((float)(0xFFFFFFu - k) + 0.5f) * 5.9604644775390625e-8f));
    return k < 0x800000u ? lo : hi;
}

__device__ __forceinline__ float turn_unit(uint32_t r) {      // U or U - 1, in (-0.5, 0.5): exact
    const int k = (int)(r >> 8);
    return ((float)(k < 0x800000 ? k : k - 0x1000000) + 0.5f) * 5.9604644775390625e-8f;
}

// the Box-Muller pair of two words: (sqrt(-2 ln u1) cos(2 pi u2), sqrt(-2 ln u1) sin(2 pi u2))
__device__ __forceinline__ void normal_pair(uint32_t r1, uint32_t r2, float& z0, float& z1) {
    const float rad = sqrtf(-2.0f * log_unit(r1));
    const float th = 6.2831855f * turn_unit(r2);
    z0 = rad * cosf(th);
    z1 = rad * sinf(th);
}

}  // namespace skrng
