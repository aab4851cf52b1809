// sk_exp, sk_log and sk_pow of include/skyrim_thermo.h: fp32 exponential and logarithm made of + - * /, comparisons, selects, int <-> float
// conversion and the bits of the exponent -- nothing from the device library -- so that a numpy float32 restatement gives the same
// bits.  Host and device: the host makes the per-level constants of the parcel ascent with the same functions.  Every includer builds
// with contraction to fma off; the pragma below pins it for these functions whatever the build line says.
#pragma once
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#define SK_HD __host__ __device__ __forceinline__
#else
#define SK_HD inline
#endif

#pragma clang fp contract(off)

namespace skthermo_math {

SK_HD uint32_t bits_of(float x) { uint32_t u; memcpy(&u, &x, 4); return u; }
SK_HD float float_of(uint32_t u) { float x; memcpy(&x, &u, 4); return x; }

SK_HD bool finite(float x) { return (bits_of(x) & 0x7f800000u) != 0x7f800000u; }

// exp(x), x clamped to [-87, 88]: n = x log2(e) rounded to the nearest integer (ties to even: adding and subtracting 1.5 * 2^23 is that
// rounding), r = (x - n LN2_HI) - n LN2_LO, the degree-7 Taylor polynomial in Horner order, then the product with 2^n
SK_HD float sk_exp(float x) {
    x = x < -87.f ? -87.f : x;
    x = x > 88.f ? 88.f : x;
    const float t = x * 1.44269504f;
    const float n = (t + 12582912.f) - 12582912.f;
    const float r = (x - n * 0.693359375f) - n * -2.12194440e-4f;
    float p = 1.98412698e-4f;
    p = p * r + 1.38888889e-3f;
    p = p * r + 8.33333333e-3f;
    p = p * r + 4.16666667e-2f;
    p = p * r + 1.66666667e-1f;
    p = p * r + 0.5f;
    p = ((p * r) * r + r) + 1.f;
    return p * float_of((uint32_t)((int)n + 127) << 23);
}

// log(x) of a positive, normal, finite x = m 2^e with m in [sqrt(1/2), sqrt(2)): s = (m - 1) / (m + 1), the atanh series to s^11 in
// Horner order, and e ln 2 in two parts
SK_HD float sk_log(float x) {
    const uint32_t u = bits_of(x);
    int e = (int)(u >> 23) - 126;
    float m = float_of((u & 0x007fffffu) | 0x3f000000u);           // [0.5, 1)
    const bool lo = m < 0.70710678f;
    m = lo ? m + m : m;
    e = lo ? e - 1 : e;
    const float s = (m - 1.f) / (m + 1.f), z = s * s;
    float p = 0.181818182f;
    p = p * z + 0.222222222f;
    p = p * z + 0.285714286f;
    p = p * z + 0.4f;
    p = p * z + 0.666666667f;
    p = p * z + 2.f;
    const float ef = (float)e;
    return (ef * -2.12194440e-4f + s * p) + ef * 0.693359375f;
}

SK_HD float sk_pow(float a, float b) { return sk_exp(b * sk_log(a)); }

}  // namespace skthermo_math
