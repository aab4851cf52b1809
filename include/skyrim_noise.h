/* C ABI of the spherical (spatially correlated) initial-condition perturbations: random spherical-harmonic coefficients of an isotropic
 * Gaussian field with a prescribed spectrum, and the step that puts the synthesised field on an initial condition.
 *
 * Conventions of skyrim_ens.h: all data pointers are device pointers; every call is asynchronous on `stream` (a hipStream_t); nothing is
 * allocated inside; the return code is 0, SKNOISE_E_ARG or SKNOISE_E_HIP; argument errors are found before anything touches the GPU, so
 * they are reported on a machine without one.
 *
 * ---- the field -----------------------------------------------------------------------------------------------------------------------
 * Per member, history level and channel (field index f = level * C + c) one real field on the sphere, unit variance at every point:
 *   y(theta_k, phi_j) = sum_{m < lmax} c_m sum_{l < lmax} Pbar_l^m(cos theta_k) [Re a_lm cos(m phi_j) - Im a_lm sin(m phi_j)],  c_0 = 1, c_m = 2
 * with the orthonormal Pbar_l^m (Condon-Shortley phase) of skyrim_amd/sfno/sht.py: exactly ShtMatrices(grid="equiangular").synthesis followed
 * by .idft, on the rows of a pole-to-pole equiangular grid (theta_k = pi k / (n_lat_full - 1)) or its first rows.
 *
 * Spectrum (float64 on the host, skyrim_amd/noise.py `spectrum`): for 1 <= l < lmax
 *   s_l = (kappa^2 + l (l + 1))^(-alpha / 2),  kappa = a / length_scale,  a = 6371 km,  alpha = 2 by default
 *   sigma_l = s_l / sqrt(sum_l' (2 l' + 1) s_l'^2 / (4 pi)),   sigma_0 = 0 (no shift of the global mean)
 * so that sum_l (2 l + 1) sigma_l^2 / (4 pi) = 1: by the addition theorem the variance is 1 at EVERY latitude -- but only with every order
 * present, so mmax = lmax always.  lmax <= min(n_lat_full, n_lon / 2); the default is min(256, n_lat_full, n_lon / 2).
 *
 * Coefficients.  (r0, r1, r2, r3) = Philox4x32-10(counter = (l, m >> 1, f, 1), key = (seed, member)) and its four words give four standard
 * normals n0..n3 by exactly the uniform / Box-Muller mapping of skens_perturb (skyrim_ens.h; one device function, csrc/philox.h):
 * (n0, n1) from (r0, r1), (n2, n3) from (r2, r3).  Even m takes (n_re, n_im) = (n0, n1), odd m takes (n2, n3).
 *   a_l0 = (sigma_l n0, 0);     a_lm = sigma_l sqrt(1/2) (n_re, n_im)  for 1 <= m <= l;     everything else (l = 0, m > l) is exactly +0.
 * Counter word 3 is 1: white noise uses 0, so the streams are disjoint; values above 1 are reserved for later draws of the same member
 * (per-step stochastic noise).  A coefficient's bits depend on (seed, member, f, l, m) only: not on lmax, on the number of members or
 * fields of a call, or on batching.
 *
 * The power of two e.  The synthesis GEMM (sksfno_gemm_run, three MFMA terms) splits its A operand -- the coefficients, then the
 * longitude spectrum -- into fp16 hi / lo planes.  Coefficients that carried perturb_scale * std[c] would underflow fp16 for humidity
 * channels, and small sigma_l would push the lo plane into subnormals.  So the kernel writes a_lm * 2^e (its table is sigma_l 2^e) and
 * the amplitude g[c] carries 2^-e: both exact.  Rule (noise.py `scale_exponent`): with sigma_min / sigma_max the smallest / largest
 * non-zero sigma_l,
 *   e = the smallest integer with sigma_min 2^e >= 2^-2
 *       (a draw of typical size then has |a| 2^e >= 2^-2: its hi plane is normal, and so is its lo plane, which holds about 2^-12 |a| 2^e >= 2^-14);
 *   refused (ValueError) unless 6.5 sigma_max 2^e <= 2^14
 *       (no normal exceeds sqrt(50 ln 2) = 5.89; a factor 4 under fp16's largest finite value 65504, which leaves the sum over l of the
 *        longitude spectrum its room: the second GEMM splits that, and it is checked against 65504 in the tests).
 * The dynamic range sigma_max / sigma_min that fits is therefore at least 2^14 / 6.5 / 2^-1 = 5041.
 *
 * Member.   x_m[i] = fmaf(g[c(i)], y'_m[i], x0[i]),   g[c] = fl32(perturb_scale * std[c] * 2^-e),   y' = 2^e y as synthesised.
 * Member 0 is a bit copy of x0; nothing is synthesised for it.
 *
 * ---- sknoise_coeffs ------------------------------------------------------------------------------------------------------------------
 * Writes the coefficients of members member_first .. member_first + n_members - 1 for the F fields f_first .. f_first + F - 1, layout
 *   out[member][l][m][re / im][F]      l, m < lmax; F fastest -- what the Legendre GEMM of SfnoEngine._synthesis reads with C = F
 * (n_members * lmax * lmax * 2 * F floats), zeros included.  sigma[l] is a DEVICE table of lmax floats, sigma_l 2^e.  In fp32:
 *   m = 0:   sigma[l] * n0                       m >= 1:   (sigma[l] * 0.70710678f) * n
 * Bound against float64 arithmetic on the same words (z the float64 normal, t = sigma[l] or sigma[l] sqrt(1/2)): skens_perturb's normals
 * are within 3.7e-6 of z, and fl(sqrt(1/2)) and the two products round once each, so
 *   |value - t z| <= t (3.7e-6 + 3 u |z|) (1 + 2^-20),   u = 2^-24.
 * One Philox block serves an (l, order pair, f); for odd lmax the last pair's second order is discarded.
 *
 * ---- sknoise_apply -------------------------------------------------------------------------------------------------------------------
 *   out[i] = fmaf(g[c(i)], y[i], x0[i])     i < n = L * C * chan_stride,   c(i) = (i / chan_stride) % C
 * one rounding per element; where g[c] is 0 the element is a bit copy of x0 (the sign of a zero and a non-finite y included).
 * 16-byte aligned x0, y and out take the vector path (a scalar path covers the tail and 4-byte aligned pointers).
 *
 * ---- the synthesis and its error -----------------------------------------------------------------------------------------------------
 * Two calls of sksfno_gemm_run per member (noise.py `Synthesis`): the Legendre GEMM, one batch per order m, contracting l >= floor32(m)
 * (k_lo_step = 1) into the longitude spectrum t[m][re / im][F][lat]; the inverse-DFT GEMM, one batch per field, contracting (m, re / im).
 * Error of an output element against exact arithmetic on the coefficients the device holds, a' = a 2^e:
 *   |y'_device - y'| <= u (k S + Q),   k = 18 lmax + 32,   u = 2^-24
 *   S = sum_m c_m sum_l |Pbar_l^m| (|Re a'_lm| |cos m phi| + |Im a'_lm| |sin m phi|)       (the field's double sum, every addend's absolute value)
 *   Q = 1/2 [ sum_m c_m sum_l (|Re a'_lm| + |Im a'_lm| + 2 |Pbar_l^m|)  +  sum_m sum_l |Pbar_l^m| (|Re a'_lm| + |Im a'_lm|)  +  4 lmax ]
 * Derivation, per GEMM with contraction length K (lmax, then 2 lmax):
 *   - operands: x = x_hi + x_lo + r, |r| <= 2^-22 |x| + 2^-25 (two fp16 roundings; the second addend is the spacing of fp16 subnormals,
 *     met by the lo plane wherever |x| < 2^-3 and by both planes under 2^-14 -- Legendre functions of high order near the poles, cosines
 *     near their zeros); the same for the matrix element w, after its fp32 rounding (u |w|).  The product keeps hi hi + lo hi + hi lo and
 *     drops lo lo <= 2^-22 |x w|: per addend (3 * 2^-22 + u) |x w| + 2^-25 (|x| + |w|) = 13 u |x w| + (u / 2)(|x| + |w|);
 *   - fp32 accumulation of 3 K products, each addition charged 2 u of the running absolute sum (covers an accumulator that truncates):
 *     6 K u sum |x w|;
 *   so |error| <= (6 K + 13) u sum_k |x_k w_k| + (u / 2) sum_k (|x_k| + |w_k|), rounded up to 6 K + 16 for the second-order terms.
 * Chaining: the first GEMM's error enters the second multiplied by |idft| <= c_m -- its S term sums to (6 lmax + 16) u S, its floor term to
 * the first bracket of Q; the second GEMM adds (12 lmax + 16) u S (its sum |x w| is at most S (1 + 2^-10)) and the floor terms
 * sum |t| <= the second bracket and sum |idft| <= 4 lmax.  A bound of the pure form k u S does not exist: where Pbar underflows fp16, S
 * loses the addend but the error keeps 2^-25 |a'|.  In the tested cases Q is at most a few per cent of k S (the tests print it).  Both pole rows hold only m = 0, and are
 * constant along longitude within the same bound. */
#ifndef SKYRIM_NOISE_H
#define SKYRIM_NOISE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SKNOISE_ABI_VERSION 1
#define SKNOISE_E_ARG (-1) /* bad argument: NULL or misaligned pointer, a count outside its range */
#define SKNOISE_E_HIP (-2) /* the launch failed */
#define SKNOISE_MAX_LMAX 4096

int sknoise_abi_version(void);

int sknoise_coeffs(float* out, const float* sigma, int lmax, int F, uint32_t f_first, uint32_t seed, uint32_t member_first, int n_members,
                   void* stream);

int sknoise_apply(const float* x0, const float* y, const float* g, float* out, size_t n, size_t chan_stride, int C, void* stream);

#ifdef __cplusplus
}
#endif
#endif
