/* C ABI of the per-step stochastic perturbations of the ensembles (SPPT and additive noise): spherical-harmonic coefficients
 * of a random pattern that is correlated in space AND in time, and the step that puts the synthesised pattern on one model step.
 *
 * Conventions of skyrim_noise.h: all data pointers are device pointers; every call is asynchronous on `stream` (a hipStream_t); nothing is
 * allocated inside; the return code is 0, SKSTOCH_E_ARG or SKSTOCH_E_HIP; argument errors are found before anything touches the GPU, so
 * they are reported on a machine without one.  skyrim_noise.h stays at its ABI version 1: this header adds to it and changes nothing in it.
 *
 * ---- the pattern ---------------------------------------------------------------------------------------------------------------------
 * Per member and field f, at step k >= 1, the coefficient state p_k [l][m][re / im] of a real field on the sphere (the field, the spectrum
 * sigma_l, the power of two e and the synthesis are those of skyrim_noise.h):
 *   p_1 = a(draw = 1)                                                 a fresh draw of the stationary distribution
 *   p_k = fmaf(phi, p_{k-1}, fl32(psi * a(draw = k)))    k >= 2      one first-order autoregressive step per coefficient
 *   phi = fl32(exp(-dt / tau)),   psi = fl32(sqrt(1 - exp(-2 dt / tau)))      float64 on the host, rounded once; tau = 0: phi = 0, psi = 1
 * With phi^2 + psi^2 = 1 every p_k has the variance of a draw, sigma_l^2 per degree, so the synthesised pattern has unit variance at every
 * point at every step, and corr(p_k, p_{k+j}) = phi^j: the decorrelation time is tau.
 *
 * a(draw) is the coefficient set of sknoise_coeffs with another Philox counter:
 *   (r0, r1, r2, r3) = Philox4x32-10(counter = (l, m >> 1, f, 1 + draw), key = (seed, member))
 * draw = 0 IS sknoise_coeffs, bit for bit (the initial-condition perturbation); draws 1, 2, ... are the values skyrim_noise.h reserves for
 * "later draws of the same member".  draw < 2^32 - 1, so that 1 + draw never wraps to 0, the counter word of white noise (skyrim_ens.h).
 * A coefficient's bits depend on (seed, member, f, l, m, draw) only: not on lmax, on the number of members or fields of a call, or on
 * batching.  The rollout (skyrim_amd/stochastic.py) gives the additive fields the indices f = 0 .. C - 1 and the ONE SPPT pattern f = C, so
 * the streams are disjoint.
 *
 * Range.  |p_k| <= (phi + psi) max |a| <= sqrt(2) max |a| (induction: |p_1| <= max |a| and phi + psi <= sqrt(2) on the unit circle), so an
 * evolved state exceeds a fresh draw by at most sqrt(2).  The power of two e of skyrim_noise.h leaves a factor 4 under fp16's largest
 * finite value; sqrt(2) fits inside it, and the same e and the same synthesis serve the evolved state.
 *
 * ---- skstoch_coeffs ------------------------------------------------------------------------------------------------------------------
 * sknoise_coeffs with the counter word 1 + draw: layout out[member][l][m][re / im][F] (F fastest; n_members * lmax * lmax * 2 * F floats,
 * zeros included), sigma a DEVICE table of lmax floats (sigma_l 2^e), the same fp32 arithmetic
 *   m = 0:   sigma[l] * n0                       m >= 1:   (sigma[l] * 0.70710678f) * n
 * the same exact +0 for l = 0, m > l and the imaginary part of m = 0, the same bound against float64, the same argument checks.
 *
 * ---- skstoch_evolve ------------------------------------------------------------------------------------------------------------------
 * One autoregressive step of the state p (the layout of `out`), in place: for EVERY element
 *   p = fmaf(phi, p, fl32(psi * fresh)),      fresh = what skstoch_coeffs writes there for this `draw`
 * two roundings per element.  Where fresh is a structural zero the element becomes fmaf(phi, p, +0): a state that began as a draw holds
 * +0 there and keeps +0, for every finite phi and psi >= 0.  phi and psi are fp32 values from the host and must be finite.  One kernel: the state is
 * read once, the Philox block is made in registers, the state is written once; nothing else crosses HBM.
 *
 * ---- skstoch_apply -------------------------------------------------------------------------------------------------------------------
 * Puts the patterns on ONE member's step from the state xp to the state xn, n = L * C * chan_stride elements each.  Per element i, with
 * c = (i / chan_stride) % C and q = i % chan_stride:
 *   d      = fl32(xn[i] - xp[i])                                        the step's tendency
 *   w      = fminf(fmaxf(fl32(gs[c] * r[q]), -lim), lim)                the clipped multiplier (a NaN product gives -lim)
 *   t      = gs[c] == 0 ? xn[i] : fmaf(w, d, xn[i])                     SPPT: xn + w (xn - xp)
 *   out[i] = ga[c] == 0 ? t : fmaf(ga[c], y[i], t)                      additive
 * r is ONE plane of chan_stride floats, shared by every channel and level: SPPT's single pattern, so that the balance between the
 * variables of a column survives.  y holds n floats, one field per channel.  gs and ga hold C floats each:
 *   gs[c] = fl32(amplitude 2^-e),   ga[c] = fl32(additive_scale std[c] 2^-e)          (r and y are 2^e times unit-variance fields)
 * 0 < lim <= 1 keeps 1 + w >= 0: a tendency is damped or amplified, never reversed.
 * r and gs together, or y and ga together, may be NULL: that term is skipped (and xp, which only the SPPT term reads, may then be NULL
 * as well).  Both terms NULL, or one pointer of a pair without the other, is an argument error.  out may be xn (in place, what the rollout
 * does); it may not be xp.  Where both amplitudes of a channel are 0 the element is a bit copy of xn, whatever r and y hold.
 * 16-byte aligned xp, xn, y and out take the vector path (r as well where its plane index allows it); a scalar path covers the tail and
 * 4-byte aligned pointers.  HBM traffic: three state-sized streams with the SPPT term alone (xp, xn, out), three with the additive term
 * alone (xn, y, out), four with both. */
#ifndef SKYRIM_STOCH_H
#define SKYRIM_STOCH_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SKSTOCH_ABI_VERSION 1
#define SKSTOCH_E_ARG (-1) /* bad argument: NULL or misaligned pointer, a count or a factor outside its range */
#define SKSTOCH_E_HIP (-2) /* the launch failed */
#define SKSTOCH_MAX_LMAX 4096
#define SKSTOCH_MAX_DRAW 0xFFFFFFFEu

int skstoch_abi_version(void);

int skstoch_coeffs(float* out, const float* sigma, int lmax, int F, uint32_t f_first, uint32_t seed, uint32_t member_first, int n_members,
                   uint32_t draw, void* stream);

int skstoch_evolve(float* p, const float* sigma, int lmax, int F, uint32_t f_first, uint32_t seed, uint32_t member_first, int n_members,
                   uint32_t draw, float phi, float psi, void* stream);

int skstoch_apply(const float* xp, const float* xn, const float* r, const float* y, const float* gs, const float* ga, float lim, float* out,
                  size_t n, size_t chan_stride, int C, void* stream);

#ifdef __cplusplus
}
#endif
#endif
