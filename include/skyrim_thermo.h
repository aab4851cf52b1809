/* C ABI of column thermodynamics on the device: dew point, humidity conversion, potential and equivalent potential temperature of a
 * level, the K and total-totals indices, the height of the 0 C level, and the CAPE and lifted index of a lifted parcel -- of M member
 * states of one valid time, made where the states lie in HBM and written as compact channels per member, beside those of
 * skyrim_derive.h and in the same buffer.
 *
 * Conventions of skyrim_derive.h: all data pointers are device pointers; every call is asynchronous on `stream` (a hipStream_t); nothing
 * is allocated inside; the return code is 0, SKTHERMO_E_ARG or SKTHERMO_E_HIP; argument errors are found before anything touches the GPU,
 * so they are reported on a machine without one.
 *
 * ---- skthermo_run ---------------------------------------------------------------------------------------------------------------------
 * States are contiguous float32 (C, H, W): a DEVICE array of M member pointers (1 <= M <= SKTHERMO_MAX_MEMBERS).  Output: float32
 * out[m * member_stride + (d * H + j) * W + i], 0 <= d < D.  The program is n_ops <= SKTHERMO_MAX_OPS ops, a HOST array inside the
 * descriptor.  Each op names its input channels (in [0, C)) and one output slot per result (in [0, D), or -1: that result is not computed
 * and nothing is written for it; at least one slot of an op is >= 0; no slot is written by two results).  Slots no op names, and
 * everything else in `out`, are not touched.
 *
 * Arithmetic.  Everything is fp32, every operation rounded on its own (the library is built with -ffp-contract=off), in the order written
 * here, and made of + - * /, comparisons, selects, int <-> float conversion and the bits of the exponent alone: no expf, logf or powf of
 * the device library is called.  A numpy float32 restatement therefore gives the same bits.
 *   sk_exp(x): x clamped to [-87, 88]; n = rint(x * 1.44269504) (ties to even); r = (x - n * 0.693359375) - n * -2.12194440e-4;
 *      P = 1.98412698e-4; P = P r + c for c = 1.38888889e-3, 8.33333333e-3, 4.16666667e-2, 1.66666667e-1, 0.5;
 *      sk_exp = (((P r) r + r) + 1) * 2^n.
 *   sk_log(x), x positive, normal and finite: x = m 2^e with m in [0.5, 1) (frexp); if m < 0.70710678: m = m + m, e = e - 1;
 *      s = (m - 1) / (m + 1); z = s s; P = 0.181818182; P = P z + c for c = 0.222222222, 0.285714286, 0.4, 0.666666667, 2;
 *      sk_log = (e * -2.12194440e-4 + s P) + e * 0.693359375.
 *   sk_pow(a, b) = sk_exp(b * sk_log(a)).
 * Every decimal constant here and below is the fp32 number nearest to it.
 *
 * Formulas (Bolton 1980), eps = 0.622, 1 - eps = 0.378, kappa = 0.2854, R_d = 287.04, T0 = 273.15, LN1000 = sk_log(1000); p in hPa, T in K:
 *   es(T)      = 6.112 * sk_exp((17.67 * (T - T0)) / (T - 29.65))
 *   e(m, T, p) = SKTHERMO_Q (m = specific humidity):        (m * p) / (eps + 0.378 * m)
 *                SKTHERMO_R (m = relative humidity in %):   (m / 100) * es(T)
 *                then e = e < E_MIN ? E_MIN : e, E_MIN = 1e-10 hPa: q = 0 and r = 0 are finite everywhere.  Supersaturation is allowed.
 *   w(e, p)    = (eps * e') / (p - e'), e' = e > 0.5 p ? 0.5 p : e          (the mixing ratio; the cap keeps it finite: w <= eps)
 *   td(e)      : le = sk_log(e / 6.112); td = (243.5 * le) / (17.67 - le) + T0                                   (the inverse of es)
 *   tl(T, td)  = 1 / (1 / (td - 56) + sk_log(T / td) / 800) + 56                                                      (Bolton 15)
 *   thetae(T, TL, lq, w), lq = ln(1000 / p):                                                                         (Bolton 43)
 *                a = sk_exp((kappa * (1 - 0.28 * w)) * lq); b = sk_exp(((3.376 / TL - 0.00254) * (w * 1000)) * (1 + 0.81 * w));
 *                thetae = (T * a) * b
 *   thetae_sat(T, p, lq) = thetae(T, T, lq, w(es(T), p))
 *   tv(T, w)   = (T * (1 + w / eps)) / (1 + w)
 *
 * SKTHERMO_MOIST   one level.  in_t[0] = t, in_m[0] = the moisture plane, p[0] = the level in hPa; out[0 .. 3] = td, other, thetae, theta:
 *      lq = LN1000 - sk_log(p); e = e(m, t, p); td = td(e);
 *      other = (100 * e) / es(t) with SKTHERMO_Q (relative humidity in %), (eps * e) / (p - 0.378 * e) with SKTHERMO_R (specific humidity);
 *      thetae = thetae(t, tl(t, td), lq, w(e, p)); theta = t * sk_exp(kappa * lq).
 *      When theta is the only result asked for, the moisture plane is not read.
 * SKTHERMO_INDEX   in_t[0 .. 2] = t850, t700, t500; in_m[0 .. 1] = moisture at 850 and 700; out[0] = kx, out[1] = tt:
 *      td850 = td(e(m850, t850, 850)); td700 = td(e(m700, t700, 700));
 *      kx = ((t850 - t500) + (td850 - T0)) - (t700 - td700)      (degrees C);     tt = (t850 - t500) + (td850 - t500).
 *      All five planes are read whichever result is asked for.
 * SKTHERMO_FREEZE  n_levels = L (2 <= L <= SKTHERMO_MAX_LEVELS), bottom-up: in_t[k] = t_k, in_z[k] = z_k; out[0] = the z of the 0 C level,
 *      in the units of z.  Scan k = L - 1 down to 0 over the unmasked levels (see "Surface"), u = the unmasked level last seen (above k):
 *      a = t_k - T0, b = t_u - T0; the layer crosses when ((a >= 0 and b <= 0) or (a <= 0 and b >= 0)) and a != b; the first layer
 *      that crosses gives z_k + (z_u - z_k) * (a / (a - b)).  If none crosses: z of the lowest unmasked level.
 * SKTHERMO_PARCEL  n_levels = L, bottom-up: in_t[k] = t_k, in_m[k] = moisture, p[k] in hPa, strictly decreasing, in_z[k] = z_k (read
 *      only when `zs` is given); out[0 .. 2] = cape (J/kg), li (K), p_src (hPa).
 *      Host constants, made with the functions above: lnp_k = sk_log(p_k); ex_k = sk_exp(kappa * (lnp_k - LN1000)); lq_k = LN1000 - lnp_k;
 *      for the layer k -> k + 1 and node s = 1 .. NSUB (SKTHERMO_NSUB = 8): a_s = s / NSUB; lp = lnp_k + a_s * (lnp_{k+1} - lnp_k);
 *      pp = sk_exp(lp); lq = LN1000 - lp; ex = sk_exp(kappa * (lp - LN1000)); h_k = (lnp_k - lnp_{k+1}) / NSUB.
 *      K_top = the highest level with p >= p_top; K_500 = the level with p == 500 (li needs one, and p_top <= 500).
 *      Per level: e_k, w_k = w(e_k, p_k), tv_k = tv(t_k, w_k).
 *      Source.  SKTHERMO_SRC_LOWEST: the lowest unmasked level.  SKTHERMO_SRC_MAX_THETAE: among the unmasked levels with p >= p_src_min,
 *      the one with the largest thetae(t_k, tl(t_k, td(e_k)), lq_k, w_k), the lower one of equals; when there is none, the lowest
 *      unmasked level.  With the source S: T0 = t_S, TL = tl(T0, td(e_S)), the = thetae(T0, TL, lq_S, w_S), th0 = T0 / ex_S,
 *      lq_lcl = lq_S - sk_log(TL / T0) / kappa   (the parcel is saturated at the nodes with lq > lq_lcl, i.e. above
 *      p_LCL = p_S (TL / T0)^(1 / kappa)).
 *      Ascent.  Tprev = T0, Bprev = 0, cape_sum = 0.  For k = S .. K_top - 1, stopping below the first masked level above S, and
 *      s = 1 .. NSUB, with exprev = ex_k at s = 1 and the previous node's ex after it:
 *         tenv = tv_k + a_s * (tv_{k+1} - tv_k);  Tdry = th0 * ex;
 *         the moist adiabat, thetae_sat(T, pp, lq) = the, by SKTHERMO_NITER = 3 secant updates from the starting pair Ta = Tprev,
 *         Tb = (Tprev / exprev) * ex  (the last node's parcel, and the same brought dry-adiabatically to this node: they bracket the root):
 *            Fa = thetae_sat(Ta, pp, lq) - the;  three times: Fb = thetae_sat(Tb, pp, lq) - the; d = Fb - Fa;
 *            step = d != 0 ? (Fb * (Tb - Ta)) / d : 0; Ta = Tb; Fa = Fb; Tb = Tb - step;
 *         T = lq > lq_lcl ? Tb : Tdry;  wp = lq > lq_lcl ? w(es(T), pp) : w_S;  B = tv(T, wp) - tenv;  B = B > 0 ? B : 0;
 *         cape_sum = cape_sum + (0.5 * (B + Bprev)) * h_k;  Bprev = B;  Tprev = T.
 *      cape = R_d * cape_sum: the trapezoid rule of R_d * integral of max(tv_parcel - tv_env, 0) d ln p on NSUB sub-intervals per layer,
 *      uniform in ln p, the environment's tv linear in ln p, the integrand clamped at the nodes.
 *      li = t_{K_500} - Tprev after the last node of the layer that ends at K_500; 0 when S = K_500; NaN when S lies above K_500 or the
 *      ascent stopped below it.  p_src = p_S.
 *      CIN, the LFC and the EL are not offered: thirteen levels do not locate them, and CIN jumps where an LFC appears.
 * in_*, p and out entries an op does not use are ignored.
 *
 * Surface.  `zs` (NULL: no mask) is a DEVICE plane (H, W) of the surface geopotential in the units of z.  A level with z_k < zs is
 * masked: no candidate as a source, not integrated through (the ascent stops below it), skipped by FREEZE.  A column whose levels are
 * all masked gives NaN.  MOIST and INDEX do not read it.  Without it, levels below the ground are treated as air.
 *
 * Non-finite input.  A point at which an op reads a non-finite value (a state plane it names, or zs) gives NaN (0x7fc00000) in every
 * requested result of that op at that point, by an explicit test of the inputs, and nowhere else.
 *
 * Shape of the computation.  One launch covers all members and all ops (a program whose column ops hold more than
 * SKTHERMO_LEVELS_PER_LAUNCH levels in total, or whose PARCEL ops differ in their pressure levels, is split into launches of whole ops).
 * A wave takes one tile of one op of one member: member and op are wave-uniform (scalar registers).  MOIST, INDEX and FREEZE walk the
 * plane 512 points at a time; when every member pointer, `zs` and `out` are 16-byte aligned and member_stride and H W are multiples of 4,
 * a lane loads and stores 16 bytes (four columns), otherwise the scalar path runs.  A PARCEL tile is 64 columns, one per lane on both
 * paths: the ascent is bound by the vector ALU, not by memory, and one column per lane keeps the sixteen tv_k and the ascent's state in
 * registers (docs/experiments.md has the compiler's figures).  The level loops are unrolled; layers and moist solves that no lane of
 * a wave needs are skipped, which changes no result.  Both paths do the same arithmetic per point: their results are bit-equal.  No
 * scratch memory, no LDS, no atomics.
 *
 * Bounds.  Against the same algorithm in float64 (np.exp, np.log, the secant iteration run to convergence) on the same fp32 inputs,
 * the largest differences measured over 100 000 random columns per configuration (13 levels, both moisture kinds, sources forced to
 * levels 0 .. 3; 200 000 arguments for the functions), and what the tests assert (four times that, for the corners another sample meets):
 *                     measured        asserted
 *   sk_exp  [-87, 88]       8.2e-8 relative                         3.3e-7
 *   sk_log  [1e-30, 1e30]   9.8e-8 relative to max(|log|, 1)        4.0e-7
 *   cape                    0.030 J/kg                              0.12 J/kg
 *   li                      9.6e-5 K                                3.9e-4 K
 *   td                      2.7e-5 K                                1.1e-4 K
 *   rh                      1.8e-4 %                                7.2e-4 %
 *   q                       1.5e-6 relative to max(q, 1e-5)         6.0e-6
 *   thetae                  1.2e-4 K                                4.8e-4 K
 *   theta                   2.8e-5 K                                1.1e-4 K
 *   kx, tt                  3.9e-5 K                                1.6e-4 K
 *   zdeg0                   0.059 m2/s2                             0.24 m2/s2
 *
 * Limits: C H W <= 2^30 and D H W <= 2^30 (32-bit byte offsets), member_stride >= D H W, member, zs and output pointers 4-byte aligned.
 * `member_align` is the caller's statement of the alignment, in bytes, that ALL M member pointers share (4 or 16) -- the library
 * cannot read the device array. */
#ifndef SKYRIM_THERMO_H
#define SKYRIM_THERMO_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SKTHERMO_ABI_VERSION 1
#define SKTHERMO_E_ARG (-1) /* bad argument: NULL or misaligned pointer, a count, index, level or slot outside its range, a slot written twice */
#define SKTHERMO_E_HIP (-2) /* a launch failed */
#define SKTHERMO_MAX_MEMBERS 64
#define SKTHERMO_MAX_OPS 16
#define SKTHERMO_MAX_LEVELS 16
#define SKTHERMO_LEVELS_PER_LAUNCH 48
#define SKTHERMO_NSUB 8
#define SKTHERMO_NITER 3

#define SKTHERMO_MOIST 1
#define SKTHERMO_INDEX 2
#define SKTHERMO_FREEZE 3
#define SKTHERMO_PARCEL 4

#define SKTHERMO_Q 0
#define SKTHERMO_R 1

#define SKTHERMO_SRC_LOWEST 0
#define SKTHERMO_SRC_MAX_THETAE 1

typedef struct {
    int32_t kind;                          /* SKTHERMO_MOIST ... */
    int32_t n_levels;                      /* FREEZE, PARCEL: L; ignored otherwise */
    int32_t moisture;                      /* SKTHERMO_Q or SKTHERMO_R: what the in_m planes hold; ignored by FREEZE */
    int32_t source;                        /* PARCEL: SKTHERMO_SRC_* */
    int32_t in_t[SKTHERMO_MAX_LEVELS];     /* MOIST: t; INDEX: t850, t700, t500; FREEZE, PARCEL: t_k */
    int32_t in_m[SKTHERMO_MAX_LEVELS];     /* MOIST: moisture; INDEX: moisture at 850, 700; PARCEL: moisture at level k */
    int32_t in_z[SKTHERMO_MAX_LEVELS];     /* FREEZE: z_k; PARCEL: z_k, read only with zs */
    float p[SKTHERMO_MAX_LEVELS];          /* MOIST: p[0]; PARCEL: p_k, strictly decreasing; hPa, positive and finite */
    float p_src_min;                       /* PARCEL with SRC_MAX_THETAE: candidates have p >= p_src_min (700 is customary) */
    float p_top;                           /* PARCEL: integrate up to the highest level with p >= p_top (100 is customary); p[0] >= p_top > 0 */
    int32_t out[4];                        /* MOIST: td, other, thetae, theta; INDEX: kx, tt; FREEZE: zdeg0; PARCEL: cape, li, p_src; -1: not computed */
} skthermo_op;

typedef struct {
    const float* const* members; /* device array of M device pointers */
    int M;
    int member_align;            /* bytes every member pointer is aligned to (4 or 16) */
    int C, H, W;
    int D;                       /* output channels per member */
    float* out;                  /* [M][member_stride], the first D H W elements of each member's part are the planes */
    size_t member_stride;        /* in elements */
    const float* zs;             /* [H][W] surface geopotential, or NULL */
    int n_ops;
    skthermo_op ops[SKTHERMO_MAX_OPS];
} skthermo_desc;

int skthermo_abi_version(void);

int skthermo_run(const skthermo_desc* desc, void* stream);

#ifdef __cplusplus
}
#endif
#endif
