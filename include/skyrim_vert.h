/* C ABI of vertical interpolation on the device: fields of M member states of one valid time on chosen surfaces -- a pressure, a height
 * above mean sea level or above the ground, an isentrope, an isotherm -- made where the states lie in HBM and written as compact channels
 * per member, beside those of skyrim_derive.h and skyrim_thermo.h and in the same buffer.
 *
 * Conventions of skyrim_thermo.h: all data pointers are device pointers; every call is asynchronous on `stream` (a hipStream_t); nothing
 * is allocated inside; the return code is 0, SKVERT_E_ARG or SKVERT_E_HIP; argument errors are found before anything touches the GPU,
 * so they are reported on a machine without one.
 *
 * ---- skvert_run -----------------------------------------------------------------------------------------------------------------------
 * States are contiguous float32 (C, H, W): a DEVICE array of M member pointers (1 <= M <= SKVERT_MAX_MEMBERS).  Output: float32
 * out[m * member_stride + (d * H + j) * W + i], 0 <= d < D.  The program is n_ops <= SKVERT_MAX_OPS ops, a HOST array inside the
 * descriptor.  Slots no op names, and everything else in `out`, are not touched.
 *
 * An op is ONE coordinate over one column of L levels (2 <= L <= SKVERT_MAX_LEVELS, bottom-up, p[k] in hPa strictly decreasing), up to
 * SKVERT_MAX_TARGETS target values of it and up to SKVERT_MAX_FIELDS fields.  fields[f].out[t] is the slot of field f on target t (in
 * [0, D), or -1: not computed, nothing written; at least one slot of an op is >= 0; no slot is written twice).
 *
 * Arithmetic.  Everything is fp32, every operation rounded on its own (the library is built with -ffp-contract=off), in the order written
 * here.  sk_exp and sk_log are those of skyrim_thermo.h (csrc/thermo_math.h); kappa = 0.2854, LN1000 = sk_log(1000).  Host constants of
 * an op, made with them: lnp_k = sk_log(p[k]); ex_k = sk_exp(kappa * (LN1000 - lnp_k)).  A numpy float32 restatement gives the same bits.
 *
 * Coordinate.  c_k is the coordinate at level k, tau the target:
 *   SKVERT_P      c_k = lnp_k;        tau = target[t] = sk_log(P), made by the caller; no plane is read for c
 *   SKVERT_Z      c_k = z_k (in_c);   tau = target[t] = g Z (geopotential, g = 9.80665)
 *   SKVERT_Z_AGL  c_k = z_k (in_c);   tau = zs + target[t] per column, one rounded addition; needs `zs`
 *   SKVERT_THETA  c_k = t_k * ex_k (in_c = t_k): the theta of SKTHERMO_MOIST bit for bit;  tau = target[t] in K
 *   SKVERT_T      c_k = t_k (in_c);   tau = target[t] in K
 *
 * Mask.  With `zs` (a DEVICE plane (H, W) of the surface geopotential in the units of z; NULL: none) a level with z_k < zs is masked.
 * Z and Z_AGL test their own planes; THETA and T name their z planes in in_z, which are read for the mask alone and only with `zs`;
 * SKVERT_P reads neither z nor `zs` unless `mask` is 1 (then it needs both).  Without `zs`, levels below the ground are treated as air.
 *
 * The search (SKTHERMO_FREEZE's, for any coordinate).  Scan k = L - 1 down to 0 over the unmasked levels, u = the unmasked level last
 * seen (above k):  a = c_k - tau, b = c_u - tau;  the layer crosses when ((a >= 0 and b <= 0) or (a <= 0 and b >= 0)) and a != b;  the
 * FIRST layer from the top that crosses gives frac = a / (a - b).  Each coordinate plane is read once per op.
 *
 * Fields.  With k, u and frac of the crossing:
 *   SKVERT_PLAIN     in_a[k] = f_k:            out = f_k + (f_u - f_k) * frac
 *   SKVERT_SPEED     in_a[k] = u_k, in_b = v_k: both as PLAIN, then uu = u u, vv = v v, out = sqrtf(uu + vv)   (the SPEED of skyrim_derive.h)
 *   SKVERT_THETA_F   in_a[k] = t_k:            PLAIN with f_k = t_k * ex_k
 *   SKVERT_PRESSURE  no planes:                out = sk_exp(lnp_k + (lnp_u - lnp_k) * frac), in hPa
 * Field values are read at the two levels of the crossing only.
 *
 * Surface node (SKVERT_Z_AGL, PLAIN and SPEED).  node_a (and node_b for v) >= 0 names a surface channel, SKVERT_NODE_ZS stands for `zs`
 * itself as the value (a z field); `gh` is its height as geopotential (g * 10 for u10m, g * 2 for t2m, 0 for zs).  The node is level -1 of
 * THAT field's column: c = zs + gh (one rounded addition), its value the surface channel.  It is scanned last, against the lowest
 * unmasked level, with the same test and the same formula, when no layer above crossed.  Fields without a node do not see it.
 *
 * No crossing.  outside = SKVERT_NAN: 0x7fc00000.  SKVERT_NEAREST: the field's value at the unmasked level whose |c - tau| is smallest,
 * the lower one of equals (the node counts as the lowest level of a field that has one; PRESSURE gives sk_exp(lnp_k)).  A column whose
 * levels are all masked gives NaN in either mode.
 *
 * Non-finite input.  A point at which an op reads a non-finite value gives NaN (0x7fc00000) in every requested result of that op at
 * that point, by an explicit test, and nowhere else.  What an op reads at a point: every coordinate and mask plane at every level, `zs`
 * when it is used, the node channels of its fields with a requested slot, and the field values at the levels each requested (field,
 * target) pair takes its result from.
 *
 * Shape of the computation.  A wave takes one 512-point tile of one op of one member (member and op are wave-uniform); a lane's address
 * is the member pointer plus a 32-bit byte offset.  When every member pointer, `zs` and `out` are 16-byte aligned and member_stride and
 * H W are multiples of 4, a lane loads the coordinate planes and stores 16 bytes (four columns); otherwise the scalar path runs; the
 * results are bit-equal.  The levels of a crossing are per-lane values; the plane they select is found by compare-and-select over the
 * wave-uniform level loop, never by indexing registers.  An op with several fields reads their values twice (once for the non-finite
 * test, which spans the fields, once for the result); the second read is served by the caches.  A call whose ops do not fit one
 * launch's argument block is split into launches of whole ops.  No scratch memory, no LDS, no atomics.
 *
 * Bounds, against exact arithmetic on the same fp32 inputs (planes, targets, lnp_k, ex_k), for columns where the same layer is chosen,
 * u = 2^-24, tiny = 2^-100 (underflow):
 *   PLAIN     |out - exact| <= 7 u (|f_k| + |f_u|) + tiny.
 *       a = (c_k - tau)(1 + d1), b = (c_u - tau)(1 + d2).  At a crossing a and b have opposite signs (or one is 0), so |a - b| = |a| + |b|
 *       and a - b = (c_k - c_u)(1 + e), |e| <= u: the difference does not cancel.  frac = a / fl(a - b) carries d1, e, the rounding of
 *       a - b and that of the quotient: 4 roundings, |frac - frac*| <= 4 u frac* to first order, 0 <= frac* <= 1.  f_u - f_k, the product
 *       and the sum add three: out = (f_k + (f_u - f_k) frac* (1 + 6 u')) (1 + u''), so
 *       |out - exact| <= 6 u |f_u - f_k| frac* + u max(|f_k|, |f_u|) <= 7 u (|f_k| + |f_u|); the terms of order u^2 are below 1e-6 of that.
 *   THETA_F   the same with 8 u: f_k = t_k * ex_k is rounded once more.
 *   THETA and Z_AGL round c or tau before the search (one product, one sum).  With rho = u max(|c_k|, |c_u|, |tau|) / |c_u - c_k|:
 *       frac(c + dc, tau + dtau) - frac = (dc_k (1 - frac) + dc_u frac - dtau) / (c_k - c_u + dc_k - dc_u).  THETA has |dc| <= u |c|, dtau = 0:
 *       at most rho / (1 - 2 rho); Z_AGL has dc = 0: at most rho.  To first order the coefficient is 1; the bound stated and tested,
 *       + |f_u - f_k| * 2 rho, holds for rho <= 1/4 and is added to the above.
 *   SPEED     the bound of s in skyrim_derive.h applied to the interpolated u and v with their PLAIN bounds.
 *   PRESSURE against float64 (np.exp, np.log of the same p[k], the same algorithm), largest relative difference over 100 000 random
 *       columns per coordinate kind (numpy restatement), and what the tests assert (four times that):
 *                     measured        asserted
 *   p@                      1.7e-5 relative                         6.7e-5
 *       (the coordinates of the sample are half a kelvin a level apart at the least; a - b of such a layer carries the rounding of two
 *       temperatures near 250 K, which the layer's ln p then scales: the figure is that of the thinnest layers, not of sk_exp)
 *
 * Limits: C H W <= 2^30 and D H W <= 2^30 (32-bit byte offsets), member_stride >= D H W, member, zs and output pointers 4-byte aligned.
 * `member_align` is the caller's statement of the alignment, in bytes, that ALL M member pointers share (4 or 16) -- the library
 * cannot read the device array. */
#ifndef SKYRIM_VERT_H
#define SKYRIM_VERT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SKVERT_ABI_VERSION 1
#define SKVERT_E_ARG (-1) /* bad argument: NULL or misaligned pointer, a count, index, level, kind or slot outside its range, a slot written twice */
#define SKVERT_E_HIP (-2) /* a launch failed */
#define SKVERT_MAX_MEMBERS 64
#define SKVERT_MAX_OPS 16
#define SKVERT_MAX_LEVELS 16
#define SKVERT_MAX_TARGETS 4
#define SKVERT_MAX_FIELDS 8

#define SKVERT_P 1
#define SKVERT_Z 2
#define SKVERT_Z_AGL 3
#define SKVERT_THETA 4
#define SKVERT_T 5

#define SKVERT_PLAIN 1
#define SKVERT_SPEED 2
#define SKVERT_THETA_F 3
#define SKVERT_PRESSURE 4

#define SKVERT_NAN 0
#define SKVERT_NEAREST 1

#define SKVERT_NODE_NONE (-1) /* the field has no surface node */
#define SKVERT_NODE_ZS (-2)   /* the node's value is zs itself */

typedef struct {
    int32_t kind;                        /* SKVERT_PLAIN ... */
    int32_t in_a[SKVERT_MAX_LEVELS];     /* PLAIN: f_k; SPEED: u_k; THETA_F: t_k */
    int32_t in_b[SKVERT_MAX_LEVELS];     /* SPEED: v_k */
    int32_t node_a, node_b;              /* Z_AGL, PLAIN and SPEED: the surface channel of the node (node_b: of v), SKVERT_NODE_ZS or SKVERT_NODE_NONE */
    float gh;                            /* the node's height above the ground as geopotential, >= 0 */
    int32_t out[SKVERT_MAX_TARGETS];     /* the slot of this field on target t, or -1 */
} skvert_field;

typedef struct {
    int32_t coord;                       /* SKVERT_P ... */
    int32_t n_levels, n_targets, n_fields;
    int32_t outside;                     /* SKVERT_NAN or SKVERT_NEAREST */
    int32_t mask;                        /* SKVERT_P: 1 = mask by in_z and zs; ignored otherwise */
    int32_t in_c[SKVERT_MAX_LEVELS];     /* Z, Z_AGL: z_k; THETA, T: t_k */
    int32_t in_z[SKVERT_MAX_LEVELS];     /* THETA, T, P with mask: z_k, read only with zs */
    float p[SKVERT_MAX_LEVELS];          /* hPa, strictly decreasing, positive and finite */
    float target[SKVERT_MAX_TARGETS];    /* finite; P: sk_log of the pressure */
    skvert_field fields[SKVERT_MAX_FIELDS];
} skvert_op;

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
    skvert_op ops[SKVERT_MAX_OPS];
} skvert_desc;

int skvert_abi_version(void);

int skvert_run(const skvert_desc* desc, void* stream);

#ifdef __cplusplus
}
#endif
#endif
