/* C ABI of derived fields on the device: nonlinear functions of several channels -- wind speed, thickness, integrated vapour transport,
 * vorticity and divergence -- of M member states of one valid time, made where the states lie in HBM and written as D compact channels
 * per member.  The ensemble statistics (skyrim_ens.h) and the scorer (skyrim_score.h) then read the derived planes like any others.
 *
 * Conventions of skyrim_track.h, skyrim_score.h and skyrim_ens.h: all data pointers are device pointers; every call is asynchronous on
 * `stream` (a hipStream_t); nothing is allocated inside; the return code is 0, SKDERIVE_E_ARG or SKDERIVE_E_HIP; argument errors are
 * found before anything touches the GPU, so they are reported on a machine without one.
 *
 * ---- skderive_run ---------------------------------------------------------------------------------------------------------------------
 * States are contiguous float32 (C, H, W): a DEVICE array of M member pointers (1 <= M <= SKDERIVE_MAX_MEMBERS), rows j = latitudes as
 * the model orders them, columns i = longitudes, periodic.  Output: float32 out[m * member_stride + (d * H + j) * W + i], 0 <= d < D.
 * The program is n_ops <= SKDERIVE_MAX_OPS ops, a HOST array inside the descriptor.  Each op names its input channels (in [0, C)) and one
 * output slot per result (in [0, D), or -1: that result is not computed and nothing is written for it; at least one slot of an op is
 * >= 0; no slot is written by two results).  Slots no op names, and everything else in `out`, are not touched.
 *
 * All arithmetic is fp32 per point, every operation rounded on its own: the library is built with contraction to fma OFF
 * (-ffp-contract=off), and the order of operations is the one written here.  Nothing is masked: a non-finite input gives non-finite
 * outputs at the points that read it and nowhere else.
 *
 * SKDERIVE_SPEED   in_a[0] = u, in_b[0] = v;  out[0] = s:
 *      uu = u u;  vv = v v;  s = sqrtf(uu + vv)
 * SKDERIVE_DIFF    in_a[0] = a, in_b[0] = b;  out[0] = a - b
 * SKDERIVE_COLUMN  n_levels = L (2 <= L <= SKDERIVE_MAX_LEVELS); level k: in_a[k] = q_k, in_b[k] = u_k, in_c[k] = v_k, weight[k] = w_k
 *      (fp32, from the host);  out[0 .. 3] = ivtu, ivtv, ivt, iwv:
 *      t_k = w_k q_k;  iwv = (..(t_0 + t_1) + ..) + t_{L-1};  ivtu = (..(t_0 u_0 + t_1 u_1) + ..) + t_{L-1} u_{L-1};  ivtv likewise with v;
 *      ivt = sqrtf(ivtu ivtu + ivtv ivtv), as SPEED.  Sums run in level order k = 0 .. L - 1.  Each q plane is read once, and each u and v
 *      plane once (not at all when only iwv is asked for), whichever outputs are requested.
 * SKDERIVE_VORTDIV in_a[0] = u, in_b[0] = v;  out[0] = vo, out[1] = div;  needs `rowc`, a DEVICE table [H][4] of fp32 made by the host.
 *      With e / w = columns (i +- 1) mod W, n = row min(j + 1, H - 1), s = row max(j - 1, 0) and (A, B+, B-) = rowc[j][0 .. 2]:
 *         t1 = A (v_e - v_w);  t2 = B+ u_n;  t3 = B- u_s;  vo  = t1 - (t2 - t3)         (the zeta of skyrim_track.h)
 *         d1 = A (u_e - u_w);  d2 = B+ v_n;  d3 = B- v_s;  div = d1 + (d2 - d3)
 *      Interior rows 1 .. H - 2: the coefficients mean what they mean in skyrim_track.h, lat in radians, a = 6371000 m:
 *         A = 1 / (2 a cos(lat_j) dlon),  B+ = cos(lat_{j+1}) / (a cos(lat_j) (lat_{j+1} - lat_{j-1})),  B- = cos(lat_{j-1}) / (same).
 *      Rows 0 and H - 1 follow `edge_first` / `edge_last`:
 *         SKDERIVE_EDGE_ONESIDED (the row is not a pole): the same formula; n or s is the row itself (the clamp above), and the host writes
 *            B+- with lat_n - lat_s of the two rows that are read: the meridional difference is one-sided.
 *         SKDERIVE_EDGE_POLE: every point of the row gets the polar-cap value, from Stokes' and Gauss' theorems on the cap bounded by
 *            the neighbouring row r (1 or H - 2):  vo = (float)((double)rowc[j][0] ubar),  div = (float)((double)rowc[j][1] vbar), where
 *            ubar, vbar = the float64 means of u and v over row r, summed in a fixed order (lane l of a 64-lane wave sums the columns
 *            l, l + 64, .. in that order; the lanes are then combined by the xor butterfly 32, 16, .. 1) and divided by W.  The host
 *            supplies rowc[j][0] = +-cos(lat_r) / (a (1 - |sin(lat_r)|)), + at the north pole, - at the south pole, and
 *            rowc[j][1] = -rowc[j][0] (outflow from the pole is positive divergence).
 *      The library cannot read the table, so no access depends on its contents; it checks H >= 3 and W >= 4.
 * in_* and out entries an op does not use are ignored.
 *
 * Shape of the computation.  One launch covers all members and all ops (a program with more than SKDERIVE_LEVELS_PER_LAUNCH column levels
 * in total is split into launches of whole ops); a second tiny launch writes the pole rows.  A wave takes one tile of one op of one
 * member: member and op are wave-uniform (scalar registers), a lane's address is the member's pointer plus one 32-bit byte offset.
 * SPEED, DIFF and COLUMN walk the H W points of a plane 512 at a time.  VORTDIV tiles are 8 rows by 62 lanes: lanes 0 and 63 hold the
 * halo columns, the east and west neighbours come from lane shuffles, and a tile's rows slide through registers, so each of the ten
 * rows it needs is loaded once.  When every member pointer and `out` are 16-byte aligned, member_stride and W are multiples of 4, a lane
 * loads and stores 16 bytes (four columns); otherwise the scalar path runs.  Both paths do the same arithmetic per point: their
 * results are bit-equal.  No scratch memory, no LDS, no atomics.
 *
 * Bounds, against exact arithmetic on the same fp32 inputs (states, weights and rowc): |out - exact| <= k u S + tiny, u = 2^-24, k = the
 * number of fp32 roundings on the path (plus one for the products of roundings), S = the output's formula with every signed addend
 * replaced by its absolute value:
 *   s:     k = 4, S = s.  One rounding per product and one for the sum, all addends >= 0: relative 2u under the root; the root halves it
 *          and adds its own rounding: 3u.  tiny = 2^-74 (a product that underflows moves the root by at most sqrt(2^-149)).
 *   diff:  k = 1, S = |a| + |b|, tiny = 0 (a difference of fp32 numbers does not underflow to a wrong value).
 *   iwv:   k = L, S = sum_k |w_k q_k|: one rounding per term, L - 1 additions, each term passes through at most L roundings.
 *   ivtu:  k = L + 3 (L + 1 roundings per term: two products, L - 1 additions), S_u = sum_k |w_k q_k u_k|;  ivtv likewise, S_v.
 *   ivt:   k = L + 7, S = sqrt(S_u^2 + S_v^2): the errors of ivtu and ivtv move the root by at most (L + 3) u sqrt(S_u^2 + S_v^2) (the
 *          Euclidean norm is 1-Lipschitz), and the root of the computed components carries 4 u ivt <= 4 u S as for s.  tiny = 2^-74.
 *   vo:    k = 4, S = |A| (|v_e| + |v_w|) + |B+ u_n| + |B- u_s|, exactly as skyrim_track.h counts it (3 roundings on the longest path);
 *   div:   k = 4, S = |A| (|u_e| + |u_w|) + |B+ v_n| + |B- v_s|.
 *   pole:  |out - exact| <= (u + 2^-40) |rowc| mean_i |x_{r,i}| + tiny: one rounding to fp32; 2^-40 covers the float64 sum, the division
 *          and the product, as in skyrim_score.h.
 *   tiny = 2^-126 for the sums and differences of products (iwv, ivtu, ivtv, vo, div, pole): at most k products round in the
 *   subnormal range, each off by at most 2^-150.
 *
 * Limits: C H W <= 2^30 and D H W <= 2^30 (32-bit byte offsets), member_stride >= D H W, H >= 3, W >= 4, member and output pointers 4-byte
 * aligned, rowc 16-byte aligned (required with a VORTDIV op, else ignored).  `member_align` is the caller's statement of the alignment, in bytes,
 * that ALL M member pointers share (4 or 16) -- the library cannot read the device array. */
#ifndef SKYRIM_DERIVE_H
#define SKYRIM_DERIVE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SKDERIVE_ABI_VERSION 1
#define SKDERIVE_E_ARG (-1) /* bad argument: NULL or misaligned pointer, a count, index or slot outside its range, a slot written twice */
#define SKDERIVE_E_HIP (-2) /* a launch failed */
#define SKDERIVE_MAX_MEMBERS 64
#define SKDERIVE_MAX_OPS 16
#define SKDERIVE_MAX_LEVELS 16
#define SKDERIVE_LEVELS_PER_LAUNCH 128

#define SKDERIVE_SPEED 1
#define SKDERIVE_DIFF 2
#define SKDERIVE_COLUMN 3
#define SKDERIVE_VORTDIV 4

#define SKDERIVE_EDGE_ONESIDED 1
#define SKDERIVE_EDGE_POLE 2

typedef struct {
    int32_t kind;                          /* SKDERIVE_SPEED ... */
    int32_t n_levels;                      /* COLUMN: L; ignored otherwise */
    int32_t in_a[SKDERIVE_MAX_LEVELS];     /* SPEED, VORTDIV: u; DIFF: a; COLUMN: q_k */
    int32_t in_b[SKDERIVE_MAX_LEVELS];     /* SPEED, VORTDIV: v; DIFF: b; COLUMN: u_k */
    int32_t in_c[SKDERIVE_MAX_LEVELS];     /* COLUMN: v_k */
    float weight[SKDERIVE_MAX_LEVELS];     /* COLUMN: w_k */
    int32_t out[4];                        /* SPEED: s; DIFF: a - b; VORTDIV: vo, div; COLUMN: ivtu, ivtv, ivt, iwv; -1: not computed */
} skderive_op;

typedef struct {
    const float* const* members; /* device array of M device pointers */
    int M;
    int member_align;            /* bytes every member pointer is aligned to (4 or 16) */
    int C, H, W;
    int D;                       /* output channels per member */
    float* out;                  /* [M][member_stride], the first D H W elements of each member's part are the planes */
    size_t member_stride;        /* in elements */
    const float* rowc;           /* [H][4]; required with a VORTDIV op */
    int edge_first, edge_last;   /* SKDERIVE_EDGE_*: rows 0 and H - 1 of VORTDIV; ignored without one */
    int n_ops;
    skderive_op ops[SKDERIVE_MAX_OPS];
} skderive_desc;

int skderive_abi_version(void);

int skderive_run(const skderive_desc* desc, void* stream);

#ifdef __cplusplus
}
#endif
#endif
