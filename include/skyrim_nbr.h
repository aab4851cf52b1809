/* C ABI of neighbourhood fields on the device: the maximum, minimum, area-weighted mean and the fraction above a threshold of a channel
 * over the great-circle disc around every grid point, folded per member into a buffer that has the layout of skderive_run's `out`, so the
 * ensemble statistics (skyrim_ens.h), the scorer (skyrim_score.h), the event counter (skyrim_event.h) and the point sampler
 * (skyrim_point.h) read a neighbourhood field like any other plane.  It is the spatial sibling of skyrim_agg.h.
 *
 * Conventions of skyrim_agg.h: all data pointers are device pointers; sknbr_run is asynchronous on `stream` (a hipStream_t); nothing is
 * allocated inside and no workspace is needed; the return code is 0, SKNBR_E_ARG or SKNBR_E_HIP; argument errors are found before
 * anything touches the GPU, so they are reported on a machine without one.  sknbr_check is host-only: the argument checks of sknbr_run
 * and nothing else.
 *
 * ---- the disc ----------------------------------------------------------------------------------------------------------------------------
 * The grid is regular in longitude (W columns that close the circle) and has H rows.  The library does not know latitudes or kilometres:
 * a radius is an integer table the host makes once (skyrim_amd/neighbourhood.py `discs`), `half`, int32 (H, 2 reach + 1) on the device:
 * half[j * (2 reach + 1) + reach + d] = n says that the disc around any point (j, i) of row j holds, of row j + d, the columns
 * i - n ... i + n (periodic), or the whole row, each of its W points once, when 2 n + 1 >= W; n = -1: no point of that row.  The kernel
 * reads a negative n, and a row j + d outside the grid, as "no point", and n > W / 2 as W / 2, so that no table makes it read out of bounds.
 * S(j, i) is the set of the distinct grid points so named; N = |S|.  `weights`: one float64 per row (the host passes the area weights,
 * verify.area_weights), used by MEAN only.
 *
 * ---- sknbr_run ---------------------------------------------------------------------------------------------------------------------------
 * States are contiguous float32 (C, H, W): a DEVICE array of M member pointers (1 <= M <= SKNBR_MAX_MEMBERS).  Output: float32
 * out[m * member_stride + (d * H + j) * W + i], 0 <= d < D.  The program is n_ops <= SKNBR_MAX_OPS ops, a HOST array inside the
 * descriptor; each op reads the input channel `in` (in [0, C)) over the discs of the radius `radius` (an index in [0, n_radii)) and writes
 * the slot `out` (in [0, D)).  No slot is named twice.  Slots no op names, and everything beyond D H W of a member's part, are not touched.
 * With x the values of the channel on S = S(j, i):
 *
 * SKNBR_MAX / SKNBR_MIN   the largest / smallest value of S: an exact selection.  NaN if any value of S is NaN.  Infinities compare as
 *                         numbers.  When +0.0 and -0.0 are both extreme the sign of the result is unspecified.
 * SKNBR_FRAC_ABOVE        (float)((double)count / (double)N), count = the number of points of S with x > thr (strict; thr = +inf counts
 *                         nothing, thr = -inf every value but -inf).  Unweighted.  NaN if any value of S is NaN; infinities compare as
 *                         numbers.  Exact: count and N are integers, the quotient is rounded once to float64 and once to float32.
 * SKNBR_MEAN              area-weighted: (float)(sum_r w_r s_r / sum_r w_r n_r) over the rows r of S, s_r the sum of the row's n_r values
 *                         in S, in float64 (below).  NaN if any value of S is NaN or +-inf.
 * `thr` is ignored by the kinds that do not use it.  Every NaN written is the quiet NaN 0x7fc00000.
 *
 * Containment.  A non-finite input changes the outputs of exactly the points whose disc contains it, for the ops that read that channel
 * of that member, and nothing else: non-finite values are COUNTED per range (an integer prefix) and only the finite values enter a
 * sum, so no NaN and no inf - inf travels along a row.
 *
 * ---- what was built ----------------------------------------------------------------------------------------------------------------------
 * The row is the unit: within one (centre row, source row) pair the half-width is the same for every column.  A workgroup of 256 lanes
 * owns one (member, op, centre row): a block of B = 1 centre rows and a group of one op, the smallest case of the form in which a
 * workgroup owns several of each.  It streams the source rows j - reach ... j + reach that the table does not mark empty through LDS,
 * in ascending order (the next row is fetched into registers while the present one is worked on), and builds per source row what the op
 * needs:
 *   MAX, MIN      a doubling table: level k holds the extreme of 2^k consecutive periodic points; two row buffers, level k made from level
 *                 k - 1, up to k = floor(log2(2 n + 1)); a range is the extreme of two overlapping entries.  A whole row: k = ceil(log2 W).
 *   FRAC_ABOVE    inclusive integer prefixes of (x > thr) and of (x is NaN); a periodic range costs two or three reads.
 *   MEAN          an inclusive float64 prefix of the finite values (a non-finite value enters as 0) and an integer prefix of the
 *                 non-finite ones.
 * Each lane keeps the accumulators of its columns (i = lane + 256 q, q < SKNBR_MAX_W / 256) in registers and writes each output once.
 * The input rows of a disc are read once per (op, centre row), 2 reach + 1 times in all per op: from the caches, the plane itself comes
 * from HBM once.  No atomics, no scratch memory, every sum in a fixed order: two runs give the same bits.
 *
 * Accuracy.  MAX, MIN and FRAC_ABOVE are exact.  MEAN: the prefix of a row is made by 256 lanes -- lane t sums its ceil(W / 256)
 * consecutive values in order, an inclusive scan combines the lanes' totals -- so every prefix is a sum of at most W values in a fixed
 * order and carries at most (W - 1) u A_r, u = 2^-53, A_r the sum of |x| over the finite values of the WHOLE source row r; a periodic range
 * is made from at most three prefixes with two additions: |s_r - exact| <= 3 (W + 1) u A_r.  One product with w_r, at most R additions over
 * the R rows of the disc in ascending order (numerator and denominator alike), one division, one rounding to float32:
 *     |mean - exact| <= 2^-24 |exact| + 2^-149 + (3 (W + 1) + 2 R + 8) u sum_r w_r A_r / sum_r w_r n_r     to first order in u.
 * The second term is far below the first unless a row holds values many orders of magnitude larger than the disc's.
 *
 * Limits: W <= SKNBR_MAX_W, reach <= SKNBR_MAX_REACH, C H W <= 2^30 and D H W <= 2^30 (32-bit offsets), member_stride >= D H W,
 * C, H, W, D >= 1, 1 <= n_radii <= SKNBR_MAX_RADII, `members` and `weights` 8-byte aligned, `out` and every `half` 4-byte aligned.
 * `member_align` is the caller's statement of the alignment, in bytes, that ALL M member pointers share (4 or 16) -- the library cannot
 * read the device array; both give the same bits. */
#ifndef SKYRIM_NBR_H
#define SKYRIM_NBR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SKNBR_ABI_VERSION 1
#define SKNBR_E_ARG (-1) /* bad argument: NULL or misaligned pointer, a count, channel, slot, kind, radius or size outside its range, a slot named twice */
#define SKNBR_E_HIP (-2) /* a launch failed */
#define SKNBR_MAX_MEMBERS 64
#define SKNBR_MAX_OPS 16
#define SKNBR_MAX_RADII 4
#define SKNBR_MAX_W 2048    /* columns of a row: what the row buffers in LDS hold */
#define SKNBR_MAX_REACH 128 /* rows on either side of the centre row */

#define SKNBR_MAX 1
#define SKNBR_MIN 2
#define SKNBR_MEAN 3
#define SKNBR_FRAC_ABOVE 4

typedef struct {
    int32_t kind;   /* SKNBR_MAX ... */
    int32_t in;     /* input channel */
    int32_t out;    /* slot of the result */
    int32_t radius; /* index into `radii` */
    float thr;      /* FRAC_ABOVE */
} sknbr_op;

typedef struct {
    int32_t reach;       /* rows on either side */
    const int32_t* half; /* device (H, 2 reach + 1) */
} sknbr_radius;

typedef struct {
    const float* const* members; /* device array of M device pointers */
    int M;
    int member_align;            /* bytes every member pointer is aligned to (4 or 16) */
    int C, H, W;
    int D;                       /* slots per member */
    float* out;                  /* [M][member_stride], the first D H W elements of each member's part are the slots */
    size_t member_stride;        /* in elements */
    const double* weights;       /* device (H): the row weights of MEAN */
    int n_radii;
    sknbr_radius radii[SKNBR_MAX_RADII];
    int n_ops;
    sknbr_op ops[SKNBR_MAX_OPS];
} sknbr_desc;

int sknbr_abi_version(void);

/* host only: 0 or SKNBR_E_ARG, the argument checks of sknbr_run */
int sknbr_check(const sknbr_desc* desc);

int sknbr_run(const sknbr_desc* desc, void* stream);

#ifdef __cplusplus
}
#endif
#endif
