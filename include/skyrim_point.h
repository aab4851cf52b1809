/* C ABI of point extraction on the device: M member states of one valid time on a latitude-longitude grid (H, W) are sampled at P
 * scattered points -- stations, cities, wind farms -- where the states lie in HBM, and written as nc compact channels of P values per
 * member.  Only those M nc P numbers then cross to the host.
 *
 * Scattered points are not a product of a row axis and a column axis, so skyrim_regrid.h's two tables cannot serve them.  A point is one
 * RECORD instead: the one or two row taps and the one or two column taps that regridding would give the same point on a node of a target
 * grid.  The record keeps the two axes apart -- not four (index, weight) pairs -- so that the arithmetic below is that of skyrim_regrid.h
 * at these tap counts, and a point on a node of a regrid target gets that node's value bit for bit.  The library knows nothing of methods
 * (bilinear, nearest): it applies the records the host makes.
 *
 * Conventions of skyrim_regrid.h, skyrim_derive.h and skyrim_agg.h: all data pointers are device pointers; every call is asynchronous on
 * `stream` (a hipStream_t); nothing is allocated inside; the return code is 0, SKPOINT_E_ARG or SKPOINT_E_HIP; argument errors are found
 * before anything touches the GPU, so they are reported on a machine without one.
 *
 * ---- skpoint_gather -------------------------------------------------------------------------------------------------------------------
 * States are contiguous float32 (C, H, W): a DEVICE array of M member pointers (1 <= M <= SKPOINT_MAX_MEMBERS), rows j = latitudes as the
 * model orders them, columns i = longitudes, periodic.  `channels` is a HOST list inside the descriptor of nc channel indices
 * (1 <= nc <= SKPOINT_MAX_CHANNELS, each in [0, C), any order, repeats allowed).  `records` is a DEVICE array of P skpoint_rec
 * (1 <= P <= SKPOINT_MAX_POINTS), 32 bytes each.  Output: float32 out[m * member_stride + k * P + p] for the k-th listed channel and the
 * p-th record; nothing else in `out` is touched.
 *
 * A record names the source row `row` (and row + 1 when nr == 2) with the weights wr0 (and wr1), and the source column `col` (and
 * (col + 1) mod W when ncol == 2) with the weights wc0 (and wc1).  The weights beyond a count are padding and are not used.
 *
 * All arithmetic is fp32, every operation rounded on its own: the library is built with contraction to fma OFF (-ffp-contract=off).  The
 * accumulator STARTS AS THE FIRST PRODUCT, not as 0.  With x the plane of the channel:
 *      v(c)  = wr0 x[row][c]                               (nr == 1)
 *            = wr0 x[row][c] + wr1 x[row + 1][c]           (nr == 2)
 *      out   = wc0 v(col)                                  (ncol == 1)
 *            = wc0 v(col) + wc1 v((col + 1) mod W)         (ncol == 2)
 * This is the formula of skyrim_regrid.h at one or two taps per axis.  Three properties follow:
 *   - a single tap of weight 1.0 on both axes is a bit copy: -0 stays -0, a quiet NaN keeps its payload;
 *   - nothing is masked: a non-finite input reaches exactly the points whose taps read it;
 *   - the result does not depend on the order of the records, on P or on the other records of the call.
 *
 * The library cannot read the records on the host, so NO ACCESS DEPENDS ON THEIR CONTENTS BEYOND A CLAMP: row is clamped into [0, H - 1],
 * row + 1 to min(., H - 1), col wraps at W (into [0, W - 1], whatever its sign), nr and ncol are clamped into [1, 2].  A wrong record gives
 * a wrong number, never an access outside a member's (C, H, W).
 *
 * Shape of the computation.  One workgroup of 256 lanes takes one tile of 256 points of one (member, chunk of SKPOINT_CHUNK listed
 * channels).  Member and channel are wave-uniform: the member pointer and the channel's plane offset are scalar loads, a lane's address
 * is the member's pointer plus one 32-bit byte offset.  A lane loads its record once, as two 16-byte loads, and forms its (up to) four
 * tap offsets once.  It then walks the chunk's channels in groups of four whose (up to) sixteen loads are all issued before the first is
 * used -- nothing else hides the latency of a gather here -- and stores; the store is coalesced over p.  The tap counts are run-time
 * values (a tap a lane does not use aliases its first one: the load is valid, costs no further line, and its value is dropped); no
 * indexed register arrays, no scratch, no LDS, no atomics.
 * The host should sort the points by (row, col) before the upload so that neighbouring lanes touch neighbouring lines, and undo the
 * permutation after the copy back; the library knows nothing of this.
 *
 * Bound, against exact arithmetic on the same fp32 inputs and fp32 weights: |out - exact| <= k u S + tiny with u = 2^-24,
 *      S = sum_t sum_s |wc_t wr_s x[r_s][c_t]|,    k = nr + ncol + 1,    tiny = 2^-126.
 * The count: a term wc_t wr_s x passes through one rounding for the product wr_s x, at most nr - 1 for the addition of the vertical sum,
 * one for the product with wc_t and at most ncol - 1 for the addition of the horizontal sum: nr + ncol roundings, each a factor (1 + d),
 * |d| <= u.  (1 + u)^(nr + ncol) - 1 <= (nr + ncol + 1) u while (nr + ncol)^2 u <= 1, which 4^2 2^-24 satisfies: the "+ 1" pays for the
 * products of roundings.  tiny: at most nr ncol + ncol <= 6 products round in the subnormal range, each off by at most 2^-150, and an
 * inner one is carried to the output through one further weight; 2^-126 covers that while |wc| <= 2^13.
 *
 * ---- skpoint_validate -----------------------------------------------------------------------------------------------------------------
 * Checks a HOST copy of the records before they are uploaded: 0 when P >= 1, H >= 1, W >= 2 and for every record row in [0, H - 1], not
 * (nr == 2 and row == H - 1), col in [0, W - 1], nr and ncol in {1, 2}, every USED weight (wr0, wc0, wr1 when nr == 2, wc1 when
 * ncol == 2) finite and not zero; SKPOINT_E_ARG otherwise or for a NULL pointer.  Touches no GPU.
 *
 * Limits: C H W <= 2^30 and nc P <= 2^30 (32-bit byte offsets), member_stride >= nc P, H >= 1, W >= 2, member and output pointers 4-byte
 * aligned, the member-pointer array 8-byte aligned, the records 16-byte aligned. */
#ifndef SKYRIM_POINT_H
#define SKYRIM_POINT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SKPOINT_ABI_VERSION 1
#define SKPOINT_E_ARG (-1) /* bad argument: NULL or misaligned pointer, a count, size, index or stride outside its range, a bad record */
#define SKPOINT_E_HIP (-2) /* a launch failed */
#define SKPOINT_MAX_MEMBERS 64
#define SKPOINT_MAX_CHANNELS 256
#define SKPOINT_MAX_POINTS (1 << 20)
#define SKPOINT_CHUNK 8 /* listed channels one workgroup walks */

typedef struct {
    int32_t row, col;  /* first row tap, first column tap */
    int32_t nr, ncol;  /* taps per axis, 1 or 2 */
    float wr0, wr1;    /* row weights */
    float wc0, wc1;    /* column weights */
} skpoint_rec;

typedef struct {
    const float* const* members; /* device array of M device pointers */
    int M;
    int C, H, W;                 /* the source states */
    int nc;                      /* channels sampled */
    int32_t channels[SKPOINT_MAX_CHANNELS];
    const skpoint_rec* records;  /* device, [P] */
    int P;
    float* out;                  /* [M][member_stride], the first nc P elements of each member's part are the values */
    size_t member_stride;        /* in elements */
} skpoint_desc;

int skpoint_abi_version(void);

int skpoint_gather(const skpoint_desc* desc, void* stream);

int skpoint_validate(const skpoint_rec* host_records, int P, int H, int W);

#ifdef __cplusplus
}
#endif
#endif
