/* C ABI of regridding on the device: M member states of one valid time on a latitude-longitude grid (H, W) are mapped to another
 * latitude-longitude grid (Ho, Wo) -- coarser (first-order conservative), finer (bilinear), or a regional box (any method) -- where the
 * states lie in HBM, and written as nc compact channels per member.  The ensemble statistics (skyrim_ens.h) and the scorer
 * (skyrim_score.h) then read the regridded planes like any others.
 *
 * On such grids every method is a SEPARABLE, BANDED linear map: an output row reads a run of consecutive source rows, an output column a
 * run of consecutive (periodic) source columns.  The library knows nothing of methods; it applies two small tables the host makes.
 *
 * Conventions of skyrim_derive.h, skyrim_track.h, skyrim_score.h and skyrim_ens.h: all data pointers are device pointers; every call is
 * asynchronous on `stream` (a hipStream_t); nothing is allocated inside; the return code is 0, SKREGRID_E_ARG or SKREGRID_E_HIP; argument
 * errors are found before anything touches the GPU, so they are reported on a machine without one.
 *
 * ---- skregrid_run ---------------------------------------------------------------------------------------------------------------------
 * States are contiguous float32 (C, H, W): a DEVICE array of M member pointers (1 <= M <= SKREGRID_MAX_MEMBERS), rows j = latitudes as
 * the model orders them, columns i = longitudes, periodic.  `channels` is a HOST list inside the descriptor of nc channel indices
 * (1 <= nc <= SKREGRID_MAX_CHANNELS, each in [0, C), any order, repeats allowed).  Output: float32
 * out[m * member_stride + (k * Ho + J) * Wo + I] for the k-th listed channel; nothing else in `out` is touched.
 *
 * A table (skregrid_table, one for the rows and one for the columns, the same layout) is three DEVICE arrays over the n_out outputs of
 * its axis: start[n_out] (int32), count[n_out] (int32, 1 <= count <= SKREGRID_MAX_TAPS) and weight[n_out][SKREGRID_MAX_TAPS] (fp32, the
 * entries beyond count are padding and are not read).  The row taps of output row J are the source rows start + t, t < count; the column
 * taps of output column I are the source columns (start + t) mod W.
 *
 * All arithmetic is fp32, every operation rounded on its own: the library is built with contraction to fma OFF (-ffp-contract=off).
 * Sums run in tap order and the accumulator STARTS AS THE FIRST PRODUCT, not as 0.  With wr_t, r_t the nr row taps of J and wc_t, c_t the
 * nc column taps of I:
 *      v[i]      = (..(wr_0 x[r_0][i] + wr_1 x[r_1][i]) + ..) + wr_{nr-1} x[r_{nr-1}][i]       for the source columns i of the row strip
 *      out[J][I] = (..(wc_0 v[c_0]    + wc_1 v[c_1])    + ..) + wc_{nc-1} v[c_{nc-1}]
 * A single tap of weight 1.0 on both axes is therefore a bit copy: -0 stays -0, a quiet NaN keeps its payload.  Nothing is masked: a
 * non-finite input reaches exactly the outputs whose taps read it (v of a column no column tap of the row names is never used).
 *
 * The library cannot read the tables, so NO ACCESS DEPENDS ON THEIR CONTENTS BEYOND A CLAMP: start is clamped into [0, H - 1] (rows) or
 * [0, W - 1] (columns), count into [1, SKREGRID_MAX_TAPS], every row index to min(., H - 1), every column index wraps at W.  A wrong
 * table gives wrong numbers, never an access outside a member's (C, H, W) or the table's own n_out entries.
 *
 * Shape of the computation.  One workgroup of 256 lanes takes one (member, channel, output row) and walks those with the grid's stride,
 * output row fastest, so neighbouring workgroups share their boundary source row in the L2.  Member, channel and row are wave-uniform:
 * the member pointer, the channel and the row taps are scalar loads, a lane's address is the member's pointer plus one 32-bit byte offset.
 *   1. vertical pass: a lane owns source columns and accumulates the nr rows in registers, four rows in flight; every global load is
 *      coalesced, 16 bytes per lane when `member_align` is 16 and W is a multiple of 4, else 4 bytes (the scalar path: the same
 *      arithmetic per point, bit-equal results).  v goes to an LDS strip of W floats (<= 32 KiB).
 *   2. after one barrier, a lane per output column takes its nc taps from the strip (its weights come four at a time, 16 bytes, from the
 *      column table) and stores; the store is coalesced.
 * The tap loops have run-time counts; weights are never held in an indexed register array.  No scratch memory, no atomics.
 *
 * Bound, against exact arithmetic on the same fp32 inputs and fp32 weights: |out - exact| <= k u S + tiny with u = 2^-24,
 *      S = sum_t sum_s |wc_t wr_s x[r_s][c_t]|,    k = nr + nc + 1,    tiny = 2^-126.
 * The count: a term wc_t wr_s x passes through one rounding for the product wr_s x, at most nr - 1 for the additions of the vertical sum
 * (the first two terms meet all nr - 1 of them, later ones fewer), one for the product with wc_t and at most nc - 1 for the additions of
 * the horizontal sum: nr + nc roundings, each a factor (1 + d), |d| <= u.  (1 + u)^(nr + nc) - 1 <= (nr + nc + 1) u while
 * (nr + nc)^2 u <= 1, which 64^2 2^-24 satisfies: the "+ 1" pays for the products of roundings.  tiny: at most nr nc + nc <= 1056
 * products round in the subnormal range, each off by at most 2^-150, and an inner one is carried to the output through one further
 * weight; 2^-126 covers that while |wc| <= 2^13.
 *
 * ---- skregrid_validate ----------------------------------------------------------------------------------------------------------------
 * Checks HOST copies of one table before they are uploaded: 0 when n_out >= 1, n_src >= 1, every start in [0, n_src - 1], every count in
 * [1, min(SKREGRID_MAX_TAPS, n_src)], start + count <= n_src unless `periodic`, every weight within count finite and not zero;
 * SKREGRID_E_ARG otherwise or for a NULL pointer.  Touches no GPU.
 *
 * Limits: C H W <= 2^30 and nc Ho Wo <= 2^30 (32-bit byte offsets), member_stride >= nc Ho Wo, H >= 2, 4 <= W <= SKREGRID_MAX_W, Ho >= 1,
 * Wo >= 1, member and output pointers 4-byte aligned, the six table pointers 16-byte aligned.  `member_align` is the caller's statement of
 * the alignment, in bytes, that ALL M member pointers share (4 or 16) -- the library cannot read the device array. */
#ifndef SKYRIM_REGRID_H
#define SKYRIM_REGRID_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SKREGRID_ABI_VERSION 1
#define SKREGRID_E_ARG (-1) /* bad argument: NULL or misaligned pointer, a count, size, index or stride outside its range, a bad table entry */
#define SKREGRID_E_HIP (-2) /* a launch failed */
#define SKREGRID_MAX_MEMBERS 64
#define SKREGRID_MAX_CHANNELS 256
#define SKREGRID_MAX_TAPS 32
#define SKREGRID_MAX_W 8192

typedef struct {
    const int32_t* start;  /* [n_out] */
    const int32_t* count;  /* [n_out] */
    const float* weight;   /* [n_out][SKREGRID_MAX_TAPS] */
} skregrid_table;

typedef struct {
    const float* const* members; /* device array of M device pointers */
    int M;
    int member_align;            /* bytes every member pointer is aligned to (4 or 16) */
    int C, H, W;                 /* the source states */
    int Ho, Wo;                  /* the target grid: n_out of `rows` and of `cols` */
    int nc;                      /* channels regridded */
    int32_t channels[SKREGRID_MAX_CHANNELS];
    skregrid_table rows, cols;
    float* out;                  /* [M][member_stride], the first nc Ho Wo elements of each member's part are the planes */
    size_t member_stride;        /* in elements */
} skregrid_desc;

int skregrid_abi_version(void);

int skregrid_run(const skregrid_desc* desc, void* stream);

int skregrid_validate(const int32_t* start, const int32_t* count, const float* weight, int n_out, int n_src, int periodic);

#ifdef __cplusplus
}
#endif
#endif
