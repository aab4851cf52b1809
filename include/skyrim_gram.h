/* C ABI of ensemble scenarios on the device: the Gram matrix of M member states of one valid time -- the M x M area-weighted inner
 * products of the members' differences over a region -- made where the states lie in HBM, and fields that are linear combinations of
 * the members.  Clusters (scenarios), EOFs of the spread, representative members and the energy score are functions of that one small
 * matrix; the host does them in float64 (skyrim_amd/scenarios.py).  Only M'^2 doubles per channel go back to the caller.
 *
 * Conventions of skyrim_score.h and skyrim_point.h: all data pointers are device pointers; every call is asynchronous on `stream` (a
 * hipStream_t); nothing is allocated inside; the return code is 0, SKGRAM_E_ARG or SKGRAM_E_HIP; argument errors are found before
 * anything touches the GPU, so they are reported on a machine without one.
 *
 * ---- skgram_run -----------------------------------------------------------------------------------------------------------------------
 * States are contiguous float32 (C, H, W): M members (a DEVICE array of M pointers) and, optionally, a truth state y that is treated as
 * one more column with index M: M' = M + 1 with a truth, M' = M without; 2 <= M and M' <= SKGRAM_MAX_MEMBERS.  `channels` is a HOST list
 * inside the descriptor of nc channel indices (1 <= nc <= SKGRAM_MAX_CHANNELS, each in [0, C), any order, repeats allowed).  The region
 * is the rows [j0, j0 + nj) and the ni columns i0, i0 + 1, ... taken mod W (a box may cross the date line; 1 <= ni <= W, 0 <= i0 < W).
 * lat_weight holds H float64 weights w_j (any scale).
 *
 * Per point, in fp32:   d_m = x_m - x_0   (m = 0 .. M - 1),   d_M = y - x_0.
 * Member 0 is the origin, as in skyrim_score.h, so the roundings are relative to the spread and not to the field; d_0 is exactly 0.
 * Output, per listed channel cc: the M' x M' float64 matrix
 *      Gd[cc][m][n] = sum_j w_j sum_i d_m d_n            over the region,
 * at out[cc out_stride + m M' + n] (out_stride >= M'^2 doubles), written in full, bitwise symmetric; nothing else in `out` is touched.
 * Centring about the ensemble mean is NOT done here: double-centring a Gram matrix is exact M x M algebra, G = J Gd J with
 * J = I - 11'/M, which the host does in float64.  That keeps the kernel free of a cross-lane mean and the MFMA inputs plain differences.
 *
 * Shape of the computation.  A TILE is SKGRAM_TILE = 256 consecutive region points of ONE row (the last tile of a row is shorter), so a
 * tile has one weight.  The tiles of a channel are numbered row-major, t = (j - j0) ceil(ni / TILE) + q, and dealt to
 * G = min(number of tiles, SKGRAM_GROUPS) workgroups of 256 lanes per channel: workgroup g takes t = g, g + G, ...  For a tile, wave
 * v of the four stages the points 64 v .. 64 v + 63: lane = point, the member pointer is wave-uniform (one scalar load of the pointer
 * table per member), the loads of sixteen members are issued before the first is used, and each is one coalesced 256-byte segment.  The
 * lane subtracts its x_0 value and stores d into LDS as [member][point] with a row pitch of TILE + 1 words, so that the 32 members of
 * an operand read fall into 32 different banks.  Every member value of the region is read from HBM once.  After a barrier wave v takes
 * the 32 point pairs of the same quarter of the tile and feeds them to v_mfma_f32_32x32x2_f32: lane l holds member l & 31 at point
 * 64 v + 2 p + (l >> 5), and because A is the transpose of B for a Gram matrix, ONE register is both operands.
 * M' <= 32: one 32 x 32 accumulator block; M' <= 64: three, (lo, lo), (lo, hi), (hi, hi) -- the fourth is the transpose and is mirrored
 * at the output.  Lanes of padding members and points past a short tile's end feed 0.
 * The fp32 accumulator chain of a wave is one quarter tile: at most SKGRAM_CHAIN = 64 points.  It is then converted to float64,
 * multiplied by w_j and added to float64 accumulators in registers, which live across the workgroup's tiles.  At the end the four
 * waves' float64 blocks are added in the order 0, 1, 2, 3 through LDS and stored as the workgroup's partial [cc][g][block][32][32] in
 * the caller's workspace.  A second kernel sums the G partials of an entry in a fixed two-level order -- chunks of 32 partials in
 * ascending g, then the chunk sums in ascending order -- reading the partials' entry (min(m, n), max(m, n)) for [m][n] and [n][m].
 * No floating-point atomics, no scratch, no indexed register arrays.  The assignment of points to accumulators and the order of every
 * sum depend on the descriptor alone -- not on the device's CU count, not on timing: two calls give the same bits.
 *
 * Bound, against exact arithmetic on the same fp32 inputs, with u = 2^-24:
 *      |Gd[m][n] - exact| <= ((SKGRAM_CHAIN + 3) u + 2^-40) sum_j w_j sum_i |d_m| |d_n|      (|w_j|: the weights' absolute values).
 * The count: d_m and d_n carry one rounding each; the MFMA result is a k-ordered fmaf chain with one rounding per product, so a
 * product passes through at most SKGRAM_CHAIN roundings of the chain: SKGRAM_CHAIN + 2 factors (1 + d), |d| <= u, and
 * (1 + u)^(n) - 1 <= (n + 1) u while n^2 u <= 1, which 66^2 2^-24 satisfies.  2^-40 covers the float64 part: the product with w_j, at
 * most 2^12 additions in a workgroup's accumulator (the limit on the tiles below), 3 across the waves and 48 across the partials,
 * fewer than 2^13 roundings of 2^-53.  Products that underflow fp32 (|d_m d_n| < 2^-126) are outside the bound.
 *
 * Non-finite values.  Nothing is masked.  A non-finite value of member m != 0 (or of the truth, m = M) inside the region makes row m
 * and column m of ITS channel's matrix non-finite and no other entry: an MFMA output element depends on its own row and column operands
 * only.  A non-finite value of member 0 makes every d, and so the whole channel's matrix, non-finite.  No other channel is touched.
 *
 * ---- skgram_combine -------------------------------------------------------------------------------------------------------------------
 * K fields (1 <= K <= SKGRAM_MAX_OUT) that are linear combinations of the M members (2 <= M <= SKGRAM_MAX_MEMBERS): for every listed
 * channel and every point of the full (H, W) plane, in fp32, every operation rounded on its own (the library is built with contraction
 * to fma OFF):
 *      acc = b[k] x_0;      for m = 1 .. M - 1 ascending:   acc = acc + coef[k M + m] (x_m - x_0);      out[((k nc + cc) H + j) W + i] = acc.
 * coef[k M + 0] is not used.  `coef` (K x M) and `b` (K) are DEVICE float32 arrays.  One streaming kernel: a lane owns one point, each
 * member plane is read once for all K outputs, member and channel are wave-uniform (the coefficients are scalar loads), and the loads
 * of a group of eight members are issued before their use.  Instantiated on K, so the K accumulators are registers.  Nothing else in
 * `out` is touched.  A non-finite member value reaches the outputs at its point.
 *
 * Limits: C H W <= 2^30 (a member's address is its pointer, wave-uniform, plus ONE 32-bit per-lane byte offset); W >= 1, H >= 1;
 * nj ceil(ni / SKGRAM_TILE) <= 2^21 tiles per channel; K nc H W <= 2^30.  Member, truth and fp32 output pointers need 4-byte alignment
 * (all loads are single words: there is no vector path and no alignment statement), the member-pointer array, lat_weight, `out` of
 * skgram_run and `workspace` 8-byte alignment; `workspace` holds skgram_workspace_bytes(M', nc, nj, ni) bytes. */
#ifndef SKYRIM_GRAM_H
#define SKYRIM_GRAM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SKGRAM_ABI_VERSION 1
#define SKGRAM_E_ARG (-1) /* bad argument: NULL or misaligned pointer, a count, size or index outside its range, a workspace too small */
#define SKGRAM_E_HIP (-2) /* a launch failed */
#define SKGRAM_MAX_MEMBERS 64  /* M' */
#define SKGRAM_MAX_CHANNELS 32
#define SKGRAM_MAX_OUT 8       /* K of skgram_combine */
#define SKGRAM_TILE 256        /* points staged through LDS at a time */
#define SKGRAM_CHAIN 64        /* points of one fp32 accumulator chain: a wave's quarter of a tile */
#define SKGRAM_GROUPS 512      /* workgroups (= partials) per channel at most */

typedef struct {
    const float* const* members; /* device array of M device pointers */
    int M;
    const float* truth;          /* (C, H, W) or NULL: column M */
    int C, H, W;
    int nc;                      /* channels */
    int32_t channels[SKGRAM_MAX_CHANNELS];
    int j0, nj;                  /* rows [j0, j0 + nj) */
    int i0, ni;                  /* columns (i0 + q) mod W, q = 0 .. ni - 1 */
    const double* lat_weight;    /* [H] */
    double* out;                 /* [nc][out_stride], the first M'^2 elements of each channel's part are its matrix */
    size_t out_stride;           /* in doubles, >= M'^2 */
    void* workspace;
    size_t workspace_bytes;
} skgram_desc;

typedef struct {
    const float* const* members; /* device array of M device pointers */
    int M;
    int C, H, W;
    int nc;
    int32_t channels[SKGRAM_MAX_CHANNELS];
    const float* coef;           /* device, [K][M] */
    const float* b;              /* device, [K] */
    int K;
    float* out;                  /* [K][nc][H][W] */
} skgram_combine_desc;

int skgram_abi_version(void);

/* bytes of workspace skgram_run needs for M' columns (the truth counted), nc channels and a region of nj rows and ni columns; 0 for
 * arguments skgram_run would refuse */
size_t skgram_workspace_bytes(int Mp, int nc, int nj, int ni);

int skgram_run(const skgram_desc* desc, void* stream);

int skgram_combine(const skgram_combine_desc* desc, void* stream);

#ifdef __cplusplus
}
#endif
#endif
