/* C ABI of the two device passes of a breeding cycle (skyrim_amd/breeding.py): the area-weighted squared norm of every
 * member's difference from the control forecast, per channel, and the rescaled differences put back on the analysis, for all members
 * and all channels in one launch each.
 *
 * Conventions of skyrim_ens.h and skyrim_gram.h: all data pointers are device pointers; every call is asynchronous on `stream` (a
 * hipStream_t); nothing is allocated inside; the return code is 0, SKBREED_E_ARG or SKBREED_E_HIP; argument errors are found before
 * anything touches the GPU, so they are reported on a machine without one.  The library is built with contraction to fma OFF: every
 * operation below is rounded on its own.
 *
 * States are contiguous float32 (C, H, W), one history level.  The control state is a pointer of its own; the M members
 * (1 <= M <= SKBREED_MAX_MEMBERS) are a DEVICE array of M pointers, as in skyrim_ens.h.  The library cannot read that array, so the
 * caller gives the same M pointers a second time as a HOST array (`members_host`, `out_host`): NULL pointers, alignment and aliasing are
 * checked on the host copy, and the kernels read the device copy.  1 <= C <= SKBREED_MAX_CHANNELS, H >= 1, W >= 1, C H W <= 2^30 (an
 * address is a wave-uniform pointer plus one 32-bit per-lane byte offset).  State pointers need 4-byte alignment; when the control, every
 * member (and for skbreed_apply x_0 and every output) are 16-byte aligned and the row length allows it (W % 4 == 0 for the norms,
 * H W % 4 == 0 for the apply) the kernels load and store four floats at a time.  The two paths assign the same points to the same
 * accumulators in the same order: they give the same bits.
 *
 * ---- skbreed_norms --------------------------------------------------------------------------------------------------------------------
 *      S[m][c] = sum_j w_j sum_i d^2,      d = fl32(y_m[c][j][i] - y_0[c][j][i])         m < M, c < C
 * lat_weight holds H float64 weights w_j (any scale).  `S` is double [M][C], written in full; nothing else is touched.  d is ONE fp32
 * subtraction; d d is formed in float64, where it is exact (24 x 24 bits); everything from there on is float64.  No float atomics.
 *
 * Shape and order of the computation.  A TILE is SKBREED_TILE = 256 consecutive points of ONE row (the last tile of a row is shorter),
 * so a tile has one weight.  The tiles of a channel are numbered row-major, t = j ceil(W / TILE) + q, and dealt to
 * G = skbreed_groups(C, H, W) workgroups per channel, each ONE wave of 64 lanes: workgroup g takes t = g, g + G, ... in ascending order.
 * Lane l owns the points 4 l .. 4 l + 3 of the tile.  It reads its four y_0 values once per tile and keeps them in registers while it walks
 * the pointer table: the member pointer is wave-uniform (a scalar load), the loads of SKBREED_STAGE = 8 members are issued before the
 * first is used.  Per (tile, member) the lane forms
 *      p = ((d_0 d_0 + d_1 d_1) + d_2 d_2) + d_3 d_3            (points past the row's end give d = 0)
 *      a[m][l] = a[m][l] + w_j p
 * where a[m][l] is the lane's float64 accumulator of member m; the M x 64 accumulators live in LDS across the workgroup's tiles (no
 * indexed register arrays, no scratch).  At the end lane m sums a[m][0], a[m][1], ..., a[m][63] in ascending order and stores the
 * workgroup's partial [g][c][m] in the caller's workspace (skbreed_workspace_bytes(M, C, H, W) bytes).  A second, small kernel sums the G
 * partials of an entry in ascending g.  The assignment of points to accumulators and the order of every sum depend on the descriptor
 * alone -- not on the device's CU count, not on timing, not on the alignment path: two calls give the same bits.
 *
 * Bound, against exact arithmetic on the same fp32 inputs and float64 weights:
 *      |S[m][c] - exact| <= k 2^-53 sum_j |w_j| sum_i d^2,        k = min(3 + 1 + ceil(tiles / G) + 63 + (G - 1) + 1, H W + H + 2).
 * The count: every addend w_j d^2 is non-negative for non-negative weights (for weights of mixed sign the bound holds with |w_j|), so no
 * sum cancels and an addend's relative error is at most the number n of roundings it passes through, (1 + 2^-53)^n - 1 <= (n + 1) 2^-53
 * (n <= 2^26 here).  d d is exact.  On its way to S an addend passes through at most 3 additions inside p, 1 product with w_j,
 * ceil(tiles / G) additions in the lane's accumulator, 63 additions over the lanes and G - 1 over the partials.  An addition of an exact 0
 * does not round, and a sum of n non-zero terms, in whatever tree, has at most n - 1 additions whose operands are both non-zero: that
 * gives the second form: at most H W - 1 additions and one product on any path, n <= H W and n + 1 below H W + H + 2 (what one serial
 * sum over the plane with one product per row would need), which is the smaller count on small planes.
 *
 * Non-finite values.  Nothing is masked.  A non-finite value of member m in channel c makes S[m][c] non-finite and no other entry:
 * a[m][.] of that workgroup is the only accumulator it reaches.  A non-finite value of y_0 in channel c makes d of every member
 * non-finite there: column c, and no other column (a workgroup works on one channel).
 *
 * ---- skbreed_apply --------------------------------------------------------------------------------------------------------------------
 * For every member m < M, every channel c and every point, in fp32, every operation rounded on its own:
 *      t = y_m - y_0;      out_m = (f[m][c] == 0) ? x_0 : x_0 + f[m][c] t
 * `f` is a DEVICE table float [M][C].  Where f[m][c] is exactly 0 (of either sign) the element is a bit copy of x_0 -- a select, as in
 * sknoise_apply -- whatever t is: the sign of a zero of x_0 survives, a non-finite t does not reach the output.  Where f is non-zero a
 * non-finite value of x_0, y_0, y_m or f reaches exactly the elements that read it.  A negative f gives the mirrored member of a pair.
 * out_m may be any buffer that does not overlap x_0, y_0, the y of ANOTHER member or another output; out_m == y_m (in place) is allowed:
 * a lane reads its elements of y_m before it writes them, and nobody else reads them.  A partial overlap of out_m and y_m is refused.
 * One launch covers all members: a workgroup of 256 lanes takes 1024 points of one channel plane, reads x_0 and y_0 once and keeps them in
 * registers across the members; member and output pointers and f[m][c] are wave-uniform (scalar loads), the loads of SKBREED_STAGE
 * members are issued before the first is used.  The result is bit-equal to the same three numpy fp32 operations. */
#ifndef SKYRIM_BREED_H
#define SKYRIM_BREED_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SKBREED_ABI_VERSION 1
#define SKBREED_E_ARG (-1) /* bad argument: NULL or misaligned pointer, a count or size outside its range, a workspace too small, aliasing */
#define SKBREED_E_HIP (-2) /* a launch failed */
#define SKBREED_MAX_MEMBERS 64   /* SKENS_MAX_MEMBERS */
#define SKBREED_MAX_CHANNELS 256
#define SKBREED_TILE 256         /* points of one row a wave takes at a time: four per lane */
#define SKBREED_STAGE 8          /* members whose loads are in flight together */
#define SKBREED_MAX_GROUPS 256   /* workgroups (= partials) per channel at most */

typedef struct {
    const float* y0;                  /* (C, H, W): the control forecast */
    const float* const* members;      /* device array of M device pointers: y_m */
    const float* const* members_host; /* HOST array of the same M pointers */
    int M;
    int C, H, W;
    const double* lat_weight;         /* [H] */
    double* S;                        /* [M][C] */
    void* workspace;
    size_t workspace_bytes;
} skbreed_norms_desc;

typedef struct {
    const float* x0;                  /* (C, H, W): the analysis */
    const float* y0;                  /* (C, H, W): the control forecast */
    const float* const* members;      /* device array of M device pointers: y_m */
    const float* const* members_host; /* HOST array of the same M pointers */
    float* const* out;                /* device array of M device pointers: out_m */
    float* const* out_host;           /* HOST array of the same M pointers */
    int M;
    int C, H, W;
    const float* f;                   /* device, [M][C] */
} skbreed_apply_desc;

int skbreed_abi_version(void);

/* workgroups per channel of skbreed_norms: min(tiles, max(1, min(SKBREED_MAX_GROUPS, ceil(4096 / C)))), tiles = H ceil(W / SKBREED_TILE);
 * 0 for sizes skbreed_norms would refuse */
int skbreed_groups(int C, int H, int W);

/* bytes of workspace skbreed_norms needs (the partials, double [G][C][M]); 0 for arguments skbreed_norms would refuse */
size_t skbreed_workspace_bytes(int M, int C, int H, int W);

int skbreed_norms(const skbreed_norms_desc* desc, void* stream);

int skbreed_apply(const skbreed_apply_desc* desc, void* stream);

#ifdef __cplusplus
}
#endif
#endif
