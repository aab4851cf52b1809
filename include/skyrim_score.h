/* C ABI of forecast verification on the device: the scores of M member states (M = 1: a deterministic forecast) against a truth state,
 * area-weighted per channel, made where the states lie in HBM.  Only a few doubles per channel go back to the caller.
 *
 * Conventions of skyrim_io.h and skyrim_ens.h: all data pointers are device pointers; every call is asynchronous on `stream` (a
 * hipStream_t); nothing is allocated inside; the return code is 0, SKSCORE_E_ARG or SKSCORE_E_HIP; argument errors are found before
 * anything touches the GPU, so they are reported on a machine without one.
 *
 * ---- skscore_run ---------------------------------------------------------------------------------------------------------------------
 * States are contiguous float32 (C, H, W): M members (a DEVICE array of M pointers, 1 <= M <= SKSCORE_MAX_MEMBERS), the truth y and,
 * for the ACC sums, a climatology c.  Channels [c0, c0 + nc) are scored.  lat_weight holds H float64 weights w_j (any positive scale).
 *
 * Per point (all in fp32, sums in member order m = 0 .. M - 1):
 *   e_m = x_m - y                                        the error, so that roundings are relative to the error and not to the field
 *   eb  = (sum_m e_m) / M                                the error of the ensemble mean
 *   A   = (sum_m |e_m|) / M
 *   d_m = x_m - x_0,  db = (sum_m d_m) / M
 *   v   = sum_m (d_m - db)^2 / (M - 1)                   the unbiased member variance (the same number as with e_m - eb: a variance does
 *                                                        not move with the origin; with d_m equal members give exactly 0); 0 for M = 1
 *   B   = sum_{i < M - 1} (i + 1)(M - 1 - i) (s_{i+1} - s_i) / (M (M - 1))
 *                                                        s = the member values ascending (a bitonic network in registers).  This equals
 *                                                        sum_{m<n} |x_m - x_n| / (M (M - 1)) = sum_i (2i - M + 1) s_i / (M (M - 1)):
 *                                                        gap i lies between (i + 1)(M - 1 - i) pairs.  Every addend is >= 0, the integer
 *                                                        factor is exact, so B is accurate relative to B itself.  0 for M = 1
 *   r   = #{m : x_m < y}                                 strict, no tie-breaking: 0 .. M
 *   a   = y - c,  f = eb + a                             anomalies of the truth and of the ensemble mean
 *
 * Per channel, with the area mean <t> = sum_j w_j sum_i t_ji / (W sum_j w_j), one double each in out[cc][slot] (cc = channel - c0):
 *   flag SKSCORE_DET :  SKSCORE_BIAS = <eb>,  SKSCORE_MAE = <|eb|>,  SKSCORE_MSE = <eb^2>
 *   flag SKSCORE_VAR :  SKSCORE_VARIANCE = <v>
 *   flag SKSCORE_CRPS:  SKSCORE_ABS = <A>,  SKSCORE_PAIR = <B>,  SKSCORE_CRPS_FAIR = <A> - <B>   (the fair estimator; M = 1: equal to MAE)
 *   flag SKSCORE_ACC :  SKSCORE_FA = <f a>,  SKSCORE_FF = <f^2>,  SKSCORE_AA = <a^2>             (needs `clim`)
 *   flag SKSCORE_RANK:  counts[cc][j][r] = number of points of row j with rank r, r = 0 .. M: exact int32 (needs `counts`, [nc][H][M + 1])
 * Slots of groups that were not asked for are NOT written, and what they need is not computed: the M = 1 instantiation carries no
 * sort, nor does any call without SKSCORE_CRPS.  A non-finite member or truth value makes every requested slot of ITS channel non-finite
 * (a non-finite climatology value: the three ACC slots) and touches no other channel; rank counts are integers and follow the
 * comparison (false for NaN).  Nothing is masked.
 *
 * Shape of the computation.  Stage 1, one pass: every member value and every truth value of the range is read from HBM once.  One wave
 * owns one latitude row: each lane forms the fp32 per-point terms above for the points i = lane, lane + 64, ... (4 consecutive points
 * per lane where alignment allows), adds each term to a FLOAT64 accumulator of its own, and a 6-step butterfly over the 64 lanes in
 * float64 gives the row sums, stored as row partials [nc][H][SKSCORE_PARTIALS] in the caller's workspace.  Rank counts are added up per
 * row with integer atomics in LDS (integer addition does not depend on order) and stored by the row's wave.  Stage 2, a small kernel:
 * one workgroup per channel multiplies the row partials by w_j and sums the H rows in float64 -- thread t the rows t, t + 256, ... in
 * ascending order, then a fixed tree over the 256 threads.  No floating-point atomics anywhere: results are bitwise reproducible.
 *
 * Bound.  With u = 2^-24, every fp32 rounding happens inside ONE point's term; all sums over points are float64.  Against exact
 * arithmetic on the same fp32 inputs, |slot - exact| <= (k u + 2^-40) S, where S is the slot's formula with every signed addend replaced
 * by its absolute value (D = sum |d_m| / M, g_m = |d_m| + D):
 *   BIAS, MAE, ABS:  k = M + 1,   S = <A>            M - 1 additions of terms with one rounding each, one division
 *   MSE:             k = 2M + 3,  S = <A^2>
 *   VARIANCE:        k = 2M + 7,  S = <sum g_m^2 / (M - 1)>
 *   PAIR:            k = M + 1,   S = <B>            CRPS_FAIR:  k = M + 1,  S = <A> + <B>
 *   FA:              k = M + 4,   S = <(A + |a|) |a|>;     FF:  k = 2M + 5,  S = <(A + |a|)^2>;     AA:  k = 3,  S = <a^2>
 * (2^-40 covers the float64 sums: W / 64 + H / 256 + 16 roundings of 2^-53 on a path, fewer than 2^13 for grids of up to 2^18 points
 * a side.)  No path holds more than 2M + 7 fp32 roundings.
 *
 * Limits: C * H * W <= 2^30 (a member's address is its pointer, wave-uniform, plus ONE 32-bit per-lane byte offset).  Member, truth
 * and climatology pointers need 4-byte alignment; when all are 16-byte aligned (`member_align` = 16: the caller's statement for the M
 * member pointers, which the library cannot read) and W is a multiple of the lane's vector width, the vector path is taken.  The two
 * paths give a lane different points of its row, so their float64 sums may differ in the last bits; each path is reproducible.  `workspace` needs 8-byte alignment and skscore_workspace_bytes(C, H, M, flags) bytes. */
#ifndef SKYRIM_SCORE_H
#define SKYRIM_SCORE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SKSCORE_ABI_VERSION 1
#define SKSCORE_E_ARG (-1) /* bad argument: NULL or misaligned pointer, a count outside its range, a workspace too small */
#define SKSCORE_E_HIP (-2) /* the launch failed */
#define SKSCORE_MAX_MEMBERS 64

/* flags: the groups of outputs */
#define SKSCORE_DET 1
#define SKSCORE_VAR 2
#define SKSCORE_CRPS 4
#define SKSCORE_ACC 8
#define SKSCORE_RANK 16
#define SKSCORE_ALL_FLAGS 31

/* slots of out[cc][SKSCORE_SLOTS] */
#define SKSCORE_BIAS 0
#define SKSCORE_MAE 1
#define SKSCORE_MSE 2
#define SKSCORE_VARIANCE 3
#define SKSCORE_CRPS_FAIR 4
#define SKSCORE_ABS 5
#define SKSCORE_PAIR 6
#define SKSCORE_FA 7
#define SKSCORE_FF 8
#define SKSCORE_AA 9
#define SKSCORE_SLOTS 10
#define SKSCORE_PARTIALS 9 /* doubles per (channel, row) in the workspace */

int skscore_abi_version(void);

/* bytes of workspace a call on (C, H, .) states needs for any channel range; 0 for arguments skscore_run would refuse */
size_t skscore_workspace_bytes(int C, int H, int M, int flags);

typedef struct {
    const float* const* members; /* device array of M device pointers */
    int M;
    int member_align;            /* bytes every member pointer is aligned to (4 or 16) */
    const float* truth;          /* (C, H, W) */
    const float* clim;           /* (C, H, W); required with SKSCORE_ACC, else ignored */
    int C, H, W;
    int c0, nc;                  /* the channel range; nc == 0 launches nothing */
    const double* lat_weight;    /* [H] */
    int flags;                   /* SKSCORE_DET | ... : at least one */
    double* out;                 /* [nc][SKSCORE_SLOTS]; required unless flags == SKSCORE_RANK */
    int32_t* counts;             /* [nc][H][M + 1]; required with SKSCORE_RANK */
    void* workspace;
    size_t workspace_bytes;
} skscore_desc;

int skscore_run(const skscore_desc* desc, void* stream);

#ifdef __cplusplus
}
#endif
#endif
