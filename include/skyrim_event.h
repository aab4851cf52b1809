/* C ABI of event verification on the device: for threshold events "x > thr", the joint counts of (observed, members above) per latitude
 * row and the neighbourhood sums of the fractions skill score, made where the M member states and the truth lie in HBM.  Only integers
 * leave the kernels; every weight and every ratio (Brier, reliability, ROC, contingency scores, FSS) is float64 on the host
 * (skyrim_amd/events.py).
 *
 * Conventions of skyrim_score.h: all data pointers are device pointers; every call is asynchronous on `stream` (a hipStream_t); nothing is
 * allocated inside; the return code is 0, SKEVENT_E_ARG or SKEVENT_E_HIP; argument errors are found before anything touches the GPU, so
 * they are reported on a machine without one.
 *
 * ---- skevent_run ---------------------------------------------------------------------------------------------------------------------
 * States are contiguous float32 (C, H, W): M members (a DEVICE array of M pointers, 1 <= M <= SKEVENT_MAX_MEMBERS) and the truth y.
 * n_events <= SKEVENT_MAX_CHANNELS event channels are named by channel[e] (any order, repeats allowed), each with
 * 1 <= n_thr[e] <= SKEVENT_MAX_THRESHOLDS thresholds thr[e][t]; channel, n_thr and thr are HOST arrays inside the descriptor.
 *
 * Per point of channel[e] and threshold thr = thr[e][t]:
 *   k = #{m : x_m > thr}     0 .. M      strict, as skens_stats' exceed.  A NaN compares false.
 *   o = [y > thr]            0 or 1
 *
 * Joint counts.  counts[e][t][j][o][k], int32 [n_events][SKEVENT_MAX_THRESHOLDS][H][2][M + 1], is the number of points of latitude row j
 * with that (o, k).  Every bin of every (e, t < n_thr[e], j) is written, zeros included; entries with t >= n_thr[e] are not touched.
 *
 * Neighbourhood sums (n_scales > 0).  Scale s has a half-height hy[s] >= 0 in rows (a host array) and a half-width hx[s][j] in columns
 * (a DEVICE int32 table [n_scales][H], read by centre row).  The window of point (j, i) is
 *   rows     [j - hy, j + hy] intersected with [0, H),
 *   columns  i - hx_j .. i + hx_j, periodic in longitude, hx_j clamped in the kernel to [0, (W - 1) / 2]: a window never laps itself.
 * It holds n_j = (rows) * (2 hx_j + 1) points, the same for every point of a row.  With Sf the window sum of k and So the window sum of
 * o, three int64 row sums are written to sums[e][t][s][j][3], int64 [n_events][SKEVENT_MAX_THRESHOLDS][n_scales][H][3]:
 *   ( sum_i (Sf - M So)^2,  sum_i Sf^2,  sum_i (M So)^2 )
 * (t >= n_thr[e]: not touched).  The host divides by (M n_j)^2 and weights the rows: FSS = 1 - <(Pf - Po)^2> / (<Pf^2> + <Po^2>) with
 * Pf = Sf / (M n_j), Po = So / n_j.  The call is refused unless W (M (2 hy_max + 1) W)^2 < 2^63: no sum can overflow.
 *
 * There is no floating-point arithmetic on the device beyond the comparisons, and no floating-point atomic: every output is an exact
 * integer, bitwise reproducible and the same on the vector and the scalar load path.
 *
 * Shape of the computation.  Count pass, ONE launch for all event channels: a workgroup of four waves owns one (e, latitude row) at a
 * time; every member value and truth value of the row is read from HBM once (16-byte loads when `member_align` = 16, the truth is
 * 16-byte aligned and W is a multiple of 4; 4-byte loads otherwise), k and o are formed in registers for the row's thresholds, and the
 * row's (o, k) histogram is added up in LDS with integer adds.  The four corner bins (k = 0 or k = M) are counted per wave with a
 * ballot and a population count into wave-uniform counters, never with LDS adds: for a rare event nearly every point falls into one of
 * them, and 64 lanes adding to one LDS word would serialise.  With scales, k and o are also stored as two uint8 planes per (e, t) in the
 * workspace: planes[e][t][0 = k, 1 = o][H][W], uint8 [n_events][SKEVENT_MAX_THRESHOLDS][2][H][W].  Neighbourhood pass: one workgroup per
 * (e, t, s, row) sums the planes over the row window into int32 column sums in LDS (2 W 4 bytes), a workgroup prefix scan turns them
 * into prefix sums, every lane takes Sf and So of its columns as differences of two prefix entries (the wrap adds the row total), forms
 * the three squares in int64, and an integer reduction gives the row's three sums.
 *
 * Limits: C * H * W <= 2^30 (32-bit byte offsets, as skscore_run); with scales W <= SKEVENT_MAX_WIDTH.  Member and truth pointers need
 * 4-byte alignment, counts 4, hx 4, sums 8, the workspace 16 and skevent_workspace_bytes(n_events, H, W, n_scales) bytes. */
#ifndef SKYRIM_EVENT_H
#define SKYRIM_EVENT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SKEVENT_ABI_VERSION 1
#define SKEVENT_E_ARG (-1) /* bad argument: NULL or misaligned pointer, a count or index outside its range, a workspace too small */
#define SKEVENT_E_HIP (-2) /* the launch failed */
#define SKEVENT_MAX_MEMBERS 64
#define SKEVENT_MAX_CHANNELS 16
#define SKEVENT_MAX_THRESHOLDS 4
#define SKEVENT_MAX_SCALES 4
#define SKEVENT_MAX_WIDTH 8192

int skevent_abi_version(void);

/* bytes of workspace a call needs (the uint8 planes; 0 without scales); 0 for arguments skevent_run would refuse */
size_t skevent_workspace_bytes(int n_events, int H, int W, int n_scales);

typedef struct {
    const float* const* members; /* device array of M device pointers */
    int M;
    int member_align;            /* bytes every member pointer is aligned to (4 or 16) */
    const float* truth;          /* (C, H, W) */
    int C, H, W;
    int n_events;                /* 0 launches nothing */
    int channel[SKEVENT_MAX_CHANNELS];
    int n_thr[SKEVENT_MAX_CHANNELS];
    float thr[SKEVENT_MAX_CHANNELS][SKEVENT_MAX_THRESHOLDS]; /* not NaN */
    int32_t* counts;             /* [n_events][SKEVENT_MAX_THRESHOLDS][H][2][M + 1] */
    int n_scales;                /* 0: the count pass alone; what follows is then ignored */
    int hy[SKEVENT_MAX_SCALES];
    const int32_t* hx;           /* [n_scales][H] */
    int64_t* sums;               /* [n_events][SKEVENT_MAX_THRESHOLDS][n_scales][H][3] */
    void* workspace;
    size_t workspace_bytes;
} skevent_desc;

int skevent_run(const skevent_desc* desc, void* stream);

#ifdef __cplusplus
}
#endif
#endif
