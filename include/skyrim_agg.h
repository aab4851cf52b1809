/* C ABI of time-window aggregates on the device: the maximum, minimum, sum (mean), the count above a threshold (hours above) and the
 * time of the extreme of a channel over a window of lead times, folded per member, one call per lead time, into an accumulator that
 * stays in HBM across the lead times.  The accumulator has the layout of skderive_run's `out`, so the ensemble statistics
 * (skyrim_ens.h), the scorer (skyrim_score.h) and the event counter (skyrim_event.h) read a closed window like any other planes.
 *
 * Conventions of skyrim_derive.h: all data pointers are device pointers; every call is asynchronous on `stream` (a hipStream_t);
 * nothing is allocated inside; the return code is 0, SKAGG_E_ARG or SKAGG_E_HIP; argument errors are found before anything touches
 * the GPU, so they are reported on a machine without one.
 *
 * ---- skagg_update -------------------------------------------------------------------------------------------------------------------
 * One call per lead time.  States are contiguous float32 (C, H, W): a DEVICE array of M member pointers (1 <= M <= SKAGG_MAX_MEMBERS).
 * Accumulator: float32 acc[m * member_stride + (d * H + j) * W + i], 0 <= d < D.  The program is n_ops <= SKAGG_MAX_OPS ops, a HOST
 * array inside the descriptor.  Each op reads the input channel `in` (in [0, C)) and updates the slot `out` (in [0, D)); a MAX or MIN
 * op may also update the slot `when` (in [0, D), or -1: none).  `phase` is a set of bits: SKAGG_FIRST -- this lead time opens the op's
 * window, SKAGG_LAST -- it closes it; a window of one lead time sets both.  `stamp` is what `when` records: the host sets it to the
 * lead time in hours.  No slot is named twice within a call, `out` and `when` taken together.
 *
 * With x the input at a point, a the old value of `out` and w the old value of `when` there, all fp32, every operation rounded on its
 * own (the library is built with contraction to fma OFF, -ffp-contract=off):
 *
 * SKAGG_MAX          with FIRST:  a' = x,  w' = (x != x) ? x : stamp
 *                    otherwise:   take = (x > a) || (x != x);  if take: a' = x, w' = (x != x) ? x : stamp;  if not: a' = a, w' = w.
 *                    The first lead time that attains the maximum wins a tie (-0.0 does not replace +0.0, nor +0.0 -0.0: neither is
 *                    greater).  A NaN is sticky in both slots: once a is NaN no comparison is true, and a NaN input is always taken.
 *                    w' is written only if when >= 0.
 * SKAGG_MIN          the same with x < a.
 * SKAGG_SUM          with FIRST:  a' = x;  otherwise: a' = a + x -- the sum runs in the order of the calls.
 *                    with LAST, after that:  a' = a' * scale.  The host passes float32(1 / n) for a mean and 1.0f for a total.
 * SKAGG_COUNT_ABOVE  b = (x != x) ? x : ((x > thr) ? 1.0f : 0.0f);  with FIRST: a' = b;  otherwise: a' = a + b;
 *                    with LAST, after that:  a' = a' * scale.  The host passes the step length in hours: the result is "hours above".
 *                    `>` is strict; thr = +inf counts nothing, thr = -inf counts every value but -inf.
 * `when`, `thr` and `scale` are ignored by the kinds that do not use them, except that when >= 0 on SUM or COUNT_ABOVE is an error.
 *
 * Without FIRST the slots of an op are read and must have been written by earlier calls.  With FIRST they are never read: no memset is
 * needed, the accumulator may hold anything.  Slots no op names, and everything beyond D H W of a member's part, are not touched.
 * Nothing is masked: a non-finite input changes the slots of the ops that read it, in that member, at that point, and nothing else.
 *
 * Shape of the computation.  One launch covers all members and all ops.  The host sorts the ops into groups that read the same input
 * channel; a wave takes one tile of 512 points of one group of one member: member and group are wave-uniform (scalar registers), a lane's
 * address is the member's pointer (or the member's part of `acc`) plus one 32-bit byte offset.  A tile loads its points of the input
 * channel ONCE and then runs the group's ops on them one after the other, so max, mean and hours-above of one channel cost one read of
 * that plane per member and call, plus the read (without FIRST) and the write of each slot.  When every member pointer and `acc` are
 * 16-byte aligned, member_stride and H W are multiples of 4, a lane loads and stores 16 bytes (four points); otherwise the scalar path
 * runs.  Both paths do the same arithmetic per point: their results are bit-equal.  No scratch memory, no LDS, no atomics.
 *
 * Bytes per call and member, P = 4 H W: P per distinct input channel, plus per op P (write of `out`) + P without FIRST (its read), and
 * the same again for `when`.
 *
 * Accuracy.  MAX, MIN and `when` are exact selections.  COUNT_ABOVE is exact while the count is below 2^24, up to the one rounding of
 * the product with `scale`.  SUM of n terms in call order, then one product: |a' - exact| <= (n + 1) u sum_k |x_k| |scale| to first
 * order, u = 2^-24 (n - 1 additions and one product, each term passes through at most n roundings, and one more for scale itself when
 * it is float32(1 / n)).
 *
 * Limits: C H W <= 2^30 and D H W <= 2^30 (32-bit byte offsets), member_stride >= D H W, C, H, W, D >= 1, `members` 8-byte aligned, `acc`
 * 4-byte aligned.  `member_align` is the caller's statement of the alignment, in bytes, that ALL M member pointers share (4 or 16) -- the
 * library cannot read the device array. */
#ifndef SKYRIM_AGG_H
#define SKYRIM_AGG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SKAGG_ABI_VERSION 1
#define SKAGG_E_ARG (-1) /* bad argument: NULL or misaligned pointer, a count, channel, slot, kind or phase outside its range, a slot named twice */
#define SKAGG_E_HIP (-2) /* a launch failed */
#define SKAGG_MAX_MEMBERS 64
#define SKAGG_MAX_OPS 16

#define SKAGG_MAX 1
#define SKAGG_MIN 2
#define SKAGG_SUM 3
#define SKAGG_COUNT_ABOVE 4

#define SKAGG_FIRST 1
#define SKAGG_LAST 2

typedef struct {
    int32_t kind;  /* SKAGG_MAX ... */
    int32_t in;    /* input channel */
    int32_t out;   /* slot of the value */
    int32_t when;  /* MAX, MIN: slot of the stamp of the extreme, or -1 */
    int32_t phase; /* SKAGG_FIRST | SKAGG_LAST */
    float thr;     /* COUNT_ABOVE */
    float scale;   /* SUM, COUNT_ABOVE: the factor applied with LAST */
} skagg_op;

typedef struct {
    const float* const* members; /* device array of M device pointers */
    int M;
    int member_align;            /* bytes every member pointer is aligned to (4 or 16) */
    int C, H, W;
    int D;                       /* slots per member */
    float* acc;                  /* [M][member_stride], the first D H W elements of each member's part are the slots */
    size_t member_stride;        /* in elements */
    float stamp;                 /* what `when` records: the lead time in hours */
    int n_ops;
    skagg_op ops[SKAGG_MAX_OPS];
} skagg_desc;

int skagg_abi_version(void);

int skagg_update(const skagg_desc* desc, void* stream);

#ifdef __cplusplus
}
#endif
#endif
