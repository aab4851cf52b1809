/* C ABI of the ensemble helpers: perturbed members of one initial condition, and the statistics of M member states in one pass.
 *
 * Conventions of skyrim_io.h: all data pointers are device pointers; every call is asynchronous on `stream` (a hipStream_t); nothing is
 * allocated inside; the return code is 0, SKENS_E_ARG or SKENS_E_HIP; argument errors are found before anything touches the GPU, so they
 * are reported on a machine without one.
 *
 * ---- skens_perturb -------------------------------------------------------------------------------------------------------------------
 *   out[j][i] = x0[i] + scale * std[c(i)] * z(seed, member_first + j, i)        j < n_members, i < n
 * x0 is a flat (L, C, H, W) float32 tensor of n = L * C * chan_stride elements (L history levels, chan_stride = H * W);
 * c(i) = (i / chan_stride) % C indexes std[C].  Member 0 is the control: a bit copy of x0.  `out` holds the n_members states of the call
 * one after the other (n elements each).
 *
 * z is standard normal from a counter-based generator: a member's bits depend on (seed, member, i) and on nothing else -- not on
 * n_members, not on how members are batched into calls.  With g = i / 4 (integer division):
 *   (r0, r1, r2, r3) = Philox4x32-10(counter = (g, 0, 0, 0), key = (seed, member))
 *        [multipliers 0xD2511F53 / 0xCD9E8D57, key increments 0x9E3779B9 / 0xBB67AE85 (Random123)]
 *   U(r) = ((r >> 8) + 0.5) * 2^-24                  in (0, 1), never 0 or 1
 *   element 4g + 0:  sqrt(-2 ln U(r0)) * cos(2 pi U(r1))
 *   element 4g + 1:  sqrt(-2 ln U(r0)) * sin(2 pi U(r1))
 *   element 4g + 2:  sqrt(-2 ln U(r2)) * cos(2 pi U(r3))
 *   element 4g + 3:  sqrt(-2 ln U(r2)) * sin(2 pi U(r3))
 * in fp32 with the accurate (not the __fast) variants of logf / log1pf, sqrtf, sinf and cosf.  U has 25 significant bits in its upper half,
 * so it is never rounded to fp32: for r >> 8 >= 2^23 ln U is log1pf(-(1 - U)) and the angle is fl(fl(2 pi) * (U - 1)); 1 - U and U - 1
 * are exact there, as U is below (csrc/ens_ops.hip).  n is at most 2^32 - 16, so the counter is (g, 0, 0, 0).
 *
 * ---- skens_stats ---------------------------------------------------------------------------------------------------------------------
 * One pass over M member states: for every element j of the flat range [offset, offset + n) the M values x_m = members[m][offset + j]
 * (offset + n <= 2^30: the kernel addresses with 32-bit byte offsets) are read once, held in registers, and every requested output is written at RANGE-RELATIVE index j (mean[j], exceed[k * n + j],
 * quant[q * n + j]).  An output pointer that is NULL is not computed.
 *
 *   d_m    = x_m - x_0,   a = (sum_m d_m) / M                     fp32, summed in member order
 *   mean   = x_0 + a
 *   spread = sqrt(sum_m (d_m - a)^2 / M)                          population standard deviation (ddof = 0), summed in member order
 *   min, max                                                      comparisons only
 *   exceed[k] = (number of members with x_m > thr[k]) / M         k < n_thr <= SKENS_MAX_THRESHOLDS
 *   quant[q]  = s[q_index[q]] + q_frac[q] * (s[q_index[q] + 1] - s[q_index[q]])      q < n_quant <= SKENS_MAX_QUANTILES
 *               s = the M values in ascending order; numpy's "linear" method: h = (M - 1) * level, q_index = floor(h), q_frac = h - floor(h),
 *               both formed by the caller in double (q_index == M - 1 takes s[M - 1]); 0 <= q_index < M and 0 <= q_frac < 1 are checked.
 *
 * Centring on member 0 is what keeps the mean of members that differ by 1e-3 sigma exact to the spread.  The inputs are
 * physical fields: nothing is rescaled against overflow of (d - a)^2.  Where all members are equal spread is exactly 0; where any member
 * is non-finite mean is non-finite (min, max and quant follow fminf / fmaxf there).
 *
 * `members` is a DEVICE array of M pointers, 1 <= M <= SKENS_MAX_MEMBERS; `thr` is a HOST array (passed by value to the kernel), as are
 * q_index and q_frac.  Member and output pointers need 4-byte alignment; 16-byte aligned ones take the vector path (`member_align`: the
 * caller's statement of the alignment, in bytes, that ALL M member pointers share -- the library cannot read the device array). */
#ifndef SKYRIM_ENS_H
#define SKYRIM_ENS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SKENS_ABI_VERSION 1
#define SKENS_E_ARG (-1) /* bad argument: NULL or misaligned pointer, a count outside its range */
#define SKENS_E_HIP (-2) /* the launch failed */
#define SKENS_MAX_MEMBERS 64
#define SKENS_MAX_THRESHOLDS 4
#define SKENS_MAX_QUANTILES 4

int skens_abi_version(void);

int skens_perturb(const float* x0, const float* std, float* out, size_t n, size_t chan_stride, int C, float scale, uint32_t seed,
                  uint32_t member_first, int n_members, void* stream);

typedef struct {
    const float* const* members; /* device array of M device pointers */
    int M;
    int member_align;            /* bytes every member pointer is aligned to (4 or 16) */
    size_t offset, n;            /* the flat element range */
    float* mean;                 /* [n] or NULL */
    float* spread;               /* [n] or NULL */
    float* min;                  /* [n] or NULL */
    float* max;                  /* [n] or NULL */
    float* exceed;               /* [n_thr][n] or NULL (then n_thr must be 0) */
    int n_thr;
    float thr[SKENS_MAX_THRESHOLDS];
    float* quant;                /* [n_quant][n] or NULL (then n_quant must be 0) */
    int n_quant;
    int q_index[SKENS_MAX_QUANTILES];
    float q_frac[SKENS_MAX_QUANTILES];
} skens_stats_desc;

int skens_stats(const skens_stats_desc* desc, void* stream);

#ifdef __cplusplus
}
#endif
#endif
