/* C ABI of climate-relative extremes on the device: the M members of one valid time are compared with a QUANTILE CLIMATE -- Q planes per
 * field, the climate's value at Q probability levels at every grid point -- and give the Extreme Forecast Index (EFI), the Shift of Tails
 * (SOT) and the fraction of members beyond a climate percentile (skclim_extremes); and the climate itself is made from N sample states
 * (skclim_quantiles).
 *
 * Conventions of skyrim_point.h and skyrim_ens.h: all data pointers are device pointers; every call is asynchronous on `stream` (a
 * hipStream_t); nothing is allocated inside; the return code is 0, SKCLIM_E_ARG or SKCLIM_E_HIP; argument errors are found before anything
 * touches the GPU, so they are reported on a machine without one.  All arithmetic is fp32, every operation rounded on its own: the library
 * is built with contraction to fma OFF (-ffp-contract=off); the ONE fused operation is named where it stands.  NAN below is the one quiet
 * NaN 0x7FC00000.  No atomics, no scratch (no register array is indexed at run time), 32-bit byte offsets.
 *
 * ---- skclim_extremes ------------------------------------------------------------------------------------------------------------------
 * `members`: a DEVICE array of M pointers to contiguous float32 states (C, H, W), 1 <= M <= SKCLIM_MAX_MEMBERS; `member_align`: the
 * caller's statement of the alignment, in bytes, that ALL M member pointers share (4 or 16), as in skens_stats.  `channels`: a HOST list of
 * nf channel indices (1 <= nf <= SKCLIM_MAX_FIELDS, each in [0, C), any order, repeats allowed).  `clim`: float32 clim[f][i][H W] on the
 * device for listed field f and level i < Q, 2 <= Q <= SKCLIM_MAX_LEVELS.  HOST tables in the descriptor: p[Q] strictly increasing in
 * [0, 1]; A[Q - 1], B[Q - 1], rdp[Q - 1]; floor[nf] (-inf: none).  The host forms the tables in double and rounds them once to fp32:
 *      G(p) = -2 acos(sqrt p)           K(p) = -sqrt(p (1 - p)) - acos(sqrt p)
 *      A_i = G(p_{i+1}) - G(p_i)        B_i = K(p_{i+1}) - K(p_i)        rdp_i = 1 / (p_{i+1} - p_i)
 * the integrals of 1 / sqrt(p (1 - p)) and of p / sqrt(p (1 - p)) over the interval, finite at p = 0 and p = 1 (sum A = pi, sum B = pi / 2
 * over [0, 1]).  Checked: p strictly increasing in [0, 1] as fp32, A, B and rdp finite and > 0, floor not NaN.
 *
 * Outputs, each a device pointer or NULL (a NULL output is not computed; at least one is given), plane-major per listed field:
 *      efi[f][H W]        sot[s][f][H W], s < n_sot        prob[t][f][H W], t < n_prob
 * Nothing else in any buffer is written.  sot != NULL exactly when n_sot > 0, prob != NULL exactly when n_prob > 0.
 *
 * Per point and listed field, x_m the M member values and c_i the Q climate values, each read as fl(v + 0.0f), so -0 is +0:
 *   non-finite input: if any x_m or any c_i is not finite, EVERY output of this (field, point) is NAN.  Nothing else is masked.
 *   EFI = (2 / pi) int_0^1 (p - F(p)) / sqrt(p (1 - p)) dp with F piecewise linear through the fraction of members at or below each
 *   climate level, integrated analytically per interval and normalised over the intervals in use:
 *      n_i = the number of members with x_m <= c_i (an integer),  F_i = fl(float(n_i) / float(M))
 *      for i = 0 .. Q - 2 in ascending order
 *          b = fl(fl(F_{i+1} - F_i) rdp_i)      a = fl(F_i - fl(b p_i))      t = fl(fl(B_i - fl(a A_i)) - fl(b B_i))
 *          interval i is ACTIVE where c_{i+1} > floor[f];  over the active ones, from num = den = +0:  num = fl(num + t), den = fl(den + B_i)
 *      efi = min(max(fl(num / den), -1), 1);  with no active interval efi = +0.
 *   The counts are "<=" because F is a distribution function: a member ON a climate level has reached it (P(X <= c)), and a climate with
 *   a spike (many levels equal to the same value) then counts the members on the spike at its FIRST level.  floor[f] leaves out the part
 *   of the climate at a bound (CAPE or precipitation identically 0).  All members above c_{Q-1}: every n_i = 0, t = B_i bit for bit,
 *   num == den, efi = exactly 1.  All members at or below c_0: t = fl(B_i - A_i), efi = -1 to rounding, clamped from below.
 *   SOT request s = (q_index, q_frac, k_ref, k_base), n_sot <= SKCLIM_MAX_SOT, 0 <= q_index < M, 0 <= q_frac < 1, k_ref and k_base in
 *   [0, Q): with s[] the members in ascending order (comparisons only: the bitonic network over the bucket's slots, +inf in empty ones)
 *      Qf  = s[q_index] + q_frac (s[q_index + 1] - s[q_index])      skens_stats' quantile bit for bit: the difference carried exactly
 *            (two-sum: d + e) and Qf = fma(q_frac, e, fma(q_frac, d, s[q_index])) -- the fused operations; q_index == M - 1 takes s[M - 1]
 *      sot = fl(fl(Qf - c[k_ref]) / fl(c[k_ref] - c[k_base]));  NAN where c[k_ref] == c[k_base].
 *   The host picks the indices (tail q >= 0.5: base q, ref 1 - (1 - q) / 10; tail q < 0.5: base q, ref q / 10).  No sort without a request.
 *   Tail odds, request t = (k, below), n_prob <= SKCLIM_MAX_PROB: fl(float(n) / float(M)), n the number of members with x_m > c_k
 *   (below == 0) or x_m < c_k (below != 0).
 *
 * Shape of the computation.  A lane owns one point, or four consecutive points on the 16-byte path (member_align == 16, H W a multiple
 * of 4, clim and every output 16-byte aligned, M <= 16), of one listed field; member and field are wave-uniform.  The M values sit in
 * registers, bucketed by MB in {8, 16, 32, 64} with +inf in the empty slots; the climate is streamed one plane at a time, the next plane's
 * load issued before the current one is counted, and a count is a fully unrolled compare-and-add over the MB slots.  By hand count at
 * Q = 101, M = 50 (MB = 64), 721 x 1440: (M + Q) 4 = 604 bytes per point, 627 MB, 0.1 ms at 6 TB/s; Q MB = 6464 compare-and-add pairs
 * per point, 1.3e10 lane operations, 0.35 ms at 256 CUs x 64 lanes x 2.4 GHz.  The two are of one order; the compares are the larger.
 *
 * Bounds, against the same formulas in exact arithmetic on the same fp32 inputs and the DOUBLE tables, u = 2^-24:
 *      |efi - exact| <= u ((Q + 12) R + Q),     R = sum_active T_i / sum_active B_i,     T_i = B_i + (1 + rdp_i p_i) A_i + rdp_i B_i
 *   The count: F_i carries one rounding (|F| <= 1); F_{i+1} - F_i two inherited and one own, 3 u absolute; b = that times rdp_i, whose
 *   table rounding and the product's add 2: 5 u rdp_i; b p_i 7 u rdp_i p_i; a at most 8 u (1 + rdp_i p_i); a A_i 10 u (1 + rdp_i p_i) A_i;
 *   B_i - a A_i  2 u B_i + 11 u (1 + rdp_i p_i) A_i; b B_i  7 u rdp_i B_i; t at most 12 u T_i.  The sum over at most Q - 1 intervals adds
 *   (Q - 2) u sum |t_i| <= (Q - 2) u sum T_i; den carries (Q - 1) u relative, the division one more, and |num / den| <= 1 + small.  One
 *   unit in (Q + 12) pays for the products of roundings.  This is a worst case over the data (|F| <= 1 and |F_{i+1} - F_i| <= 1 are all
 *   it uses), so measured errors lie far below it.
 *      |sot - exact| <= u (2 X / |c_ref - c_base| + 4 |sot|) + 2^-126,     X = max(|s[q_index]|, |s[q_index + 1]|)      (fp32 q_frac as given)
 *   Qf carries the two roundings of its two fused operations, each at most u X; the numerator one more, the denominator one, the division one.
 *
 * ---- skclim_quantiles -----------------------------------------------------------------------------------------------------------------
 * `samples`: a DEVICE array of N pointers to contiguous float32 states (C, H, W), 1 <= N <= SKCLIM_MAX_SAMPLES (the member-table form; C
 * is small, the caller keeps only the fields it wants).  `channels`: nf listed channels as above.  Levels: HOST q_index[Q], q_frac[Q],
 * 1 <= Q <= SKCLIM_MAX_LEVELS, numpy's "linear" method h = (N - 1) level, q_index = floor(h), q_frac = h - floor(h), formed in double by
 * the caller; 0 <= q_index < N and 0 <= q_frac < 1 AS FP32 are checked (a fraction that rounds to 1.0f is the next index with fraction
 * 0).  Output: clim[f][i][H W], the layout skclim_extremes reads.
 *
 * Per point and listed field: the N values are read as fl(v + 0.0f).  If any is not finite all Q outputs of the point are NAN.  Otherwise
 * they are sorted ascending, comparisons only (any correct sort gives the same bits), and with j = q_index[i], f = q_frac[i]
 *      out_i = min(fl(s[j] + fl(f fl(s[j + 1] - s[j]))), s[j + 1])          j == N - 1 takes s[N - 1]
 * The min makes the planes non-decreasing in the level whatever the rounding does (level i' > i reads j' >= j, and out_i <= s[j + 1]).
 *
 * Shape of the computation.  A workgroup of 1024 lanes takes a tile of T consecutive points of one listed field, T = min(256,
 * 32768 / NP) with NP = N rounded up to a power of two: 128 KiB of the CU's 160 KiB of LDS hold the T columns, sample-major ([n][T]), +inf
 * beyond N.  The columns are sorted there by one bitonic network over NP whose T NP / 2 compare-exchanges of a stage are spread over the
 * 1024 lanes (the LDS allows one workgroup per CU, so it holds all the waves), a barrier between stages.  The Q planes are then written
 * by all 16 waves, a wave taking (level, run of up to 64 points) units in turn, so the level's table entries are scalar loads and a
 * store is coalesced over the points.  A sample plane is read in runs of T points: 4 T bytes, 64 bytes at N = 2048 (T = 16), 128 at
 * N = 1000, a whole 1 KiB only for N <= 128.  A 64-byte run uses half of every 128-byte line it touches, so the read of the samples
 * costs up to twice its bytes there; this is a build-once job and the sort, not the read, is its time (N = 1000: 55 stages over 32 Ki
 * slots per 32 points).
 *
 * Bound, against exact arithmetic on the same sorted fp32 values and the DOUBLE fraction: |out - exact| <= u (3 |s[j + 1] - s[j]| +
 * max(|s[j]|, |s[j + 1]|)) + 2^-148: the difference, the product and q_frac's own rounding, each relative to the difference, and the sum.
 * The min moves the result towards the exact value only.
 *
 * Limits of both: C H W <= 2^30 and nf Q H W <= 2^30 (32-bit byte offsets; the caller splits the fields of a request over calls where
 * the second needs it), member, sample, clim and output pointers 4-byte aligned, the pointer arrays 8-byte aligned. */
#ifndef SKYRIM_CLIM_H
#define SKYRIM_CLIM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SKCLIM_ABI_VERSION 1
#define SKCLIM_E_ARG (-1) /* bad argument: NULL or misaligned pointer, a count, size, index, level or table entry outside its range */
#define SKCLIM_E_HIP (-2) /* a launch failed */
#define SKCLIM_MAX_MEMBERS 64
#define SKCLIM_MAX_FIELDS 16
#define SKCLIM_MAX_LEVELS 128
#define SKCLIM_MAX_SOT 4
#define SKCLIM_MAX_PROB 8
#define SKCLIM_MAX_SAMPLES 2048

typedef struct {
    int32_t q_index;  /* of the sorted members */
    float q_frac;
    int32_t k_ref, k_base; /* climate levels */
} skclim_sot;

typedef struct {
    int32_t k;     /* climate level */
    int32_t below; /* 0: members above c_k, otherwise members below */
} skclim_prob;

typedef struct {
    const float* const* members; /* device array of M device pointers */
    int M;
    int member_align;            /* bytes every member pointer is aligned to (4 or 16) */
    int C, H, W;                 /* the member states */
    int nf;                      /* listed fields */
    int32_t channels[SKCLIM_MAX_FIELDS];
    const float* clim;           /* device, [nf][Q][H W] */
    int Q;
    float p[SKCLIM_MAX_LEVELS];
    float A[SKCLIM_MAX_LEVELS], B[SKCLIM_MAX_LEVELS], rdp[SKCLIM_MAX_LEVELS]; /* Q - 1 entries each */
    float floor[SKCLIM_MAX_FIELDS];
    int n_sot;
    skclim_sot sot_req[SKCLIM_MAX_SOT];
    int n_prob;
    skclim_prob prob_req[SKCLIM_MAX_PROB];
    float* efi;                  /* [nf][H W] or NULL */
    float* sot;                  /* [n_sot][nf][H W] or NULL (then n_sot must be 0) */
    float* prob;                 /* [n_prob][nf][H W] or NULL (then n_prob must be 0) */
} skclim_extremes_desc;

typedef struct {
    const float* const* samples; /* device array of N device pointers */
    int N;
    int C, H, W;                 /* the sample states */
    int nf;
    int32_t channels[SKCLIM_MAX_FIELDS];
    int Q;
    int32_t q_index[SKCLIM_MAX_LEVELS];
    float q_frac[SKCLIM_MAX_LEVELS];
    float* clim;                 /* device, [nf][Q][H W] */
} skclim_quantiles_desc;

int skclim_abi_version(void);

int skclim_extremes(const skclim_extremes_desc* desc, void* stream);

int skclim_quantiles(const skclim_quantiles_desc* desc, void* stream);

/* the argument checks of the two calls alone: 0 or SKCLIM_E_ARG for exactly the descriptors the calls take or refuse.  They touch no GPU
 * and read no device memory, so a caller (and a test on a machine without a GPU) can try a descriptor before its buffers exist */
int skclim_extremes_check(const skclim_extremes_desc* desc);
int skclim_quantiles_check(const skclim_quantiles_desc* desc);

/* T, the points of a workgroup's tile in skclim_quantiles for N samples (0 for N outside its range) */
int skclim_tile_points(int N);

#ifdef __cplusplus
}
#endif
#endif
