/* C ABI of zonal power spectra on the device: the power per zonal wavenumber of the M member states of one valid time, of their mean,
 * of their spread and, with a truth, of the truth and of the errors, along latitude circles and averaged over latitude bands -- made
 * where the states lie in HBM.  Only nc x nb x n_slots x K doubles go back to the caller (skyrim_amd/spectra.py).
 *
 * Conventions of skyrim_gram.h and skyrim_score.h: all data pointers are device pointers; every call is asynchronous on `stream` (a
 * hipStream_t); nothing is allocated inside; the return code is 0, SKSPEC_E_ARG or SKSPEC_E_HIP; argument errors are found before
 * anything touches the GPU, so they are reported on a machine without one.
 *
 * ---- skspec_run -----------------------------------------------------------------------------------------------------------------------
 * States are contiguous float32 (C, H, W): M members (a DEVICE array of M pointers, 1 <= M <= SKSPEC_MAX_MEMBERS) and, optionally, a
 * truth state y.  `channels` is a HOST list inside the descriptor of nc channel indices (1 <= nc <= SKSPEC_MAX_CHANNELS, each in
 * [0, C), any order, repeats allowed).  The nb bands (1 <= nb <= SKSPEC_MAX_BANDS) are the row ranges [j0[b], j1[b]) with
 * 0 <= j0 < j1 <= H; they may overlap.  lat_weight holds H float64 weights w_j (any scale; a band whose weights sum to 0 gives
 * non-finite values).  `twiddles` holds the 2 W floats of skspec_twiddles(W, .), uploaded by the caller.
 * W = 2^a 3^b 5^c with SKSPEC_MIN_W <= W <= SKSPEC_MAX_W; any other W is SKSPEC_E_ARG.
 *
 * Definition.  For a row of W values d:  F_k = (1/W) sum_n d_n e^(-2 pi i k n / W),  k = 0 .. K - 1,  K = floor(W/2) + 1.  The row's power
 * is P_k = c_k |F_k|^2 with c_0 = 1, c_k = 2 for 0 < k < W/2 and c_{W/2} = 1 (W even), so that sum_k P_k is the row's mean square
 * exactly (Parseval).  (WeatherBench 2 doubles the Nyquist bin as well; this library does not, to keep that identity.)  The band value
 * is sum_j w_j P_jk / sum_j w_j over the band's rows.  Output: float64 out[nc][nb][n_slots][K], written in full, nothing else touched;
 * n_slots = 3 without a truth and 6 with one.  |.|^2 below is what c_k and the band mean are applied to:
 *      slot 0  member        (1/M) sum_m |F(x_m)|^2
 *      slot 1  mean          |F(xbar)|^2
 *      slot 2  spread        (1/(M-1)) sum_m |F(x_m - xbar)|^2,  exactly 0 for M = 1
 *      slot 3  truth         |F(y)|^2
 *      slot 4  error_mean    |F(xbar - y)|^2
 *      slot 5  error_member  (1/M) sum_m |F(x_m - y)|^2
 *
 * Numerics.  Member 0 is the origin, as in skyrim_score.h and skyrim_gram.h.  Only differences are transformed, each formed in fp32 at
 * the point:  f_0 = x_0 - x_0[j][0] (the row's first value),  d_m = x_m - x_0 (m = 1 .. M - 1; d_0 is exactly 0 and is not
 * transformed),  d_y = y - x_0.  F_0 = F(f_0), and its k = 0 coefficient gets x_0[j][0] back in float64.  All slots are |G|^2 of fixed
 * linear combinations of F_0, D_m = F(d_m), S = sum_m D_m and D_y, formed in float64 from the fp32 transforms:
 *      member: F_0 + D_m;  mean: F_0 + S/M;  truth: F_0 + D_y;  error_mean: S/M - D_y;  error_member: D_m - D_y;
 *      spread: (sum_m |D_m|^2 - |S|^2 / M) / (M - 1) -- equal members give exactly 0, and the cancellation is relative to the spread.
 * The transform is an fp32 Stockham mixed-radix FFT in LDS (skyrim_amd/csrc/spec_fft.h): radix-4 passes, then a radix-2 pass if a factor 2 is
 * left, then the radix-3 and the radix-5 passes; the twiddles come from the caller's table (exact values rounded once to fp32).  Real
 * sequences are transformed as COMPLEX ones, two at a time: f_0 alone (imaginary part 0), d_y alone, then the pairs (d_1, d_2),
 * (d_3, d_4), ... (an odd last one alone).  f_0 and d_y are not paired with anything because a pair shares one rounding error, which is
 * relative to the LARGER of the two; members are exchangeable, so their differences are of one size.  The two spectra are separated,
 * scaled by 1/W and everything after that -- the combinations, |G|^2, the product with w_j, the sums over members and rows -- is
 * float64.
 *
 * Shape of the computation.  The rows that lie in at least one band are cut at every band edge into segments, and each segment into
 * chunks of at most min(SKSPEC_CHUNK, nc) rows (fewer channels, shorter chunks: a launch of one channel still fills the device);
 * chunks are numbered in ascending row order.  One workgroup per (chunk, channel) takes its rows one after the other.  Per row: x_0's
 * row is read once (coalesced) and kept in LDS; every other member row and the truth row is read once, coalesced, subtracted and
 * written to the transform's LDS planes; so every member value is read from HBM once.  A pass runs W / R butterflies over the
 * workgroup's lanes between two barriers, from one pair of planes to the other.  Lane t owns the bins k = t, t + L, ... (L lanes): F_0,
 * D_y, S and the real accumulators of its bins are float64 REGISTERS (the kernel is instantiated on the number of bins per lane: 1 or
 * 3 with L = 256, and for W > 1534 5 with L = 512), so the LDS holds the row of x_0 and the two pairs of planes only:
 * 20 (W + W/32) bytes, 29 KiB at W = 1440 (five workgroups per CU), 83 KiB at W = 4096 (one).  At the end of a row the lane adds w_j
 * times its six values to its own entries of the chunk's partial [cc][chunk][slot][K] in the caller's workspace (the first row stores).  A second kernel sums
 * the partials of a band's chunks in ascending order, multiplies by c_k and divides by the band's weight sum (64 interleaved partial
 * sums in ascending rows, then those in ascending order).  No floating-point atomics, no scratch, no indexed register arrays.  The
 * assignment of rows to accumulators and the order of every sum depend on the descriptor alone -- not on the device's CU count, not on
 * timing: two calls give the same bits.  The library is built with contraction to fma off.
 *
 * Bound, against exact arithmetic on the same fp32 differences, with u = 2^-24.  A complex transform of the pair (a, b) errs by
 *      |Fhat_k - F_k| <= c_W u sqrt(rms(a)^2 + rms(b)^2)     for both members of the pair and every k,
 * rms(.) being the root mean square of the transformed sequence, and
 *      c_W = 1.02 sum over the passes of (3.25 + sqrt(R) rho_R),     rho_2 = 1, rho_4 = 2, rho_3 = 5.25, rho_5 = 7.25.
 * The count, per pass, in the l2 norm of the whole sequence relative to its own: a twiddle is exact to u and the four-product complex
 * multiplication to sqrt(5) u (Brent, Percival, Zimmermann 2007), 3.25 u together; an output of a butterfly then differs from the exact
 * sum of its R inputs v_t by at most rho_R u sum_t |v_t| -- R = 2: one addition; R = 4: two levels of additions; R = 3, 5: a rounded
 * constant and a multiplication per term (3.25 u) and R - 1 additions -- which is at most sqrt(R) rho_R u of the butterfly's output norm
 * sqrt(R) |v|_2.  Later passes are sqrt(R) times unitary maps and keep the ratio; 1.02 covers the second order.  The error of one
 * coefficient is at most the norm of the error, and |F|_2 = rms by Parseval; separating the two spectra of a pair is float64.
 * c_1440 (4, 4, 2, 3, 3, 5) = 64.6; skspec_bound_factor(W) returns c_W.  Per slot, with eps_G the same linear combination of the
 * transforms' eps taken with absolute coefficients:
 *      |Phat - P| <= c_k (2 |G| eps_G + eps_G^2) + 2^-40 c_k A       per row, carried through the band mean with |w_j|,
 * summed over m with the slot's 1/M or 1/(M - 1) where the slot is a sum, and A = the slot's value with the terms of G taken by their
 * moduli, e.g. (|F_0| + |D_m|)^2 for member and (sum_m |D_m| / M + |D_y|)^2 for error_mean (for the spread: 2 sum_m |D_m|^2 / (M - 1)).
 * 2^-40 covers the float64 part: fewer than 2^13 roundings of 2^-53 in the combinations, the member sums (M <= 64), the row sums and
 * the chunk sums (H <= 2^12 rows are summed per band).  Values that underflow fp32 are outside the bound.
 *
 * Non-finite values.  Nothing is masked.  A non-finite value in a row makes every coefficient of its transform (and of its pair's
 * partner) non-finite, and so every slot that depends on that transform, for the bands that hold the row and in its channel only:
 * a member m >= 1 reaches member, mean, spread, error_mean and error_member but not truth; the truth reaches truth, error_mean and
 * error_member; member 0 reaches every slot.  No other channel and no band without that row is touched.
 *
 * Limits: C H W <= 2^30 (a member's address is its pointer plus one 32-bit element offset); H <= SKSPEC_MAX_H.  Member and truth
 * pointers need 4-byte alignment (all loads are single words), the member-pointer array, lat_weight, twiddles, `out` and `workspace`
 * 8-byte alignment; `workspace` holds skspec_workspace_bytes(...) bytes. */
#ifndef SKYRIM_SPEC_H
#define SKYRIM_SPEC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SKSPEC_ABI_VERSION 1
#define SKSPEC_E_ARG (-1) /* bad argument: NULL or misaligned pointer, a count, size or index outside its range, a workspace too small */
#define SKSPEC_E_HIP (-2) /* a launch failed */
#define SKSPEC_MAX_MEMBERS 64
#define SKSPEC_MAX_CHANNELS 32
#define SKSPEC_MAX_BANDS 8
#define SKSPEC_MIN_W 2
#define SKSPEC_MAX_W 4096
#define SKSPEC_MAX_H 4096
#define SKSPEC_CHUNK 8         /* rows of one workgroup (= one partial) at most: min(SKSPEC_CHUNK, nc) */
#define SKSPEC_SLOTS 6         /* with a truth; 3 without */

typedef struct {
    const float* const* members; /* device array of M device pointers */
    int M;
    const float* truth;          /* (C, H, W) or NULL */
    int C, H, W;
    int nc;                      /* channels */
    int32_t channels[SKSPEC_MAX_CHANNELS];
    int nb;                      /* bands */
    int32_t j0[SKSPEC_MAX_BANDS], j1[SKSPEC_MAX_BANDS]; /* rows [j0, j1) */
    const double* lat_weight;    /* [H] */
    const float* twiddles;       /* [W][2], skspec_twiddles */
    double* out;                 /* [nc][nb][n_slots][K] */
    void* workspace;
    size_t workspace_bytes;
} skspec_desc;

int skspec_abi_version(void);

/* tw[2 n] = cos(2 pi n / W), tw[2 n + 1] = -sin(2 pi n / W), n = 0 .. W - 1: float64 values rounded to fp32.  HOST memory.  0, or
 * SKSPEC_E_ARG for a W skspec_run would refuse or a NULL pointer */
int skspec_twiddles(int W, float* tw);

/* c_W of the bound; 0 for a W skspec_run would refuse */
double skspec_bound_factor(int W);

/* bytes of workspace skspec_run needs: only M, truth (NULL or not), H, W, nc, nb, j0 and j1 of `desc` are read; 0 for arguments
 * skspec_run would refuse */
size_t skspec_workspace_bytes(const skspec_desc* desc);

int skspec_run(const skspec_desc* desc, void* stream);

#ifdef __cplusplus
}
#endif
#endif
