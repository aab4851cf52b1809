/* C ABI of cyclone detection on the device: the candidate centres of M member states of one valid time, found where the states lie in
 * HBM.  Only 32-byte candidate records go back to the caller; the host links them into tracks (skyrim_amd/tracks.py).
 *
 * Conventions of skyrim_score.h and skyrim_ens.h: all data pointers are device pointers; every call is asynchronous on `stream` (a
 * hipStream_t); nothing is allocated inside; the return code is 0, SKTRACK_E_ARG or SKTRACK_E_HIP; argument errors are found before
 * anything touches the GPU, so they are reported on a machine without one.
 *
 * ---- sktrack_detect ------------------------------------------------------------------------------------------------------------------
 * States are contiguous float32 (C, H, W): a DEVICE array of M member pointers (1 <= M <= SKTRACK_MAX_MEMBERS), rows j = latitudes as
 * the model orders them, columns i = longitudes, periodic.  Channels: msl, u10, v10, u850, v850 and, for the warm core, z_up and z_lo
 * (both -1: no warm-core criterion).  Centres are sought on the band of rows [j0, j1).
 *
 * Geometry is integer on the device.  For each criterion r in {msl, vort, wind, core} the host hands over h_r[j1 - j0][2 D_r + 1]
 * (int32): for band row j and row offset dj in [-D_r, D_r], h_r[j - j0][dj + D_r] is the largest k >= 0 for which the great-circle
 * (haversine) distance from (lat_j, 0) to (lat_{j+dj}, k dlon) is <= R_r on a sphere of radius 6371 km, and -1 when row j + dj is outside
 * the grid or out of reach.  The window of centre (j, i) is the set {(j + dj, (i + di) mod W) : |di| <= h_r[j - j0][dj + D_r]}: the kernel
 * compares integers and never computes a distance, so the window is an exact set.  The host makes the tables in float64 and refuses
 * radii for which a half-width reaches W / 2, a window contains the first or the last row of the grid (a pole row; the vorticity stencil
 * needs the rows above and below every window point), or the 3 x 3 neighbourhood of a band row is not inside its msl window.  The library
 * cannot read the tables, so it checks what makes every access in bounds whatever they hold: 1 <= j0 - D_r and j1 - 1 + D_r <= H - 2
 * for every r in use, and it clamps a half-width to (W - 1) / 2.
 *
 * Row coefficients rowc[H][4] (float32, made in float64 on the host and rounded), with lat in radians, a = 6371000 m:
 *   rowc[j][0] = A_j  = 1 / (2 a cos(lat_j) dlon)
 *   rowc[j][1] = B+_j = cos(lat_{j+1}) / (a cos(lat_j) (lat_{j+1} - lat_{j-1}))
 *   rowc[j][2] = B-_j = cos(lat_{j-1}) / (a cos(lat_j) (lat_{j+1} - lat_{j-1}))
 *   rowc[j][3] = sgn(lat_j): -1, 0 or +1            (rows 0 and H - 1: all four are 0 and are never read)
 *
 * Criteria for a centre c = (j, i) of member m, idx = j W + i.  All comparisons are fp32; a NaN compares false everywhere:
 *   1. Pressure minimum (exact).  p_c <= thr_msl, and every other point q of the msl window has p_c < p_q, or p_c == p_q and
 *      idx_c < idx_q: (p_c, idx_c) is the lexicographic minimum of its window, ties go to the lower index, a plateau yields one
 *      centre.  Written this way a NaN at the centre or anywhere in the window means no centre there.
 *   2. Cyclonic vorticity.  vort = max over the vort window of zeta_q sgn(lat_row(q)) >= thr_vort, with, at 850 hPa and in this
 *      order of operations, each one rounded to fp32 and none contracted into an fma:
 *         t1 = A_j (v[j][i+1] - v[j][i-1]);   t2 = B+_j u[j+1][i];   t3 = B-_j u[j-1][i];   zeta = t1 - (t2 - t3)
 *   3. Wind.  wind = max over the wind window of sqrtf(u10 u10 + v10 v10) >= thr_wind (two products, one sum, one square root, not
 *      contracted).  This value is the reported intensity.
 *   4. Warm core (only with z_up, z_lo >= 0).  tau = z_up - z_lo and d_q = tau_q - tau_c in fp32 over the N points of the core window
 *      (the centre included); core = (float)((double)max_q d_q - (sum_q (double)d_q) / N) >= thr_core.
 * The maxima start from -inf and take x where x > best, so a NaN never enters one; a NaN d_q makes `core` NaN and the centre fails.
 *
 * Output.  sktrack_record is 32 bytes {int32 member, j, i; float msl, vort, wind, core; int32 pad = 0}; msl = p_c, bit for bit;
 * core = 0 without the warm-core criterion.  The call first sets *count to 0; every centre takes the slot atomicAdd(count, 1) (an integer
 * atomic; there is no floating-point atomic anywhere) and writes its record only if slot < capacity: the counter keeps counting, the
 * order of the records is arbitrary (sort by (member, j, i)), and nothing else in the buffer is touched.
 *
 * Shape of the computation.  Kernel 1, the prefilter: one wave per (member, band row), 62 points per wave step with a one-point halo on
 * either side shared through lane shuffles; a point survives when it is the lexicographic minimum of its 3 x 3 neighbourhood and
 * p_c <= thr_msl.  Each member's msl band is read from HBM once.  Two survivors are never neighbours, so a member has at most
 * ceil(Hb / 2) ceil(W / 2) of them (Hb = j1 - j0): survivors are appended as (member, idx) pairs to a list in the workspace,
 * sktrack_workspace_bytes(M, Hb, W) = 16 + 8 M ceil(Hb / 2) ceil(W / 2).  Kernel 2: one wave per survivor walks the rows of each window
 * with its 64 lanes along the longitude and reduces over the wave -- a lexicographic minimum, three maxima, one float64 sum and the
 * point count -- in the order 1, 2, 3, 4, leaving at the first criterion that fails.  Member pointers are wave-uniform (scalar
 * registers); the per-lane part of an address is one 32-bit byte offset.
 *
 * Bounds, against exact arithmetic on the same fp32 inputs (states and rowc), u = 2^-24:
 *   msl:   exact.
 *   vort:  |vort - exact| <= 4 u max_q (|A| (|v_e| + |v_w|) + |B+ u_n| + |B- u_s|) over the vort window.  Per point: t1 carries two
 *          roundings (2u |t1|, |t1| <= |A| (|v_e| + |v_w|)), t2 and t3 one each, t2 - t3 one (u |t2 - t3| <= u (|t2| + |t3|)), the last
 *          subtraction one (u |zeta| <= u (|t1| + |t2| + |t3|)): 3 u (sum of the terms' absolute values) to first order; k = 4 covers the
 *          products of roundings.  The sign factor and the maximum are exact, and a maximum moves by at most the largest error under it.
 *   wind:  |wind - exact| <= 4 u wind: the sum under the root has relative error 2u (one rounding per product, one for the sum, all
 *          addends >= 0), the root halves it and adds its own rounding (correctly rounded or within 1 ulp = 2u): 3u, k = 4 as above.
 *   core:  |core - exact| <= (12 u + 2^-40) T, T = max |tau_q| over the core window, tau exact: d_q carries u (|tau_q| + |tau_c| + |d_q|)
 *          <= 4 u T, the maximum and the mean of the d_q each move by at most that, and the final rounding to fp32 adds u |core| <= 4 u T;
 *          2^-40 covers the float64 sum and division.
 *
 * Limits: C H W <= 2^30, W >= 3, member pointers 4-byte aligned (there is no vector path: nothing else is required of them), tables and
 * records 4-byte, the workspace 8-byte aligned. */
#ifndef SKYRIM_TRACK_H
#define SKYRIM_TRACK_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SKTRACK_ABI_VERSION 1
#define SKTRACK_E_ARG (-1) /* bad argument: NULL or misaligned pointer, a count or index outside its range, a workspace too small */
#define SKTRACK_E_HIP (-2) /* a launch failed */
#define SKTRACK_MAX_MEMBERS 64

typedef struct {
    int32_t member, j, i;
    float msl, vort, wind, core;
    int32_t pad;
} sktrack_record;

int sktrack_abi_version(void);

/* bytes of workspace a call on M members and a band of Hb rows of W points needs; 0 for arguments sktrack_detect would refuse */
size_t sktrack_workspace_bytes(int M, int Hb, int W);

typedef struct {
    const float* const* members; /* device array of M device pointers */
    int M;
    int C, H, W;
    int ch_msl, ch_u10, ch_v10, ch_u850, ch_v850;
    int ch_zup, ch_zlo;          /* both -1: no warm-core criterion */
    int j0, j1;                  /* the band of centre rows [j0, j1) */
    float thr_msl, thr_vort, thr_wind, thr_core;
    const int32_t* h_msl;        /* [j1 - j0][2 d_msl + 1] */
    const int32_t* h_vort;
    const int32_t* h_wind;
    const int32_t* h_core;       /* ignored without the warm core */
    int d_msl, d_vort, d_wind, d_core;
    const float* rowc;           /* [H][4] */
    sktrack_record* records;     /* [capacity] */
    int capacity;
    int32_t* count;              /* one int32: set to 0, then incremented once per centre */
    void* workspace;
    size_t workspace_bytes;
} sktrack_desc;

int sktrack_detect(const sktrack_desc* desc, void* stream);

#ifdef __cplusplus
}
#endif
#endif
