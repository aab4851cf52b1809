/* C ABI of the gfx950 DLWP (cubed-sphere U-Net) call.
 *
 * Replaces what the reference reaches through earth2mip.networks.dlwp.load(...) (the reference's skyrim/core/models/dlwp.py:25):
 * one forward of modulus's DLWP with earth2mip's regrids around it.  One call, all on `stream`, no host synchronisation:
 *   skdlwp_ingest     two raw lat-lon states -> normalise -> sparse LL->CS gather; + TISR of each level, land-sea mask, topography
 *                     -> channels-last cube activations [face][y][x][C]
 *   skdlwp_conv       x 11: cube-padded 3 x 3 conv (or the 1 x 1 output conv) as an implicit GEMM; 2 x 2 average pooling, nearest
 *                     upsampling and the skip concatenation are folded into its operand loader; bias + clamped leaky ReLU in the epilogue
 *   skdlwp_egress     sparse CS->LL gather of the 14 output channels -> de-normalise -> the t+6 h and t+12 h states
 * The host side (skyrim_amd/dlwp/engine.py) owns the buffers, the prepared weights and the order of the calls.
 * All pointers are device pointers; calls are asynchronous on `stream` (a hipStream_t); nothing is allocated inside.  Argument checks
 * run before any HIP call, so they work without a GPU.  Every conv product runs as three fp16 MFMA terms (hi/lo operand planes, fp32
 * accumulation).  Cube cells are numbered f n^2 + y n + x (face f < 6, row y, column x; face layout: skyrim_amd/dlwp/spec.py). */
#ifndef SKYRIM_DLWP_H
#define SKYRIM_DLWP_H

#ifdef __cplusplus
extern "C" {
#endif

#define SKDLWP_ABI_VERSION 1
#define SKDLWP_E_ARG (-1) /* bad argument */
#define SKDLWP_E_HIP (-2) /* a HIP call failed */

int skdlwp_abi_version(void);
const char* skdlwp_error_string(int code);

/* dst[n][k] (ld = ldw, a multiple of 8 >= K, zero beyond K) = fp16 hi/lo split of src[n * sn + k * sk]; hi plane at dst, lo plane
 * at dst + plane (elements, >= N * ldw).  The conv weights, as [cout][tap][cin] rows (k = tap cin + c). */
int skdlwp_prepare_weight(const float* src, long long sn, long long sk, int N, int K, void* dst, long long plane, int ldw, void* stream);

/* out[cell][ld_out] for cell < cells = 6 n^2, one thread per cell:
 *   for each level l in (0: x0, 1: x1):  channels c < C:  sum_j S[j] (x_l[c][col[j]] - center[c]) * inv_scale[c]   over the CSR row
 *                                        then TISR at days_l:  max(cos zenith(lat, lon), 0) - 1/pi   (float64)
 *   then statics[cell][0] (land-sea mask), statics[cell][1] (normalised topography), zeros up to ld_out.
 * x0, x1: [C][points] raw states (the older and the newer level); row_ptr [cells + 1], col, S: the LL->CS map (any number of
 * non-zeros per row); lat / lon: cell centres in degrees; days_l: the level's TISR time in days since J2000.0 (2000-01-01 12:00 UTC).
 * C <= 8, ld_out a multiple of 8 >= 2 (C + 1) + 2. */
typedef struct skdlwp_ingest_desc {
    const float* x0;
    const float* x1;
    const float* center;
    const float* inv_scale;
    const int* row_ptr;
    const int* col;
    const float* S;
    const double* lat;
    const double* lon;
    const float* statics;
    double days0, days1;
    float* out;
    int channels, cells, points, ld_out;
} skdlwp_ingest_desc;

int skdlwp_ingest(const skdlwp_ingest_desc* d, void* stream);

/* One conv at face size n: out[cell][0 .. cout) (row stride ld_out) = act(sum_k A[cell][k] W_face[n][k] + bias_face[n]).
 * The input channels are src0's c0 channels, then src1's c1 (the skip; c1 = 0: none), both multiples of 8; src0 is read
 *   mode0 = 0: at face size n,   1: at 2 n as the mean of the 2 x 2 block,   2: at n / 2, nearest (upsampling by 2).
 * taps = 9: k = (3 (dy + 1) + dx + 1) (c0 + c1) + c reads cell (y + dy, x + dx); a cell outside the face comes from the neighbouring face
 *   through pad (int32 [6][4][2]: (face, quarter turns) per side top, bottom, left, right -- spec.py PAD); a corner is the mean of the
 *   two halo cells next to it.  On face flip_face dy runs mirrored (the face is mirrored in rows around its conv).
 * taps = 1: k = c reads the cell itself.
 * Weights: w = prepared [2][cout][taps (c0 + c1)] (equatorial for faces 0-3, then polar for faces 4-5, w_polar elements apart, lo planes
 * w_plane elements after the hi planes); bias [2][cout].  act = 1: leaky ReLU (slope) then min(., clamp_max); act = 0: none.
 * No workgroup covers cells of two faces. */
typedef struct skdlwp_conv_desc {
    const float* src0;
    const float* src1;
    const int* pad;
    const void* w;
    long long w_plane, w_polar;
    int ldw;
    const float* bias;
    float* out;
    int n, c0, c1, mode0, taps, cout, ld_out, act, flip_face;
    float slope, clamp_max;
} skdlwp_conv_desc;

int skdlwp_conv(const skdlwp_conv_desc* d, void* stream);

/* out6[c][p] = scale[c] sum_j S[j] y[col[j]][c] + center[c],   out12[c][p] = scale[c] sum_j S[j] y[col[j]][C + c] + center[c]
 * for points p < points over the CS->LL CSR rows (row_ptr [points + 1]); y: [cells][ld_y] cube output, ld_y a multiple of 4 >= 2 C. */
typedef struct skdlwp_egress_desc {
    const float* y;
    const int* row_ptr;
    const int* col;
    const float* S;
    const float* center;
    const float* scale;
    float* out6;
    float* out12;
    int channels, cells, points, ld_y;
} skdlwp_egress_desc;

int skdlwp_egress(const skdlwp_egress_desc* d, void* stream);

#ifdef __cplusplus
}
#endif
#endif
