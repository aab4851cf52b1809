/* C ABI of the gfx950 FourCastNet v1 (AFNO) step.
 *
 * Replaces what the reference reaches through earth2mip.networks.fcn.load(...) (the reference's skyrim/core/models/fourcastnet.py:24-25):
 * the forward of the published AFNONet (patch embedding, 12 AFNO blocks, linear head) on torch.  Per step:
 *   skfcn_patch_embed    x (raw state) -> normalise -> 8x8 / stride-8 convolution + bias + pos_embed        -> tokens [T][E]
 *   skfcn_spectral_run   LayerNorm1 -> truncated rfft2 (DFT GEMMs) -> block-diagonal complex MLP (ONE kernel: skfcn_spectral_mlp)
 *                        -> irfft2 -> + LayerNorm1 output + block input                                       (in place on the tokens)
 *   skfcn_mlp_run        LayerNorm2 -> fc1 -> erf-GELU -> fc2 -> + residual as ONE kernel (the hidden activation stays on chip)
 *   skfcn_head_run       tokens x head^T (de-normalisation folded in), scattered into the (C, H, W) state
 * The host side (skyrim_amd/fcn/engine.py) owns the buffers, the prepared matrices and the order of the calls.
 * All pointers are device pointers; calls are asynchronous on `stream` (a hipStream_t); nothing is allocated inside.  Argument
 * checks run before any HIP call, so they work without a GPU.  Every product runs as three fp16 MFMA terms (hi/lo operand
 * planes, fp32 accumulation). */
#ifndef SKYRIM_FCN_H
#define SKYRIM_FCN_H

#ifdef __cplusplus
extern "C" {
#endif

#define SKFCN_ABI_VERSION 1
#define SKFCN_E_ARG (-1) /* bad argument */
#define SKFCN_E_HIP (-2) /* a HIP call failed */

int skfcn_abi_version(void);
const char* skfcn_error_string(int code);

/* dst[n][k] (ld = ldw, a multiple of 8 >= K, zero beyond K) = fp16 hi/lo split of src[n * sn + k * sk]; hi plane at dst,
 * lo plane at dst + plane (elements, >= N * ldw).  Constant matrices of the GEMM-shaped calls (patch embedding, DFTs, head). */
int skfcn_prepare_weight(const float* src, long long sn, long long sk, int N, int K, void* dst, long long plane, int ldw, void* stream);

/* Fragment-order fp16 hi/lo planes of `batch` expand / contract pairs for the fused MLP kernels:
 * w1: batch x [H][K], w2: batch x [N][H] fp32 contiguous (K, H, N multiples of 32) -> w1f: batch x 2 H K, w2f: batch x 2 N H elements. */
int skfcn_prepare_mlp_weights(const float* w1, const float* w2, int K, int H, int N, int batch, void* w1f, void* w2f, void* stream);

/* out[t][e] = sum_{c, p1, p2} ((x[c][hh P + p1][ww P + p2] * kscale[k] + kshift[k]) * W[e][k]) + bias[e] + pos[t][e],
 * t = hh (Wimg / P) + ww, k = (c P + p1) P + p2.  The patch is gathered from the raw state (no im2col buffer); the affine
 * (input normalisation) runs before the fp16 split. */
typedef struct skfcn_patch_embed_desc {
    const float* x;                 /* [cin][himg][wimg] */
    const float* kscale;            /* [cin P P] */
    const float* kshift;            /* [cin P P] */
    const void* w;                  /* skfcn_prepare_weight of [embed][cin P P] */
    long long w_plane;
    int ldw;
    const float* bias;              /* [embed] */
    const float* pos;               /* [T][embed] */
    float* out;                     /* [T][embed] */
    int cin, himg, wimg, patch, embed;
} skfcn_patch_embed_desc;

int skfcn_patch_embed(const skfcn_patch_embed_desc* d, void* stream);

/* out[r][:] = LayerNorm(x[r][:]) * gamma + beta over C channels, r < rows; C a multiple of 4, <= 1024 */
int skfcn_layer_norm(const float* x, const float* gamma, const float* beta, float* out, long long rows, int C, float eps, void* stream);

/* Block-diagonal complex MLP of the AFNO filter, both layers in ONE kernel, in place on a spectrum.  Mode q < rows, block b < nblocks
 * (block size 96): the real parts of its channels 96 b + [0, 96) are at z[(q / m1) * sm2 + (q % m1) * sm + 96 b + i], the imaginary
 * parts im_off further.  With v = (re, im) (192 values):
 *   o1 = ReLU(W1e[b] v + b1e[b]),  z <- softshrink(W2e[b] o1 + b2e[b], lambda)
 * W1e / W2e are the real 192 x 192 forms [[Wr^T, -Wi^T], [Wi^T, Wr^T]] of the complex weights, prepared by skfcn_prepare_mlp_weights
 * (batch = nblocks); b1e / b2e: [nblocks][192] (re | im).  o1 never leaves registers. */
typedef struct skfcn_spectral_mlp_desc {
    float* z;
    long long rows, sm, sm2, im_off;
    int m1, nblocks;
    const void* w1f;
    const void* w2f;
    const float* b1e;
    const float* b2e;
    float lambda;
} skfcn_spectral_mlp_desc;

int skfcn_spectral_mlp(const skfcn_spectral_mlp_desc* d, void* stream);

/* One AFNO filter plus the block's double skip, in place on the tokens t [h][w][C] (T = h w):
 *   u = LayerNorm1(t);  U = rfft2(u) truncated to longitude modes m < km (all h latitude frequencies);  S = skfcn_spectral_mlp(U);
 *   t <- irfft2(S, (h, w)) + u + t        (ortho normalisation; the C2R drops the imaginary part of the m = 0 column)
 * Spectra are [2 h][km][C] (index (2 freq + re/im)); the four DFTs are GEMMs against prepared matrices:
 *   fw [2 km][w]   (row ri km + m),    fl [2 h][2 h] (latitude forward),    il [2 h][2 h] (inverse),    iw [w][2 km] (C2R).
 * u, s0, s1 are workspaces: [T][C], [2 h km C], [2 h km C] floats. */
typedef struct skfcn_spectral_desc {
    float* t;
    float* u;
    float* s0;
    float* s1;
    const float* gamma;
    const float* beta;
    float eps;
    const void *fw, *fl, *il, *iw;             /* prepared (skfcn_prepare_weight) */
    long long fw_plane, fl_plane, il_plane, iw_plane;
    int fw_ld, fl_ld, il_ld, iw_ld;
    int h, w, C, km, nblocks;
    const void* w1f;
    const void* w2f;
    const float* b1e;
    const float* b2e;
    float lambda;
} skfcn_spectral_desc;

int skfcn_spectral_run(const skfcn_spectral_desc* d, void* stream);

/* out[r] = x[r] + W2 GELU(W1 LayerNorm(x[r]) + b1) + b2 as ONE kernel (r < rows, any row count; out != x).  C in {192, 768}, hidden a
 * multiple of 32; w1f / w2f from skfcn_prepare_mlp_weights(K = C, H = hidden, N = C).  The hidden activation never reaches memory. */
typedef struct skfcn_mlp_desc {
    const float* x;
    float* out;
    long long rows;
    int C, hidden;
    const float* gamma;
    const float* beta;
    float eps;
    const void* w1f;
    const void* w2f;
    const float* b1;
    const float* b2;
} skfcn_mlp_desc;

int skfcn_mlp_run(const skfcn_mlp_desc* d, void* stream);

/* y[c][hh P + p1][ww P + p2] = sum_e t[hh (wimg / P) + ww][e] W[n][e] + bias[n],  n = (p1 P + p2) cout + c.
 * W: skfcn_prepare_weight of [P P cout][embed] (the output de-normalisation folded in: rows * std_c, bias = mean_c). */
typedef struct skfcn_head_desc {
    const float* t;
    const void* w;
    long long w_plane;
    int ldw;
    const float* bias;
    float* out;
    int cout, himg, wimg, patch, embed;
} skfcn_head_desc;

int skfcn_head_run(const skfcn_head_desc* d, void* stream);

#ifdef __cplusplus
}
#endif
#endif
