/* C ABI of the gfx950 FuXi (Swin V2 U-Transformer) call.
 *
 * Replaces what the reference reaches through earth2studio's FuXi ONNX graphs (the reference's skyrim/core/models/fuxi.py:53-54): one
 * call of one cascade stage, levels t - 6 h and t -> t + 6 h.  All on `stream`, no host synchronisation:
 *   skfuxi_embed             two raw states -> per-channel affine -> Conv3d (2 x 4 x 4) as an implicit GEMM; + bias + Linear(12, C) of
 *                            the time encoding in the epilogue -> tokens [180 x 360][C]
 *   skfuxi_layer_norm        out = res + LayerNorm(x) per row (res = NULL: no residual)
 *   skfuxi_conv              3 x 3 conv (stride 1 or 2, zero padding) or 1 x 1 GEMM on channels-last grids, implicit GEMM; the loader
 *                            reads its source plain or GroupNorm-applied + SiLU, or the concatenation of two sources; epilogue: store, or
 *                            the 2 x 2 pixel shuffle of a stride-2 transposed conv
 *   skfuxi_gn_stats          GroupNorm mean / rstd per group: fixed-order reduction, no atomics
 *   skfuxi_gn_residual       out = x + SiLU(GroupNorm(a))
 *   skfuxi_linear            out = act(A W^T + bias) over token rows; or the head: + bias, scattered 4 x 4 into (C, 4 H, 4 W)
 *   skfuxi_window_attention  Swin V2 cosine window attention (shifted or not) with the continuous position bias table
 *   skfuxi_resample          bilinear (Hs, Ws) -> (Ho, Wo) per channel + de-normalisation -> the state
 * The host side (skyrim_amd/fuxi/engine.py) owns the buffers, the prepared weights and the order of the calls.  All pointers are device
 * pointers; calls are asynchronous on `stream` (a hipStream_t); nothing is allocated inside.  Argument checks run before any HIP call, so
 * they work without a GPU.  Every product runs as three fp16 MFMA terms (hi/lo operand planes, fp32 accumulation); softmax, the norms
 * and the cosine normalisation run in fp32.  Grids are row-major (lat, lon); activations channels-last [lat][lon][C]. */
#ifndef SKYRIM_FUXI_H
#define SKYRIM_FUXI_H

#ifdef __cplusplus
extern "C" {
#endif

#define SKFUXI_ABI_VERSION 1
#define SKFUXI_E_ARG (-1)    /* bad argument */
#define SKFUXI_E_HIP (-2)    /* a HIP call failed */
#define SKFUXI_E_WINDOW (-3) /* the attention window does not tile the token grid */

int skfuxi_abi_version(void);
const char* skfuxi_error_string(int code);

/* dst[n][k] (ld = ldw, a multiple of 8 >= K, zero beyond K) = fp16 hi/lo split of src[n * sn + k * sk]; hi plane at dst, lo plane at
 * dst + plane (elements, >= N * ldw). */
int skfuxi_prepare_weight(const float* src, long long sn, long long sk, int N, int K, void* dst, long long plane, int ldw, void* stream);

/* Cube embedding.  Token m = (i, j) of the (n_lat / 4) x (n_lon / 4) grid, k = ((c 2 + l) 4 + dh) 4 + dw (Conv3d weight order), reading
 * x_l[c][4 i + dh][4 j + dw] (x0: t - 6 h, x1: t) as (x - mean[c]) * inv_std[c] before the fp16 split:
 *   tvec[n] = tb[n] + sum_e tw[n][e] temb[e]            (a small kernel first; tvec: caller-owned [C] scratch)
 *   out[m][n] = sum_k A[m][k] W[n][k] + bias[n] + tvec[n]
 * n_lon a multiple of 4, C a multiple of 4. */
typedef struct skfuxi_embed_desc {
    const float* x0;
    const float* x1;
    const float* mean;
    const float* inv_std;
    const void* w;
    long long w_plane;
    int ldw;
    const float* bias;
    const float* tw;
    const float* tb;
    float temb[12];
    float* tvec;
    float* out;
    int channels, n_lat, n_lon, C;
} skfuxi_embed_desc;

int skfuxi_embed(const skfuxi_embed_desc* d, void* stream);

/* out[r][c] = (res ? res[r][c] : 0) + (x[r][c] - mean_r) rstd_r gamma[c] + beta[c]; C a multiple of 4, at most 1536.  out may be res. */
int skfuxi_layer_norm(const float* x, const float* res, const float* gamma, const float* beta, float* out, long long rows, int C, float eps,
                      void* stream);

/* Conv on channels-last grids: out pixel (y, x) of h_out x w_out, k = tap (c0 + c1) + c.
 *   taps = 9: tap = 3 ky + kx reads input pixel (stride y + ky - 1, stride x + kx - 1), zero outside the h_in x w_in grid;
 *   taps = 1: reads (y, x) (stride 1).
 * Channel c < c0 comes from src0, else channel c - c0 of src1 (c1 = 0: none); c0, c1 multiples of 8.  gn_stats != NULL: src0 is read as
 * SiLU((v - mean_g) rstd_g gamma[c] + beta[c]), g = c / (c0 / groups), gn_stats = [groups][2] (mean, rstd) -- padding stays zero.
 * shuffle = 0: out[(y w_out + x)][n] = acc + bias[n], n < cout.
 * shuffle = 1: N = 4 cout columns n = (2 dy + dx) cout + co; out[((2 y + dy) 2 w_out + 2 x + dx)][co] = acc + bias[co].
 * Weights: prepared [N][taps (c0 + c1)]. */
typedef struct skfuxi_conv_desc {
    const float* src0;
    const float* src1;
    const float* gn_stats;
    const float* gn_gamma;
    const float* gn_beta;
    const void* w;
    long long w_plane;
    int ldw;
    const float* bias;
    float* out;
    int h_in, w_in, h_out, w_out, c0, c1, taps, stride, groups, cout, shuffle;
} skfuxi_conv_desc;

int skfuxi_conv(const skfuxi_conv_desc* d, void* stream);

/* stats[g] = (mean, 1 / sqrt(var + eps)) over rows x (C / groups) channels of group g of x [rows][C] (biased variance, float64 sums in a
 * fixed order: the same bits every run). */
int skfuxi_gn_stats(const float* x, long long rows, int C, int groups, float eps, float* stats, void* stream);

/* out[r][c] = x[r][c] + SiLU((a[r][c] - mean_g) rstd_g gamma[c] + beta[c]);  C a multiple of 4.  out may be x. */
int skfuxi_gn_residual(const float* x, const float* a, const float* stats, const float* gamma, const float* beta, float* out, long long rows,
                       int C, int groups, void* stream);

/* mode 0: out[m][n] = act(sum_k a[m][k] W[n][k] + bias[n]), act 1: exact-erf GELU, 0: none.
 * mode 1 (head): token m = (i, j) of a grid w_tok wide, n = (c P + p1) P + p2 (P = patch): out[c][P i + p1][P j + p2] = acc + bias[n],
 * out = [N / P^2][h_img][P w_tok] with h_img = P (M / w_tok).
 * K a multiple of 8, M K < 2^30. */
typedef struct skfuxi_linear_desc {
    const float* a;
    const void* w;
    long long w_plane;
    int ldw;
    const float* bias;
    float* out;
    int M, N, K, act, mode, w_tok, patch;
} skfuxi_linear_desc;

int skfuxi_linear(const skfuxi_linear_desc* d, void* stream);

/* Window attention of a Swin V2 block over an H x W token grid.  qkv [H W][3 C] (q | k | v, head h at 64 h; q and v biases already
 * added), out [H W][C].  The grid is rolled by (-sh, -sw) (token (ys, xs) of the shifted grid is token ((ys + sh) % H, (xs + sw) % W));
 * windows of wh x ww tokens of the shifted grid; out is written back at the unrolled token.  Per head:
 *   score(q, k) = <q / max(|q|, norm_eps), k / max(|k|, norm_eps)> exp(min(logit_scale[h], logit_max)) + cpb[h][(rq - rk + wh - 1)(2 ww - 1)
 *                 + cq - ck + ww - 1] + (mask_value if q and k lie in different Swin regions of the shifted grid)
 * regions: per axis [0, n - win), [n - win, n - s), [n - s, n) when that axis is shifted; mask_lon = 0: longitude not masked (periodic).
 * softmax over the window's keys (online, key tiles of 32), then sum of p v.  Head dim 64.  SKFUXI_E_WINDOW if (wh, ww) does not tile. */
typedef struct skfuxi_attn_desc {
    const float* qkv;
    float* out;
    const float* cpb;
    const float* logit_scale;
    int H, W, C, heads, wh, ww, sh, sw, mask_lon;
    float mask_value, logit_max, norm_eps;
} skfuxi_attn_desc;

int skfuxi_window_attention(const skfuxi_attn_desc* d, void* stream);

/* out[c][y][x] = mean[c] + std[c] bilinear(src[c], y, x) from (h_src, w_src) to (h_out, w_out) as torch's F.interpolate(mode="bilinear",
 * align_corners) computes it. */
typedef struct skfuxi_resample_desc {
    const float* src;
    const float* mean;
    const float* std;
    float* out;
    int channels, h_src, w_src, h_out, w_out, align_corners;
} skfuxi_resample_desc;

int skfuxi_resample(const skfuxi_resample_desc* d, void* stream);

#ifdef __cplusplus
}
#endif
#endif
