/* C ABI of the gfx950 FengWu (cross-modal Swin transformer) call.
 *
 * Replaces what the reference reaches through earth2studio's FengWu ONNX graph (the reference's skyrim/core/models/fengwu.py): one call,
 * levels t - 6 h and t -> t + 6 h.  All on `stream`, no host synchronisation:
 *   skfw_embed             every modality's patch embedding in one launch: its channel slice of both raw states, normalised, zero rows
 *                          padded, Conv2d (4 x 4, stride 4) as an implicit GEMM + bias -> tokens [mods][h1 w1][C]
 *   skfw_layer_norm        LayerNorm of token rows, batched over modalities (per-modality gamma / beta); or the 2 x 2 patch-merge gather
 *                          followed by its LayerNorm
 *   skfw_linear            out = act(A W^T + bias) (+ residual), batched over modalities; A may be two sources along K (the skip);
 *                          or the patch expand: the 2 x 2 pixel shuffle, cropped to the kept rows
 *   skfw_window_attention  scaled dot-product window attention, head dim 32, over a padded (Z, H, W) token grid: 2-D windows batched over
 *                          modalities (Z = 1) or 3-D windows over (modality, lat, lon); shifts by token indexing; the bias (and the shift
 *                          mask folded into it) read from a dense table
 *   skfw_recover           every modality's ConvTranspose2d (4 x 4, stride 4) as a GEMM with a 4 x 4 scatter, cropped to n_lat rows,
 *                          de-normalised into its planes of the state
 * One call of the default network is  7 + 7 (enc_depths[0] + enc_depths[1] + fuser_depth + dec_depths[0] + dec_depths[1])  launches
 * (161): embed, its LayerNorm, 7 per Swin block (LayerNorm, QKV, attention, proj + residual, LayerNorm, fc1 + GELU, fc2 + residual),
 * merge gather + LayerNorm, merge linear, expand, skip linear, recovery.
 * The host side (skyrim_amd/fengwu/engine.py) owns the buffers, the prepared weights, the bias tables and the order of the calls.  All
 * pointers are device pointers; calls are asynchronous on `stream` (a hipStream_t); nothing is allocated inside.  Argument checks run
 * before any HIP call, so they work without a GPU.  Every product runs as three fp16 MFMA terms (hi/lo operand planes, fp32
 * accumulation); LayerNorm and softmax run in fp32.  States are [channels][n_lat][n_lon]; activations channels-last, modality-major
 * [mods][lat][lon][C]. */
#ifndef SKYRIM_FENGWU_H
#define SKYRIM_FENGWU_H

#ifdef __cplusplus
extern "C" {
#endif

#define SKFW_ABI_VERSION 1
#define SKFW_E_ARG (-1)    /* bad argument */
#define SKFW_E_HIP (-2)    /* a HIP call failed */
#define SKFW_E_WINDOW (-3) /* the attention window does not tile its padded token grid */
#define SKFW_MAX_MODS 8

int skfw_abi_version(void);
const char* skfw_error_string(int code);

/* dst[n][k] (ld = ldw, a multiple of 8 >= K, zero beyond K) = fp16 hi/lo split of src[n * sn + k * sk]; hi plane at dst, lo plane at
 * dst + plane (elements, >= N * ldw). */
int skfw_prepare_weight(const float* src, long long sn, long long sk, int N, int K, void* dst, long long plane, int ldw, void* stream);

/* Patch embedding of every modality z < mods (grid z of the launch).  Token m = (i, j) of h_tok x (n_lon / 4), k = (p 4 + dh) 4 + dw,
 * plane p = l cnt + c (l = 0: x0 = t - 6 h, 1: x1 = t; c < cnt = ch_cnt[z]), reading x_l[ch_off[z] + c][4 i + dh - lat_front][4 j + dw]
 * as (x - mean) * inv_std, zero outside the n_lat rows; k >= 32 cnt reads zero (a smaller modality's weight is zero-padded to K):
 *   out[z][m][n] = sum_k A[m][k] W[z][n][k] + bias[z C + n]
 * W: prepared [mods][C][K] (hi planes w_sb elements apart, then the lo planes w_plane further).  K = 32 max cnt, n_lon and C multiples
 * of 4. */
typedef struct skfw_embed_desc {
    const float* x0;
    const float* x1;
    const float* mean;
    const float* inv_std;
    const void* w;
    long long w_plane, w_sb;
    int ldw;
    const float* bias;
    float* out;
    int mods, n_lat, n_lon, lat_front, h_tok, C, K;
    int ch_off[SKFW_MAX_MODS], ch_cnt[SKFW_MAX_MODS];
} skfw_embed_desc;

int skfw_embed(const skfw_embed_desc* d, void* stream);

/* LayerNorm of `rows` rows of C per batch entry z < batch (gamma, beta: [batch][C]; x, out: [batch][rows][C]):
 *   out[z][r][c] = (x[z][r][c] - mean_r) rstd_r gamma[z][c] + beta[z][c]
 * merge = 1: row r = (i, j) of the (rows / (w_src / 2)) x (w_src / 2) grid gathers C = 4 c_src from x [batch][h_src][w_src][c_src] as
 * [x(2i, 2j) ; x(2i + 1, 2j) ; x(2i, 2j + 1) ; x(2i + 1, 2j + 1)] with source row 2i + dy - front, zero outside [0, h_src) (Swin's
 * patch merge).  C a multiple of 4 (of 16 with merge), at most 1536. */
typedef struct skfw_ln_desc {
    const float* x;
    const float* gamma;
    const float* beta;
    float* out;
    long long rows;
    int batch, C, merge, h_src, w_src, front;
    float eps;
} skfw_ln_desc;

int skfw_layer_norm(const skfw_ln_desc* d, void* stream);

/* Batched linear, grid z < batch:  acc[m][n] = sum_k A[z][m][k] W[z][n][k],  A[z][m][k] = a[z a_sb + m lda + k] for k < k_split, else
 * a2[z a2_sb + m lda2 + k - k_split] (a2 = NULL: one source, k_split ignored).
 * mode 0: out[z o_sb + m N + n] = act(acc + bias[z b_sb + n]) + (res ? res[z o_sb + m N + n] : 0); act 1: exact-erf GELU; out may be res.
 * mode 1 (patch expand): token m = (y, x) of a grid w_tok wide, n = (2 dy + dx) Co + c (Co = N / 4):
 *        out[z o_sb + ((2 y + dy - front) 2 w_tok + 2 x + dx) Co + c] = acc + bias[z b_sb + n], rows 2 y + dy - front outside [0, h_out) dropped.
 * bias may be NULL (none).  K, lda, lda2, k_split multiples of 8; N a multiple of 4; M lda, M lda2 < 2^30. */
typedef struct skfw_linear_desc {
    const float* a;
    const float* a2;
    const void* w;
    long long w_plane, w_sb;
    int ldw;
    const float* bias;
    const float* res;
    float* out;
    long long a_sb, a2_sb, o_sb, b_sb;
    int batch, M, N, K, lda, lda2, k_split, act, mode, w_tok, h_out, front;
} skfw_linear_desc;

int skfw_linear(const skfw_linear_desc* d, void* stream);

/* Window attention over a token grid (Z, H, W) zero-padded to (Zp, Hp, Wp) (fz, fh, fw rows in front), batch entry b < batch.
 * qkv [batch][Z H W][3 C] (q | k | v, head h at 32 h, biases added); a padded token's q, k, v are qkv_bias[b][3 C] (the qkv linear of a
 * zero row).  The padded grid is rolled by (-sz, -sh, -sw): shifted-grid token (zs, ys, xs) is padded token ((zs + sz) % Zp, ...).  Windows
 * of wz x wh x ww tokens of the shifted grid, local index i = (iz wh + iy) ww + ix.  Window (a, b, .) of the (Zp / wz) x (Hp / wh) rows of
 * windows reads table type t = ta types_y + tb, ta = a if types_z == Zp / wz, else (types_z == 2 ? a == last : 0), tb likewise:
 *   score(i, j) = scale <q_i, k_j> + table[b table_sb + ((t heads + h) N + i) N + j]        (N = wz wh ww)
 * softmax over the window's keys (online, key tiles of 32), then sum of p v -> out [batch][Z H W][C] at the unrolled, unpadded token
 * (padded queries are not written).  Head dim 32.  SKFW_E_WINDOW if (wz, wh, ww) does not tile (Zp, Hp, Wp). */
typedef struct skfw_attn_desc {
    const float* qkv;
    const float* qkv_bias;
    const float* table;
    float* out;
    long long table_sb;
    int batch, Z, H, W, Zp, Hp, Wp, fz, fh, fw, wz, wh, ww, sz, sh, sw, types_z, types_y, C, heads;
    float scale;
} skfw_attn_desc;

int skfw_window_attention(const skfw_attn_desc* d, void* stream);

/* Recovery of every modality z < mods: token m = (i, j) of h_tok x w_tok, n = (c 4 + p1) 4 + p2 (N = 16 c_max; c < ch_cnt[z] kept):
 *   out[ch_off[z] + c][4 i + p1 - lat_front][4 j + p2] = (sum_k a[z][m][k] W[z][n][k] + bias[z c_max + c]) std[ch] + mean[ch]
 * rows outside [0, n_lat) dropped; out [channels][n_lat][4 w_tok].  W: prepared [mods][16 c_max][C], C a multiple of 8. */
typedef struct skfw_recover_desc {
    const float* a;
    const void* w;
    long long w_plane, w_sb;
    int ldw;
    const float* bias;
    const float* mean;
    const float* std;
    float* out;
    int mods, h_tok, w_tok, C, c_max, n_lat, lat_front;
    int ch_off[SKFW_MAX_MODS], ch_cnt[SKFW_MAX_MODS];
} skfw_recover_desc;

int skfw_recover(const skfw_recover_desc* d, void* stream);

#ifdef __cplusplus
}
#endif
#endif
