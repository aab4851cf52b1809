// FuXi (Swin V2 U-Transformer) call behind include/skyrim_fuxi.h.
//
//   embed        gemm.h's pipeline with ALEmbed: the 2 x 4 x 4 cube of a token gathered from the two raw levels, the per-channel affine
//                applied before the fp16 split; EpFuxi adds the bias and the time-encoding vector
//   conv         gemm.h's pipeline with ALConv: 3 x 3 taps (stride 1 / 2, zero padding) or 1 x 1 over channels-last grids, the source
//                read plain, GroupNorm-applied + SiLU, or as the concatenation of two sources; EpFuxi stores or pixel-shuffles (2 x 2)
//   linear       gemm.h's pipeline with ALFast rows; EpFuxi: bias (+ GELU), or the head's 4 x 4 scatter into (C, 4 H, 4 W)
//   attention    window_attn.h's body (one wave = 16 queries of one (window, head), online softmax over key tiles of 32) with head
//                dim 64; FxAttn supplies the 2-D roll, the cosine normalisation of q and k with the clamped logit scale, and the
//                continuous position bias + region mask of a score
//   row kernels  LayerNorm (+ residual: rownorm.h), GroupNorm statistics (float64, fixed order), GroupNorm + SiLU + residual, bilinear
//                resample
#include <hip/hip_runtime.h>

#include "../../include/skyrim_fuxi.h"
#include "rownorm.h"
#include "strided_gemm.h"
#include "window_attn.h"

namespace skp {

typedef TileCfg<128, 128, 32, 2, 4> TFx;     // 8 waves of 64 x 32

// ---- cube embedding loader: token m = (i, j), k = ((c 2 + l) 4 + dh) 4 + dw; a chunk of 8 = two rows dh of 4 pixels ------------- //
struct ALEmbed {
    static constexpr bool kDirect = false;
    const float* x0;
    const float* x1;
    const float* mean;
    const float* inv_std;
    int M, K, wt, n_lon;
    long long hw;
    struct Row { long long off; int ok; };
    struct Raw { float v[8]; int c; };
    __device__ __forceinline__ Row row(int m) const {
        if (m >= M) return Row{0, 0};
        const int i = m / wt, j = m - i * wt;
        return Row{(long long)(4 * i) * n_lon + 4 * j, 1};
    }
    __device__ __forceinline__ void issue(const Row& r, int k, Raw& o) const {
#pragma unroll
        for (int i = 0; i < 8; ++i) o.v[i] = 0.f;
        o.c = -1;
        if (!r.ok || k >= K) return;
        const int cl = k >> 4, dh = (k >> 2) & 3;            // (c, l) pair and the first of the chunk's two rows
        const int c = cl >> 1;
        const float* p = ((cl & 1) ? x1 : x0) + c * hw + r.off + (long long)dh * n_lon;
        const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + n_lon);
        o.v[0] = a.x; o.v[1] = a.y; o.v[2] = a.z; o.v[3] = a.w; o.v[4] = b.x; o.v[5] = b.y; o.v[6] = b.z; o.v[7] = b.w;
        o.c = c;
    }
    __device__ __forceinline__ void finish(const Raw& r, float (&v)[8]) const {
        if (r.c < 0) {
#pragma unroll
            for (int i = 0; i < 8; ++i) v[i] = 0.f;
            return;
        }
        const float mu = mean[r.c], is = inv_std[r.c];
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = (r.v[i] - mu) * is;
    }
    __device__ __forceinline__ uint4 direct(const Raw&) const { return make_uint4(0, 0, 0, 0); }
};

__device__ __forceinline__ float silu(float x) { return x / (1.0f + expf(-x)); }

// ---- conv loader: output pixel m = (y, x), k = tap (c0 + c1) + c ----------------------------------------------------------------- //
struct ALConv {
    static constexpr bool kDirect = false;
    const float* src0;
    const float* src1;
    const float* gn_stats;
    const float* gamma;
    const float* beta;
    int M, K, h_in, w_in, w_out, c0, c1, cin, taps, stride, cpg;
    struct Row { int y, x, ok; };
    struct Raw { float v[8]; int c; };                       // c: src0 channel of v[0] to GroupNorm-apply, -1: none / zero chunk
    __device__ __forceinline__ Row row(int m) const {
        if (m >= M) return Row{0, 0, 0};
        const int y = m / w_out;
        return Row{y, m - y * w_out, 1};
    }
    __device__ __forceinline__ void issue(const Row& r, int k, Raw& o) const {
#pragma unroll
        for (int i = 0; i < 8; ++i) o.v[i] = 0.f;
        o.c = -1;
        if (!r.ok || k >= K) return;
        const int tap = k / cin, c = k - tap * cin;
        int iy = r.y, ix = r.x;
        if (taps == 9) {
            iy = r.y * stride + tap / 3 - 1;
            ix = r.x * stride + tap % 3 - 1;
            if (iy < 0 || iy >= h_in || ix < 0 || ix >= w_in) return;      // zero padding (after the activation)
        }
        const long long pix = (long long)iy * w_in + ix;
        const float* p = c < c0 ? src0 + pix * c0 + c : src1 + pix * c1 + (c - c0);
        load8(p, o.v);
        if (gn_stats != nullptr && c < c0) o.c = c;
    }
    __device__ __forceinline__ void finish(const Raw& r, float (&v)[8]) const {
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = r.v[i];
        if (r.c >= 0) {
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int c = r.c + i, g = c / cpg;
                v[i] = silu((v[i] - gn_stats[2 * g]) * gn_stats[2 * g + 1] * gamma[c] + beta[c]);
            }
        }
    }
    __device__ __forceinline__ uint4 direct(const Raw&) const { return make_uint4(0, 0, 0, 0); }
};

// ---- epilogue: mode 0 store (+ bias, + add vector, GELU), 1 pixel shuffle 2 x 2, 2 head scatter P x P ---------------------------- //
enum { EP_STORE = 0, EP_SHUFFLE = 1, EP_HEAD = 2 };

struct EpFuxi {
    static constexpr bool kDualOrder = false;
    template <class TC> __device__ __forceinline__ void init(char*, int, int) const {}
    float* out;
    const float* bias;
    const float* add;          // EP_STORE: a second per-column vector (the time encoding), or null
    int mode, act, ldo;        // ldo: EP_STORE row stride; EP_SHUFFLE: cout
    int w_tok, P;              // EP_SHUFFLE: w_tok = input grid width; EP_HEAD: token grid width, patch
    long long hw;              // EP_HEAD: output plane size
    template <class TC, bool SWAP>
    __device__ __forceinline__ void run(f32x4 (&acc)[TC::FM][TC::FN], int m0w, int n0w, int lane, int, int, char*, int M, int N, int) const {
        static_assert(SWAP, "swapped order: a lane holds 4 consecutive columns of one row");
        const int l15 = lane & 15, l4 = (lane >> 4) * 4;
#pragma unroll
        for (int a = 0; a < TC::FM; ++a) {
            const int m = m0w + a * 16 + l15;
            if (m >= M) continue;
#pragma unroll
            for (int b = 0; b < TC::FN; ++b) {
                const int n = n0w + b * 16 + l4;
                if (n >= N) continue;
                float v[4];
                if (mode == EP_STORE) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        float t = acc[a][b][r] + (n + r < N ? bias[n + r] + (add ? add[n + r] : 0.f) : 0.f);
                        v[r] = act ? gelu_erf(t) : t;
                    }
                    float* o = out + (long long)m * ldo + n;
                    if (n + 3 < N) {
                        *reinterpret_cast<float4*>(o) = make_float4(v[0], v[1], v[2], v[3]);
                    } else {
#pragma unroll
                        for (int r = 0; r < 4; ++r)
                            if (n + r < N) o[r] = v[r];
                    }
                } else if (mode == EP_SHUFFLE) {
                    const int co = n % ldo, q = n / ldo;             // ldo % 4 == 0: the 4 columns share q
                    const int y = m / w_tok, x = m - y * w_tok;
                    const long long pix = (long long)(2 * y + (q >> 1)) * (2 * w_tok) + 2 * x + (q & 1);
#pragma unroll
                    for (int r = 0; r < 4; ++r) v[r] = acc[a][b][r] + bias[co + r];
                    *reinterpret_cast<float4*>(out + pix * ldo + co) = make_float4(v[0], v[1], v[2], v[3]);
                } else {
                    const int i = m / w_tok, j = m - i * w_tok, wimg = P * w_tok;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int nn = n + r;
                        if (nn >= N) continue;
                        const int c = nn / (P * P), rem = nn - c * P * P, p1 = rem / P, p2 = rem - p1 * P;
                        out[c * hw + (long long)(P * i + p1) * wimg + P * j + p2] = acc[a][b][r] + bias[nn];
                    }
                }
            }
        }
    }
};

__global__ void __launch_bounds__(256) time_vec_kernel(const float* __restrict__ tw, const float* __restrict__ tb, skfuxi_embed_desc d) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= d.C) return;
    float s = tb[n];
#pragma unroll
    for (int e = 0; e < 12; ++e) s += tw[n * 12 + e] * d.temb[e];
    d.tvec[n] = s;
}

// ---- LayerNorm (+ residual): one wavefront per row, the row in registers (C <= 1536: 6 float4 per lane) ------------------------------ //
constexpr int kLnVec = 6;

__global__ void __launch_bounds__(256) ln_res_kernel(const float* __restrict__ x, const float* res, const float* __restrict__ gamma,
                                                     const float* __restrict__ beta, float* out, long long rows, int C, float eps) {
    const long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    row_layer_norm<kLnVec>(RowContig{reinterpret_cast<const float4*>(x + r * C)}, gamma, beta, res ? res + r * C : nullptr, out + r * C, C, eps);
}

// ---- GroupNorm: statistics (one workgroup per group, float64 partial sums in a fixed order), apply + SiLU + residual --------------- //
constexpr int kGnThreads = 1024;

__global__ void __launch_bounds__(kGnThreads) gn_stats_kernel(const float* __restrict__ x, long long rows, int C, int cpg, float eps, float* stats) {
    __shared__ double red[2][kGnThreads];
    const int g = blockIdx.x, tid = threadIdx.x;
    const long long n = rows * cpg;
    double s = 0.0, q = 0.0;
    for (long long e = tid; e < n; e += kGnThreads) {
        const long long r = e / cpg;
        const int c = (int)(e - r * cpg);
        const double v = x[r * C + (long long)g * cpg + c];
        s += v;
        q += v * v;
    }
    red[0][tid] = s;
    red[1][tid] = q;
    __syncthreads();
    for (int w = kGnThreads / 2; w > 0; w >>= 1) {
        if (tid < w) {
            red[0][tid] += red[0][tid + w];
            red[1][tid] += red[1][tid + w];
        }
        __syncthreads();
    }
    if (tid == 0) {
        const double mean = red[0][0] / (double)n;
        const double var = fmax(red[1][0] / (double)n - mean * mean, 0.0);
        stats[2 * g] = (float)mean;
        stats[2 * g + 1] = (float)(1.0 / sqrt(var + (double)eps));
    }
}

__global__ void __launch_bounds__(256) gn_residual_kernel(const float* x, const float* __restrict__ a, const float* __restrict__ stats,
                                                          const float* __restrict__ gamma, const float* __restrict__ beta, float* out,
                                                          long long n4, int C, int cpg) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    const int c0 = (int)((4 * i) % C);
    const float4 av = reinterpret_cast<const float4*>(a)[i], xv = reinterpret_cast<const float4*>(x)[i];
    const float in[4] = {av.x, av.y, av.z, av.w}, xr[4] = {xv.x, xv.y, xv.z, xv.w};
    float o[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int c = c0 + r, g = c / cpg;
        o[r] = xr[r] + silu((in[r] - stats[2 * g]) * stats[2 * g + 1] * gamma[c] + beta[c]);
    }
    reinterpret_cast<float4*>(out)[i] = make_float4(o[0], o[1], o[2], o[3]);
}

// ---- window attention ---------------------------------------------------------------------------------------------------------- //
__device__ __forceinline__ int region(int i, int n, int win, int s) { return s == 0 ? 0 : (i < n - win ? 0 : (i < n - s ? 1 : 2)); }

struct FxAttn {
    static constexpr int HD = 64;
    const skfuxi_attn_desc& d;
    int head, wy, wx;                  // the window's place in the shifted grid
    int swm;                           // the longitude shift as the mask sees it (0: periodic, no mask)
    const float* cpb;                  // the head's (2 wh - 1) x (2 ww - 1) position-bias table
    long long tq;                      // the query: its token, window row / column and mask region
    int qr, qc, qreg;
    __device__ __forceinline__ FxAttn(const skfuxi_attn_desc& d_, int win, int head_)
        : d(d_), head(head_), wy(win / (d_.W / d_.ww)), wx(win - wy * (d_.W / d_.ww)), swm(d_.mask_lon ? d_.sw : 0),
          cpb(d_.cpb + (long long)head_ * (2 * d_.wh - 1) * (2 * d_.ww - 1)) {}
    // token of window-local (r, c): shifted-grid position, rolled back to the stored grid
    __device__ __forceinline__ long long token(int r, int c) const {
        int yo = wy * d.wh + r + d.sh, xo = wx * d.ww + c + d.sw;
        if (yo >= d.H) yo -= d.H;
        if (xo >= d.W) xo -= d.W;
        return (long long)yo * d.W + xo;
    }
    __device__ __forceinline__ int reg(int r, int c) const { return 3 * region(wy * d.wh + r, d.H, d.wh, d.sh) + region(wx * d.ww + c, d.W, d.ww, swm); }
    __device__ __forceinline__ void query(int i) {
        qr = i / d.ww;
        qc = i - qr * d.ww;
        tq = token(qr, qc);
        qreg = reg(qr, qc);
    }
    __device__ __forceinline__ const float* row(int i, int part) const {
        const int r = i / d.ww;
        return d.qkv + token(r, i - r * d.ww) * (3ll * d.C) + part * d.C + head * HD;
    }
    // |v| over the 64 values of a row that the four lanes (l15, 0..3) hold, floored at norm_eps
    __device__ __forceinline__ float norm(const float (&v)[2][8]) const {
        float ss = 0.f;
#pragma unroll
        for (int ch = 0; ch < 2; ++ch)
#pragma unroll
            for (int j = 0; j < 8; ++j) ss += v[ch][j] * v[ch][j];
        ss += __shfl_xor(ss, 16);
        ss += __shfl_xor(ss, 32);
        return fmaxf(sqrtf(ss), d.norm_eps);
    }
    __device__ __forceinline__ void scale(float (&v)[2][8], float f) const {
#pragma unroll
        for (int ch = 0; ch < 2; ++ch)
#pragma unroll
            for (int j = 0; j < 8; ++j) v[ch][j] *= f;
    }
    __device__ __forceinline__ void prep_q(float (&v)[2][8]) const { scale(v, expf(fminf(d.logit_scale[head], d.logit_max)) / norm(v)); }
    __device__ __forceinline__ void prep_k(float (&v)[2][8]) const { scale(v, 1.0f / norm(v)); }
    __device__ __forceinline__ float score(float s, int key) const {
        const int kr = key / d.ww, kc = key - kr * d.ww;
        float v = s + cpb[(qr - kr + d.wh - 1) * (2 * d.ww - 1) + (qc - kc + d.ww - 1)];
        if (reg(kr, kc) != qreg) v += d.mask_value;
        return v;
    }
    __device__ __forceinline__ float* out() const { return d.out + tq * d.C + head * HD; }
};

__global__ void __launch_bounds__(256) window_attn_kernel(const skfuxi_attn_desc d) {
    window_attn_body(FxAttn(d, blockIdx.x, blockIdx.y), d.wh * d.ww, blockIdx.z);
}

// ---- bilinear resample + de-normalisation ------------------------------------------------------------------------------------- //
__device__ __forceinline__ float src_coord(int o, int n_in, int n_out, int align) {
    if (align) return n_out > 1 ? (float)o * ((float)(n_in - 1) / (float)(n_out - 1)) : 0.f;
    const float s = ((float)o + 0.5f) * ((float)n_in / (float)n_out) - 0.5f;
    return s < 0.f ? 0.f : s;
}

__global__ void __launch_bounds__(256) resample_kernel(const skfuxi_resample_desc d) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long per = (long long)d.h_out * d.w_out;
    if (i >= per * d.channels) return;
    const int c = (int)(i / per);
    const int rem = (int)(i - c * per), y = rem / d.w_out, x = rem - y * d.w_out;
    const float sy = src_coord(y, d.h_src, d.h_out, d.align_corners), sx = src_coord(x, d.w_src, d.w_out, d.align_corners);
    const int y0 = (int)sy, x0 = (int)sx;
    const int y1 = y0 + 1 < d.h_src ? y0 + 1 : d.h_src - 1, x1 = x0 + 1 < d.w_src ? x0 + 1 : d.w_src - 1;
    const float ly = sy - (float)y0, lx = sx - (float)x0;
    const float* p = d.src + (long long)c * d.h_src * d.w_src;
    const float v = (1.f - ly) * ((1.f - lx) * p[(long long)y0 * d.w_src + x0] + lx * p[(long long)y0 * d.w_src + x1]) +
                    ly * ((1.f - lx) * p[(long long)y1 * d.w_src + x0] + lx * p[(long long)y1 * d.w_src + x1]);
    d.out[i] = v * d.std[c] + d.mean[c];
}

}  // namespace skp

using namespace skp;

extern "C" {

int skfuxi_abi_version(void) { return SKFUXI_ABI_VERSION; }

const char* skfuxi_error_string(int code) {
    switch (code) {
        case 0: return "success";
        case SKFUXI_E_ARG: return "invalid argument";
        case SKFUXI_E_HIP: return "HIP runtime error";
        case SKFUXI_E_WINDOW: return "the attention window does not tile the token grid";
        default: return "unknown error code";
    }
}

int skfuxi_prepare_weight(const float* src, long long sn, long long sk, int N, int K, void* dst, long long plane, int ldw, void* stream) {
    return prepare_weight_f16(src, sn, sk, N, K, dst, plane, ldw, stream, SKFUXI_E_ARG, SKFUXI_E_HIP);
}

int skfuxi_embed(const skfuxi_embed_desc* d, void* stream) {
    if (!d || !d->x0 || !d->x1 || !d->mean || !d->inv_std || !d->w || !d->bias || !d->tw || !d->tb || !d->tvec || !d->out || d->channels <= 0 ||
        d->C <= 0 || (d->C & 3) || d->n_lat < 4 || d->n_lon < 4 || (d->n_lon & 3) || !aligned16(d->x0) || !aligned16(d->x1) || !aligned16(d->out))
        return SKFUXI_E_ARG;
    const int K = 32 * d->channels, wt = d->n_lon / 4, M = (d->n_lat / 4) * wt;
    if (d->ldw < K || (d->ldw & 7) || d->w_plane < (long long)d->C * d->ldw || (long long)M * d->C >= (1ll << 31)) return SKFUXI_E_ARG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(time_vec_kernel, dim3((unsigned)((d->C + 255) / 256)), dim3(256), 0, s, d->tw, d->tb, *d);
    if (hipGetLastError() != hipSuccess) return SKFUXI_E_HIP;
    const ALEmbed al{d->x0, d->x1, d->mean, d->inv_std, M, K, wt, d->n_lon, (long long)d->n_lat * d->n_lon};
    const EpFuxi ep{d->out, d->bias, d->tvec, EP_STORE, 0, d->C, 0, 0, 0};
    return run_gemm<TFx>(al, ep, d->w, d->w_plane, d->ldw, M, d->C, K, s) == hipSuccess ? 0 : SKFUXI_E_HIP;
}

int skfuxi_layer_norm(const float* x, const float* res, const float* gamma, const float* beta, float* out, long long rows, int C, float eps, void* stream) {
    if (!x || !gamma || !beta || !out || rows <= 0 || C <= 0 || (C & 3) || C > 4 * 64 * kLnVec || !aligned16(x) || !aligned16(out) ||
        (res && !aligned16(res)))
        return SKFUXI_E_ARG;
    hipLaunchKernelGGL(ln_res_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, static_cast<hipStream_t>(stream), x, res, gamma, beta, out, rows, C, eps);
    return hip_status(SKFUXI_E_HIP);
}

int skfuxi_conv(const skfuxi_conv_desc* d, void* stream) {
    if (!d || !d->src0 || !d->w || !d->bias || !d->out || d->c0 <= 0 || (d->c0 & 7) || d->c1 < 0 || (d->c1 & 7) || (d->c1 > 0 && !d->src1) ||
        (d->taps != 9 && d->taps != 1) || (d->stride != 1 && d->stride != 2) || (d->taps == 1 && d->stride != 1) || d->h_in <= 0 || d->w_in <= 0 ||
        d->h_out <= 0 || d->w_out <= 0 || d->cout <= 0 || (d->cout & 3) || d->shuffle < 0 || d->shuffle > 1 || !aligned16(d->src0) ||
        !aligned16(d->src1) || !aligned16(d->out))
        return SKFUXI_E_ARG;
    if (d->taps == 9 && ((d->h_out - 1) * d->stride > d->h_in || (d->w_out - 1) * d->stride > d->w_in)) return SKFUXI_E_ARG;
    if (d->taps == 1 && (d->h_out != d->h_in || d->w_out != d->w_in)) return SKFUXI_E_ARG;
    if (d->gn_stats && (!d->gn_gamma || !d->gn_beta || d->groups <= 0 || d->c0 % d->groups)) return SKFUXI_E_ARG;
    const int cin = d->c0 + d->c1, K = d->taps * cin, M = d->h_out * d->w_out, N = d->shuffle ? 4 * d->cout : d->cout;
    if (d->ldw < K || (d->ldw & 7) || d->w_plane < (long long)N * d->ldw || (long long)d->h_in * d->w_in * cin >= (1ll << 31) ||
        (long long)M * N >= (1ll << 31))
        return SKFUXI_E_ARG;
    const ALConv al{d->src0, d->src1, d->gn_stats, d->gn_gamma, d->gn_beta, M, K, d->h_in, d->w_in, d->w_out, d->c0, d->c1, cin, d->taps,
                    d->stride, d->gn_stats ? d->c0 / d->groups : 1};
    const EpFuxi ep{d->out, d->bias, nullptr, d->shuffle ? EP_SHUFFLE : EP_STORE, 0, d->cout, d->w_out, 0, 0};
    return run_gemm<TFx>(al, ep, d->w, d->w_plane, d->ldw, M, N, K, static_cast<hipStream_t>(stream)) == hipSuccess ? 0 : SKFUXI_E_HIP;
}

int skfuxi_gn_stats(const float* x, long long rows, int C, int groups, float eps, float* stats, void* stream) {
    if (!x || !stats || rows <= 0 || C <= 0 || groups <= 0 || C % groups || groups > 65535) return SKFUXI_E_ARG;
    hipLaunchKernelGGL(gn_stats_kernel, dim3(groups), dim3(kGnThreads), 0, static_cast<hipStream_t>(stream), x, rows, C, C / groups, eps, stats);
    return hip_status(SKFUXI_E_HIP);
}

int skfuxi_gn_residual(const float* x, const float* a, const float* stats, const float* gamma, const float* beta, float* out, long long rows,
                       int C, int groups, void* stream) {
    if (!x || !a || !stats || !gamma || !beta || !out || rows <= 0 || C <= 0 || (C & 3) || groups <= 0 || C % groups || !aligned16(x) ||
        !aligned16(a) || !aligned16(out))
        return SKFUXI_E_ARG;
    const long long n4 = rows * C / 4;
    hipLaunchKernelGGL(gn_residual_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), x, a, stats, gamma,
                       beta, out, n4, C, C / groups);
    return hip_status(SKFUXI_E_HIP);
}

int skfuxi_linear(const skfuxi_linear_desc* d, void* stream) {
    if (!d || !d->a || !d->w || !d->bias || !d->out || d->M <= 0 || d->N <= 0 || d->K <= 0 || (d->K & 7) || d->act < 0 || d->act > 1 ||
        d->mode < 0 || d->mode > 1 || d->ldw < d->K || (d->ldw & 7) || d->w_plane < (long long)d->N * d->ldw || (long long)d->M * d->K >= (1ll << 30) ||
        !aligned16(d->a) || !aligned16(d->out))
        return SKFUXI_E_ARG;
    if (d->mode == 0 && ((d->N & 3) || (long long)d->M * d->N >= (1ll << 31))) return SKFUXI_E_ARG;
    const int P = d->patch;
    if (d->mode == 1 && (P <= 0 || d->w_tok <= 0 || d->M % d->w_tok || d->N % (P * P) || d->act)) return SKFUXI_E_ARG;
    const ALFast<true> al{d->a, d->M, d->K, 1 << 30, d->K, 0, 1};
    EpFuxi ep{d->out, d->bias, nullptr, d->mode ? EP_HEAD : EP_STORE, d->act, d->N, d->w_tok, P, 0};
    if (d->mode == 1) ep.hw = (long long)(P * (d->M / d->w_tok)) * (P * d->w_tok);
    return run_gemm<TFx>(al, ep, d->w, d->w_plane, d->ldw, d->M, d->N, d->K, static_cast<hipStream_t>(stream)) == hipSuccess ? 0 : SKFUXI_E_HIP;
}

int skfuxi_window_attention(const skfuxi_attn_desc* d, void* stream) {
    if (!d || !d->qkv || !d->out || !d->cpb || !d->logit_scale || d->heads <= 0 || d->C != 64 * d->heads || d->H <= 0 || d->W <= 0 ||
        d->wh < 2 || d->ww < 2 || !aligned16(d->qkv) || !aligned16(d->out) || (long long)d->H * d->W * 3 * d->C >= (1ll << 31))
        return SKFUXI_E_ARG;
    if (d->H % d->wh || d->W % d->ww) return SKFUXI_E_WINDOW;
    if (d->sh < 0 || d->sh >= d->wh || d->sw < 0 || d->sw >= d->ww) return SKFUXI_E_ARG;
    const int nwin = (d->H / d->wh) * (d->W / d->ww), N = d->wh * d->ww;
    if (d->heads > 65535 || (N + 63) / 64 > 65535) return SKFUXI_E_ARG;
    hipLaunchKernelGGL(window_attn_kernel, dim3(nwin, d->heads, (N + 63) / 64), dim3(256), 0, static_cast<hipStream_t>(stream), *d);
    return hip_status(SKFUXI_E_HIP);
}

int skfuxi_resample(const skfuxi_resample_desc* d, void* stream) {
    if (!d || !d->src || !d->mean || !d->std || !d->out || d->channels <= 0 || d->h_src <= 0 || d->w_src <= 0 || d->h_out <= 0 || d->w_out <= 0 ||
        d->align_corners < 0 || d->align_corners > 1)
        return SKFUXI_E_ARG;
    const long long total = (long long)d->channels * d->h_out * d->w_out;
    hipLaunchKernelGGL(resample_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), *d);
    return hip_status(SKFUXI_E_HIP);
}

}  // extern "C"
