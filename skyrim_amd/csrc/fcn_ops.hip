// FourCastNet v1 (AFNO) step behind include/skyrim_fcn.h.
//
//   patch embedding   gemm.h's pipeline with a loader that gathers the 8 x 8 patch of a token straight from the raw (C, H, W)
//                     state (input normalisation as a per-k affine before the fp16 split) and EpStrided's bias + pos_embed epilogue
//   spectral filter   LayerNorm1, then four DFT GEMMs against prepared matrices (strided_gemm.h) around the block-diagonal
//                     complex MLP (fcn_mlp_kernel, SPEC mode); the inverse longitude DFT's epilogue adds u and the block input
//   token MLP         LayerNorm2 -> fc1 -> GELU -> fc2 -> + residual as ONE kernel (fcn_mlp_kernel, TOKEN mode)
//   head              gemm.h's pipeline, an epilogue that scatters the (p1, p2, c) columns of a token into the (C, H, W) output
//
// fcn_mlp_kernel: a wavefront owns 16 rows for the whole kernel.  Their input vectors live in registers as MFMA B-operand fragments
// (fp16 hi/lo, 3 MFMA terms, fp32 accumulation); the hidden layer is walked in chunks of 32 units whose accumulators, after bias +
// activation + hi/lo split, ARE the B-operand fragments of the second layer (the k order of the second layer's weights is permuted at
// prepare time to match, sfno_chain.hip).  Weights are read in fragment order straight from global memory (L2), 1 KiB per wave and
// fragment, through a ring of in-flight loads that runs across the two layers and across chunks.  gfx950 only.
#include <hip/hip_runtime.h>

#include "../../include/skyrim_fcn.h"
#include "rownorm.h"
#include "strided_gemm.h"

namespace skp {

typedef TileCfg<128, 128, 32, 2, 4> TF;     // 8 waves, 64 x 32 wave tiles: the tile of the strided GEMMs here

// ---- patch loader: token m = (hh, ww), k = (c, p1, p2) ------------------------------------------------------------------------ //
struct ALPatch {
    static constexpr bool kDirect = false;
    const float* x;
    int M, K, wt, P, wimg;
    long long hw;
    const float* kscale;
    const float* kshift;
    struct Row { long long off; int ok; };
    struct Raw { float v[8]; int k; };
    __device__ __forceinline__ Row row(int m) const {
        if (m >= M) return Row{0, 0};
        const int hh = m / wt, ww = m - hh * wt;
        return Row{(long long)hh * P * wimg + (long long)ww * P, 1};
    }
    __device__ __forceinline__ void issue(const Row& r, int k, Raw& o) const {
#pragma unroll
        for (int i = 0; i < 8; ++i) o.v[i] = 0.f;
        o.k = -1;
        if (!r.ok || k >= K) return;
        o.k = k;
        const int pp = P * P;
        if (P == 8 && k + 8 <= K) {                   // one patch row: 8 consecutive pixels
            const int c = k / pp, p1 = (k - c * pp) >> 3;
            const float* p = x + r.off + c * hw + (long long)p1 * wimg;
#pragma unroll
            for (int i = 0; i < 8; ++i) o.v[i] = p[i];
        } else {
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int kk = k + i;
                if (kk < K) {
                    const int c = kk / pp, rem = kk - c * pp, p1 = rem / P, p2 = rem - p1 * P;
                    o.v[i] = x[r.off + c * hw + (long long)p1 * wimg + p2];
                }
            }
        }
    }
    __device__ __forceinline__ void finish(const Raw& r, float (&v)[8]) const {
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = (r.k >= 0 && r.k + i < K) ? r.v[i] * kscale[r.k + i] + kshift[r.k + i] : 0.f;
    }
    __device__ __forceinline__ uint4 direct(const Raw&) const { return make_uint4(0, 0, 0, 0); }
};

// ---- head epilogue: + bias, scatter column n = (p1 P + p2) cout + c of token m = (hh, ww) to out[c][hh P + p1][ww P + p2] ---- //
struct EpHead {
    static constexpr bool kDualOrder = false;
    template <class TC> __device__ __forceinline__ void init(char*, int, int) const {}
    float* out;
    const float* bias;
    int cout, wt, P, wimg;
    long long hw;
    template <class TC, bool SWAP>
    __device__ __forceinline__ void run(f32x4 (&acc)[TC::FM][TC::FN], int m0w, int n0w, int lane, int, int, char*, int M, int N, int) const {
        static_assert(SWAP, "swapped order: a lane holds 4 consecutive columns of one token");
        const int l15 = lane & 15, l4 = (lane >> 4) * 4;
#pragma unroll
        for (int a = 0; a < TC::FM; ++a) {
            const int m = m0w + a * 16 + l15;
            if (m >= M) continue;
            const int hh = m / wt, ww = m - hh * wt;
            const long long base = (long long)hh * P * wimg + (long long)ww * P;
#pragma unroll
            for (int b = 0; b < TC::FN; ++b)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int n = n0w + b * 16 + l4 + r;
                    if (n >= N) continue;
                    const int pp = n / cout, c = n - pp * cout, p1 = pp / P, p2 = pp - p1 * P;
                    out[c * hw + base + (long long)p1 * wimg + p2] = acc[a][b][r] + bias[n];
                }
        }
    }
};

// strided GEMM out = A W^T (+ bias, residuals) with two-level row addressing for A and out (strided_gemm.h)
hipError_t dft_gemm(const float* a, int a_m1, long long a_sm, long long a_sm2, long long a_sk, const void* w, long long w_plane, int ldw,
                    float* out, int o_m1, long long o_sm, long long o_sm2, long long o_sn, const float* res_pre, const float* res_post,
                    int M, int N, int K, hipStream_t s) {
    const ALStrided al{a, M, K, a_m1, a_sm, a_sm2, a_sk, nullptr, nullptr, nullptr, 0, 0};
    const EpStrided ep{out, nullptr, res_pre, res_post, o_m1, 0, o_sm, o_sm2, o_sn};
    return run_gemm<TF>(al, ep, w, w_plane, ldw, M, N, K, s);
}

// ---- LayerNorm over the channels of a row: one wavefront per row, two passes in registers (C <= 1024: 4 float4 per lane) ---- //
__global__ void __launch_bounds__(256) layer_norm_kernel(const float* __restrict__ x, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                         float* __restrict__ out, long long rows, int C, float eps) {
    const long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    row_layer_norm<4>(RowContig{reinterpret_cast<const float4*>(x + r * C)}, gamma, beta, nullptr, out + r * C, C, eps);
}

// ---- the fused two-layer MLP ----------------------------------------------------------------------------------------------------- //
enum { MLP_TOKEN = 0, MLP_SPEC = 1 };

struct MlpArgs {
    const float* x;          // TOKEN: [rows][K];  SPEC: the spectrum (two-level rows, re / im halves)
    float* out;
    long long rows, sm, sm2, im_off;
    int m1, nch;             // nch: hidden chunks of 32
    const f16* w1f;
    const f16* w2f;
    const float* b1;
    const float* b2;
    const float* gamma;
    const float* beta;
    float eps, lambda;
};

typedef OpT<f16>::v8 v8;

// K inputs, N outputs per row; the grid's y index selects the spectral block (SPEC).  D: depth of the ring of weight-fragment loads.
template <int MODE, int K, int N, int NWAVES, int D>
__global__ void __launch_bounds__(64 * NWAVES) __attribute__((amdgpu_waves_per_eu(1, 1))) fcn_mlp_kernel(const MlpArgs a) {
    constexpr int KS = K / 32, CF = N / 16, NS1 = 2 * KS, PER = NS1 + CF, HALF = K / 2;
    static_assert(PER % D == 0, "the ring's slots repeat from chunk to chunk");
    const int lane = threadIdx.x & 63, l15 = lane & 15, g = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long long r0 = ((long long)blockIdx.x * NWAVES + wave) * 16;
    if (r0 >= a.rows) return;                              // no barriers in this kernel
    const long long row = r0 + l15 < a.rows ? r0 + l15 : a.rows - 1;
    const int blk = blockIdx.y;
    long long base;
    if constexpr (MODE == MLP_TOKEN) base = row * K;
    else base = (row / a.m1) * a.sm2 + (row % a.m1) * a.sm + (long long)blk * HALF;
    const float* xr = a.x + base;
    auto col = [&](int k) -> long long {                    // element k of the row's input / output vector
        if constexpr (MODE == MLP_TOKEN) return k;
        else return k < HALF ? k : a.im_off + (k - HALF);
    };

    // ---- input fragments: lane (l15, g) holds channels 32 ks + 8 g + [0..7] of row l15 ----
    v8 xh[KS], xl[KS];
    {
        float mean = 0.f, rstd = 1.f;
        if constexpr (MODE == MLP_TOKEN) {
            float s = 0.f;
            for (int ks = 0; ks < KS; ++ks) {
                const float4 p = *reinterpret_cast<const float4*>(xr + 32 * ks + 8 * g), q = *reinterpret_cast<const float4*>(xr + 32 * ks + 8 * g + 4);
                s += ((p.x + p.y) + (p.z + p.w)) + ((q.x + q.y) + (q.z + q.w));
            }
            s += __shfl_xor(s, 16);
            s += __shfl_xor(s, 32);
            mean = s / (float)K;
            float v = 0.f;
            for (int ks = 0; ks < KS; ++ks) {
                const float4 p = *reinterpret_cast<const float4*>(xr + 32 * ks + 8 * g), q = *reinterpret_cast<const float4*>(xr + 32 * ks + 8 * g + 4);
                const float e[8] = {p.x - mean, p.y - mean, p.z - mean, p.w - mean, q.x - mean, q.y - mean, q.z - mean, q.w - mean};
#pragma unroll
                for (int i = 0; i < 8; ++i) v += e[i] * e[i];
            }
            v += __shfl_xor(v, 16);
            v += __shfl_xor(v, 32);
            rstd = rsqrtf(v / (float)K + a.eps);
        }
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const int k0 = 32 * ks + 8 * g;
            const float* p = xr + col(k0);
            const float4 p0 = *reinterpret_cast<const float4*>(p), p1 = *reinterpret_cast<const float4*>(p + 4);
            float v[8] = {p0.x, p0.y, p0.z, p0.w, p1.x, p1.y, p1.z, p1.w};
            if constexpr (MODE == MLP_TOKEN) {
                const float4 g0 = *reinterpret_cast<const float4*>(a.gamma + k0), g1 = *reinterpret_cast<const float4*>(a.gamma + k0 + 4);
                const float4 b0 = *reinterpret_cast<const float4*>(a.beta + k0), b1 = *reinterpret_cast<const float4*>(a.beta + k0 + 4);
                const float gm[8] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w}, bt[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
#pragma unroll
                for (int i = 0; i < 8; ++i) v[i] = (v[i] - mean) * rstd * gm[i] + bt[i];
            }
            uint4 o[2];
            split8<f16, 2>(v, o);
            xh[ks] = as_v8<f16>(o[0]);
            xl[ks] = as_v8<f16>(o[1]);
        }
    }

    f32x4 yacc[CF];
#pragma unroll
    for (int c = 0; c < CF; ++c) yacc[c] = f32x4{0.f, 0.f, 0.f, 0.f};

    // fragment s of chunk j: s < NS1 -> W1 fragment (16-unit row block 2 j + (s & 1), k block s >> 1); else W2 fragment (output block s - NS1)
    const int H = a.nch * 32;
    const f16* w1 = a.w1f + (long long)blk * 2 * H * K + lane * 8;
    const f16* w2 = a.w2f + (long long)blk * 2 * N * H + lane * 8;
    const float* b1 = a.b1 + (long long)blk * H;
    auto frag = [&](int j, int s) -> const f16* {
        if (s < NS1) return w1 + ((((long long)(2 * j + (s & 1)) * KS + (s >> 1)) * 2) << 9);
        return w2 + ((((long long)j * CF + (s - NS1)) * 2) << 9);
    };
    uint4 ring[D][2];
    auto fetch = [&](const f16* p, uint4 (&dst)[2]) {
        dst[0] = *reinterpret_cast<const uint4*>(p);
        dst[1] = *reinterpret_cast<const uint4*>(p + 512);
    };
#pragma unroll
    for (int d = 0; d < D; ++d) fetch(frag(0, d), ring[d]);

    for (int j = 0; j < a.nch; ++j) {
        const int jn = j + 1 < a.nch ? j + 1 : j;          // the ring runs into the next chunk (the last chunk re-reads itself)
        f32x4 hacc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
        for (int s = 0; s < NS1; ++s) {
            const uint4 wh = ring[s % D][0], wl = ring[s % D][1];
            fetch(s + D < PER ? frag(j, s + D) : frag(jn, s + D - PER), ring[s % D]);
            const int ks = s >> 1, n = s & 1;
            hacc[n] = OpT<f16>::mfma(as_v8<f16>(wl), xh[ks], hacc[n]);
            hacc[n] = OpT<f16>::mfma(as_v8<f16>(wh), xl[ks], hacc[n]);
            hacc[n] = OpT<f16>::mfma(as_v8<f16>(wh), xh[ks], hacc[n]);
        }
        // bias + activation + split: the lane's hidden units 16 n + 4 g + r are k-slots 4 n + r of the second layer's fragment
        uint4 hh, hl;
        {
            const float4 c0 = *reinterpret_cast<const float4*>(b1 + 32 * j + 4 * g), c1 = *reinterpret_cast<const float4*>(b1 + 32 * j + 16 + 4 * g);
            float v[8] = {hacc[0][0] + c0.x, hacc[0][1] + c0.y, hacc[0][2] + c0.z, hacc[0][3] + c0.w,
                          hacc[1][0] + c1.x, hacc[1][1] + c1.y, hacc[1][2] + c1.z, hacc[1][3] + c1.w};
            if constexpr (MODE == MLP_TOKEN) {
#pragma unroll
                for (int i = 0; i < 8; i += 2) {
                    const f32x2 t = gelu_erf2(f32x2{v[i], v[i + 1]});
                    v[i] = t.x; v[i + 1] = t.y;
                }
            } else {
#pragma unroll
                for (int i = 0; i < 8; ++i) v[i] = fmaxf(v[i], 0.f);
            }
            uint4 o[2];
            split8<f16, 2>(v, o);
            hh = o[0]; hl = o[1];
        }
#pragma unroll
        for (int s = NS1; s < PER; ++s) {
            const uint4 wh = ring[s % D][0], wl = ring[s % D][1];
            fetch(s + D < PER ? frag(j, s + D) : frag(jn, s + D - PER), ring[s % D]);
            const int c = s - NS1;
            yacc[c] = OpT<f16>::mfma(as_v8<f16>(wl), as_v8<f16>(hh), yacc[c]);
            yacc[c] = OpT<f16>::mfma(as_v8<f16>(wh), as_v8<f16>(hl), yacc[c]);
            yacc[c] = OpT<f16>::mfma(as_v8<f16>(wh), as_v8<f16>(hh), yacc[c]);
        }
    }

    // ---- epilogue: yacc[c][r] is output 16 c + 4 g + r of row l15.  Loads before stores. ----
    const bool live = r0 + l15 < a.rows;
    const float* b2 = a.b2 + (long long)blk * N;
    float* orow = a.out + base;
    if constexpr (MODE == MLP_TOKEN) {
        if (!live) return;
        constexpr int G = CF % 12 == 0 ? 12 : CF;           // residual loads in groups, each before its group's stores
#pragma unroll
        for (int c0 = 0; c0 < CF; c0 += G) {
            float4 res[G], bb[G];
#pragma unroll
            for (int c = 0; c < G; ++c) {
                res[c] = *reinterpret_cast<const float4*>(xr + 16 * (c0 + c) + 4 * g);
                bb[c] = *reinterpret_cast<const float4*>(b2 + 16 * (c0 + c) + 4 * g);
            }
#pragma unroll
            for (int c = 0; c < G; ++c) {
                const f32x4 y = yacc[c0 + c];
                *reinterpret_cast<float4*>(orow + 16 * (c0 + c) + 4 * g) =
                    make_float4(y[0] + bb[c].x + res[c].x, y[1] + bb[c].y + res[c].y, y[2] + bb[c].z + res[c].z, y[3] + bb[c].w + res[c].w);
            }
        }
    } else {
        if (!live) return;
        const float lam = a.lambda;
#pragma unroll
        for (int c = 0; c < CF; ++c) {
            const float4 bb = *reinterpret_cast<const float4*>(b2 + 16 * c + 4 * g);
            float v[4] = {yacc[c][0] + bb.x, yacc[c][1] + bb.y, yacc[c][2] + bb.z, yacc[c][3] + bb.w};
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i] = v[i] > lam ? v[i] - lam : (v[i] < -lam ? v[i] + lam : 0.f);
            *reinterpret_cast<float4*>(orow + col(16 * c + 4 * g)) = make_float4(v[0], v[1], v[2], v[3]);
        }
    }
}

template <int MODE, int K, int N, int D>
hipError_t launch_mlp(const MlpArgs& a, int blocks_y, hipStream_t s) {
    constexpr int NWAVES = 4;
    const unsigned gx = (unsigned)((a.rows + 16 * NWAVES - 1) / (16 * NWAVES));
    hipLaunchKernelGGL((fcn_mlp_kernel<MODE, K, N, NWAVES, D>), dim3(gx, blocks_y), dim3(64 * NWAVES), 0, s, a);
    return hipGetLastError();
}

// ---- prepare: w1 [H][K] -> w1f[((j16 KS + ks) 2 + plane)][lane][e] = W1[16 j16 + (lane & 15)][32 ks + 8 (lane >> 4) + e];
//               w2 [N][H] -> w2f[((j CF + c) 2 + plane)][lane][e] = W2[16 c + (lane & 15)][32 j + 16 (e >> 2) + 4 (lane >> 4) + (e & 3)] ---- //
__global__ void prep_mlp_w1_kernel(const float* __restrict__ w1, f16* __restrict__ out, int H, int K, long long total) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int KS = K / 32;
    const int e = (int)(i & 7), lane = (int)((i >> 3) & 63);
    long long q = i >> 9;
    const int ks = (int)(q % KS);
    q /= KS;
    const int j16 = (int)(q % (H / 16));
    const long long b = q / (H / 16);
    const float v = w1[b * H * K + (long long)(16 * j16 + (lane & 15)) * K + 32 * ks + 8 * (lane >> 4) + e];
    const f16 h = (f16)v;
    const long long o = b * 2 * H * K + ((((long long)j16 * KS + ks) * 2) << 9) + lane * 8 + e;
    out[o] = h;
    out[o + 512] = (f16)(v - (float)h);
}

__global__ void prep_mlp_w2_kernel(const float* __restrict__ w2, f16* __restrict__ out, int N, int H, long long total) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int CF = N / 16;
    const int e = (int)(i & 7), lane = (int)((i >> 3) & 63);
    long long q = i >> 9;
    const int c = (int)(q % CF);
    q /= CF;
    const int j = (int)(q % (H / 32));
    const long long b = q / (H / 32);
    const int hid = 32 * j + 16 * (e >> 2) + 4 * (lane >> 4) + (e & 3);
    const float v = w2[b * N * H + (long long)(16 * c + (lane & 15)) * H + hid];
    const f16 h = (f16)v;
    const long long o = b * 2 * N * H + ((((long long)j * CF + c) * 2) << 9) + lane * 8 + e;
    out[o] = h;
    out[o + 512] = (f16)(v - (float)h);
}

bool spec_args_ok(const skfcn_spectral_mlp_desc* d) {
    return d && d->z && d->w1f && d->w2f && d->b1e && d->b2e && d->rows > 0 && d->m1 > 0 && d->nblocks > 0 && d->nblocks <= 65535 &&
           d->sm >= 0 && d->sm2 >= 0 && d->im_off > 0 && !(d->sm & 3) && !(d->sm2 & 3) && !(d->im_off & 3) && d->lambda >= 0.f;
}

hipError_t spectral_mlp(const skfcn_spectral_mlp_desc* d, hipStream_t s) {
    MlpArgs a{};
    a.x = d->z; a.out = d->z;
    a.rows = d->rows; a.sm = d->sm; a.sm2 = d->sm2; a.im_off = d->im_off; a.m1 = d->m1;
    a.nch = 192 / 32;
    a.w1f = static_cast<const f16*>(d->w1f); a.w2f = static_cast<const f16*>(d->w2f);
    a.b1 = d->b1e; a.b2 = d->b2e; a.lambda = d->lambda;
    return launch_mlp<MLP_SPEC, 192, 192, 8>(a, d->nblocks, s);
}

}  // namespace skp

using namespace skp;

extern "C" {

int skfcn_abi_version(void) { return SKFCN_ABI_VERSION; }

const char* skfcn_error_string(int code) {
    switch (code) {
        case 0: return "success";
        case SKFCN_E_ARG: return "invalid argument";
        case SKFCN_E_HIP: return "HIP runtime error";
        default: return "unknown error code";
    }
}

int skfcn_prepare_weight(const float* src, long long sn, long long sk, int N, int K, void* dst, long long plane, int ldw, void* stream) {
    return prepare_weight_f16(src, sn, sk, N, K, dst, plane, ldw, stream, SKFCN_E_ARG, SKFCN_E_HIP);
}

int skfcn_prepare_mlp_weights(const float* w1, const float* w2, int K, int H, int N, int batch, void* w1f, void* w2f, void* stream) {
    if (!w1 || !w2 || !w1f || !w2f || K <= 0 || H <= 0 || N <= 0 || batch <= 0 || (K & 31) || (H & 31) || (N & 31)) return SKFCN_E_ARG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const long long t1 = (long long)batch * H * K, t2 = (long long)batch * N * H;
    hipLaunchKernelGGL(prep_mlp_w1_kernel, dim3((unsigned)((t1 + 255) / 256)), dim3(256), 0, s, w1, static_cast<f16*>(w1f), H, K, t1);
    hipLaunchKernelGGL(prep_mlp_w2_kernel, dim3((unsigned)((t2 + 255) / 256)), dim3(256), 0, s, w2, static_cast<f16*>(w2f), N, H, t2);
    return hip_status(SKFCN_E_HIP);
}

int skfcn_patch_embed(const skfcn_patch_embed_desc* d, void* stream) {
    if (!d || !d->x || !d->kscale || !d->kshift || !d->w || !d->bias || !d->pos || !d->out || d->cin <= 0 || d->patch <= 0 || d->embed <= 0 ||
        d->himg < d->patch || d->wimg < d->patch || d->himg % d->patch || d->wimg % d->patch)
        return SKFCN_E_ARG;
    const int K = d->cin * d->patch * d->patch;
    if ((K & 7) || d->ldw < K || (d->ldw & 7) || d->w_plane < (long long)d->embed * d->ldw) return SKFCN_E_ARG;
    const int wt = d->wimg / d->patch, M = (d->himg / d->patch) * wt;
    const ALPatch al{d->x, M, K, wt, d->patch, d->wimg, (long long)d->himg * d->wimg, d->kscale, d->kshift};
    const EpStrided ep{d->out, d->bias, nullptr, d->pos, 1 << 30, 0, d->embed, 0, 1};
    const hipError_t e = run_gemm<TF>(al, ep, d->w, d->w_plane, d->ldw, M, d->embed, K, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? 0 : SKFCN_E_HIP;
}

int skfcn_layer_norm(const float* x, const float* gamma, const float* beta, float* out, long long rows, int C, float eps, void* stream) {
    if (!x || !gamma || !beta || !out || rows <= 0 || C <= 0 || (C & 3) || C > 1024) return SKFCN_E_ARG;
    hipLaunchKernelGGL(layer_norm_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, static_cast<hipStream_t>(stream), x, gamma, beta, out, rows, C, eps);
    return hip_status(SKFCN_E_HIP);
}

int skfcn_spectral_mlp(const skfcn_spectral_mlp_desc* d, void* stream) {
    if (!spec_args_ok(d)) return SKFCN_E_ARG;
    return spectral_mlp(d, static_cast<hipStream_t>(stream)) == hipSuccess ? 0 : SKFCN_E_HIP;
}

int skfcn_spectral_run(const skfcn_spectral_desc* d, void* stream) {
    if (!d || !d->t || !d->u || !d->s0 || !d->s1 || !d->gamma || !d->beta || !d->fw || !d->fl || !d->il || !d->iw || d->h <= 0 || d->w <= 0 ||
        d->C <= 0 || (d->C & 3) || d->C > 1024 || d->nblocks <= 0 || d->C != 96 * d->nblocks || d->km <= 0 || d->km > d->w / 2 + 1)
        return SKFCN_E_ARG;
    const int h = d->h, w = d->w, C = d->C, km = d->km;
    if (d->fw_ld < w || d->fl_ld < 2 * h || d->il_ld < 2 * h || d->iw_ld < 2 * km || ((d->fw_ld | d->fl_ld | d->il_ld | d->iw_ld) & 7) ||
        d->fw_plane < 2ll * km * d->fw_ld || d->fl_plane < 2ll * h * d->fl_ld || d->il_plane < 2ll * h * d->il_ld || d->iw_plane < (long long)w * d->iw_ld)
        return SKFCN_E_ARG;
    const long long T = (long long)h * w, KC = (long long)km * C, BIG = 1 << 30;
    if (T * C >= (1ll << 31) || (long long)h * C >= (1ll << 31)) return SKFCN_E_ARG;
    const skfcn_spectral_mlp_desc sm{d->s1, (long long)h * km, C, 2 * KC, KC, km, d->nblocks, d->w1f, d->w2f, d->b1e, d->b2e, d->lambda};
    if (!spec_args_ok(&sm)) return SKFCN_E_ARG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    int rc = skfcn_layer_norm(d->t, d->gamma, d->beta, d->u, T, C, d->eps, stream);
    if (rc) return rc;
    // longitude R2C:  s0[h][ri][m][c] = sum_w u[h][w][c] fw[ri km + m][w]
    if (dft_gemm(d->u, C, 1, (long long)w * C, C, d->fw, d->fw_plane, d->fw_ld, d->s0, C, 1, 2 * KC, C, nullptr, nullptr, h * C, 2 * km, w, s) != hipSuccess)
        return SKFCN_E_HIP;
    // latitude forward:  s1[kk][ri'][m][c] = sum_{h, ri} s0[h][ri][m][c] fl[2 kk + ri'][2 h + ri]
    if (dft_gemm(d->s0, (int)BIG, 1, 0, KC, d->fl, d->fl_plane, d->fl_ld, d->s1, (int)BIG, 1, 0, KC, nullptr, nullptr, (int)KC, 2 * h, 2 * h, s) != hipSuccess)
        return SKFCN_E_HIP;
    if (spectral_mlp(&sm, s) != hipSuccess) return SKFCN_E_HIP;
    // latitude inverse:  s0[h][ri][m][c] = sum_{kk, ri'} s1[kk][ri'][m][c] il[2 h + ri][2 kk + ri']
    if (dft_gemm(d->s1, (int)BIG, 1, 0, KC, d->il, d->il_plane, d->il_ld, d->s0, (int)BIG, 1, 0, KC, nullptr, nullptr, (int)KC, 2 * h, 2 * h, s) != hipSuccess)
        return SKFCN_E_HIP;
    // longitude C2R + u + t:  t[h][w][c] += u[h][w][c] + sum_{ri, m} s0[h][ri][m][c] iw[w][ri km + m]
    if (dft_gemm(d->s0, C, 1, 2 * KC, C, d->iw, d->iw_plane, d->iw_ld, d->t, C, 1, (long long)w * C, C, d->u, d->t, h * C, w, 2 * km, s) != hipSuccess)
        return SKFCN_E_HIP;
    return 0;
}

int skfcn_mlp_run(const skfcn_mlp_desc* d, void* stream) {
    if (!d || !d->x || !d->out || d->x == d->out || !d->gamma || !d->beta || !d->w1f || !d->w2f || !d->b1 || !d->b2 || d->rows <= 0 ||
        (d->C != 192 && d->C != 768) || d->hidden <= 0 || (d->hidden & 31) || d->rows * d->C >= (1ll << 31))
        return SKFCN_E_ARG;
    MlpArgs a{};
    a.x = d->x; a.out = d->out; a.rows = d->rows; a.m1 = 1;
    a.nch = d->hidden / 32;
    a.w1f = static_cast<const f16*>(d->w1f); a.w2f = static_cast<const f16*>(d->w2f);
    a.b1 = d->b1; a.b2 = d->b2; a.gamma = d->gamma; a.beta = d->beta; a.eps = d->eps;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const hipError_t e = d->C == 768 ? launch_mlp<MLP_TOKEN, 768, 768, 4>(a, 1, s) : launch_mlp<MLP_TOKEN, 192, 192, 8>(a, 1, s);
    return e == hipSuccess ? 0 : SKFCN_E_HIP;
}

int skfcn_head_run(const skfcn_head_desc* d, void* stream) {
    if (!d || !d->t || !d->w || !d->bias || !d->out || d->cout <= 0 || d->patch <= 0 || d->embed <= 0 || (d->embed & 7) ||
        d->himg < d->patch || d->wimg < d->patch || d->himg % d->patch || d->wimg % d->patch)
        return SKFCN_E_ARG;
    const int N = d->patch * d->patch * d->cout, wt = d->wimg / d->patch, M = (d->himg / d->patch) * wt;
    if (d->ldw < d->embed || (d->ldw & 7) || d->w_plane < (long long)N * d->ldw || (long long)M * d->embed >= (1ll << 30)) return SKFCN_E_ARG;
    const ALFast<true> al{d->t, M, d->embed, 1 << 30, d->embed, 0, 1};
    const EpHead ep{d->out, d->bias, d->cout, wt, d->patch, d->wimg, (long long)d->himg * d->wimg};
    const hipError_t e = run_gemm<TF>(al, ep, d->w, d->w_plane, d->ldw, M, N, d->embed, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? 0 : SKFCN_E_HIP;
}

}  // extern "C"
