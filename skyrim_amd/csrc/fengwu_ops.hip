// FengWu (cross-modal Swin transformer) call behind include/skyrim_fengwu.h.
//
//   GEMMs        gemm.h's pipeline, one batched kernel: grid z = the modality (or 1 for the fuser); A, W, bias and output advance by a
//                per-modality stride.  Loaders: ALEmb (a modality's channel slice of both raw states, normalised before the fp16 split,
//                zero rows outside the grid), ALFast rows (strided_gemm.h), ALCat (two sources along K: the skip linear).  EpFw: bias
//                (+ GELU) (+ residual), the 2 x 2 pixel shuffle of the patch expand with its crop, the 4 x 4 scatter of the recovery
//                with its crop and de-normalisation
//   attention    one wave = 16 queries of one (window, head, batch entry); key tiles of 32 with an online softmax.  S^T = K Q^T and
//                O^T = V^T P^T on v_mfma_f32_16x16x32_f16 (three hi/lo terms; head dim 32 = one k-step).  Windows of 1-, 2- or 3-D
//                over a padded (Z, H, W) grid; the shift and the padding are token indexing (a padded token reads the qkv bias); the
//                position bias and the shift mask come from one dense table row per query
//   row kernels  LayerNorm over token rows, batched over modalities; the patch merge's 2 x 2 gather feeds the same kernel
#include <hip/hip_runtime.h>

#include "../../include/skyrim_fengwu.h"
#include "strided_gemm.h"

namespace skp {

typedef TileCfg<128, 128, 32, 2, 4> TFw;     // 8 waves of 64 x 32

struct FwBatch {
    long long a, a2, w, o, b;                 // per-entry element strides of A, the second A source, W (hi plane), out, bias
    int off[SKFW_MAX_MODS], cnt[SKFW_MAX_MODS];
};

// ---- patch-embedding loader: token m = (i, j), k = (p 4 + dh) 4 + dw; a chunk of 8 = two rows dh of 4 pixels --------------------- //
struct ALEmb {
    static constexpr bool kDirect = false;
    const float* x0;
    const float* x1;
    const float* mean;
    const float* inv_std;
    int M, K, wt, n_lat, front, cnt;
    long long hw;
    struct Row { int y0, x, ok; };
    struct Raw { float v[8]; int c, ok0, ok1; };
    __device__ __forceinline__ Row row(int m) const {
        if (m >= M) return Row{0, 0, 0};
        const int i = m / wt;
        return Row{4 * i - front, 4 * (m - i * wt), 1};
    }
    __device__ __forceinline__ void issue(const Row& r, int k, Raw& o) const {
#pragma unroll
        for (int i = 0; i < 8; ++i) o.v[i] = 0.f;
        o.c = -1;
        o.ok0 = o.ok1 = 0;
        if (!r.ok || k >= K) return;
        const int p = k >> 4, dh = (k >> 2) & 3;
        if (p >= 2 * cnt) return;                            // a smaller modality: zero K tail
        const int l = p >= cnt ? 1 : 0, c = p - l * cnt;
        const int y = r.y0 + dh;
        const float* base = (l ? x1 : x0) + c * hw + r.x;
        o.c = c;
        if (y >= 0 && y < n_lat) {
            const float4 a = *reinterpret_cast<const float4*>(base + (long long)y * (4 * wt));
            o.v[0] = a.x; o.v[1] = a.y; o.v[2] = a.z; o.v[3] = a.w;
            o.ok0 = 1;
        }
        if (y + 1 >= 0 && y + 1 < n_lat) {
            const float4 b = *reinterpret_cast<const float4*>(base + (long long)(y + 1) * (4 * wt));
            o.v[4] = b.x; o.v[5] = b.y; o.v[6] = b.z; o.v[7] = b.w;
            o.ok1 = 1;
        }
    }
    __device__ __forceinline__ void finish(const Raw& r, float (&v)[8]) const {
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = 0.f;
        if (r.c < 0) return;
        const float mu = mean[r.c], is = inv_std[r.c];
        if (r.ok0) {
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i] = (r.v[i] - mu) * is;
        }
        if (r.ok1) {
#pragma unroll
            for (int i = 4; i < 8; ++i) v[i] = (r.v[i] - mu) * is;
        }
    }
    __device__ __forceinline__ uint4 direct(const Raw&) const { return make_uint4(0, 0, 0, 0); }
    __device__ __forceinline__ void at(int z, const FwBatch& bs) {
        const int off = bs.off[z];
        x0 += off * hw;
        x1 += off * hw;
        mean += off;
        inv_std += off;
        cnt = bs.cnt[z];
    }
};

// ---- two row-major sources along K (the skip linear's [expand ; encoder stage 1]) -------------------------------------------------- //
struct ALCat {
    static constexpr bool kDirect = false;
    const float* a;
    const float* a2;
    int M, K, lda, lda2, k_split;
    struct Row { long long m; int ok; };
    struct Raw { float v[8]; };
    __device__ __forceinline__ Row row(int m) const { return Row{m, m < M ? 1 : 0}; }
    __device__ __forceinline__ void issue(const Row& r, int k, Raw& o) const {
#pragma unroll
        for (int i = 0; i < 8; ++i) o.v[i] = 0.f;
        if (!r.ok || k >= K) return;
        const float* p = k < k_split ? a + r.m * lda + k : a2 + r.m * lda2 + (k - k_split);
        const float4 x = *reinterpret_cast<const float4*>(p), y = *reinterpret_cast<const float4*>(p + 4);
        o.v[0] = x.x; o.v[1] = x.y; o.v[2] = x.z; o.v[3] = x.w; o.v[4] = y.x; o.v[5] = y.y; o.v[6] = y.z; o.v[7] = y.w;
    }
    __device__ __forceinline__ void finish(const Raw& r, float (&v)[8]) const {
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = r.v[i];
    }
    __device__ __forceinline__ uint4 direct(const Raw&) const { return make_uint4(0, 0, 0, 0); }
    __device__ __forceinline__ void at(int z, const FwBatch& bs) {
        a += z * bs.a;
        a2 += z * bs.a2;
    }
};

__device__ __forceinline__ void batch_at(ALFast<true>& al, int z, const FwBatch& bs) { al.a += z * bs.a; }
template <class AL> __device__ __forceinline__ void batch_at(AL& al, int z, const FwBatch& bs) { al.at(z, bs); }

// ---- epilogue: store (+ bias, GELU, + residual), patch expand (2 x 2 shuffle + crop), recovery (4 x 4 scatter + crop + affine) ------ //
enum { EP_STORE = 0, EP_EXPAND = 1, EP_RECOVER = 2 };

struct EpFw {
    static constexpr bool kDualOrder = false;
    template <class TC> __device__ __forceinline__ void init(char*, int, int) const {}
    float* out;
    const float* bias;          // may be null
    const float* res;           // EP_STORE: residual, may be null (may equal out)
    const float* mean;          // EP_RECOVER
    const float* std;
    int mode, act, ldo;         // EP_STORE: ldo = N; EP_EXPAND: ldo = Co
    int w_tok, h_out, front;    // EP_EXPAND / EP_RECOVER: token grid width, kept output rows, cropped front rows
    int cnt;                    // EP_RECOVER: channels kept
    long long hw;               // EP_RECOVER: plane size
    __device__ __forceinline__ void at(int z, const FwBatch& bs) {
        if (bias) bias += z * bs.b;
        if (mode == EP_RECOVER) {
            const int off = bs.off[z];
            out += off * hw;
            mean += off;
            std += off;
            cnt = bs.cnt[z];
        } else {
            out += z * bs.o;
            if (res) res += z * bs.o;
        }
    }
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
                const int n = n0w + b * 16 + l4;                  // N % 4 == 0: the 4 columns are all inside or all outside
                if (n >= N) continue;
                float v[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] = acc[a][b][r] + (bias ? bias[mode == EP_RECOVER ? (n + r) >> 4 : n + r] : 0.f);
                if (mode == EP_STORE) {
                    if (act) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) v[r] = gelu_erf(v[r]);
                    }
                    const long long o = (long long)m * ldo + n;
                    if (res) {
                        const float4 t = *reinterpret_cast<const float4*>(res + o);
                        v[0] += t.x; v[1] += t.y; v[2] += t.z; v[3] += t.w;
                    }
                    *reinterpret_cast<float4*>(out + o) = make_float4(v[0], v[1], v[2], v[3]);
                } else if (mode == EP_EXPAND) {
                    const int co = n % ldo, q = n / ldo;             // ldo % 4 == 0: the 4 columns share q
                    const int y = m / w_tok, x = m - y * w_tok;
                    const int yo = 2 * y + (q >> 1) - front;
                    if (yo < 0 || yo >= h_out) continue;
                    const long long pix = (long long)yo * (2 * w_tok) + 2 * x + (q & 1);
                    *reinterpret_cast<float4*>(out + pix * ldo + co) = make_float4(v[0], v[1], v[2], v[3]);
                } else {
                    const int i = m / w_tok, j = m - i * w_tok;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int nn = n + r, c = nn >> 4, p1 = (nn >> 2) & 3, p2 = nn & 3;
                        const int yo = 4 * i + p1 - front;
                        if (c >= cnt || yo < 0 || yo >= h_out) continue;
                        out[c * hw + (long long)yo * (4 * w_tok) + 4 * j + p2] = v[r] * std[c] + mean[c];
                    }
                }
            }
        }
    }
};

template <class AL>
__global__ void __launch_bounds__(TFw::THREADS) fw_gemm_kernel(GemmArgs<PrecF16x3, AL, EpFw> g, const FwBatch bs) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int z = blockIdx.z;
    batch_at(g.al, z, bs);
    g.ep.at(z, bs);
    g.W += z * bs.w;
    gemm_body<PrecF16x3, TFw, AL, EpFw, true>(g, smem);
}

template <class AL>
hipError_t run_gemm(const AL& al, const EpFw& ep, const FwBatch& bs, const void* w, long long w_plane, int ldw, int batch, int M, int N, int K,
                    hipStream_t s) {
    GemmArgs<PrecF16x3, AL, EpFw> g;
    g.al = al;
    g.ep = ep;
    g.W = static_cast<const f16*>(w);
    g.w_plane = w_plane;
    g.ldw = ldw;
    g.M = M; g.N = N; g.K = K;
    const dim3 grid((N + TFw::BN - 1) / TFw::BN, (M + TFw::BM - 1) / TFw::BM, batch);
    constexpr int smem = gemm_smem_bytes<PrecF16x3, TFw>() + kEpiScratch;
    static_assert(smem <= 64 * 1024, "LDS per block without the opt-in");
    hipLaunchKernelGGL((fw_gemm_kernel<AL>), grid, dim3(TFw::THREADS), smem, s, g, bs);
    return hipGetLastError();
}

// ---- LayerNorm over token rows (batched; or the 2 x 2 merge gather): one wavefront per row, the row in registers ------------------ //
constexpr int kLnVec = 6;                     // C <= 1536: 6 float4 per lane

__global__ void __launch_bounds__(256) ln_kernel(const skfw_ln_desc d) {
    const long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (r >= d.rows * d.batch) return;
    const int z = (int)(r / d.rows);
    const long long rr = r - (long long)z * d.rows;
    const int C = d.C, C4 = C >> 2;
    float4 v[kLnVec];
    if (!d.merge) {
        const float4* xr = reinterpret_cast<const float4*>(d.x + r * C);
#pragma unroll
        for (int i = 0; i < kLnVec; ++i) {
            const int c = lane + 64 * i;
            v[i] = c < C4 ? xr[c] : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    } else {
        const int cs = C >> 2, cs4 = cs >> 2, w2 = d.w_src >> 1;
        const int i = (int)(rr / w2), j = (int)(rr - (long long)i * w2);
        const float* xb = d.x + (long long)z * d.h_src * d.w_src * cs;
#pragma unroll
        for (int u = 0; u < kLnVec; ++u) {
            const int c = lane + 64 * u;
            v[u] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (c < C4) {
                const int q = c / cs4, cc = c - q * cs4;             // Swin's order: (dy, dx) = (0, 0), (1, 0), (0, 1), (1, 1)
                const int sy = 2 * i + (q & 1) - d.front, sx = 2 * j + (q >> 1);
                if (sy >= 0 && sy < d.h_src) v[u] = reinterpret_cast<const float4*>(xb + ((long long)sy * d.w_src + sx) * cs)[cc];
            }
        }
    }
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < kLnVec; ++i) s += (v[i].x + v[i].y) + (v[i].z + v[i].w);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    const float mean = s / (float)C;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < kLnVec; ++i) {
        if (lane + 64 * i < C4) {
            const float a = v[i].x - mean, b = v[i].y - mean, c = v[i].z - mean, e = v[i].w - mean;
            q += (a * a + b * b) + (c * c + e * e);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) q += __shfl_xor(q, o);
    const float rstd = rsqrtf(q / (float)C + d.eps);
    float4* orow = reinterpret_cast<float4*>(d.out + r * C);
    const float4* gp = reinterpret_cast<const float4*>(d.gamma + (long long)z * C);
    const float4* bp = reinterpret_cast<const float4*>(d.beta + (long long)z * C);
#pragma unroll
    for (int i = 0; i < kLnVec; ++i) {
        const int c = lane + 64 * i;
        if (c < C4) {
            const float4 gm = gp[c], bt = bp[c];
            orow[c] = make_float4((v[i].x - mean) * rstd * gm.x + bt.x, (v[i].y - mean) * rstd * gm.y + bt.y,
                                  (v[i].z - mean) * rstd * gm.z + bt.z, (v[i].w - mean) * rstd * gm.w + bt.w);
        }
    }
}

// ---- window attention ---------------------------------------------------------------------------------------------------------- //
typedef OpT<f16>::v8 v8;
constexpr int kHd = 32;

__device__ __forceinline__ void split_v8(const float (&v)[8], v8& h, v8& l) {
    uint4 o[2];
    split8<f16, 2>(v, o);
    h = as_v8<f16>(o[0]);
    l = as_v8<f16>(o[1]);
}

// P's scale before its fp16 split: p <= 1 stays below the fp16 maximum, and the lo plane of p >= 2^-18 stays normal
constexpr float kPScale = 32768.0f;

__device__ __forceinline__ f32x4 mfma3(const v8& ah, const v8& al, const v8& bh, const v8& bl, f32x4 c) {
    c = OpT<f16>::mfma(al, bh, c);
    c = OpT<f16>::mfma(ah, bl, c);
    return OpT<f16>::mfma(ah, bh, c);
}

__device__ __forceinline__ void load8(const float* p, float (&v)[8]) {
    const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}

__device__ __forceinline__ int type_of(int n_types, int n_win, int i) { return n_types == n_win ? i : (n_types == 2 ? (i == n_win - 1 ? 1 : 0) : 0); }

__global__ void __launch_bounds__(256) window_attn_kernel(const skfw_attn_desc d, int nqc) {
    const int lane = threadIdx.x & 63, l15 = lane & 15, g = lane >> 4;
    const int wave = threadIdx.x >> 6;
    const int win = blockIdx.x, head = blockIdx.y, bt = blockIdx.z / nqc, qc = blockIdx.z - bt * nqc;
    const int wz = d.wz, wh = d.wh, ww = d.ww, whw = wh * ww, N = wz * whw;
    const int q0 = qc * 64 + wave * 16;
    if (q0 >= N) return;                                          // wave-uniform; no barriers in this kernel
    const int nwx = d.Wp / ww, nwy = d.Hp / wh, nwz = d.Zp / wz;
    const int wx = win % nwx, wyz = win / nwx, wy = wyz % nwy, wzi = wyz / nwy;
    const long long ld = 3ll * d.C, ntok = (long long)d.Z * d.H * d.W;
    const float* qkv = d.qkv + bt * ntok * ld + head * kHd;
    const float* pb = d.qkv_bias + bt * ld + head * kHd;
    // window-local index -> shifted padded-grid coordinate -> rolled back -> unpadded token (-1: a padding token)
    auto token = [&](int i) -> long long {
        const int iz = i / whw, rem = i - iz * whw, iy = rem / ww, ix = rem - iy * ww;
        int zs = wzi * wz + iz + d.sz, ys = wy * wh + iy + d.sh, xs = wx * ww + ix + d.sw;
        if (zs >= d.Zp) zs -= d.Zp;
        if (ys >= d.Hp) ys -= d.Hp;
        if (xs >= d.Wp) xs -= d.Wp;
        const int zr = zs - d.fz, yr = ys - d.fh, xr = xs - d.fw;
        if (zr < 0 || zr >= d.Z || yr < 0 || yr >= d.H || xr < 0 || xr >= d.W) return -1;
        return ((long long)zr * d.H + yr) * d.W + xr;
    };
    auto ptr = [&](long long t, int part) -> const float* { return (t < 0 ? pb : qkv + t * ld) + part * d.C; };

    // queries: lane (l15, g) holds scale q[d = 8 g + j] of query q0 + l15 (the B operand of S^T = K Q^T)
    const int qi = q0 + l15 < N ? q0 + l15 : N - 1;
    const long long tq = token(qi);
    v8 qh, ql;
    {
        float v[8];
        load8(ptr(tq, 0) + 8 * g, v);
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] *= d.scale;
        split_v8(v, qh, ql);
    }
    const int type = type_of(d.types_z, nwz, wzi) * d.types_y + type_of(d.types_y, nwy, wy);
    const float* trow = d.table + bt * d.table_sb + (((long long)type * d.heads + head) * N + qi) * N;
    float m = -INFINITY, lsum = 0.f;
    f32x4 o[2];
#pragma unroll
    for (int b = 0; b < 2; ++b) o[b] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int k0 = 0; k0 < N; k0 += 32) {
        // S^T[key][q] for keys k0 + 16 b + (0..15): A = K[key = l15 + 16 b][d = 8 g + j]
        f32x4 s[2];
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const int key = k0 + 16 * b + l15 < N ? k0 + 16 * b + l15 : N - 1;
            float v[8];
            load8(ptr(token(key), 1) + 8 * g, v);
            v8 kh, kl;
            split_v8(v, kh, kl);
            s[b] = mfma3(kh, kl, qh, ql, f32x4{0.f, 0.f, 0.f, 0.f});
        }
        // s[b][r] = score of key k0 + 16 b + 4 g + r for query q0 + l15: + the table entry; online softmax
        float p[8];
        float mx = -INFINITY;
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int key = k0 + 16 * b + 4 * g + r;
                const float v = key < N ? s[b][r] + trow[key] : -INFINITY;
                p[4 * b + r] = v;
                mx = fmaxf(mx, v);
            }
        mx = fmaxf(mx, __shfl_xor(mx, 16));
        mx = fmaxf(mx, __shfl_xor(mx, 32));
        const float mn = fmaxf(m, mx);                  // finite: key k0 is in every tile
        const float alpha = expf(m - mn);
        m = mn;
        lsum *= alpha;
#pragma unroll
        for (int b = 0; b < 2; ++b) o[b] *= alpha;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            p[i] = p[i] == -INFINITY ? 0.f : expf(p[i] - mn);
            lsum += p[i];
        }
        // P^T as the B operand: k-slot (g, j) <-> key k0 + (j < 4 ? 4 g + j : 16 + 4 g + j - 4), exactly this lane's p[j], scaled by
        // kPScale before the split (1/kPScale is folded into 1/lsum): unscaled, a p below 2^-3 leaves a subnormal lo plane that keeps
        // only multiples of 2^-24, and over a sharp softmax of many keys those losses add up
        v8 ph, pl;
        {
            float ps[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) ps[i] = p[i] * kPScale;
            split_v8(ps, ph, pl);
        }
        const float* vp[8];
        bool vok[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int key = k0 + (j < 4 ? 4 * g + j : 12 + 4 * g + j);
            vok[j] = key < N;
            vp[j] = ptr(token(vok[j] ? key : N - 1), 2) + l15;
        }
        // O^T[d][q] += V^T P^T: A = V^T[d = 16 db + l15][k-slot (g, j)]
#pragma unroll
        for (int db = 0; db < 2; ++db) {
            float v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = vok[j] ? vp[j][16 * db] : 0.f;
            v8 vh, vl;
            split_v8(v, vh, vl);
            o[db] = mfma3(vh, vl, ph, pl, o[db]);
        }
    }
    lsum += __shfl_xor(lsum, 16);
    lsum += __shfl_xor(lsum, 32);
    if (q0 + l15 >= N || tq < 0) return;
    const float inv = (1.0f / lsum) * (1.0f / kPScale);
    // o[db][r] = O[q0 + l15][16 db + 4 g + r]
    float* op = d.out + (bt * ntok + tq) * d.C + head * kHd + 4 * g;
#pragma unroll
    for (int db = 0; db < 2; ++db)
        *reinterpret_cast<float4*>(op + 16 * db) = make_float4(o[db][0] * inv, o[db][1] * inv, o[db][2] * inv, o[db][3] * inv);
}

}  // namespace skp

using namespace skp;

static bool aligned16(const void* p) { return (reinterpret_cast<size_t>(p) & 15) == 0; }

static int hip_status() { return hipGetLastError() == hipSuccess ? 0 : SKFW_E_HIP; }

static bool mods_ok(int mods, const int* off, const int* cnt) {
    if (mods <= 0 || mods > SKFW_MAX_MODS) return false;
    for (int z = 0; z < mods; ++z)
        if (off[z] < 0 || cnt[z] <= 0) return false;
    return true;
}

extern "C" {

int skfw_abi_version(void) { return SKFW_ABI_VERSION; }

const char* skfw_error_string(int code) {
    switch (code) {
        case 0: return "success";
        case SKFW_E_ARG: return "invalid argument";
        case SKFW_E_HIP: return "HIP runtime error";
        case SKFW_E_WINDOW: return "the attention window does not tile its padded token grid";
        default: return "unknown error code";
    }
}

int skfw_prepare_weight(const float* src, long long sn, long long sk, int N, int K, void* dst, long long plane, int ldw, void* stream) {
    if (!src || !dst || N <= 0 || K <= 0 || ldw < K || (ldw & 7) || plane < (long long)N * ldw) return SKFW_E_ARG;
    const hipError_t e = prep_weight<f16, 2>(src, static_cast<f16*>(dst), plane, N, K, ldw, sn, sk, 0, 0, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? 0 : SKFW_E_HIP;
}

int skfw_embed(const skfw_embed_desc* d, void* stream) {
    if (!d || !d->x0 || !d->x1 || !d->mean || !d->inv_std || !d->w || !d->bias || !d->out || !mods_ok(d->mods, d->ch_off, d->ch_cnt) ||
        d->C <= 0 || (d->C & 3) || d->n_lat <= 0 || d->n_lon < 4 || (d->n_lon & 3) || d->h_tok <= 0 || d->lat_front < 0 ||
        !aligned16(d->x0) || !aligned16(d->x1) || !aligned16(d->out))
        return SKFW_E_ARG;
    int cmax = 0;
    for (int z = 0; z < d->mods; ++z) cmax = d->ch_cnt[z] > cmax ? d->ch_cnt[z] : cmax;
    const int wt = d->n_lon / 4, M = d->h_tok * wt;
    if (d->K != 32 * cmax || d->ldw < d->K || (d->ldw & 7) || d->w_sb < (long long)d->C * d->ldw || d->w_plane < d->mods * d->w_sb ||
        (long long)M * d->C >= (1ll << 31) || 4 * (d->h_tok - 1) - d->lat_front >= d->n_lat)
        return SKFW_E_ARG;
    FwBatch bs{0, 0, d->w_sb, (long long)M * d->C, d->C, {}, {}};
    for (int z = 0; z < d->mods; ++z) { bs.off[z] = d->ch_off[z]; bs.cnt[z] = d->ch_cnt[z]; }
    const ALEmb al{d->x0, d->x1, d->mean, d->inv_std, M, d->K, wt, d->n_lat, d->lat_front, 0, (long long)d->n_lat * d->n_lon};
    const EpFw ep{d->out, d->bias, nullptr, nullptr, nullptr, EP_STORE, 0, d->C, 0, 0, 0, 0, 0};
    return run_gemm(al, ep, bs, d->w, d->w_plane, d->ldw, d->mods, M, d->C, d->K, static_cast<hipStream_t>(stream)) == hipSuccess ? 0 : SKFW_E_HIP;
}

int skfw_layer_norm(const skfw_ln_desc* d, void* stream) {
    if (!d || !d->x || !d->gamma || !d->beta || !d->out || d->rows <= 0 || d->batch <= 0 || d->C <= 0 || (d->C & 3) || d->C > 4 * 64 * kLnVec ||
        !aligned16(d->x) || !aligned16(d->out) || !aligned16(d->gamma) || !aligned16(d->beta) || d->merge < 0 || d->merge > 1)
        return SKFW_E_ARG;
    if (d->merge && ((d->C & 15) || d->w_src < 2 || (d->w_src & 1) || d->h_src <= 0 || d->front < 0 || d->rows % (d->w_src / 2) ||
                     2 * (d->rows / (d->w_src / 2)) < d->h_src + d->front))
        return SKFW_E_ARG;
    const long long total = d->rows * d->batch;
    hipLaunchKernelGGL(ln_kernel, dim3((unsigned)((total + 3) / 4)), dim3(256), 0, static_cast<hipStream_t>(stream), *d);
    return hip_status();
}

int skfw_linear(const skfw_linear_desc* d, void* stream) {
    if (!d || !d->a || !d->w || !d->out || d->batch <= 0 || d->batch > 65535 || d->M <= 0 || d->N <= 0 || (d->N & 3) || d->K <= 0 ||
        (d->K & 7) || d->lda < 0 || (d->lda & 7) || d->act < 0 || d->act > 1 || d->mode < 0 || d->mode > 1 || d->ldw < d->K || (d->ldw & 7) ||
        d->w_sb < (long long)d->N * d->ldw || d->w_plane < d->batch * d->w_sb || !aligned16(d->a) || !aligned16(d->out) ||
        (d->res && (!aligned16(d->res) || d->mode != 0)) || (long long)d->M * d->N >= (1ll << 31))
        return SKFW_E_ARG;
    if (d->a2 && (!aligned16(d->a2) || d->k_split <= 0 || (d->k_split & 7) || d->k_split >= d->K || d->lda < d->k_split || (d->lda2 & 7) ||
                  d->lda2 < d->K - d->k_split || (long long)d->M * d->lda2 >= (1ll << 30)))
        return SKFW_E_ARG;
    if (!d->a2 && (d->lda < d->K || (long long)d->M * d->lda >= (1ll << 30))) return SKFW_E_ARG;
    if (d->mode == 1 && (d->act || (d->N & 15) || d->w_tok <= 0 || d->M % d->w_tok || d->h_out <= 0 || d->front < 0 ||
                         2 * (d->M / d->w_tok) < d->h_out + d->front))
        return SKFW_E_ARG;
    FwBatch bs{d->a_sb, d->a2_sb, d->w_sb, d->o_sb, d->b_sb, {}, {}};
    const EpFw ep{d->out, d->bias, d->res, nullptr, nullptr, d->mode ? EP_EXPAND : EP_STORE, d->act, d->mode ? d->N / 4 : d->N, d->w_tok,
                  d->h_out, d->front, 0, 0};
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipError_t e;
    if (d->a2) {
        const ALCat al{d->a, d->a2, d->M, d->K, d->lda, d->lda2, d->k_split};
        e = run_gemm(al, ep, bs, d->w, d->w_plane, d->ldw, d->batch, d->M, d->N, d->K, s);
    } else {
        const ALFast<true> al{d->a, d->M, d->K, 1 << 30, d->lda, 0, 1};
        e = run_gemm(al, ep, bs, d->w, d->w_plane, d->ldw, d->batch, d->M, d->N, d->K, s);
    }
    return e == hipSuccess ? 0 : SKFW_E_HIP;
}

int skfw_window_attention(const skfw_attn_desc* d, void* stream) {
    if (!d || !d->qkv || !d->qkv_bias || !d->table || !d->out || d->batch <= 0 || d->heads <= 0 || d->heads > 65535 || d->C != kHd * d->heads ||
        d->Z <= 0 || d->H <= 0 || d->W <= 0 || d->wz <= 0 || d->wh <= 0 || d->ww <= 0 || d->fz < 0 || d->fh < 0 || d->fw < 0 ||
        d->Zp < d->Z + d->fz || d->Hp < d->H + d->fh || d->Wp < d->W + d->fw || !aligned16(d->qkv) || !aligned16(d->qkv_bias) ||
        !aligned16(d->out) || (long long)d->batch * d->Z * d->H * d->W * 3 * d->C >= (1ll << 40))
        return SKFW_E_ARG;
    if (d->Zp % d->wz || d->Hp % d->wh || d->Wp % d->ww) return SKFW_E_WINDOW;
    const int N = d->wz * d->wh * d->ww, nwz = d->Zp / d->wz, nwy = d->Hp / d->wh;
    if (N < 2 || N > 1024 || d->sz < 0 || d->sz >= d->wz || d->sh < 0 || d->sh >= d->wh || d->sw < 0 || d->sw >= d->ww || d->table_sb < 0 ||
        (d->types_z != 1 && d->types_z != 2 && d->types_z != nwz) || (d->types_y != 1 && d->types_y != 2 && d->types_y != nwy) ||
        (d->batch > 1 && d->table_sb < (long long)d->types_z * d->types_y * d->heads * N * N))
        return SKFW_E_ARG;
    const long long nwin = (long long)nwz * nwy * (d->Wp / d->ww);
    const int nqc = (N + 63) / 64;
    if (nwin >= (1ll << 31) || (long long)d->batch * nqc > 65535) return SKFW_E_ARG;
    hipLaunchKernelGGL(window_attn_kernel, dim3((unsigned)nwin, d->heads, d->batch * nqc), dim3(256), 0, static_cast<hipStream_t>(stream), *d, nqc);
    return hip_status();
}

int skfw_recover(const skfw_recover_desc* d, void* stream) {
    if (!d || !d->a || !d->w || !d->bias || !d->mean || !d->std || !d->out || !mods_ok(d->mods, d->ch_off, d->ch_cnt) || d->h_tok <= 0 ||
        d->w_tok <= 0 || d->C <= 0 || (d->C & 7) || d->c_max <= 0 || d->n_lat <= 0 || d->lat_front < 0 || !aligned16(d->a) ||
        4 * d->h_tok < d->n_lat + d->lat_front)
        return SKFW_E_ARG;
    const int M = d->h_tok * d->w_tok, N = 16 * d->c_max;
    for (int z = 0; z < d->mods; ++z)
        if (d->ch_cnt[z] > d->c_max) return SKFW_E_ARG;
    if (d->ldw < d->C || (d->ldw & 7) || d->w_sb < (long long)N * d->ldw || d->w_plane < d->mods * d->w_sb || (long long)M * d->C >= (1ll << 30))
        return SKFW_E_ARG;
    FwBatch bs{(long long)M * d->C, 0, d->w_sb, 0, d->c_max, {}, {}};
    for (int z = 0; z < d->mods; ++z) { bs.off[z] = d->ch_off[z]; bs.cnt[z] = d->ch_cnt[z]; }
    const ALFast<true> al{d->a, M, d->C, 1 << 30, d->C, 0, 1};
    const EpFw ep{d->out, d->bias, nullptr, d->mean, d->std, EP_RECOVER, 0, N, d->w_tok, d->n_lat, d->lat_front, 0,
                  (long long)d->n_lat * 4 * d->w_tok};
    return run_gemm(al, ep, bs, d->w, d->w_plane, d->ldw, d->mods, M, N, d->C, static_cast<hipStream_t>(stream)) == hipSuccess ? 0 : SKFW_E_HIP;
}

}  // extern "C"
