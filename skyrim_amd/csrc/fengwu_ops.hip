// FengWu (cross-modal Swin transformer) call behind include/skyrim_fengwu.h.
//
//   GEMMs        gemm.h's pipeline, one batched kernel: grid z = the modality (or 1 for the fuser); A, W, bias and output advance by a
//                per-modality stride.  Loaders: ALEmb (a modality's channel slice of both raw states, normalised before the fp16 split,
//                zero rows outside the grid), ALFast rows (strided_gemm.h), ALCat (two sources along K: the skip linear).  EpFw: bias
//                (+ GELU) (+ residual), the 2 x 2 pixel shuffle of the patch expand with its crop, the 4 x 4 scatter of the recovery
//                with its crop and de-normalisation
//   attention    window_attn.h's body (one wave = 16 queries of one (window, head, batch entry), online softmax over key tiles of
//                32) with head dim 32 = one k-step.  FwAttn supplies windows of 1-, 2- or 3-D over a padded (Z, H, W) grid: the shift
//                and the padding are token indexing (a padded token reads the qkv bias); the position bias and the shift mask come
//                from one dense table row per query
//   row kernels  LayerNorm over token rows (rownorm.h), batched over modalities; the patch merge's 2 x 2 gather feeds the same kernel
#include <hip/hip_runtime.h>

#include "../../include/skyrim_fengwu.h"
#include "rownorm.h"
#include "strided_gemm.h"
#include "window_attn.h"

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
        load8(p, o.v);
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
    if (r >= d.rows * d.batch) return;
    const int z = (int)(r / d.rows), C = d.C;
    const float *gamma = d.gamma + (long long)z * C, *beta = d.beta + (long long)z * C;
    if (!d.merge) {
        row_layer_norm<kLnVec>(RowContig{reinterpret_cast<const float4*>(d.x + r * C)}, gamma, beta, nullptr, d.out + r * C, C, d.eps);
        return;
    }
    // row (i, j) of the merged grid: the 2 x 2 source tokens in Swin's order (dy, dx) = (0, 0), (1, 0), (0, 1), (1, 1); source rows cropped
    // at the front or beyond the source are zero
    const long long rr = r - (long long)z * d.rows;
    const int cs = C >> 2, cs4 = cs >> 2, w2 = d.w_src >> 1;
    const int i = (int)(rr / w2), j = (int)(rr - (long long)i * w2);
    const float* xb = d.x + (long long)z * d.h_src * d.w_src * cs;
    const auto gather = [&](int c) {
        const int q = c / cs4, cc = c - q * cs4;
        const int sy = 2 * i + (q & 1) - d.front, sx = 2 * j + (q >> 1);
        if (sy < 0 || sy >= d.h_src) return make_float4(0.f, 0.f, 0.f, 0.f);
        return reinterpret_cast<const float4*>(xb + ((long long)sy * d.w_src + sx) * cs)[cc];
    };
    row_layer_norm<kLnVec>(gather, gamma, beta, nullptr, d.out + r * C, C, d.eps);
}

// ---- window attention ---------------------------------------------------------------------------------------------------------- //
constexpr int kHd = 32;

__device__ __forceinline__ int type_of(int n_types, int n_win, int i) { return n_types == n_win ? i : (n_types == 2 ? (i == n_win - 1 ? 1 : 0) : 0); }

struct FwAttn {
    static constexpr int HD = kHd;
    const skfw_attn_desc& d;
    int bt, head, wzi, wy, wx;         // batch entry, head, the window's place in the shifted padded grid
    const float* qkv;                  // the batch entry's tokens and the row a padding token reads, both at the head's q
    const float* pb;
    const float* table;                // [N][N] of the window's type and the head
    long long tq;                      // the query: its token (-1: padding) and its table row
    const float* trow;
    __device__ __forceinline__ FwAttn(const skfw_attn_desc& d_, int win, int head_, int bt_) : d(d_), bt(bt_), head(head_) {
        const int nwx = d.Wp / d.ww, nwy = d.Hp / d.wh, nwz = d.Zp / d.wz, wyz = win / nwx, N = d.wz * d.wh * d.ww;
        wx = win % nwx;
        wy = wyz % nwy;
        wzi = wyz / nwy;
        qkv = d.qkv + bt * ((long long)d.Z * d.H * d.W) * (3ll * d.C) + head * kHd;
        pb = d.qkv_bias + bt * (3ll * d.C) + head * kHd;
        const int type = type_of(d.types_z, nwz, wzi) * d.types_y + type_of(d.types_y, nwy, wy);
        table = d.table + bt * d.table_sb + ((long long)type * d.heads + head) * N * N;
    }
    // window-local index -> shifted padded-grid coordinate -> rolled back -> unpadded token (-1: a padding token)
    __device__ __forceinline__ long long token(int i) const {
        const int whw = d.wh * d.ww, iz = i / whw, rem = i - iz * whw, iy = rem / d.ww, ix = rem - iy * d.ww;
        int zs = wzi * d.wz + iz + d.sz, ys = wy * d.wh + iy + d.sh, xs = wx * d.ww + ix + d.sw;
        if (zs >= d.Zp) zs -= d.Zp;
        if (ys >= d.Hp) ys -= d.Hp;
        if (xs >= d.Wp) xs -= d.Wp;
        const int zr = zs - d.fz, yr = ys - d.fh, xr = xs - d.fw;
        if (zr < 0 || zr >= d.Z || yr < 0 || yr >= d.H || xr < 0 || xr >= d.W) return -1;
        return ((long long)zr * d.H + yr) * d.W + xr;
    }
    __device__ __forceinline__ void query(int i) {
        tq = token(i);
        trow = table + (long long)i * (d.wz * d.wh * d.ww);
    }
    __device__ __forceinline__ const float* row(int i, int part) const {
        const long long t = token(i);
        return (t < 0 ? pb : qkv + t * (3ll * d.C)) + part * d.C;
    }
    __device__ __forceinline__ void prep_q(float (&v)[1][8]) const {
#pragma unroll
        for (int j = 0; j < 8; ++j) v[0][j] *= d.scale;
    }
    __device__ __forceinline__ void prep_k(float (&)[1][8]) const {}
    __device__ __forceinline__ float score(float s, int key) const { return s + trow[key]; }
    __device__ __forceinline__ float* out() const {
        return tq < 0 ? nullptr : d.out + (bt * ((long long)d.Z * d.H * d.W) + tq) * d.C + head * kHd;
    }
};

__global__ void __launch_bounds__(256) window_attn_kernel(const skfw_attn_desc d, int nqc) {
    const int bt = blockIdx.z / nqc;
    window_attn_body(FwAttn(d, blockIdx.x, blockIdx.y, bt), d.wz * d.wh * d.ww, blockIdx.z - bt * nqc);
}

}  // namespace skp

using namespace skp;

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
    return prepare_weight_f16(src, sn, sk, N, K, dst, plane, ldw, stream, SKFW_E_ARG, SKFW_E_HIP);
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
    return hip_status(SKFW_E_HIP);
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
    return hip_status(SKFW_E_HIP);
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
