// DLWP (cubed-sphere U-Net) call behind include/skyrim_dlwp.h.
//
//   ingest   one thread per cube cell: the LL->CS CSR row gathered over the 2 x C normalised lat-lon planes, TISR of both levels
//            (float64), mask and topography -> one channels-last row of the first conv's input
//   conv     gemm.h's pipeline with ALCube, a loader that gathers the 3 x 3 neighbourhood of a cell through the cube padding table
//            (rotated neighbour faces, corner means, the mirrored polar face) and reads its source pooled, upsampled or concatenated
//            with the skip on the way; EpCube adds the bias and applies the clamped leaky ReLU.  Rows are laid out face by face, each
//            face padded to whole tiles, so a workgroup sees one face and takes the equatorial or the polar weights from it
//   egress   one thread per lat-lon point: the CS->LL CSR row over the 14 output channels, de-normalised into the two states
#include <hip/hip_runtime.h>

#include "../../include/skyrim_dlwp.h"
#include "gemm.h"
#include "launchers.h"

namespace skp {

typedef TileCfg<128, 128, 32, 2, 4> TWide;     // cout >= 128: 8 waves of 64 x 32
typedef TileCfg<128, 64, 32, 4, 2> TNarrow;    // cout <= 64:  8 waves of 32 x 32
constexpr int kRowTile = 128;                  // BM of both: the per-face row padding unit

// ---- ingest --------------------------------------------------------------------------------------------------------------------- //
constexpr int kMaxC = 8;

// cos of the solar zenith angle (spec.py solar_position / cos_zenith, the same expressions in float64)
__device__ double cos_zenith(double days, double lat_deg, double lon_deg) {
    const double d2r = 3.14159265358979323846 / 180.0;
    const double T = days / 36525.0;
    const double M = d2r * (357.52910 + 35999.05030 * T - 0.0001559 * T * T - 0.00000048 * T * T * T);
    const double L0 = d2r * (280.46645 + 36000.76983 * T + 0.0003032 * T * T);
    const double dL = d2r * ((1.914600 - 0.004817 * T - 0.000014 * T * T) * sin(M) + (0.019993 - 0.000101 * T) * sin(2.0 * M) + 0.000290 * sin(3.0 * M));
    const double lam = L0 + dL;
    const double eps = d2r * (23.0 + 26.0 / 60.0 + 21.406 / 3600.0 -
                              (46.836769 * T - 0.0001831 * T * T + 0.00200340 * T * T * T - 0.576e-6 * T * T * T * T - 4.34e-8 * T * T * T * T * T) / 3600.0);
    const double x = cos(lam), y = cos(eps) * sin(lam), z = sin(eps) * sin(lam);
    const double r = sqrt(1.0 - z * z);
    const double dec = atan2(z, r), ra = 2.0 * atan2(y, x + r);
    const double theta = 67310.54841 + T * (876600.0 * 3600.0 + 8640184.812866 + T * (0.093104 - T * 6.2e-5));
    const double gmst = fmod(d2r * (theta / 240.0), 2.0 * 3.14159265358979323846);
    const double la = d2r * lat_deg, lo = d2r * lon_deg;
    return sin(la) * sin(dec) + cos(la) * cos(dec) * cos(gmst + lo - ra);
}

__global__ void __launch_bounds__(256) ingest_kernel(const skdlwp_ingest_desc d) {
    const int cell = blockIdx.x * 256 + threadIdx.x;
    if (cell >= d.cells) return;
    const int C = d.channels;
    float a0[kMaxC], a1[kMaxC];
#pragma unroll
    for (int c = 0; c < kMaxC; ++c) a0[c] = a1[c] = 0.f;
    const int j1 = d.row_ptr[cell + 1];
    for (int j = d.row_ptr[cell]; j < j1; ++j) {
        const long long p = d.col[j];
        const float s = d.S[j];
#pragma unroll
        for (int c = 0; c < kMaxC; ++c) {
            if (c < C) {
                const float ctr = d.center[c], inv = d.inv_scale[c];
                a0[c] += s * ((d.x0[c * (long long)d.points + p] - ctr) * inv);
                a1[c] += s * ((d.x1[c * (long long)d.points + p] - ctr) * inv);
            }
        }
    }
    const double lat = d.lat[cell], lon = d.lon[cell], inv_pi = 0.31830988618379067154;
    float* o = d.out + (long long)cell * d.ld_out;
#pragma unroll
    for (int c = 0; c < kMaxC; ++c) {
        if (c < C) {
            o[c] = a0[c];
            o[C + 1 + c] = a1[c];
        }
    }
    o[C] = (float)(fmax(cos_zenith(d.days0, lat, lon), 0.0) - inv_pi);
    o[2 * C + 1] = (float)(fmax(cos_zenith(d.days1, lat, lon), 0.0) - inv_pi);
    o[2 * C + 2] = d.statics[2 * cell];
    o[2 * C + 3] = d.statics[2 * cell + 1];
    for (int c = 2 * C + 4; c < d.ld_out; ++c) o[c] = 0.f;
}

// ---- cube conv loader: row m = face-padded cell index, k = (tap, channel) ----------------------------------------------------------- //
struct ALCube {
    static constexpr bool kDirect = false;
    const float* src0;
    const float* src1;
    const int* pad;        // [6][4][2]
    int c0, c1, cin, K, n, mode0, taps, flip, mpf;
    struct Row { int f, y, x; };           // f < 0: a padding row of the face's last tile
    struct Raw { float v[8]; };

    __device__ __forceinline__ Row row(int m) const {
        const int f = m / mpf, l = m - f * mpf;
        if (f >= 6 || l >= n * n) return Row{-1, 0, 0};
        const int y = l / n;
        return Row{f, y, l - y * n};
    }
    __device__ __forceinline__ static void add8(const float* p, float w, float (&v)[8]) {
        const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
        v[0] += w * a.x; v[1] += w * a.y; v[2] += w * a.z; v[3] += w * a.w;
        v[4] += w * b.x; v[5] += w * b.y; v[6] += w * b.z; v[7] += w * b.w;
    }
    // 8 channels from c of cell (g, y, x) at face size n, weighted by w
    __device__ __forceinline__ void add(int g, int y, int x, int c, float w, float (&v)[8]) const {
        if (c >= c0) {
            add8(src1 + ((long long)(g * n + y) * n + x) * c1 + (c - c0), w, v);
        } else if (mode0 == 0) {
            add8(src0 + ((long long)(g * n + y) * n + x) * c0 + c, w, v);
        } else if (mode0 == 1) {
            const int n2 = 2 * n;
            const float* p = src0 + ((long long)(g * n2 + 2 * y) * n2 + 2 * x) * c0 + c;
            const float q = 0.25f * w;
            add8(p, q, v);
            add8(p + c0, q, v);
            add8(p + (long long)n2 * c0, q, v);
            add8(p + (long long)(n2 + 1) * c0, q, v);
        } else {
            const int nh = n >> 1;
            add8(src0 + ((long long)(g * nh + (y >> 1)) * nh + (x >> 1)) * c0 + c, w, v);
        }
    }
    // the cell a non-corner halo cell (y, x) of face f stands for (spec.py halo_source)
    __device__ __forceinline__ void halo(int f, int y, int x, int& g, int& i, int& j) const {
        const int side = y < 0 ? 0 : (y >= n ? 1 : (x < 0 ? 2 : 3));
        g = pad[(f * 4 + side) * 2];
        const int k = pad[(f * 4 + side) * 2 + 1];
        int a = side == 0 ? n - 1 : (side == 1 ? 0 : y);
        int b = side == 2 ? n - 1 : (side == 3 ? 0 : x);
        if (k == 1) { const int t = a; a = b; b = n - 1 - t; }
        else if (k == 2) { a = n - 1 - a; b = n - 1 - b; }
        else if (k == 3) { const int t = a; a = n - 1 - b; b = t; }
        i = a;
        j = b;
    }
    __device__ __forceinline__ void issue(const Row& r, int k, Raw& o) const {
#pragma unroll
        for (int i = 0; i < 8; ++i) o.v[i] = 0.f;
        if (r.f < 0 || k >= K) return;
        const int tap = k / cin, c = k - tap * cin;
        int dy = 0, dx = 0;
        if (taps == 9) {
            dy = tap / 3 - 1;
            dx = tap - (tap / 3) * 3 - 1;
            if (r.f == flip) dy = -dy;
        }
        const int y = r.y + dy, x = r.x + dx;
        const bool yin = y >= 0 && y < n, xin = x >= 0 && x < n;
        int g, i, j;
        if (yin && xin) {
            add(r.f, y, x, c, 1.f, o.v);
        } else if (yin || xin) {
            halo(r.f, y, x, g, i, j);
            add(g, i, j, c, 1.f, o.v);
        } else {                                    // corner: mean of the two halo cells next to it
            halo(r.f, y, x < 0 ? 0 : n - 1, g, i, j);
            add(g, i, j, c, 0.5f, o.v);
            halo(r.f, y < 0 ? 0 : n - 1, x, g, i, j);
            add(g, i, j, c, 0.5f, o.v);
        }
    }
    __device__ __forceinline__ void finish(const Raw& r, float (&v)[8]) const {
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = r.v[i];
    }
    __device__ __forceinline__ uint4 direct(const Raw&) const { return make_uint4(0, 0, 0, 0); }
};

// ---- epilogue: + bias, clamped leaky ReLU, store row f n^2 + l of the face-padded row m = f mpf + l ---- //
struct EpCube {
    static constexpr bool kDualOrder = false;
    template <class TC> __device__ __forceinline__ void init(char*, int, int) const {}
    float* out;
    const float* bias;
    int nn, mpf, ldo, act;
    float slope, cmax;
    template <class TC, bool SWAP>
    __device__ __forceinline__ void run(f32x4 (&acc)[TC::FM][TC::FN], int m0w, int n0w, int lane, int, int, char*, int, int N, int) const {
        static_assert(SWAP, "swapped order: a lane holds 4 consecutive output channels of one cell");
        const int l15 = lane & 15, l4 = (lane >> 4) * 4;
#pragma unroll
        for (int a = 0; a < TC::FM; ++a) {
            const int m = m0w + a * 16 + l15;
            const int f = m / mpf, l = m - f * mpf;
            if (f >= 6 || l >= nn) continue;
            float* orow = out + (long long)(f * nn + l) * ldo;
#pragma unroll
            for (int b = 0; b < TC::FN; ++b) {
                const int n = n0w + b * 16 + l4;
                float v[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float t = acc[a][b][r] + (n + r < N ? bias[n + r] : 0.f);
                    if (act) {
                        t = t > 0.f ? t : t * slope;
                        t = t > cmax ? cmax : t;            // (NaN passes through: the non-finite check must see it)
                    }
                    v[r] = t;
                }
                if (n + 3 < N) {
                    *reinterpret_cast<float4*>(orow + n) = make_float4(v[0], v[1], v[2], v[3]);
                } else {
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (n + r < N) orow[n + r] = v[r];
                }
            }
        }
    }
};

typedef GemmArgs<PrecF16x3, ALCube, EpCube> ConvArgs;

// faces 0-3: the equatorial weights and bias; faces 4-5: the polar ones (w_polar elements / N floats further)
template <class TC>
__global__ void __launch_bounds__(TC::THREADS) cube_conv_kernel(const ConvArgs g, long long w_polar) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    ConvArgs a = g;
    if ((int)(blockIdx.y * TC::BM) / g.al.mpf >= 4) {
        a.W += w_polar;
        a.ep.bias += g.N;
    }
    gemm_body<PrecF16x3, TC, ALCube, EpCube, true>(a, smem);
}

template <class TC>
hipError_t launch_conv(const ConvArgs& g, long long w_polar, hipStream_t s) {
    dim3 grid((g.N + TC::BN - 1) / TC::BN, g.M / TC::BM);
    constexpr int smem = gemm_smem_bytes<PrecF16x3, TC>() + kEpiScratch;
    static_assert(smem <= 64 * 1024, "LDS per block");
    hipLaunchKernelGGL((cube_conv_kernel<TC>), grid, dim3(TC::THREADS), smem, s, g, w_polar);
    return hipGetLastError();
}

// ---- egress ------------------------------------------------------------------------------------------------------------------------ //
__global__ void __launch_bounds__(256) egress_kernel(const skdlwp_egress_desc d) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= d.points) return;
    const int C = d.channels;
    float acc[2 * kMaxC];
#pragma unroll
    for (int c = 0; c < 2 * kMaxC; ++c) acc[c] = 0.f;
    const int j1 = d.row_ptr[p + 1];
    for (int j = d.row_ptr[p]; j < j1; ++j) {
        const float s = d.S[j];
        const float4* y = reinterpret_cast<const float4*>(d.y + (long long)d.col[j] * d.ld_y);
#pragma unroll
        for (int q = 0; q < kMaxC / 2; ++q) {
            if (4 * q < 2 * C) {
                const float4 v = y[q];
                acc[4 * q] += s * v.x; acc[4 * q + 1] += s * v.y; acc[4 * q + 2] += s * v.z; acc[4 * q + 3] += s * v.w;
            }
        }
    }
#pragma unroll
    for (int c = 0; c < kMaxC; ++c) {
        if (c < C) {
            const float sc = d.scale[c], ctr = d.center[c];
            d.out6[c * (long long)d.points + p] = sc * acc[c] + ctr;
            d.out12[c * (long long)d.points + p] = sc * acc[C + c] + ctr;
        }
    }
}

}  // namespace skp

using namespace skp;

extern "C" {

int skdlwp_abi_version(void) { return SKDLWP_ABI_VERSION; }

const char* skdlwp_error_string(int code) {
    switch (code) {
        case 0: return "success";
        case SKDLWP_E_ARG: return "invalid argument";
        case SKDLWP_E_HIP: return "HIP runtime error";
        default: return "unknown error code";
    }
}

int skdlwp_prepare_weight(const float* src, long long sn, long long sk, int N, int K, void* dst, long long plane, int ldw, void* stream) {
    return prepare_weight_f16(src, sn, sk, N, K, dst, plane, ldw, stream, SKDLWP_E_ARG, SKDLWP_E_HIP);
}

int skdlwp_ingest(const skdlwp_ingest_desc* d, void* stream) {
    if (!d || !d->x0 || !d->x1 || !d->center || !d->inv_scale || !d->row_ptr || !d->col || !d->S || !d->lat || !d->lon || !d->statics ||
        !d->out || d->channels <= 0 || d->channels > kMaxC || d->cells <= 0 || d->points <= 0 || d->ld_out < 2 * (d->channels + 1) + 2 ||
        (d->ld_out & 7))
        return SKDLWP_E_ARG;
    hipLaunchKernelGGL(ingest_kernel, dim3((unsigned)((d->cells + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), *d);
    return hip_status(SKDLWP_E_HIP);
}

int skdlwp_conv(const skdlwp_conv_desc* d, void* stream) {
    if (!d || !d->src0 || !d->pad || !d->w || !d->bias || !d->out || d->n <= 0 || d->c0 <= 0 || (d->c0 & 7) || d->c1 < 0 || (d->c1 & 7) ||
        (d->c1 > 0 && !d->src1) || d->mode0 < 0 || d->mode0 > 2 || (d->mode0 == 2 && (d->n & 1)) || (d->taps != 9 && d->taps != 1) ||
        d->cout <= 0 || d->ld_out < d->cout || (d->ld_out & 3) || d->act < 0 || d->act > 1 || d->flip_face < -1 || d->flip_face > 5)
        return SKDLWP_E_ARG;
    const int cin = d->c0 + d->c1, K = d->taps * cin;
    if (d->ldw < K || (d->ldw & 7) || d->w_polar < (long long)d->cout * d->ldw || d->w_plane < d->w_polar + (long long)d->cout * d->ldw)
        return SKDLWP_E_ARG;
    const long long nn = (long long)d->n * d->n, mpf = (nn + kRowTile - 1) / kRowTile * kRowTile;
    if (6 * mpf >= (1ll << 31) || !aligned16(d->src0) || !aligned16(d->src1) || !aligned16(d->out)) return SKDLWP_E_ARG;
    ConvArgs g;
    g.al = ALCube{d->src0, d->src1, d->pad, d->c0, d->c1, cin, K, d->n, d->mode0, d->taps, d->flip_face, (int)mpf};
    g.ep = EpCube{d->out, d->bias, (int)nn, (int)mpf, d->ld_out, d->act, d->slope, d->clamp_max};
    g.W = static_cast<const f16*>(d->w);
    g.w_plane = d->w_plane;
    g.ldw = d->ldw;
    g.M = (int)(6 * mpf);
    g.N = d->cout;
    g.K = K;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const hipError_t e = d->cout > 64 ? launch_conv<TWide>(g, d->w_polar, s) : launch_conv<TNarrow>(g, d->w_polar, s);
    return e == hipSuccess ? 0 : SKDLWP_E_HIP;
}

int skdlwp_egress(const skdlwp_egress_desc* d, void* stream) {
    if (!d || !d->y || !d->row_ptr || !d->col || !d->S || !d->center || !d->scale || !d->out6 || !d->out12 || d->channels <= 0 ||
        d->channels > kMaxC || d->cells <= 0 || d->points <= 0 || d->ld_y < 2 * d->channels || (d->ld_y & 3) || !aligned16(d->y))
        return SKDLWP_E_ARG;
    hipLaunchKernelGGL(egress_kernel, dim3((unsigned)((d->points + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), *d);
    return hip_status(SKDLWP_E_HIP);
}

}  // extern "C"
