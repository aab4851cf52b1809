// Zonal power spectra (include/skyrim_spec.h): the members' rows through an fp32 mixed-radix FFT in LDS, the six slots in float64.
//   spec_kernel<NB, NL>  a workgroup of NL lanes walks the rows of one chunk of one channel: x_0's row to LDS, then f_0, d_y and the member pairs one
//                     complex transform after the other (spec_fft.h); lane t keeps F_0, D_y, S and the real sums of its NB bins
//                     k = t + NL b in float64 registers and adds w_j times the row's six values to the chunk's partial
//   band_kernel       sums the partials of a band's chunks in ascending order, applies c_k and divides by the band's weight sum
// Contraction to fma is off for the whole file (and on the build line): the header counts one rounding per operation.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include "../../include/skyrim_spec.h"
#include "fields.h"
#include "spec_fft.h"

#pragma clang fp contract(off)

namespace {

constexpr int LANES = 256;                 // of a workgroup: four waves
constexpr int MAX_PASS = 12;               // 2^12 = SKSPEC_MAX_W
constexpr int MAX_SEG = 2 * SKSPEC_MAX_BANDS;

struct SpecArgs {
    int M, W, K, slots;                    // slots: 3 or 6
    int n_pass, radix[MAX_PASS];
    int n_seg, n_chunks, chunk;           // chunk: rows of a chunk at most, min(SKSPEC_CHUNK, nc)
    int seg_row[MAX_SEG], seg_end[MAX_SEG], seg_chunk[MAX_SEG];      // covered segments: rows [seg_row, seg_end), first chunk
    uint32_t plane[SKSPEC_MAX_CHANNELS];   // first element of the cc-th listed channel's plane
};

struct BandArgs {
    int K, W, slots, nb, n_chunks;
    int j0[SKSPEC_MAX_BANDS], j1[SKSPEC_MAX_BANDS], c0[SKSPEC_MAX_BANDS], c1[SKSPEC_MAX_BANDS];      // rows and chunks of a band
};

using namespace skfields;

// all passes of one transform, planes (re0, im0) -> ... ; returns with the result in (re0, im0) when n_pass is even, else in (re1, im1)
template <int NL>
__device__ __forceinline__ void transform(const SpecArgs& a, float* re0, float* im0, float* re1, float* im1, const float* __restrict__ tw) {
    int Ns = 1;
    for (int p = 0; p < a.n_pass; ++p) {
        const int R = a.radix[p];
        const float* ir = (p & 1) ? re1 : re0;
        const float* ii = (p & 1) ? im1 : im0;
        float* orr = (p & 1) ? re0 : re1;
        float* oi = (p & 1) ? im0 : im1;
        const int n = a.W / R;
        __syncthreads();                                                   // the planes read here are complete
        if (R == 4)
            for (int j = threadIdx.x; j < n; j += NL) spec_butterfly<4>(ir, ii, orr, oi, tw, a.W, Ns, j);
        else if (R == 2)
            for (int j = threadIdx.x; j < n; j += NL) spec_butterfly<2>(ir, ii, orr, oi, tw, a.W, Ns, j);
        else if (R == 3)
            for (int j = threadIdx.x; j < n; j += NL) spec_butterfly<3>(ir, ii, orr, oi, tw, a.W, Ns, j);
        else
            for (int j = threadIdx.x; j < n; j += NL) spec_butterfly<5>(ir, ii, orr, oi, tw, a.W, Ns, j);
        Ns *= R;
    }
    __syncthreads();
}

// the spectra A and B of the real sequences a and b from Z = FFT(a + i b), at bin k, scaled by 1/W: float64 throughout
__device__ __forceinline__ void split(const float* re, const float* im, int W, int k, double half_inv, double& ar, double& ai, double& br, double& bi) {
    const int kc = k == 0 ? 0 : W - k;
    const double zr = re[spec_pad(k)], zi = im[spec_pad(k)], cr = re[spec_pad(kc)], ci = im[spec_pad(kc)];
    ar = (zr + cr) * half_inv;
    ai = (zi - ci) * half_inv;
    br = (zi + ci) * half_inv;
    bi = (cr - zr) * half_inv;
}

template <int NB, int NL>
__global__ void __launch_bounds__(NL) spec_kernel(const SpecArgs a, const float* const* __restrict__ members, const float* __restrict__ truth,
                                                     const double* __restrict__ lat_weight, const float* __restrict__ tw, double* __restrict__ partial) {
    extern __shared__ float lds[];
    const int P = spec_pad(a.W - 1) + 1;                                   // words of a plane
    float* x0row = lds;
    float* re0 = lds + P;
    float* im0 = re0 + P;
    float* re1 = im0 + P;
    float* im1 = re1 + P;
    const float* rr = (a.n_pass & 1) ? re1 : re0;                          // where a transform's result lies
    const float* ri = (a.n_pass & 1) ? im1 : im0;
    const int tid = threadIdx.x;
    const int chunk = blockIdx.x;
    int seg = 0;
    for (int s = 1; s < a.n_seg; ++s)
        if (chunk >= a.seg_chunk[s]) seg = s;
    const int row0 = a.seg_row[seg] + (chunk - a.seg_chunk[seg]) * a.chunk;
    const int row1 = min(row0 + a.chunk, a.seg_end[seg]);
    const uint32_t plane = a.plane[blockIdx.y];
    const float* x0p = members[0];
    const double half_inv = 0.5 / (double)a.W;
    const double Md = (double)a.M;
    double* dst = partial + ((size_t)blockIdx.y * (size_t)a.n_chunks + (size_t)chunk) * (size_t)(a.slots * a.K);

    for (int j = row0; j < row1; ++j) {
        const uint32_t base = plane + (uint32_t)j * (uint32_t)a.W;
        double f0r[NB], f0i[NB], dyr[NB], dyi[NB], sr[NB], si[NB], q[NB], am[NB], ae[NB];
        const float first = load_vec<1>(x0p, base);
        __syncthreads();                                                   // the last row's reads of the planes are done
        for (int i = tid; i < a.W; i += NL) {
            const float v = load_vec<1>(x0p, base + i);
            x0row[i] = v;
            re0[spec_pad(i)] = v - first;
            im0[spec_pad(i)] = 0.f;
        }
        transform<NL>(a, re0, im0, re1, im1, tw);
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            const int k = tid + NL * b;
            double t0, t1;
            f0r[b] = f0i[b] = 0.0;
            if (k < a.K) split(rr, ri, a.W, k, half_inv, f0r[b], f0i[b], t0, t1);
            if (k == 0) f0r[b] = f0r[b] + (double)first;
            dyr[b] = dyi[b] = sr[b] = si[b] = q[b] = 0.0;
        }
        if (truth) {
            __syncthreads();
            for (int i = tid; i < a.W; i += NL) {
                re0[spec_pad(i)] = load_vec<1>(truth, base + i) - x0row[i];
                im0[spec_pad(i)] = 0.f;
            }
            transform<NL>(a, re0, im0, re1, im1, tw);
#pragma unroll
            for (int b = 0; b < NB; ++b) {
                const int k = tid + NL * b;
                double t0, t1;
                if (k < a.K) split(rr, ri, a.W, k, half_inv, dyr[b], dyi[b], t0, t1);
            }
        }
#pragma unroll
        for (int b = 0; b < NB; ++b) {                                     // member 0: D_0 = 0
            am[b] = f0r[b] * f0r[b] + f0i[b] * f0i[b];
            ae[b] = dyr[b] * dyr[b] + dyi[b] * dyi[b];
        }
        for (int m = 1; m < a.M; m += 2) {
            const bool two = m + 1 < a.M;
            const float* xa = members[m];
            const float* xb = members[two ? m + 1 : m];
            __syncthreads();
            for (int i = tid; i < a.W; i += NL) {
                const float va = load_vec<1>(xa, base + i), vb = load_vec<1>(xb, base + i), v0 = x0row[i];
                re0[spec_pad(i)] = va - v0;
                im0[spec_pad(i)] = two ? vb - v0 : 0.f;
            }
            transform<NL>(a, re0, im0, re1, im1, tw);
#pragma unroll
            for (int b = 0; b < NB; ++b) {
                const int k = tid + NL * b;
                if (k < a.K) {
                    double dr[2], di[2];
                    split(rr, ri, a.W, k, half_inv, dr[0], di[0], dr[1], di[1]);
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        if (h == 0 || two) {
                            const double gr = f0r[b] + dr[h], gi = f0i[b] + di[h];
                            const double er = dr[h] - dyr[b], ei = di[h] - dyi[b];
                            am[b] = am[b] + (gr * gr + gi * gi);
                            ae[b] = ae[b] + (er * er + ei * ei);
                            q[b] = q[b] + (dr[h] * dr[h] + di[h] * di[h]);
                            sr[b] = sr[b] + dr[h];
                            si[b] = si[b] + di[h];
                        }
                    }
                }
            }
        }
        const double w = lat_weight[j];
        const bool store = j == row0;
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            const int k = tid + NL * b;
            if (k < a.K) {
                const double mr = sr[b] / Md, mi = si[b] / Md;
                const double gr = f0r[b] + mr, gi = f0i[b] + mi;
                double v[SKSPEC_SLOTS];
                v[0] = am[b] / Md;
                v[1] = gr * gr + gi * gi;
                v[2] = a.M > 1 ? (q[b] - (sr[b] * sr[b] + si[b] * si[b]) / Md) / (Md - 1.0) : 0.0;
                const double tr = f0r[b] + dyr[b], ti = f0i[b] + dyi[b];
                const double er = mr - dyr[b], ei = mi - dyi[b];
                v[3] = tr * tr + ti * ti;
                v[4] = er * er + ei * ei;
                v[5] = ae[b] / Md;
#pragma unroll
                for (int s = 0; s < SKSPEC_SLOTS; ++s) {
                    if (s < a.slots) {
                        double* p = dst + (size_t)s * (size_t)a.K + k;
                        const double add = v[s] * w;
                        *p = store ? add : *p + add;
                    }
                }
            }
        }
    }
}

// out[cc][b][slot][k] = c_k (sum over the band's chunks, ascending) / (sum of the band's weights).  grid: (ceil(K / 256), nb * slots, nc)
__global__ void __launch_bounds__(LANES) band_kernel(const BandArgs a, const double* __restrict__ lat_weight, const double* __restrict__ partial,
                                                     double* __restrict__ out) {
    __shared__ double wpart[64];
    __shared__ double wsum;
    const int b = blockIdx.y / a.slots, s = blockIdx.y - b * a.slots, cc = blockIdx.z;
    if (threadIdx.x < 64) {
        double t = 0.0;
        for (int j = a.j0[b] + (int)threadIdx.x; j < a.j1[b]; j += 64) t = t + lat_weight[j];
        wpart[threadIdx.x] = t;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = wpart[0];
        for (int l = 1; l < 64; ++l) t = t + wpart[l];
        wsum = t;
    }
    __syncthreads();
    const int k = blockIdx.x * LANES + threadIdx.x;
    if (k >= a.K) return;
    const size_t step = (size_t)(a.slots * a.K);
    const double* src = partial + (size_t)cc * (size_t)a.n_chunks * step + (size_t)s * (size_t)a.K + k;
    double t = src[(size_t)a.c0[b] * step];
    for (int c = a.c0[b] + 1; c < a.c1[b]; ++c) t = t + src[(size_t)c * step];
    const double ck = (k == 0 || 2 * k == a.W) ? 1.0 : 2.0;
    out[(((size_t)cc * a.nb + b) * a.slots + s) * (size_t)a.K + k] = ck * t / wsum;
}

struct Plan {
    SpecArgs s;
    BandArgs b;
    int nbins;                             // bins per lane the kernel is instantiated on
    size_t bytes, lds;
};

// the refusals that skspec_workspace_bytes shares with skspec_run, and the segments and chunks of the bands
bool plan(const skspec_desc* d, Plan* p) {
    if (!d || d->M < 1 || d->M > SKSPEC_MAX_MEMBERS || d->nc < 1 || d->nc > SKSPEC_MAX_CHANNELS || d->nb < 1 || d->nb > SKSPEC_MAX_BANDS) return false;
    if (d->H < 1 || d->H > SKSPEC_MAX_H || d->W < SKSPEC_MIN_W || d->W > SKSPEC_MAX_W) return false;
    SpecArgs& s = p->s;
    BandArgs& b = p->b;
    s = SpecArgs{};
    b = BandArgs{};
    s.n_pass = spec_factor(d->W, s.radix);
    if (s.n_pass == 0) return false;
    int edge[MAX_SEG], ne = 0;
    for (int k = 0; k < d->nb; ++k) {
        if (d->j0[k] < 0 || d->j1[k] <= d->j0[k] || d->j1[k] > d->H) return false;
        edge[ne++] = d->j0[k];
        edge[ne++] = d->j1[k];
    }
    for (int i = 1; i < ne; ++i)                                           // insertion sort, then the distinct edges
        for (int k = i; k > 0 && edge[k - 1] > edge[k]; --k) { const int t = edge[k]; edge[k] = edge[k - 1]; edge[k - 1] = t; }
    int nu = 1;
    for (int i = 1; i < ne; ++i)
        if (edge[i] != edge[nu - 1]) edge[nu++] = edge[i];
    int chunks = 0;
    s.chunk = d->nc < SKSPEC_CHUNK ? d->nc : SKSPEC_CHUNK;                 // fewer channels, shorter chunks: one channel still fills the device
    for (int i = 0; i + 1 < nu; ++i) {
        bool covered = false;
        for (int k = 0; k < d->nb; ++k) covered = covered || (d->j0[k] <= edge[i] && edge[i + 1] <= d->j1[k]);
        if (!covered) continue;
        s.seg_row[s.n_seg] = edge[i];
        s.seg_end[s.n_seg] = edge[i + 1];
        s.seg_chunk[s.n_seg] = chunks;
        ++s.n_seg;
        chunks += (edge[i + 1] - edge[i] + s.chunk - 1) / s.chunk;
    }
    s.n_chunks = chunks;
    s.M = d->M; s.W = d->W; s.K = d->W / 2 + 1; s.slots = d->truth ? SKSPEC_SLOTS : 3;
    b.K = s.K; b.W = d->W; b.slots = s.slots; b.nb = d->nb; b.n_chunks = chunks;
    for (int k = 0; k < d->nb; ++k) {                                      // a band is a run of covered segments: a run of chunks
        b.j0[k] = d->j0[k];
        b.j1[k] = d->j1[k];
        b.c1[k] = chunks;
        for (int i = 0; i < s.n_seg; ++i) {
            if (s.seg_row[i] == d->j0[k]) b.c0[k] = s.seg_chunk[i];
            if (s.seg_end[i] == d->j1[k]) b.c1[k] = i + 1 < s.n_seg ? s.seg_chunk[i + 1] : chunks;
        }
    }
    p->nbins = s.K <= LANES ? 1 : (s.K <= 3 * LANES ? 3 : 5);      // 5: over 512 lanes
    p->bytes = (size_t)d->nc * (size_t)chunks * (size_t)(s.slots * s.K) * sizeof(double);
    p->lds = (size_t)5 * (size_t)(spec_pad(d->W - 1) + 1) * sizeof(float);
    return true;
}

// every refusal of skspec_run: nothing here touches the GPU
bool valid(const skspec_desc* d, Plan* p) {
    if (!plan(d, p)) return false;
    if (!d->members || ((uintptr_t)d->members & 7) || (d->truth && ((uintptr_t)d->truth & 3))) return false;
    if (d->C < 1) return false;
    const size_t lim = (size_t)1 << 30, HW = (size_t)d->H * (size_t)d->W;
    if (HW > lim || (size_t)d->C > lim / HW) return false;
    for (int k = 0; k < d->nc; ++k)
        if (d->channels[k] < 0 || d->channels[k] >= d->C) return false;
    if (!d->lat_weight || ((uintptr_t)d->lat_weight & 7) || !d->twiddles || ((uintptr_t)d->twiddles & 7)) return false;
    if (!d->out || ((uintptr_t)d->out & 7)) return false;
    if (!d->workspace || ((uintptr_t)d->workspace & 7) || d->workspace_bytes < p->bytes) return false;
    return true;
}

}  // namespace

extern "C" int skspec_abi_version(void) { return SKSPEC_ABI_VERSION; }

extern "C" int skspec_twiddles(int W, float* tw) {
    int radix[MAX_PASS];
    if (!tw || W < SKSPEC_MIN_W || W > SKSPEC_MAX_W || spec_factor(W, radix) == 0) return SKSPEC_E_ARG;
    const double step = 6.283185307179586476925286766559 / (double)W;
    for (int n = 0; n < W; ++n) {
        tw[2 * n] = (float)std::cos(step * (double)n);
        tw[2 * n + 1] = (float)-std::sin(step * (double)n);
    }
    return 0;
}

extern "C" double skspec_bound_factor(int W) {
    int radix[MAX_PASS];
    if (W < SKSPEC_MIN_W || W > SKSPEC_MAX_W) return 0.0;
    const int n = spec_factor(W, radix);
    double c = 0.0;
    for (int p = 0; p < n; ++p) {
        const int R = radix[p];
        const double rho = R == 2 ? 1.0 : (R == 4 ? 2.0 : (R == 3 ? 5.25 : 7.25));
        c += 3.25 + std::sqrt((double)R) * rho;
    }
    return 1.02 * c;
}

extern "C" size_t skspec_workspace_bytes(const skspec_desc* d) {
    Plan p;
    return plan(d, &p) ? p.bytes : 0;
}

extern "C" int skspec_run(const skspec_desc* d, void* stream) {
    Plan p;
    if (!valid(d, &p)) return SKSPEC_E_ARG;
    hipStream_t s = (hipStream_t)stream;
    for (int k = 0; k < d->nc; ++k) p.s.plane[k] = (uint32_t)d->channels[k] * (uint32_t)d->H * (uint32_t)d->W;
    double* partial = (double*)d->workspace;
    const dim3 grid((unsigned)p.s.n_chunks, (unsigned)d->nc);
    if (p.nbins == 1)
        hipLaunchKernelGGL((spec_kernel<1, LANES>), grid, dim3(LANES), p.lds, s, p.s, d->members, d->truth, d->lat_weight, d->twiddles, partial);
    else if (p.nbins == 3)
        hipLaunchKernelGGL((spec_kernel<3, LANES>), grid, dim3(LANES), p.lds, s, p.s, d->members, d->truth, d->lat_weight, d->twiddles, partial);
    else {
        // more than 64 KiB of dynamic LDS (W > 3276) has to be asked for
        if (p.lds > 65536 && hipFuncSetAttribute((const void*)spec_kernel<5, 2 * LANES>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds) != hipSuccess)
            return SKSPEC_E_HIP;
        hipLaunchKernelGGL((spec_kernel<5, 2 * LANES>), grid, dim3(2 * LANES), p.lds, s, p.s, d->members, d->truth, d->lat_weight, d->twiddles, partial);
    }
    if (hipGetLastError() != hipSuccess) return SKSPEC_E_HIP;
    const dim3 bgrid((unsigned)((p.s.K + LANES - 1) / LANES), (unsigned)(d->nb * p.s.slots), (unsigned)d->nc);
    hipLaunchKernelGGL(band_kernel, bgrid, dim3(LANES), 0, s, p.b, d->lat_weight, partial, d->out);
    return hipGetLastError() == hipSuccess ? 0 : SKSPEC_E_HIP;
}
