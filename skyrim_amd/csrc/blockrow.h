// What the block kernels (fused_block.hip) share whatever the number of MFMA terms: the argument block, the sizes that follow from C, the
// register ring through which weight fragments leave LDS, and the stages whose code does not depend on where it is compiled -- table fill,
// row gather, GELU + split of a hidden chunk (sfno_chain.hip's too), launch.
//
// NOT here: the two LayerNorm stages (between projection and MLP, and the epilogue).  Their fp32 expressions are contracted by default, and
// which multiply fuses with which add is decided per element by the vectoriser from the instruction order it finds: in the kernels,
// y - s / C is an fma on most elements (the mean is never rounded) and a packed subtract of the rounded mean on the last few.  As a
// function (forceinline, any signature tried) the stage is simplified on its own before it is inlined, the order differs, no q += d * d
// fuses any more, and the engine's bits move (docs/experiments.md, "Pangu block kernels on shared stages").  Only text compiled IN the
// kernel keeps them.  gfx950 only.
#pragma once
#include "gemm_dma.h"

namespace skp {

template <class T>
struct BlockArgs {
    const T* ao; long long ao_plane;       // attention output, window-ordered rows, blocked layout [rows/16][C/32][16][32], hi / lo planes
    int M;                                 // stream tokens (multiple of 16)
    T* xs; long long xs_plane;             // residual stream planes, blocked layout
    const int* winv;                       // stream token -> window row of the attention output
    const T *projf, *w1f, *w2f;            // fragment-order weights (prep_rowtile_weights, prep_mlp_weights): hi / lo planes for three terms, planes = 1 (hi only) otherwise
    const float *proj_b, *g1, *e1, *b1, *b2, *g2, *e2;
    float eps;
};

// the sizes that follow from C, and the float table in LDS: proj bias, norm1 gamma / beta, fc1 bias, fc2 bias, norm2 gamma / beta
template <int C_>
struct BlockDims {
    static constexpr int C = C_, KS = C / 32, CF = C / 16, HID = 4 * C, NCH = HID / 32;
    static constexpr int NPB = C / 32;                // projection: blocks of 32 output columns
    static constexpr int T_PB = 0, T_G1 = C, T_E1 = 2 * C, T_B1 = 3 * C, T_B2 = 3 * C + HID, T_G2 = T_B2 + C, T_E2 = T_G2 + C;
    static constexpr int TAB = T_E2 + C;
};

// two consecutive 1 KiB fragments; the scheduling barrier pins the reads HERE in program order, ahead of the MFMAs that follow (fused_mlp.hip)
__device__ __forceinline__ void sk_ld2(const char* p, uint4 (&w)[2]) {
    w[0] = *reinterpret_cast<const uint4*>(p);
    w[1] = *reinterpret_cast<const uint4*>(p + 1024);
    __builtin_amdgcn_sched_barrier(0);
}

// NP fragment pairs at consecutive KiB of `st`, through a ring of RD register pairs read RD - 1 pairs ahead of their MFMAs
template <int NP, int RD, class Body>
__device__ __forceinline__ void sk_stream(const char* st, Body&& body) {
    uint4 ring[RD][2];
#pragma unroll
    for (int p = 0; p < RD - 1 && p < NP; ++p) sk_ld2(st + (p << 11), ring[p % RD]);
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        if (p + RD - 1 < NP) sk_ld2(st + ((p + RD - 1) << 11), ring[(p + RD - 1) % RD]);
        body(p, ring[p % RD][0], ring[p % RD][1]);
        __builtin_amdgcn_sched_barrier(0);
    }
}

template <class S, class T>
__device__ __forceinline__ void blk_fill_tables(float* tab, const BlockArgs<T>& a, int tid) {
    for (int i = tid; i < S::C; i += S::THREADS) {
        tab[S::T_PB + i] = a.proj_b[i]; tab[S::T_G1 + i] = a.g1[i]; tab[S::T_E1 + i] = a.e1[i];
        tab[S::T_B2 + i] = a.b2[i]; tab[S::T_G2 + i] = a.g2[i]; tab[S::T_E2 + i] = a.e2[i];
    }
    for (int i = tid; i < S::HID; i += S::THREADS) tab[S::T_B1 + i] = a.b1[i];
}

// the attention rows of the wave's tokens (row blocks rb0 .. rb0 + FM - 1) as B-operand fragments (gathered: 16 bytes per lane, 64 bytes per
// row and k-step).  LO = false: the lo plane of the attention output is not read at all, xl is zeros nobody reads
template <class S, bool LO, class T>
__device__ __forceinline__ void blk_gather_rows(const BlockArgs<T>& a, long long rb0, int l15, int g, typename OpT<T>::v8 (&xh)[S::FM][S::KS],
                                                typename OpT<T>::v8 (&xl)[S::FM][S::KS], bool (&live)[S::FM]) {
    typedef typename OpT<T>::v8 v8;
#pragma unroll
    for (int t = 0; t < S::FM; ++t) {
        live[t] = (rb0 + t) * 16 < a.M;
        const int src = live[t] ? a.winv[(rb0 + t) * 16 + l15] : 0;
        const T* p = a.ao + blk_off(src, g * 8, S::C);
#pragma unroll
        for (int ks = 0; ks < S::KS; ++ks) {
            xh[t][ks] = *reinterpret_cast<const v8*>(p + (ks << 9));
            if constexpr (LO) xl[t][ks] = *reinterpret_cast<const v8*>(p + (ks << 9) + a.ao_plane);
            else xl[t][ks] = v8{};
        }
    }
#pragma unroll
    for (int t = 0; t < S::FM; ++t) {           // consumed once here: hipcc's vmcnt waits for these loads sit BEFORE the loops (fused_mlp.hip)
#pragma unroll
        for (int ks = 0; ks < S::KS; ++ks) {
            asm volatile("" : "+v"(xh[t][ks]));
            if constexpr (LO) asm volatile("" : "+v"(xl[t][ks]));           // (zeros: no registers are pinned for them)
        }
    }
}

// bias + GELU + hi/lo split of hidden chunk j: the lane's 8 hidden units 16 n + 4 g + r become k-slots 8 g + 4 n + r of the contracting layer
template <class T, int FM>
__device__ __forceinline__ void blk_gelu_split(const f32x4 (&hacc)[FM][2], const float* b1, int j, int g, uint4 (&hh)[FM], uint4 (&hl)[FM]) {
    const float4 bb0 = *reinterpret_cast<const float4*>(b1 + j * 32 + 4 * g), bb1 = *reinterpret_cast<const float4*>(b1 + j * 32 + 16 + 4 * g);
#pragma unroll
    for (int t = 0; t < FM; ++t) {
        const f32x2 a0 = gelu_erf2(f32x2{hacc[t][0][0] + bb0.x, hacc[t][0][1] + bb0.y}), a1 = gelu_erf2(f32x2{hacc[t][0][2] + bb0.z, hacc[t][0][3] + bb0.w});
        const f32x2 a2 = gelu_erf2(f32x2{hacc[t][1][0] + bb1.x, hacc[t][1][1] + bb1.y}), a3 = gelu_erf2(f32x2{hacc[t][1][2] + bb1.z, hacc[t][1][3] + bb1.w});
        const float v[8] = {a0.x, a0.y, a1.x, a1.y, a2.x, a2.y, a3.x, a3.y};
        uint4 o[2];
        split8<T, 2>(v, o);
        hh[t] = o[0]; hl[t] = o[1];
    }
}

// one workgroup per S::BM stream tokens
template <auto Kernel, class S, class T>
hipError_t launch_rows(const BlockArgs<T>& a, hipStream_t s) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, S::SMEM);
    if (e != hipSuccess) return e;
    const unsigned grid = (unsigned)((a.M + S::BM - 1) / S::BM);
    if (grid == 0) return hipSuccess;
    hipLaunchKernelGGL(Kernel, dim3(grid), dim3(S::THREADS), S::SMEM, s, a);
    return hipGetLastError();
}

}  // namespace skp
