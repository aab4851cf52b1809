// Everything of an EarthSpecificBlock that follows the attention, as ONE kernel, in place on the residual planes:
//
//     x[t] <- x_mid + LayerNorm(norm2)( fc2( GELU( fc1( x_mid ) ) ) ),      x_mid = x[t] + LayerNorm(norm1)( ao[win(t)] Wp^T + b )
//
// t runs over the stream's tokens, win(t) = the inverse of the window table (window reverse + un-roll + crop as a GATHER of the
// attention output's rows: the stream itself is read and written in whole 1 KiB blocks, and the tile count is that of the tokens --
// 1024 tiles = 4 full rounds of the 256 CUs at 91 x 180 x 8, where the 5.5 % of padded window rows would make it 1080 = 5 rounds).
// It is a projection in the row-tile form of rowtile.hip followed by fused_mlp.hip's MLP on the same register-resident rows:
//
//   phase 1  projection: the wave's FM x 16 attention rows are MFMA B-operand fragments (hi / lo planes), the weights stream through
//            LDS in blocks of 32 output columns (two stages, one barrier per block), the C outputs of a row end up in its lane quad's
//            accumulators.
//   between  + bias, LayerNorm (in-lane sums + two shuffles), + the gathered residual row: with the perm8 row order of the prepared
//            weights the accumulators of fragment pair bp are columns 32 bp + 8 (lane >> 4) + [0..7] -- after the hi / lo split they
//            ARE input fragment bp of the MLP.  x_mid never exists in HBM.
//   phase 2  MLP exactly as fused_mlp.hip (hidden in 32-unit chunks, fc1 block in stage 0, fc2 block in stage 1 -- the projection's
//            two stages), epilogue + fc2 bias, LayerNorm, + x_mid from registers, stored as whole 1 KiB blocks.
//
// Against the two kernels it replaces: the stream is read once and written once per block instead of twice (8 of 20 bytes per
// element), one launch less, and the projection's MFMAs run inside a compute-bound kernel instead of an HBM-bound one.
//
// Two entry points.  They share the argument block, the register ring and the stages of blockrow.h (table fill, row gather, GELU + split,
// launch) and differ in their GEMM terms, their DMA and their workgroup shape.  The two LayerNorm stages (between, epilogue) are the same
// text in both and stay IN the kernels: blockrow.h says why.
//
// proj_mlp_kernel, THREE terms (wl xh + wh xl + wh xh, weights as hi / lo planes): bf16x3, term_plan 0, and what the load-time guard falls
// back to.  C = 192 two 4-wave workgroups per CU with 32 rows per wave, C = 384 one 8-wave workgroup; a three-deep register ring.
//
// proj_mlp2_kernel, TWO terms
//
//     A W^T  ~  A_hi W_hi^T + A_lo W_hi^T          (activations stay hi/lo pairs, the weights are ONE fp16 plane)
//
// Why two terms.  The prepared weights are constants; rounding them to 11 significant bits perturbs the model by 2^-12 relative per
// weight (measured on the oracle with exactly this plan -- proj, fc1, fc2 weights rounded, QKV activation rounded: 4.2e-4 per-channel
// error after one step, 5.3e-4 after four, bar 1e-3).  It removes a third of the MFMAs, HALF of the bytes that cross LDS
// (the token tile lives in registers, only weights stream through LDS) and half of the LDS-DMA traffic.
//
// Its launch shape: 4-wave workgroups, TWO per CU (one wave of each on every SIMD), two LDS slots of one chunk each and two barriers per
// 32-unit chunk:  | fc1(j) | GELU(j) | fc2(j) |.  The hi-only chunk is 24 KB at C = 384, so two workgroups fit a CU where the three-term
// kernel fits one; the two run free of each other and drift out of phase, so that one's GELU / LayerNorm / row I/O runs under the
// other's MFMAs.  What else was measured -- one 8-wave workgroup with a five-slot ring, its halves half a chunk apart, four
// accumulator chains, a one-wave-per-SIMD form with 32 / 64 rows per wave, software pipelining inside the wave, and the per-phase timing
// probes -- is in docs/experiments.md; none of it is in the tree.
//
// ONE (term-plan bits 8-11): the ACTIVATION operands too as one fp16 plane -- A_hi W only: attention output, mid-block stream and hidden
// activation are rounded to fp16 where they enter a GEMM (the residual path keeps the hi/lo pair), the attention output's lo plane is
// neither written nor read.  Half of the two-term form's MFMAs; meant for weights rounded with error feedback against these very operands
// (pangu/calibration.py), which is what pays for the activation rounding.
// gfx950 only.
#include <cstdlib>
#include "blockrow.h"
#include "launchers.h"

namespace skp {

template <int C_, int FM_, int NWAVES_, int WPE_>
struct BlockShape : BlockDims<C_> {
    using D = BlockDims<C_>;
    static constexpr int FM = FM_, NWAVES = NWAVES_, THREADS = 64 * NWAVES_, WPE = WPE_, BM = NWAVES * FM * 16;
    static constexpr int P_BLK = D::KS * 2 * 2;       // KiB per projection block / per fc1 chunk: [ks][n][plane]
    static constexpr int W2_BLK = D::CF * 2;          // KiB per fc2 chunk: [c][plane]
    static constexpr int STAGE = P_BLK * 1024;
    static constexpr int SMEM = 2 * STAGE + D::TAB * 4;
    static_assert(P_BLK % NWAVES == 0 && W2_BLK % NWAVES == 0 && W2_BLK == P_BLK && D::NPB % 2 == 0, "stages: equal size, even block count, whole DMA blocks per wave");
    static_assert(SMEM <= 160 * 1024, "LDS");
};

template <class T, class S>
__global__ void __launch_bounds__(S::THREADS) __attribute__((amdgpu_waves_per_eu(S::WPE, S::WPE)))
proj_mlp_kernel(const BlockArgs<T> a) {
    constexpr int C = S::C, FM = S::FM, KS = S::KS, CF = S::CF, NCH = S::NCH, NPB = S::NPB, NWAVES = S::NWAVES, RD = 3;
    typedef typename OpT<T>::v8 v8;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* tab = reinterpret_cast<float*>(smem + 2 * S::STAGE);
    const int tid = threadIdx.x, lane = tid & 63, l15 = lane & 15, g = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const unsigned lds_base = (unsigned)(size_t)smem;
    char* st0 = smem;                              // ring reads are st + lane * 16: with the lane offset as the base and the stage added to it,
    char* st1 = smem + S::STAGE;                   // C = 384 rebuilds LDS addresses past the 64 KiB immediate range and spills 150 bytes more

    auto dma = [&](const T* src_blocks, unsigned dst) {             // P_BLK consecutive KiB -> one stage, block b by wave b % NWAVES
        const T* src = src_blocks + lane * 8;
#pragma unroll
        for (int i = 0; i < S::P_BLK / NWAVES; ++i) {
            const int b = wave + i * NWAVES;
            glds16(src + (b << 9), dst + (unsigned)(b << 10));
        }
    };
    dma(a.projf, lds_base);
    blk_fill_tables<S>(tab, a, tid);

    const long long rb0 = (long long)blockIdx.x * (S::BM / 16) + wave * FM;
    v8 xh[FM][KS], xl[FM][KS];
    bool live[FM];
    blk_gather_rows<S, true>(a, rb0, l15, g, xh, xl, live);

    f32x4 yacc[FM][CF];
#pragma unroll
    for (int t = 0; t < FM; ++t)
#pragma unroll
        for (int c = 0; c < CF; ++c) yacc[t][c] = f32x4{0.f, 0.f, 0.f, 0.f};

    // ---- phase 1: projection, blocks of 32 output columns alternating between the two stages ------------------------------- //
#pragma unroll
    for (int j = 0; j < NPB; ++j) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();                               // block j landed; every wave is done with block j - 1
        if (j + 1 < NPB) dma(a.projf + ((long long)(j + 1) * S::P_BLK << 9), lds_base + (unsigned)(((j + 1) & 1) * S::STAGE));
        else dma(a.w1f, lds_base);                     // NPB is even: the last block sits in stage 1, stage 0 is free for fc1's chunk 0
        sk_stream<KS * 2, RD>(((j & 1) ? st1 : st0) + lane * 16, [&](int s, const uint4& wh, const uint4& wl) {      // pairs [ks][n] of (hi, lo)
            const int ks = s >> 1, c = 2 * j + (s & 1);
#pragma unroll
            for (int t = 0; t < FM; ++t) yacc[t][c] = OpT<T>::mfma(as_v8<T>(wl), xh[t][ks], yacc[t][c]);
#pragma unroll
            for (int t = 0; t < FM; ++t) yacc[t][c] = OpT<T>::mfma(as_v8<T>(wh), xl[t][ks], yacc[t][c]);
#pragma unroll
            for (int t = 0; t < FM; ++t) yacc[t][c] = OpT<T>::mfma(as_v8<T>(wh), xh[t][ks], yacc[t][c]);
        });
    }

    // ---- between: x_mid = x + LayerNorm(yacc + bias) -> the MLP's input fragments (the attention fragments are dead) ----------- //
#pragma unroll
    for (int t = 0; t < FM; ++t) {
        const T* old = a.xs + ((live[t] ? rb0 + t : 0) * KS << 9) + l15 * 32 + g * 8;
        v8 oh[KS], ol[KS];
#pragma unroll
        for (int bp = 0; bp < KS; ++bp) {
            oh[bp] = *reinterpret_cast<const v8*>(old + (bp << 9));
            ol[bp] = *reinterpret_cast<const v8*>(old + (bp << 9) + a.xs_plane);
        }
        float s = 0.f;
#pragma unroll
        for (int bp = 0; bp < KS; ++bp) {
            const int n = 32 * bp + 8 * g;
            const float4 b0 = *reinterpret_cast<const float4*>(tab + S::T_PB + n), b1 = *reinterpret_cast<const float4*>(tab + S::T_PB + n + 4);
            add8(yacc[t][2 * bp], yacc[t][2 * bp + 1], b0, b1);
#pragma unroll
            for (int r = 0; r < 4; ++r) s += yacc[t][2 * bp][r] + yacc[t][2 * bp + 1][r];
        }
        s += __shfl_xor(s, 16);
        s += __shfl_xor(s, 32);
        const float mean = s * (1.0f / C);
        float q = 0.f;
#pragma unroll
        for (int c = 0; c < CF; ++c)
#pragma unroll
            for (int r = 0; r < 4; ++r) { const float d = yacc[t][c][r] - mean; q += d * d; }
        q += __shfl_xor(q, 16);
        q += __shfl_xor(q, 32);
        const float rstd = rsqrtf(q * (1.0f / C) + a.eps);
#pragma unroll
        for (int bp = 0; bp < KS; ++bp) {
            const int n = 32 * bp + 8 * g;
            const float4 g0 = *reinterpret_cast<const float4*>(tab + S::T_G1 + n), g1 = *reinterpret_cast<const float4*>(tab + S::T_G1 + n + 4);
            const float4 e0 = *reinterpret_cast<const float4*>(tab + S::T_E1 + n), e1 = *reinterpret_cast<const float4*>(tab + S::T_E1 + n + 4);
            const f32x4 &x = yacc[t][2 * bp], &z = yacc[t][2 * bp + 1];
            const float y[8] = {(x[0] - mean) * rstd * g0.x + e0.x, (x[1] - mean) * rstd * g0.y + e0.y, (x[2] - mean) * rstd * g0.z + e0.z, (x[3] - mean) * rstd * g0.w + e0.w,
                                (z[0] - mean) * rstd * g1.x + e1.x, (z[1] - mean) * rstd * g1.y + e1.y, (z[2] - mean) * rstd * g1.z + e1.z, (z[3] - mean) * rstd * g1.w + e1.w};
            float v[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) v[i] = ((float)oh[bp][i] + (float)ol[bp][i]) + y[i];
            uint4 o[2];
            split8<T, 2>(v, o);
            xh[t][bp] = as_v8<T>(o[0]);
            xl[t][bp] = as_v8<T>(o[1]);
        }
#pragma unroll
        for (int c = 0; c < CF; ++c) yacc[t][c] = f32x4{0.f, 0.f, 0.f, 0.f};
    }

    // ---- phase 2: the MLP of fused_mlp.hip on x_mid (plain schedule: fc1(j) | GELU(j) | fc2(j), two barriers per chunk) ---------- //
    const unsigned ldsA = lds_base, ldsB = lds_base + S::STAGE;
    for (int j = 0; j < NCH; ++j) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();                               // fc1 block j landed; every wave is done with fc2 block j - 1 (j = 0: with the projection)
        dma(a.w2f + ((long long)j * S::W2_BLK << 9), ldsB);         // (W2_BLK == P_BLK)
        f32x4 hacc[FM][2];
#pragma unroll
        for (int t = 0; t < FM; ++t) { hacc[t][0] = f32x4{0.f, 0.f, 0.f, 0.f}; hacc[t][1] = f32x4{0.f, 0.f, 0.f, 0.f}; }
        sk_stream<KS * 2, RD>(st0 + lane * 16, [&](int s, const uint4& wh, const uint4& wl) {
            const int ks = s >> 1, n = s & 1;
#pragma unroll
            for (int t = 0; t < FM; ++t) hacc[t][n] = OpT<T>::mfma(as_v8<T>(wl), xh[t][ks], hacc[t][n]);
#pragma unroll
            for (int t = 0; t < FM; ++t) hacc[t][n] = OpT<T>::mfma(as_v8<T>(wh), xl[t][ks], hacc[t][n]);
#pragma unroll
            for (int t = 0; t < FM; ++t) hacc[t][n] = OpT<T>::mfma(as_v8<T>(wh), xh[t][ks], hacc[t][n]);
        });
        uint4 hh[FM], hl[FM];
        blk_gelu_split<T, FM>(hacc, tab + S::T_B1, j, g, hh, hl);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();                               // fc2 block j landed; every wave is done with fc1 block j
        if (j + 1 < NCH) dma(a.w1f + ((long long)(j + 1) * S::P_BLK << 9), ldsA);
        sk_stream<CF, RD>(st1 + lane * 16, [&](int c, const uint4& wh, const uint4& wl) {
#pragma unroll
            for (int t = 0; t < FM; ++t) yacc[t][c] = OpT<T>::mfma(as_v8<T>(wl), as_v8<T>(hh[t]), yacc[t][c]);
#pragma unroll
            for (int t = 0; t < FM; ++t) yacc[t][c] = OpT<T>::mfma(as_v8<T>(wh), as_v8<T>(hl[t]), yacc[t][c]);
#pragma unroll
            for (int t = 0; t < FM; ++t) yacc[t][c] = OpT<T>::mfma(as_v8<T>(wh), as_v8<T>(hh[t]), yacc[t][c]);
        });
    }

    // ---- epilogue: + fc2 bias, LayerNorm(norm2), + x_mid (registers), whole blocks of the stream ------------------------------------ //
#pragma unroll
    for (int t = 0; t < FM; ++t) {
        float s = 0.f;
#pragma unroll
        for (int bp = 0; bp < KS; ++bp) {
            const int n = 32 * bp + 8 * g;
            const float4 b0 = *reinterpret_cast<const float4*>(tab + S::T_B2 + n), b1 = *reinterpret_cast<const float4*>(tab + S::T_B2 + n + 4);
            add8(yacc[t][2 * bp], yacc[t][2 * bp + 1], b0, b1);
#pragma unroll
            for (int r = 0; r < 4; ++r) s += yacc[t][2 * bp][r] + yacc[t][2 * bp + 1][r];
        }
        s += __shfl_xor(s, 16);
        s += __shfl_xor(s, 32);
        const float mean = s * (1.0f / C);
        float q = 0.f;
#pragma unroll
        for (int c = 0; c < CF; ++c)
#pragma unroll
            for (int r = 0; r < 4; ++r) { const float d = yacc[t][c][r] - mean; q += d * d; }
        q += __shfl_xor(q, 16);
        q += __shfl_xor(q, 32);
        const float rstd = rsqrtf(q * (1.0f / C) + a.eps);
        if (!live[t]) continue;
        T* dst = a.xs + ((rb0 + t) * KS << 9) + l15 * 32 + g * 8;
#pragma unroll
        for (int bp = 0; bp < KS; ++bp) {
            const int n = 32 * bp + 8 * g;
            const float4 g0 = *reinterpret_cast<const float4*>(tab + S::T_G2 + n), g1 = *reinterpret_cast<const float4*>(tab + S::T_G2 + n + 4);
            const float4 e0 = *reinterpret_cast<const float4*>(tab + S::T_E2 + n), e1 = *reinterpret_cast<const float4*>(tab + S::T_E2 + n + 4);
            float oh[8], ol[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) { oh[i] = (float)xh[t][bp][i]; ol[i] = (float)xl[t][bp][i]; }
            const f32x4 &x = yacc[t][2 * bp], &z = yacc[t][2 * bp + 1];
            const float v[8] = {(oh[0] + ol[0]) + ((x[0] - mean) * rstd * g0.x + e0.x), (oh[1] + ol[1]) + ((x[1] - mean) * rstd * g0.y + e0.y),
                                (oh[2] + ol[2]) + ((x[2] - mean) * rstd * g0.z + e0.z), (oh[3] + ol[3]) + ((x[3] - mean) * rstd * g0.w + e0.w),
                                (oh[4] + ol[4]) + ((z[0] - mean) * rstd * g1.x + e1.x), (oh[5] + ol[5]) + ((z[1] - mean) * rstd * g1.y + e1.y),
                                (oh[6] + ol[6]) + ((z[2] - mean) * rstd * g1.z + e1.z), (oh[7] + ol[7]) + ((z[3] - mean) * rstd * g1.w + e1.w)};
            store8_planes<T, 2>(dst + (bp << 9), a.xs_plane, v);
        }
    }
}

template <class P>
hipError_t op_proj_mlp_fused(const Geom& g, const BlockW<typename P::T>& b, const int* winv, int res, typename P::T* Xs, const Work<P>& wk, hipStream_t s) {
    typedef typename P::T T;
    static_assert(P::NA == 2 && P::NW == 2, "3-term path");
    BlockArgs<T> a{wk.ao, wk.ao_plane, g.ntok[res], Xs, wk.xs_plane[res], winv, b.projf, b.w1f, b.w2f,
                   b.proj_b, b.n1_g, b.n1_b, b.fc1_b, b.fc2_b, b.n2_g, b.n2_b, 1e-5f};
    if (a.M % 16 != 0) return hipErrorInvalidValue;
    // the shapes fused_mlp.hip settled on: C = 192 two 4-wave workgroups per CU with 32 rows per wave, C = 384 one 8-wave workgroup
    typedef BlockShape<192, 2, 4, 2> S0;
    typedef BlockShape<384, 1, 8, 2> S1;
    if (res == 0) return launch_rows<proj_mlp_kernel<T, S0>, S0>(a, s);
    return launch_rows<proj_mlp_kernel<T, S1>, S1>(a, s);
}
template hipError_t op_proj_mlp_fused<PrecBF16x3>(const Geom&, const BlockW<bf16>&, const int*, int, bf16*, const Work<PrecBF16x3>&, hipStream_t);
template hipError_t op_proj_mlp_fused<PrecF16x3>(const Geom&, const BlockW<f16>&, const int*, int, f16*, const Work<PrecF16x3>&, hipStream_t);

template <int C_, int FM_, bool ONE_>
struct Blk2Shape : BlockDims<C_> {
    using D = BlockDims<C_>;
    static constexpr bool ONE = ONE_;
    static constexpr int FM = FM_, NWAVES = 4, THREADS = 64 * NWAVES, RD = 2, BM = NWAVES * FM * 16;
    static constexpr int SLOT_KIB = D::KS * 2;       // KiB of a projection block [ks][n] = of an fc1 chunk [ks][n] = of an fc2 chunk [c]
    static constexpr int SLOT = SLOT_KIB * 1024, NSLOT = 2;
    static constexpr int SMEM = NSLOT * SLOT + D::TAB * 4;
    static_assert(SLOT_KIB % NWAVES == 0 && D::NPB % 2 == 0 && D::NCH >= 3, "DMA pieces per wave; even projection block count");
    static_assert(SMEM <= 80 * 1024, "two workgroups per CU");
};

template <class T, class S>
__global__ void __launch_bounds__(S::THREADS) __attribute__((amdgpu_waves_per_eu(2, 2)))
proj_mlp2_kernel(const BlockArgs<T> a) {
    constexpr int C = S::C, FM = S::FM, KS = S::KS, CF = S::CF, NCH = S::NCH, NPB = S::NPB, NWAVES = S::NWAVES, RD = S::RD;
    typedef typename OpT<T>::v8 v8;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* tab = reinterpret_cast<float*>(smem + S::NSLOT * S::SLOT);
    const int tid = threadIdx.x, lane = tid & 63, l15 = lane & 15, g = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const unsigned lds_base = (unsigned)(size_t)smem;
    const char* lrd = smem + lane * 16;                          // a lane's 16 bytes of every fragment

    // SLOT_KIB consecutive KiB of `src` -> LDS `dst`, piece q by wave q % NWAVES
    auto dma1 = [&](const T* src, unsigned dst) {
        const T* s = src + lane * 8;
#pragma unroll
        for (int i = 0; i < S::SLOT_KIB / NWAVES; ++i) {
            const int q = wave + i * NWAVES;
            glds16(s + (q << 9), dst + (unsigned)(q << 10));
        }
    };
    dma1(a.projf, lds_base);
    blk_fill_tables<S>(tab, a, tid);

    const long long rb0 = (long long)blockIdx.x * (S::BM / 16) + wave * FM;
    v8 xh[FM][KS], xl[FM][KS];
    bool live[FM];
    blk_gather_rows<S, !S::ONE>(a, rb0, l15, g, xh, xl, live);

    f32x4 yacc[FM][CF];
#pragma unroll
    for (int t = 0; t < FM; ++t)
#pragma unroll
        for (int c = 0; c < CF; ++c) yacc[t][c] = f32x4{0.f, 0.f, 0.f, 0.f};

    // ---- phase 1: projection, blocks of 32 output columns alternating between the two slots -------------------------------------- //
#pragma unroll
    for (int j = 0; j < NPB; ++j) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();                               // block j landed; every wave is done with block j - 1
        if (j + 1 < NPB) dma1(a.projf + ((long long)(j + 1) * S::SLOT_KIB << 9), lds_base + (unsigned)(((j + 1) & 1) * S::SLOT));
        else dma1(a.w1f, lds_base);                    // NPB is even: the last block sits in slot 1, slot 0 is free for fc1's chunk 0
        sk_stream<KS, RD>(lrd + (j & 1) * S::SLOT, [&](int ks, const uint4& w0, const uint4& w1) {
            if constexpr (!S::ONE) {
#pragma unroll
                for (int t = 0; t < FM; ++t) yacc[t][2 * j] = OpT<T>::mfma(as_v8<T>(w0), xl[t][ks], yacc[t][2 * j]);
#pragma unroll
                for (int t = 0; t < FM; ++t) yacc[t][2 * j + 1] = OpT<T>::mfma(as_v8<T>(w1), xl[t][ks], yacc[t][2 * j + 1]);
            }
#pragma unroll
            for (int t = 0; t < FM; ++t) yacc[t][2 * j] = OpT<T>::mfma(as_v8<T>(w0), xh[t][ks], yacc[t][2 * j]);
#pragma unroll
            for (int t = 0; t < FM; ++t) yacc[t][2 * j + 1] = OpT<T>::mfma(as_v8<T>(w1), xh[t][ks], yacc[t][2 * j + 1]);
        });
    }

    // ---- between: x_mid = x + LayerNorm(yacc + bias) -> the MLP's input fragments (the attention fragments are dead) ----------- //
#pragma unroll
    for (int t = 0; t < FM; ++t) {
        const T* old = a.xs + ((live[t] ? rb0 + t : 0) * KS << 9) + l15 * 32 + g * 8;
        v8 oh[KS], ol[KS];
#pragma unroll
        for (int bp = 0; bp < KS; ++bp) {
            oh[bp] = *reinterpret_cast<const v8*>(old + (bp << 9));
            ol[bp] = *reinterpret_cast<const v8*>(old + (bp << 9) + a.xs_plane);
        }
        float s = 0.f;
#pragma unroll
        for (int bp = 0; bp < KS; ++bp) {
            const int n = 32 * bp + 8 * g;
            const float4 b0 = *reinterpret_cast<const float4*>(tab + S::T_PB + n), b1 = *reinterpret_cast<const float4*>(tab + S::T_PB + n + 4);
            add8(yacc[t][2 * bp], yacc[t][2 * bp + 1], b0, b1);
#pragma unroll
            for (int r = 0; r < 4; ++r) s += yacc[t][2 * bp][r] + yacc[t][2 * bp + 1][r];
        }
        s += __shfl_xor(s, 16);
        s += __shfl_xor(s, 32);
        const float mean = s * (1.0f / C);
        float q = 0.f;
#pragma unroll
        for (int c = 0; c < CF; ++c)
#pragma unroll
            for (int r = 0; r < 4; ++r) { const float d = yacc[t][c][r] - mean; q += d * d; }
        q += __shfl_xor(q, 16);
        q += __shfl_xor(q, 32);
        const float rstd = rsqrtf(q * (1.0f / C) + a.eps);
#pragma unroll
        for (int bp = 0; bp < KS; ++bp) {
            const int n = 32 * bp + 8 * g;
            const float4 g0 = *reinterpret_cast<const float4*>(tab + S::T_G1 + n), g1 = *reinterpret_cast<const float4*>(tab + S::T_G1 + n + 4);
            const float4 e0 = *reinterpret_cast<const float4*>(tab + S::T_E1 + n), e1 = *reinterpret_cast<const float4*>(tab + S::T_E1 + n + 4);
            const f32x4 &x = yacc[t][2 * bp], &z = yacc[t][2 * bp + 1];
            const float y[8] = {(x[0] - mean) * rstd * g0.x + e0.x, (x[1] - mean) * rstd * g0.y + e0.y, (x[2] - mean) * rstd * g0.z + e0.z, (x[3] - mean) * rstd * g0.w + e0.w,
                                (z[0] - mean) * rstd * g1.x + e1.x, (z[1] - mean) * rstd * g1.y + e1.y, (z[2] - mean) * rstd * g1.z + e1.z, (z[3] - mean) * rstd * g1.w + e1.w};
            float v[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) v[i] = ((float)oh[bp][i] + (float)ol[bp][i]) + y[i];
            uint4 o[2];
            split8<T, 2>(v, o);
            xh[t][bp] = as_v8<T>(o[0]);
            xl[t][bp] = as_v8<T>(o[1]);
            // the planes are FINISHED here: in ONE mode the lo plane is next read in the epilogue, and the compiler would rather carry the
            // eight floats `v` across the MLP loop (in scratch) and round them there
            asm volatile("" : "+v"(xh[t][bp]), "+v"(xl[t][bp]));
        }
#pragma unroll
        for (int c = 0; c < CF; ++c) yacc[t][c] = f32x4{0.f, 0.f, 0.f, 0.f};
    }

    // ---- phase 2: the MLP, W1(j) in slot 0 and W2(j) in slot 1 ---------------------------------------------------------------------- //
    f32x4 hacc[FM][2];
    uint4 hh[FM], hl[FM];
    for (int j = 0; j < NCH; ++j) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();                               // W1(j) landed in slot 0; every wave is done with W2(j - 1) / the projection in slot 1
        dma1(a.w2f + ((long long)j * S::SLOT_KIB << 9), lds_base + S::SLOT);
#pragma unroll
        for (int t = 0; t < FM; ++t) { hacc[t][0] = f32x4{0.f, 0.f, 0.f, 0.f}; hacc[t][1] = f32x4{0.f, 0.f, 0.f, 0.f}; }
        sk_stream<KS, RD>(lrd, [&](int ks, const uint4& w0, const uint4& w1) {
            if constexpr (!S::ONE) {
#pragma unroll
                for (int t = 0; t < FM; ++t) hacc[t][0] = OpT<T>::mfma(as_v8<T>(w0), xl[t][ks], hacc[t][0]);
#pragma unroll
                for (int t = 0; t < FM; ++t) hacc[t][1] = OpT<T>::mfma(as_v8<T>(w1), xl[t][ks], hacc[t][1]);
            }
#pragma unroll
            for (int t = 0; t < FM; ++t) hacc[t][0] = OpT<T>::mfma(as_v8<T>(w0), xh[t][ks], hacc[t][0]);
#pragma unroll
            for (int t = 0; t < FM; ++t) hacc[t][1] = OpT<T>::mfma(as_v8<T>(w1), xh[t][ks], hacc[t][1]);
        });
        blk_gelu_split<T, FM>(hacc, tab + S::T_B1, j, g, hh, hl);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();                               // W2(j) landed; every wave is done with W1(j)
        if (j + 1 < NCH) dma1(a.w1f + ((long long)(j + 1) * S::SLOT_KIB << 9), lds_base);
        sk_stream<CF / 2, RD>(lrd + S::SLOT, [&](int p, const uint4& w0, const uint4& w1) {
            if constexpr (!S::ONE) {
#pragma unroll
                for (int t = 0; t < FM; ++t) yacc[t][2 * p] = OpT<T>::mfma(as_v8<T>(w0), as_v8<T>(hl[t]), yacc[t][2 * p]);
#pragma unroll
                for (int t = 0; t < FM; ++t) yacc[t][2 * p + 1] = OpT<T>::mfma(as_v8<T>(w1), as_v8<T>(hl[t]), yacc[t][2 * p + 1]);
            }
#pragma unroll
            for (int t = 0; t < FM; ++t) yacc[t][2 * p] = OpT<T>::mfma(as_v8<T>(w0), as_v8<T>(hh[t]), yacc[t][2 * p]);
#pragma unroll
            for (int t = 0; t < FM; ++t) yacc[t][2 * p + 1] = OpT<T>::mfma(as_v8<T>(w1), as_v8<T>(hh[t]), yacc[t][2 * p + 1]);
        });
    }

    // ---- epilogue: + fc2 bias, LayerNorm(norm2), + x_mid (registers), whole blocks of the stream ------------------------------------ //
#pragma unroll
    for (int t = 0; t < FM; ++t) {
        float s = 0.f;
#pragma unroll
        for (int bp = 0; bp < KS; ++bp) {
            const int n = 32 * bp + 8 * g;
            const float4 b0 = *reinterpret_cast<const float4*>(tab + S::T_B2 + n), b1 = *reinterpret_cast<const float4*>(tab + S::T_B2 + n + 4);
            add8(yacc[t][2 * bp], yacc[t][2 * bp + 1], b0, b1);
#pragma unroll
            for (int r = 0; r < 4; ++r) s += yacc[t][2 * bp][r] + yacc[t][2 * bp + 1][r];
        }
        s += __shfl_xor(s, 16);
        s += __shfl_xor(s, 32);
        const float mean = s * (1.0f / C);
        float q = 0.f;
#pragma unroll
        for (int c = 0; c < CF; ++c)
#pragma unroll
            for (int r = 0; r < 4; ++r) { const float d = yacc[t][c][r] - mean; q += d * d; }
        q += __shfl_xor(q, 16);
        q += __shfl_xor(q, 32);
        const float rstd = rsqrtf(q * (1.0f / C) + a.eps);
        if (!live[t]) continue;
        T* dst = a.xs + ((rb0 + t) * KS << 9) + l15 * 32 + g * 8;
#pragma unroll
        for (int bp = 0; bp < KS; ++bp) {
            const int n = 32 * bp + 8 * g;
            const float4 g0 = *reinterpret_cast<const float4*>(tab + S::T_G2 + n), g1 = *reinterpret_cast<const float4*>(tab + S::T_G2 + n + 4);
            const float4 e0 = *reinterpret_cast<const float4*>(tab + S::T_E2 + n), e1 = *reinterpret_cast<const float4*>(tab + S::T_E2 + n + 4);
            // x_mid is converted back from the fragments HERE: left visible, the compiler reuses the floats split8 rounded in the between phase
            // and carries them through the whole MLP loop -- in scratch (C / 2 + 1 dwords per lane and tile)
            v8 mh = xh[t][bp], ml = xl[t][bp];
            asm volatile("" : "+v"(mh), "+v"(ml));
            float oh[8], ol[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) { oh[i] = (float)mh[i]; ol[i] = (float)ml[i]; }
            const f32x4 &x = yacc[t][2 * bp], &z = yacc[t][2 * bp + 1];
            const float v[8] = {(oh[0] + ol[0]) + ((x[0] - mean) * rstd * g0.x + e0.x), (oh[1] + ol[1]) + ((x[1] - mean) * rstd * g0.y + e0.y),
                                (oh[2] + ol[2]) + ((x[2] - mean) * rstd * g0.z + e0.z), (oh[3] + ol[3]) + ((x[3] - mean) * rstd * g0.w + e0.w),
                                (oh[4] + ol[4]) + ((z[0] - mean) * rstd * g1.x + e1.x), (oh[5] + ol[5]) + ((z[1] - mean) * rstd * g1.y + e1.y),
                                (oh[6] + ol[6]) + ((z[2] - mean) * rstd * g1.z + e1.z), (oh[7] + ol[7]) + ((z[3] - mean) * rstd * g1.w + e1.w)};
            store8_planes<T, 2>(dst + (bp << 9), a.xs_plane, v);
        }
    }
}

// `one`: the layer's term-plan bit 8 + l -- the activation operands as one fp16 plane too
hipError_t op_proj_mlp2(const Geom& g, const BlockW<f16>& b, const int* winv, int res, f16* Xs, const Work<PrecF16x3>& wk, hipStream_t s, int one) {
    typedef f16 T;
    BlockArgs<T> a{wk.ao, wk.ao_plane, g.ntok[res], Xs, wk.xs_plane[res], winv, b.projh, b.w1h, b.w2h,
                   b.proj_b, b.n1_g, b.n1_b, b.fc1_b, b.fc2_b, b.n2_g, b.n2_b, 1e-5f};
    if (a.M % 16 != 0) return hipErrorInvalidValue;
    typedef Blk2Shape<192, 2, true> S01;
    typedef Blk2Shape<192, 2, false> S02;
    typedef Blk2Shape<384, 1, true> S11;
    typedef Blk2Shape<384, 1, false> S12;
    if (res == 0) return one ? launch_rows<proj_mlp2_kernel<T, S01>, S01>(a, s) : launch_rows<proj_mlp2_kernel<T, S02>, S02>(a, s);
    return one ? launch_rows<proj_mlp2_kernel<T, S11>, S11>(a, s) : launch_rows<proj_mlp2_kernel<T, S12>, S12>(a, s);
}

}  // namespace skp
