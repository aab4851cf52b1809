// The register-resident MLP of the block kernels (fused_block.hip), and the weight preparation it needs:
//
//     x += LayerNorm(norm2)( fc2( GELU( fc1(x) ) ) )   in place on the residual planes.
//
// The two-kernel form (ops_mlp.hip) writes the 4C-wide hidden activation to HBM as hi/lo planes and reads it back: 32 of the
// step's 90 GB.  In the block kernels the hidden never leaves the CU, and neither do the token rows:
//
//   * a wavefront owns FM x 16 tokens for the whole kernel.  Their C input columns live in REGISTERS as MFMA B-operand fragments
//     (hi + lo planes, loaded once with 16-byte loads: one wave instruction = one 1 KiB block of the blocked layout), and so do
//     the FM x 16 x C fp32 accumulators of fc2 -- TM x C = 12288 either way (C = 192: 64 tokens, C = 384: 32 tokens), a
//     512-register wave, one wave per SIMD, 4 waves per workgroup.  Nothing of the token tile ever goes through LDS.
//   * the hidden dimension is walked in chunks of 32 units.  fc1 of a chunk leaves, in swapped order (D^T = W X^T), for token
//     l & 15 the hidden units 16 n + 4 (l >> 4) + r in a lane's accumulators -- after bias + GELU + hi/lo split those eight
//     values ARE the lane's B-operand fragment of fc2's 32-deep k-step (the prepared fc2 weights carry the matching column
//     order).  No shuffle, no LDS round trip: the same trick as P -> P V in attention.hip.
//   * LDS holds only weights: per chunk the 32 x C block of fc1 and the C x 32 block of fc2, each as hi/lo planes in FRAGMENT
//     order (prepared once: every 1 KiB = what one ds_read_b128 wave instruction consumes, lane-linear, so LDS-DMA lands it
//     conflict-free with no swizzle).  Two stages: fc2's block streams in under fc1's MFMAs, the next chunk's fc1 block under
//     fc2's.  Per chunk and CU: 49 / 98 KB of DMA against 4608 MFMA clocks (25 % / 49 % of the 43 B/clk DMA rate; the tiled
//     GEMMs sit at 58 %), 384 ds_read_b128 per wave (a third of the LDS read rate).
//   * epilogue: a token's C outputs sit in one lane quad's registers across the 4 lane groups -> LayerNorm needs two shfl_xor,
//     no LDS, no barrier.  With the perm8 row order of the fc2 weights the accumulators of fragment pair bp are columns
//     32 bp + 8 (l >> 4) + [0..7] -- exactly the columns of the input fragment of k-step bp, still in registers: the residual
//     add needs no load at all.  HBM traffic of the whole MLP: 4 B/element read + 4 B/element written + weights (L2).
//
// Schedule findings (measured on the MLP alone, before the projection was folded in front of it):
//   * weight fragments come through a ring of DEPTH = 3 register pairs, loaded two steps ahead of their MFMAs; a scheduling barrier
//     pins each read in program order -- left alone, hipcc sinks the reads back next to their first use (one pair reloaded in
//     place: read, wait, MFMAs, read, ...), and nothing else hides the LDS latency.
//   * the token-row fragments are consumed once right after their loads, so that hipcc's vmcnt waits for them sit BEFORE the
//     loops: inside they would also wait for the LDS-DMA of the block in flight, which the compiler's counter bookkeeping does not
//     know about.
//   * ms per launch at 721x1440, C = 192 / C = 384: the best shapes are those in which TWO waves share a SIMD, so that one wave's
//     GELU, LDS-DMA issue and barrier waits run under the other's MFMAs --
//       C = 192: two independent 4-wave workgroups per CU, 32 tokens per wave ........ 0.748   (one 4-wave workgroup, 64 tokens per wave: 0.808;
//                one 8-wave workgroup: 0.764 -- its waves reach the barriers, and therefore the GELU, together)
//       C = 384: one 8-wave workgroup, 16 tokens per wave (LDS holds one 107 KB set) .. 0.695   (4 waves x 32 tokens, one per SIMD: 0.761)
//     The skewed schedule (GELU of chunk j spliced into fc1 of chunk j + 1) needs 16 more registers than a wave has and spills.
//
// gfx950 only.
#include "launchers.h"

namespace skp {

// ---- prepare: fp32 master weights -> fragment-order hi/lo planes ---------------------------------------------------------------- //
//   (planes = 1: the hi plane only, blocks [(j KS + ks) 2 + n] and [j CF + c] -- proj_mlp2_kernel)
//   w1f[((j KS + ks) 2 + n) 2 + plane][lane][e] = fc1.weight[32 j + 16 n + (lane & 15)][32 ks + 8 (lane >> 4) + e]
//   w2f[(j CF + c) 2 + plane][lane][e]          = fc2.weight[perm8_col(16 c + (lane & 15))][32 j + 16 (e >> 2) + 4 (lane >> 4) + (e & 3)]
template <class T>
__global__ void prep_mlp_w1_kernel(const float* __restrict__ w1, T* __restrict__ out, int C, int planes) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;     // one (block pair, lane, e)
    const int KS = C / 32;
    const long long total = (long long)(4 * C / 32) * KS * 2 * 512;
    if (i >= total) return;
    const int e = (int)(i & 7), lane = (int)((i >> 3) & 63);
    long long q = i >> 9;
    const int n = (int)(q & 1); q >>= 1;
    const int ks = (int)(q % KS);
    const int j = (int)(q / KS);
    const float v = w1[(long long)(32 * j + 16 * n + (lane & 15)) * C + 32 * ks + 8 * (lane >> 4) + e];
    const T h = (T)v;
    const long long o = ((((long long)j * KS + ks) * 2 + n) * planes << 9) + lane * 8 + e;
    out[o] = h;
    if (planes == 2) out[o + 512] = (T)(v - (float)h);
}

template <class T>
__global__ void prep_mlp_w2_kernel(const float* __restrict__ w2, T* __restrict__ out, int C, int planes) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int CF = C / 16;
    const long long total = (long long)(4 * C / 32) * CF * 512;
    if (i >= total) return;
    const int e = (int)(i & 7), lane = (int)((i >> 3) & 63);
    const long long q = i >> 9;
    const int c = (int)(q % CF);
    const int j = (int)(q / CF);
    const int col = perm8_col(16 * c + (lane & 15));
    const int hid = 32 * j + 16 * (e >> 2) + 4 * (lane >> 4) + (e & 3);
    const float v = w2[(long long)col * (4 * C) + hid];
    const T h = (T)v;
    const long long o = ((((long long)j * CF + c) * planes) << 9) + lane * 8 + e;
    out[o] = h;
    if (planes == 2) out[o + 512] = (T)(v - (float)h);
}

template <class T>
hipError_t prep_mlp_weights(const float* w1, const float* w2, T* w1f, T* w2f, int C, hipStream_t s, int planes) {
    if ((C != 192 && C != 384) || (planes != 1 && planes != 2)) return hipErrorInvalidValue;
    const long long t1 = (long long)(4 * C / 32) * (C / 32) * 2 * 512, t2 = (long long)(4 * C / 32) * (C / 16) * 512;
    hipLaunchKernelGGL((prep_mlp_w1_kernel<T>), dim3((unsigned)((t1 + 255) / 256)), dim3(256), 0, s, w1, w1f, C, planes);
    hipLaunchKernelGGL((prep_mlp_w2_kernel<T>), dim3((unsigned)((t2 + 255) / 256)), dim3(256), 0, s, w2, w2f, C, planes);
    return hipGetLastError();
}
template hipError_t prep_mlp_weights<bf16>(const float*, const float*, bf16*, bf16*, int, hipStream_t, int);
template hipError_t prep_mlp_weights<f16>(const float*, const float*, f16*, f16*, int, hipStream_t, int);

}  // namespace skp
