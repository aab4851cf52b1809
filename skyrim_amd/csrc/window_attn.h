// Window attention of the Swin-style models (fuxi_ops.hip, fengwu_ops.hip): one wave = 16 queries of one (window, head); key tiles of
// 32 with an online softmax, so the window size is a run-time argument.  S^T = K Q^T and O^T = V^T P^T on v_mfma_f32_16x16x32_f16
// (three hi/lo terms): a lane ends with 8 scores of ONE query, which are -- permuted within the tile -- its B operand of the PV product,
// and HD / 4 outputs of that query.  No LDS, no barriers.
//
// What a model supplies (a struct passed by value, every member __forceinline__):
//   static constexpr int HD               head dimension, a multiple of 32
//   void query(int i)                     the lane's query is window-local index i: whatever score() and out() need of it
//   const float* row(int i, int part)     the head's HD values of part 0 / 1 / 2 (q / k / v) of window-local index i
//   void prep_q(float (&v)[HD / 32][8])   q before its fp16 split; lane (l15, g) holds q[32 ch + 8 g + j] of its query in v[ch][j]
//   void prep_k(float (&v)[HD / 32][8])   the same for a key
//   float score(float s, int key)         s = q . k of the lane's query and window-local key: + position bias, mask
//   float* out()                          the head's HD outputs of the lane's query, or null where nothing is stored
#pragma once
#include "common.h"

namespace skp {

typedef OpT<f16>::v8 v8;

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

// queries 64 qchunk + 16 wave + (0..15) of a window of N tokens; workgroups of 256
template <class POL>
__device__ __forceinline__ void window_attn_body(POL pol, int N, int qchunk) {
    constexpr int KC = POL::HD / 32, DB = POL::HD / 16;
    const int lane = threadIdx.x & 63, l15 = lane & 15, g = lane >> 4;
    const int q0 = qchunk * 64 + (threadIdx.x >> 6) * 16;
    if (q0 >= N) return;                                          // wave-uniform; no barriers in this kernel

    // queries: lane (l15, g) holds q[d = 32 ch + 8 g + j] of query q0 + l15 (the B operand of S^T = K Q^T)
    const int qi = q0 + l15 < N ? q0 + l15 : N - 1;
    pol.query(qi);
    v8 qh[KC], ql[KC];
    {
        const float* p = pol.row(qi, 0) + 8 * g;
        float v[KC][8];
#pragma unroll
        for (int ch = 0; ch < KC; ++ch) load8(p + 32 * ch, v[ch]);
        pol.prep_q(v);
#pragma unroll
        for (int ch = 0; ch < KC; ++ch) split_v8(v[ch], qh[ch], ql[ch]);
    }
    float m = -INFINITY, lsum = 0.f;
    f32x4 o[DB];
#pragma unroll
    for (int b = 0; b < DB; ++b) o[b] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int k0 = 0; k0 < N; k0 += 32) {
        // S^T[key][q] for keys k0 + 16 b + (0..15): A = K[key = l15 + 16 b][d = 32 ch + 8 g + j]
        f32x4 s[2];
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const int key = k0 + 16 * b + l15 < N ? k0 + 16 * b + l15 : N - 1;
            const float* p = pol.row(key, 1) + 8 * g;
            float v[KC][8];
#pragma unroll
            for (int ch = 0; ch < KC; ++ch) load8(p + 32 * ch, v[ch]);
            pol.prep_k(v);
            s[b] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ch = 0; ch < KC; ++ch) {
                v8 kh, kl;
                split_v8(v[ch], kh, kl);
                s[b] = mfma3(kh, kl, qh[ch], ql[ch], s[b]);
            }
        }
        // s[b][r] = score of key k0 + 16 b + 4 g + r for query q0 + l15: + the model's bias and mask; online softmax
        float p[8];
        float mx = -INFINITY;
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int key = k0 + 16 * b + 4 * g + r;
                const float v = key < N ? pol.score(s[b][r], key) : -INFINITY;
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
        for (int b = 0; b < DB; ++b) o[b] *= alpha;
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
            vp[j] = pol.row(vok[j] ? key : N - 1, 2) + l15;
        }
        // O^T[d][q] += V^T P^T: A = V^T[d = 16 db + l15][k-slot (g, j)]
#pragma unroll
        for (int db = 0; db < DB; ++db) {
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
    float* op = pol.out();
    if (q0 + l15 >= N || op == nullptr) return;
    const float inv = (1.0f / lsum) * (1.0f / kPScale);
    // o[db][r] = O[q0 + l15][16 db + 4 g + r]
#pragma unroll
    for (int db = 0; db < DB; ++db)
        *reinterpret_cast<float4*>(op + 16 * db + 4 * g) = make_float4(o[db][0] * inv, o[db][1] * inv, o[db][2] * inv, o[db][3] * inv);
}

}  // namespace skp
