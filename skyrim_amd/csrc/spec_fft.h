// The butterflies of the zonal-spectrum transform (include/skyrim_spec.h): one radix-R pass of a Stockham mixed-radix FFT over split
// real / imaginary fp32 planes.  Plain C++ on purpose -- host and device compile the same text, so the arithmetic can be checked on a
// CPU -- and free of fma contraction (the header counts one rounding per operation).
//   element p of a plane lies at word spec_pad(p): one pad word after every 32, so that the strided writes of the early passes
//   (stride R Ns elements between neighbouring lanes) fall into different banks
//   pass(R, Ns), butterfly j of W / R:   k = j mod Ns;   v_t = in[j + t W / R] * tw[t k W / (Ns R)]   (t = 0 .. R - 1; tw[n] = e^(-2 pi i n / W))
//                                        y_q = sum_t v_t e^(-2 pi i q t / R);   out[(j / Ns) Ns R + k + q Ns] = y_q
//   radix 2 and 4 multiply by 1, -1, -i, i only (exact); radix 3 and 5 are the literal sums y_q = v_0 + sum_{t >= 1} v_t w_R^(q t mod R),
//   added in ascending t, with w_R rounded to fp32 from float64: that is what the bound of the header counts.
#ifndef SKYRIM_SPEC_FFT_H
#define SKYRIM_SPEC_FFT_H

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SKSPEC_HD __host__ __device__ __forceinline__
#else
#define SKSPEC_HD inline
#endif

#pragma clang fp contract(off)

SKSPEC_HD int spec_pad(int p) { return p + (p >> 5); }

struct spec_c {
    float x, y;
};

// (a + i b)(c + i d), four products, one sum and one difference, each rounded
SKSPEC_HD spec_c spec_mul(spec_c a, spec_c w) {
    spec_c r;
    r.x = a.x * w.x - a.y * w.y;
    r.y = a.x * w.y + a.y * w.x;
    return r;
}
SKSPEC_HD spec_c spec_add(spec_c a, spec_c b) { return spec_c{a.x + b.x, a.y + b.y}; }
SKSPEC_HD spec_c spec_sub(spec_c a, spec_c b) { return spec_c{a.x - b.x, a.y - b.y}; }

SKSPEC_HD spec_c spec_get(const float* re, const float* im, int p) { return spec_c{re[spec_pad(p)], im[spec_pad(p)]}; }
SKSPEC_HD void spec_put(float* re, float* im, int p, spec_c v) {
    re[spec_pad(p)] = v.x;
    im[spec_pad(p)] = v.y;
}
SKSPEC_HD spec_c spec_tw(const float* tw, int n) { return spec_c{tw[2 * n], tw[2 * n + 1]}; }

// w_3^t and w_5^t, t = 1 .. R - 1: cos and -sin of 2 pi t / R, rounded from float64
#define SKSPEC_W3_1 spec_c{-0.5f, -0.8660254037844386f}
#define SKSPEC_W3_2 spec_c{-0.5f, 0.8660254037844386f}
#define SKSPEC_W5_1 spec_c{0.30901699437494745f, -0.9510565162951535f}
#define SKSPEC_W5_2 spec_c{-0.8090169943749475f, -0.5877852522924731f}
#define SKSPEC_W5_3 spec_c{-0.8090169943749475f, 0.5877852522924731f}
#define SKSPEC_W5_4 spec_c{0.30901699437494745f, 0.9510565162951535f}

// butterfly j of the pass (R, Ns) of a length-W transform
template <int R>
SKSPEC_HD void spec_butterfly(const float* in_re, const float* in_im, float* out_re, float* out_im, const float* tw, int W, int Ns, int j) {
    const int span = W / R;
    const int k = j % Ns;
    const int step = k * (W / (Ns * R));                  // tw index of t = 1
    const int o = (j / Ns) * Ns * R + k;
    const spec_c v0 = spec_get(in_re, in_im, j);
    const spec_c v1 = spec_mul(spec_get(in_re, in_im, j + span), spec_tw(tw, step));
    if (R == 2) {
        spec_put(out_re, out_im, o, spec_add(v0, v1));
        spec_put(out_re, out_im, o + Ns, spec_sub(v0, v1));
        return;
    }
    const spec_c v2 = spec_mul(spec_get(in_re, in_im, j + 2 * span), spec_tw(tw, 2 * step));
    if (R == 3) {
        spec_put(out_re, out_im, o, spec_add(spec_add(v0, v1), v2));
        spec_put(out_re, out_im, o + Ns, spec_add(spec_add(v0, spec_mul(v1, SKSPEC_W3_1)), spec_mul(v2, SKSPEC_W3_2)));
        spec_put(out_re, out_im, o + 2 * Ns, spec_add(spec_add(v0, spec_mul(v1, SKSPEC_W3_2)), spec_mul(v2, SKSPEC_W3_1)));
        return;
    }
    const spec_c v3 = spec_mul(spec_get(in_re, in_im, j + 3 * span), spec_tw(tw, 3 * step));
    if (R == 4) {
        const spec_c a = spec_add(v0, v2), b = spec_sub(v0, v2), c = spec_add(v1, v3), d = spec_sub(v1, v3);
        const spec_c md = spec_c{d.y, -d.x};              // -i d
        spec_put(out_re, out_im, o, spec_add(a, c));
        spec_put(out_re, out_im, o + Ns, spec_add(b, md));
        spec_put(out_re, out_im, o + 2 * Ns, spec_sub(a, c));
        spec_put(out_re, out_im, o + 3 * Ns, spec_sub(b, md));
        return;
    }
    if (R == 5) {
        const spec_c v4 = spec_mul(spec_get(in_re, in_im, j + 4 * span), spec_tw(tw, 4 * step));
        const spec_c w1 = SKSPEC_W5_1, w2 = SKSPEC_W5_2, w3 = SKSPEC_W5_3, w4 = SKSPEC_W5_4;
        spec_put(out_re, out_im, o, spec_add(spec_add(spec_add(spec_add(v0, v1), v2), v3), v4));
        spec_put(out_re, out_im, o + Ns,
                 spec_add(spec_add(spec_add(spec_add(v0, spec_mul(v1, w1)), spec_mul(v2, w2)), spec_mul(v3, w3)), spec_mul(v4, w4)));
        spec_put(out_re, out_im, o + 2 * Ns,
                 spec_add(spec_add(spec_add(spec_add(v0, spec_mul(v1, w2)), spec_mul(v2, w4)), spec_mul(v3, w1)), spec_mul(v4, w3)));
        spec_put(out_re, out_im, o + 3 * Ns,
                 spec_add(spec_add(spec_add(spec_add(v0, spec_mul(v1, w3)), spec_mul(v2, w1)), spec_mul(v3, w4)), spec_mul(v4, w2)));
        spec_put(out_re, out_im, o + 4 * Ns,
                 spec_add(spec_add(spec_add(spec_add(v0, spec_mul(v1, w4)), spec_mul(v2, w3)), spec_mul(v3, w2)), spec_mul(v4, w1)));
    }
}

// the radices of W = 2^a 3^b 5^c in the order they are applied: 4s, a 2, 3s, 5s; returns their number, 0 when W has another factor
inline int spec_factor(int W, int* radix) {
    int n = 0;
    if (W < 2) return 0;
    while (W % 4 == 0) { radix[n++] = 4; W /= 4; }
    if (W % 2 == 0) { radix[n++] = 2; W /= 2; }
    while (W % 3 == 0) { radix[n++] = 3; W /= 3; }
    while (W % 5 == 0) { radix[n++] = 5; W /= 5; }
    return W == 1 ? n : 0;
}

#endif
