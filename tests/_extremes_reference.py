"""numpy restatements of include/skyrim_clim.h, operation by operation in float32 (``extremes32``, ``quantiles32``), and the same formulas
in float64 with the double tables (``extremes64``, the bounds of the header beside them), plus a direct quadrature of the EFI integral."""
import math

import numpy as np

from skyrim_amd import climate as K

F32 = np.float32
NAN = np.frombuffer(np.uint32(0x7FC00000).tobytes(), np.float32)[0]
U = 2.0 ** -24


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def tables32(levels):
    t = K.tables(levels)
    return {k: v.astype(F32) for k, v in t.items()}


def fma32(a, b, c):
    """fl32(a b + c) with ONE rounding: the product is exact in float64, the float64 sum's error is known exactly (two-sum), and a float64
    sum that lies exactly between two float32 neighbours is pushed to the side the error points to."""
    a, b, c = (np.asarray(v, np.float64) for v in (a, b, c))
    p = a * b
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    r = s.astype(F32)
    d = s - r.astype(np.float64)
    up, dn = np.nextafter(r, F32(np.inf)), np.nextafter(r, F32(-np.inf))
    with np.errstate(invalid="ignore", over="ignore"):
        hu, hd = (up.astype(np.float64) - r) / 2, (r - dn.astype(np.float64)) / 2
        r = np.where((d == hu) & (err > 0), up, r)
        r = np.where((d == -hd) & (err < 0), dn, r)
    return r.astype(F32)


def member_quantile32(s, q_index, q_frac):
    """skens_stats' quantile of the sorted members s (M, n): two-sum difference, two fused operations."""
    M = s.shape[0]
    lo, hi = s[q_index], s[min(q_index + 1, M - 1)]
    f = F32(q_frac)
    nl = -lo
    d = hi + nl
    bb = d - hi
    err = (hi - (d - bb)) + (nl - bb)
    return fma32(f, err, fma32(f, d, lo))


def extremes32(x, c, levels, floor=-np.inf, sot=(), prob=()):
    """x (M, n), c (Q, n) float32 -> dict(efi (n,), sot (S, n), prob (T, n)) float32, every operation rounded on its own."""
    with np.errstate(all="ignore"):
        x, c = np.asarray(x, F32) + F32(0), np.asarray(c, F32) + F32(0)
        M, n = x.shape
        Q = c.shape[0]
        t = tables32(levels)
        p, A, B, rdp = t["p"], t["A"], t["B"], t["rdp"]
        fM, flo = F32(M), F32(floor)
        bad = ~(np.isfinite(x).all(axis=0) & np.isfinite(c).all(axis=0))
        F = np.stack([(x <= c[i]).sum(axis=0).astype(F32) / fM for i in range(Q)])
        num, den, act = np.zeros(n, F32), np.zeros(n, F32), np.zeros(n, bool)
        for i in range(Q - 1):
            b = (F[i + 1] - F[i]) * rdp[i]
            a = F[i] - b * p[i]
            ti = (B[i] - a * A[i]) - b * B[i]
            on = c[i + 1] > flo
            num = np.where(on, num + ti, num).astype(F32)
            den = np.where(on, den + B[i], den).astype(F32)
            act |= on
        efi = np.where(act, np.minimum(np.maximum(num / np.where(act, den, F32(1)), F32(-1)), F32(1)), F32(0)).astype(F32)
        efi[bad] = NAN
        s = np.sort(x, axis=0)
        so = np.empty((len(sot), n), F32)
        for k, (qi, qf, kr, kb) in enumerate(sot):
            r = (member_quantile32(s, qi, qf) - c[kr]) / (c[kr] - c[kb])
            so[k] = np.where(bad | (c[kr] == c[kb]), NAN, r)
        po = np.empty((len(prob), n), F32)
        for k, (lev, below) in enumerate(prob):
            cnt = (x < c[lev]).sum(axis=0) if below else (x > c[lev]).sum(axis=0)
            po[k] = np.where(bad, NAN, cnt.astype(F32) / fM)
        return dict(efi=efi, sot=so, prob=po)


def extremes64(x, c, levels, floor=-np.inf, sot=()):
    """The same formulas in float64 on the same fp32 inputs with the DOUBLE tables, and the header's bounds:
    dict(efi, efi_bound (n,), sot, sot_bound (S, n)).  Points with a non-finite input are NaN."""
    with np.errstate(all="ignore"):
        x, c = np.asarray(x, F32).astype(np.float64), np.asarray(c, F32).astype(np.float64)
        M, n = x.shape
        Q = c.shape[0]
        t = K.tables(levels)
        p, A, B, rdp = t["p"], t["A"], t["B"], t["rdp"]
        bad = ~(np.isfinite(x).all(axis=0) & np.isfinite(c).all(axis=0))
        F = np.stack([(x <= c[i]).sum(axis=0) / M for i in range(Q)])
        num, den, T = np.zeros(n), np.zeros(n), np.zeros(n)
        for i in range(Q - 1):
            b = (F[i + 1] - F[i]) * rdp[i]
            a = F[i] - b * p[i]
            on = c[i + 1] > np.float64(F32(floor))
            num += np.where(on, B[i] - a * A[i] - b * B[i], 0.0)
            den += np.where(on, B[i], 0.0)
            T += np.where(on, B[i] + (1 + rdp[i] * p[i]) * A[i] + rdp[i] * B[i], 0.0)
        efi = np.where(den > 0, np.clip(num / np.where(den > 0, den, 1.0), -1, 1), 0.0)
        bound = np.where(den > 0, U * ((Q + 12) * T / np.where(den > 0, den, 1.0) + Q), 0.0)
        efi[bad] = np.nan
        s = np.sort(x, axis=0)
        so, sb = np.empty((len(sot), n)), np.empty((len(sot), n))
        for k, (qi, qf, kr, kb) in enumerate(sot):
            lo, hi = s[qi], s[min(qi + 1, M - 1)]
            qv = lo + np.float64(F32(qf)) * (hi - lo)
            dn = c[kr] - c[kb]
            so[k] = np.where(bad | (dn == 0), np.nan, (qv - c[kr]) / dn)
            sb[k] = U * (2 * np.maximum(np.abs(lo), np.abs(hi)) / np.abs(dn) + 4 * np.abs(so[k])) + 2.0 ** -126
        return dict(efi=efi, efi_bound=bound, sot=so, sot_bound=sb)


def efi_quadrature(x, c, levels, n=200001):
    """The integral (2 / pi) int (p - F(p)) / sqrt(p (1 - p)) dp for ONE point by the substitution p = sin^2(theta / 2), which removes
    both end-point singularities: dp / sqrt(p (1 - p)) = d theta.  F piecewise linear through the member fractions at the levels, the
    whole of [levels[0], levels[-1]] in use (no floor), normalised as the header does by the same integral of p."""
    x, c, p = np.asarray(x, np.float64), np.asarray(c, np.float64), np.asarray(levels, np.float64)
    F = np.array([(x <= ci).mean() for ci in c])
    th0, th1 = 2 * np.arcsin(np.sqrt(p[0])), 2 * np.arcsin(np.sqrt(p[-1]))
    th = np.linspace(th0, th1, n)
    pp = np.sin(th / 2) ** 2
    trap = lambda y: float(np.sum((y[1:] + y[:-1]) * np.diff(th)) / 2)       # noqa: E731
    return trap(pp - np.interp(pp, p, F)) / trap(pp)


def quantiles32(s, levels):
    """s (N, n) float32 samples -> (Q, n) float32: the header's interpolation and clamp; a point with a non-finite sample is NaN."""
    with np.errstate(all="ignore"):
        s = np.asarray(s, F32) + F32(0)
        N = s.shape[0]
        bad = ~np.isfinite(s).all(axis=0)
        srt = np.sort(np.where(bad, F32(0), s), axis=0)
        qi, qf = K.positions(levels, N)
        out = np.empty((len(qi), s.shape[1]), F32)
        for i, (j, f) in enumerate(zip(qi, qf.astype(F32))):
            lo, hi = srt[j], srt[min(j + 1, N - 1)]
            out[i] = np.minimum(lo + f * (hi - lo), hi)
        out[:, bad] = NAN
        return out


def quantile_bound(s, levels):
    """(np.quantile in float64, the header's bound) for finite s (N, n)."""
    s64 = np.sort(np.asarray(s, F32).astype(np.float64), axis=0)
    N = s64.shape[0]
    qi, _ = K.positions(levels, N)
    exact = np.quantile(s64, np.asarray(levels, np.float64), axis=0, method="linear")
    lo, hi = s64[qi], s64[np.minimum(qi + 1, N - 1)]
    return exact, U * (3 * np.abs(hi - lo) + np.maximum(np.abs(lo), np.abs(hi))) + 2.0 ** -148


def field(M, C, H, W, seed):
    """(M, C, H, W) float32 of mixed magnitude, the recipe of ``field`` in tests/test_point_kernels_gpu.py: a temperature, a geopotential,
    winds of both signs, a tiny humidity."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((M, C, H, W), dtype=np.float32)
    scale = np.array([250.0, 54000.0, 25.0, 8.0, 1e-3, 1e-30, 1e5, 3.0, 0.02] * 8)[:C]
    shift = np.array([250.0, 5e4, 0.0, 0.0, 5e-3, 0.0, 1e5, -3.0, 0.0] * 8)[:C]
    x *= scale.astype(np.float32)[None, :, None, None]
    x += shift.astype(np.float32)[None, :, None, None]
    return x
