"""Float64 restatement of include/skyrim_derive.h on the same fp32 inputs, written from the header's text: each function returns the
exact value and the magnitude S of the header's bound per point; ``K`` and ``TINY`` hold the rounding counts and the underflow terms.
The row table and the column weights are made here on their own, not taken from skyrim_amd/derived.py."""
from __future__ import annotations

import numpy as np

U = 2.0 ** -24
SLACK64 = 2.0 ** -40
A_M = 6371000.0
G = 9.80665
ONESIDED, POLE = 1, 2


def f64(x):
    return np.asarray(x, np.float32).astype(np.float64)


def bound(k, S, tiny):
    return k * U * S + tiny


def speed(u, v):
    """(s, S): k = 4, tiny = 2^-74."""
    u, v = f64(u), f64(v)
    s = np.sqrt(u * u + v * v)
    return s, s


K_SPEED, TINY_SPEED = 4, 2.0 ** -74
K_DIFF, TINY_DIFF = 1, 0.0
K_VORTDIV, TINY_SUM = 4, 2.0 ** -126


def diff(a, b):
    a, b = f64(a), f64(b)
    return a - b, np.abs(a) + np.abs(b)


def column(q, u, v, w):
    """q, u, v: (L, ...) fp32 planes, w: (L,) fp32 weights -> {name: (value, S, k, tiny)} for ivtu, ivtv, ivt, iwv."""
    q, u, v = f64(q), f64(u), f64(v)
    w = f64(w).reshape((-1,) + (1,) * (q.ndim - 1))
    L = q.shape[0]
    t = w * q
    iwv, S_w = t.sum(axis=0), np.abs(t).sum(axis=0)
    ivtu, S_u = (t * u).sum(axis=0), np.abs(t * u).sum(axis=0)
    ivtv, S_v = (t * v).sum(axis=0), np.abs(t * v).sum(axis=0)
    return dict(ivtu=(ivtu, S_u, L + 3, TINY_SUM), ivtv=(ivtv, S_v, L + 3, TINY_SUM),
                ivt=(np.sqrt(ivtu ** 2 + ivtv ** 2), np.sqrt(S_u ** 2 + S_v ** 2), L + 7, TINY_SPEED), iwv=(iwv, S_w, L, TINY_SUM))


def column_weights(levels_hpa):
    """w_k = 100 dp_k / g: trapezoid in pressure, half an interval at the ends (float64)."""
    p = [float(x) for x in levels_hpa]
    n = len(p)
    w = []
    for k in range(n):
        lo = p[k - 1] if k > 0 else p[k]
        hi = p[k + 1] if k + 1 < n else p[k]
        w.append(100.0 * 0.5 * (hi - lo) / G)
    return np.array(w)


def row_table(lat, lon):
    """(rowc float32 (H, 4), edge_first, edge_last) from the header's formulas."""
    lat = np.asarray(lat, np.float64)
    H, W = lat.size, len(lon)
    dlam = 2.0 * np.pi / W
    phi = np.deg2rad(lat)
    rowc = np.zeros((H, 4))
    edges = {}
    for j in range(H):
        edge = j == 0 or j == H - 1
        if edge and abs(lat[j]) == 90.0:
            r = 1 if j == 0 else H - 2
            f = np.cos(phi[r]) / (A_M * (1.0 - abs(np.sin(phi[r]))))
            f = f if lat[j] > 0 else -f
            rowc[j] = [f, -f, 0, 0]
            edges[j] = POLE
            continue
        n, s = (j + 1 if j + 1 < H else j), (j - 1 if j > 0 else j)
        if edge:
            edges[j] = ONESIDED
        den = A_M * np.cos(phi[j]) * (phi[n] - phi[s])
        rowc[j] = [1.0 / (2 * A_M * np.cos(phi[j]) * dlam), np.cos(phi[n]) / den, np.cos(phi[s]) / den, np.sign(lat[j])]
    return rowc.astype(np.float32), edges[0], edges[H - 1]


def vortdiv(u, v, rowc, edge_first, edge_last, exact_rowc=None):
    """u, v: (H, W) -> {"vo": (value, bound), "div": (value, bound)} per point; the bound is the header's, pole rows included.
    ``exact_rowc``: float64 coefficients instead of the fp32 table (the analytic checks)."""
    u, v = np.asarray(u, np.float64) if exact_rowc is not None else f64(u), np.asarray(v, np.float64) if exact_rowc is not None else f64(v)
    rc = np.asarray(exact_rowc, np.float64) if exact_rowc is not None else f64(rowc)
    H, W = u.shape
    jn, js = np.minimum(np.arange(H) + 1, H - 1), np.maximum(np.arange(H) - 1, 0)
    A, Bp, Bm = rc[:, 0:1], rc[:, 1:2], rc[:, 2:3]
    e, w = lambda x: np.roll(x, -1, axis=1), lambda x: np.roll(x, 1, axis=1)      # noqa: E731
    vo = A * (e(v) - w(v)) - (Bp * u[jn] - Bm * u[js])
    S_vo = np.abs(A) * (np.abs(e(v)) + np.abs(w(v))) + np.abs(Bp * u[jn]) + np.abs(Bm * u[js])
    dv = A * (e(u) - w(u)) + (Bp * v[jn] - Bm * v[js])
    S_dv = np.abs(A) * (np.abs(e(u)) + np.abs(w(u))) + np.abs(Bp * v[jn]) + np.abs(Bm * v[js])
    b_vo, b_dv = bound(K_VORTDIV, S_vo, TINY_SUM), bound(K_VORTDIV, S_dv, TINY_SUM)
    for j, r, flag in ((0, 1, edge_first), (H - 1, H - 2, edge_last)):
        if flag == POLE:
            vo[j], dv[j] = rc[j, 0] * u[r].mean(), rc[j, 1] * v[r].mean()
            b_vo[j] = (U + SLACK64) * abs(rc[j, 0]) * np.abs(u[r]).mean() + TINY_SUM
            b_dv[j] = (U + SLACK64) * abs(rc[j, 1]) * np.abs(v[r]).mean() + TINY_SUM
    return dict(vo=(vo, b_vo), div=(dv, b_dv))
