"""Float64 restatement of regridding (include/skyrim_regrid.h, skyrim_amd/regrid.py), written independently of both: the weights of the
three methods as dense (n_out, n_src) matrices -- the conservative ones as overlap integrals by direct interval arithmetic, cell against
cell -- the operation on tables, and the header's bound  k u S + tiny,  k = nr + nc + 1,  u = 2^-24,  tiny = 2^-126."""
from __future__ import annotations

import math

import numpy as np

U = 2.0 ** -24
TINY = 2.0 ** -126
MAX_TAPS = 32


# ---- cells -------------------------------------------------------------------------------------------------------------------------------- #
def lat_cells(lat):
    """[(lo, hi)] in sin(latitude) per row: bounds midway between neighbours, the outer ones half a spacing beyond, clipped to the poles."""
    lat = [float(v) for v in lat]
    n = len(lat)
    cells = []
    for j in range(n):
        a = (lat[j - 1] + lat[j]) / 2 if j > 0 else lat[0] - (lat[1] - lat[0]) / 2
        b = (lat[j] + lat[j + 1]) / 2 if j < n - 1 else lat[-1] + (lat[-1] - lat[-2]) / 2
        a, b = max(-90.0, min(90.0, a)), max(-90.0, min(90.0, b))
        sa, sb = math.sin(math.radians(a)), math.sin(math.radians(b))
        cells.append((min(sa, sb), max(sa, sb)))
    return cells


def _eastward(lon):
    out, add = [], 0.0
    for k, v in enumerate(lon):
        v = float(v) % 360.0
        if k and v + add <= out[-1]:
            add += 360.0
        out.append(v + add)
    return out


def lon_cells(lon, periodic):
    """[(west, east)] in degrees, eastward: bounds midway between neighbours; the outer ones close the circle (``periodic``) or lie half
    a spacing beyond."""
    u = _eastward(lon)
    n = len(u)
    cells = []
    for i in range(n):
        if periodic:
            w = (u[i - 1] + u[i]) / 2 if i > 0 else (u[-1] - 360.0 + u[0]) / 2
            e = (u[i] + u[i + 1]) / 2 if i < n - 1 else (u[-1] + u[0] + 360.0) / 2
        else:
            w = (u[i - 1] + u[i]) / 2 if i > 0 else u[0] - (u[1] - u[0]) / 2
            e = (u[i] + u[i + 1]) / 2 if i < n - 1 else u[-1] + (u[-1] - u[-2]) / 2
        cells.append((w, e))
    return cells


def _overlap(a, b, c, d):
    return max(0.0, min(b, d) - max(a, c))


# ---- the weights, dense ------------------------------------------------------------------------------------------------------------------- #
def conservative_rows(src_lat, dst_lat):
    """(A, coverage): A[J, j] = overlap of the cells in sin(lat) / the covered part of cell J; coverage[J] = covered share."""
    s, d = lat_cells(src_lat), lat_cells(dst_lat)
    A, cov = np.zeros((len(d), len(s))), np.zeros(len(d))
    for J, (lo, hi) in enumerate(d):
        for j, (a, b) in enumerate(s):
            A[J, j] = _overlap(lo, hi, a, b)
        cov[J] = A[J].sum() / (hi - lo)
        A[J] /= A[J].sum()
    return A, cov


def conservative_cols(src_lon, dst_lon):
    s, d = lon_cells(src_lon, True), lon_cells(dst_lon, False)
    A = np.zeros((len(d), len(s)))
    for I, (w, e) in enumerate(d):
        for i, (a, b) in enumerate(s):
            A[I, i] = sum(_overlap(w, e, a + 360.0 * k, b + 360.0 * k) for k in (-2, -1, 0, 1, 2))
        A[I] /= A[I].sum()
    return A


def bilinear_rows(src_lat, dst_lat):
    src = [float(v) for v in src_lat]
    A = np.zeros((len(dst_lat), len(src)))
    for J, phi in enumerate(float(v) for v in dst_lat):
        for j in range(len(src) - 1):
            a, b = src[j], src[j + 1]
            if min(a, b) - 1e-9 <= phi <= max(a, b) + 1e-9:
                t = min(1.0, max(0.0, (phi - a) / (b - a)))
                A[J, j], A[J, j + 1] = 1.0 - t, t
                break
        else:
            raise ValueError(f"row {J} outside the source")
    return A


def bilinear_cols(src_lon, dst_lon):
    u = _eastward(src_lon)
    n = len(u)
    A = np.zeros((len(dst_lon), n))
    for I, lam in enumerate(float(v) for v in dst_lon):
        x = u[0] + (lam - u[0]) % 360.0
        for i in range(n):
            a, b = u[i], (u[i + 1] if i < n - 1 else u[0] + 360.0)
            if a <= x <= b:
                t = (x - a) / (b - a)
                A[I, i] += 1.0 - t
                A[I, (i + 1) % n] += t
                break
    return A


def nearest_rows(src_lat, dst_lat):
    A = np.zeros((len(dst_lat), len(src_lat)))
    for J, phi in enumerate(dst_lat):
        best = min(range(len(src_lat)), key=lambda j: (abs(float(src_lat[j]) - float(phi)), j))
        A[J, best] = 1.0
    return A


def nearest_cols(src_lon, dst_lon):
    A = np.zeros((len(dst_lon), len(src_lon)))
    for I, lam in enumerate(dst_lon):
        dist = lambda i: abs((float(src_lon[i]) - float(lam) + 180.0) % 360.0 - 180.0)      # noqa: E731
        A[I, min(range(len(src_lon)), key=lambda i: (dist(i), i))] = 1.0
    return A


def matrices(src_lat, src_lon, dst_lat, dst_lon, method):
    """(rows (Ho, H), cols (Wo, W)) float64."""
    if method == "conservative":
        return conservative_rows(src_lat, dst_lat)[0], conservative_cols(src_lon, dst_lon)
    if method == "bilinear":
        return bilinear_rows(src_lat, dst_lat), bilinear_cols(src_lon, dst_lon)
    return nearest_rows(src_lat, dst_lat), nearest_cols(src_lon, dst_lon)


def area_weights(lat):
    return np.array([hi - lo for lo, hi in lat_cells(lat)])


def area_mean(x, lat):
    w = area_weights(lat)
    return float((w[:, None] * np.asarray(x, np.float64)).sum() / (w.sum() * x.shape[-1]))


# ---- the operation on tables ---------------------------------------------------------------------------------------------------------------- #
def taps(start, count, n_src, periodic):
    """Per output the source indices its taps read."""
    return [[(int(s) + t) % n_src if periodic else int(s) + t for t in range(int(n))] for s, n in zip(start, count)]


def apply(x, rows, cols):
    """(exact, bound) float64 (Ho, Wo) of one fp32 plane x (H, W) under the tables ``rows`` / ``cols`` = (start, count, weight fp32
    (n, 32)): exact arithmetic (float64) on the same fp32 inputs and fp32 weights, S = sum sum |wr wc x|, k = nr + nc + 1."""
    x = np.asarray(x, np.float64)
    H, W = x.shape
    (rs, rn, rw), (cs, cn, cw) = rows, cols
    R = np.zeros((len(rs), H))
    for J, idx in enumerate(taps(rs, rn, H, False)):
        for t, j in enumerate(idx):
            R[J, j] += float(rw[J, t])
    Cm = np.zeros((len(cs), W))
    for I, idx in enumerate(taps(cs, cn, W, True)):
        for t, i in enumerate(idx):
            Cm[I, i] += float(cw[I, t])
    with np.errstate(invalid="ignore"):
        exact = R @ x @ Cm.T
        S = np.abs(R) @ np.abs(x) @ np.abs(Cm).T
    k = np.asarray(rn, np.float64)[:, None] + np.asarray(cn, np.float64)[None, :] + 1.0
    return exact, k * U * S + TINY


def reached(rows, cols, H, W, j, i):
    """The boolean (Ho, Wo) set of outputs whose taps read the source point (j, i)."""
    (rs, rn, _), (cs, cn, _) = rows, cols
    r = np.array([j in idx for idx in taps(rs, rn, H, False)])
    c = np.array([i in idx for idx in taps(cs, cn, W, True)])
    return r[:, None] & c[None, :]
