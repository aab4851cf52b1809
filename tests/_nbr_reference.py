"""A numpy restatement of include/skyrim_nbr.h, driven by ``neighbourhood.discs``: MAX, MIN and FRAC_ABOVE restated exactly (shifted
copies of the source rows, not the kernel's doubling table or prefixes), MEAN in exact arithmetic (``math.fsum`` per row of a disc, the
weighted quotient in rationals) as the reference its bound is measured against, and a brute-force builder of the discs that tests every
pair of nodes by the haversine distance."""
from __future__ import annotations

import math
from fractions import Fraction

import numpy as np

from skyrim_amd import neighbourhood as N

QNAN = np.float32(np.nan)
assert QNAN.view(np.uint32) == 0x7FC00000


def grid(H, W, south_pole=True):
    """Latitudes from 90 down (to -90, or without the last row when ``south_pole`` is False), W longitudes from 0."""
    lat = np.linspace(90.0, -90.0, H if south_pole else H + 1)[:H]
    return lat, np.arange(W) * (360.0 / W)


# ---- the discs, pair by pair --------------------------------------------------------------------------------------------------------- #
def pair_distances(lat, lon) -> np.ndarray:
    """(H, W, H, W) float64: the haversine distance in km between every two nodes, cos(lat) of a pole row exactly 0."""
    phi, c = np.deg2rad(np.asarray(lat, np.float64)), N._cos_lat(np.asarray(lat, np.float64))
    lam = np.deg2rad(np.asarray(lon, np.float64))
    return N.haversine_km(phi[:, None, None, None], phi[None, None, :, None], lam[None, None, None, :] - lam[None, :, None, None],
                          c[:, None, None, None], c[None, None, :, None])


def brute_sets(lat, lon, radius_km) -> np.ndarray:
    """(H, W, H, W) bool: node (r, c) lies within ``radius_km`` of node (j, i)."""
    return pair_distances(lat, lon) <= float(radius_km)


def table_sets(reach, half, W) -> np.ndarray:
    """(H, W, H, W) bool: the sets S(j, i) a disc table names, point by point."""
    H = half.shape[0]
    S = np.zeros((H, W, H, W), bool)
    for j in range(H):
        for d in range(-reach, reach + 1):
            n, r = int(half[j, reach + d]), j + d
            if n < 0:
                continue
            assert 0 <= r < H, "a table names a row off the grid"
            for i in range(W):
                if 2 * n + 1 >= W:
                    S[j, i, r, :] = True
                else:
                    S[j, i, r, np.arange(i - n, i + n + 1) % W] = True
    return S


# ---- MAX, MIN, FRAC_ABOVE ------------------------------------------------------------------------------------------------------------ #
def _fold(x, reach, half, init, combine, whole):
    """(H, W): ``combine`` over the points of every disc of the plane ``x``; ``whole(rows)``: the fold of whole rows, (R, 1)."""
    H, W = x.shape
    acc = np.full((H, W), init, x.dtype)
    for d in range(-reach, reach + 1):
        n = half[:, reach + d].astype(np.int64)
        rows = np.nonzero(n >= 0)[0]
        if rows.size == 0:
            continue
        src, nn = x[rows + d], n[rows]
        full = 2 * nn + 1 >= W
        if full.any():
            acc[rows[full]] = combine(acc[rows[full]], whole(src[full]))
        for s in range(0, int(nn[~full].max()) + 1 if (~full).any() else 0):
            sel = ~full & (nn >= s)
            acc[rows[sel]] = combine(acc[rows[sel]], np.roll(src[sel], s, axis=1))
            if s:
                acc[rows[sel]] = combine(acc[rows[sel]], np.roll(src[sel], -s, axis=1))
    return acc


def count(mask, reach, half):
    """(H, W) int64: the points of every disc at which ``mask`` holds."""
    return _fold(mask.astype(np.int64), reach, half, 0, np.add, lambda rows: rows.sum(axis=1, keepdims=True))


def one(x, kind, reach, half, thr=0.0):
    """One MAX, MIN or FRAC_ABOVE plane, float32 (H, W), of the float32 plane ``x``."""
    x = np.asarray(x, np.float32)
    nan = count(np.isnan(x), reach, half) > 0
    if kind == N.MAX:
        out = _fold(np.where(np.isnan(x), -np.inf, x).astype(np.float32), reach, half, -np.inf, np.maximum, lambda rows: rows.max(axis=1, keepdims=True))
    elif kind == N.MIN:
        out = _fold(np.where(np.isnan(x), np.inf, x).astype(np.float32), reach, half, np.inf, np.minimum, lambda rows: rows.min(axis=1, keepdims=True))
    elif kind == N.FRAC_ABOVE:
        with np.errstate(invalid="ignore"):
            above = count(x > np.float32(thr), reach, half)
        total = N.disc_points(half, x.shape[1])[:, None]
        out = (above.astype(np.float64) / total.astype(np.float64)).astype(np.float32)
    else:
        raise ValueError(kind)
    out = out.astype(np.float32)
    out[nan] = QNAN
    return out


def fields(x, ops, tables, fill):
    """The (M, D, H, W) output of the MAX, MIN and FRAC_ABOVE ops of ``ops`` over x (M, C, H, W); the slots of MEAN ops and the unnamed
    ones keep ``fill``.  ``tables``: (reach, half) per radius."""
    out = np.array(fill, np.float32, copy=True)
    for m in range(x.shape[0]):
        for op in ops:
            if op.kind != N.MEAN:
                out[m, op.out] = one(x[m, op.channel], op.kind, *tables[op.radius], op.thr)
    return out


# ---- MEAN ------------------------------------------------------------------------------------------------------------------------------ #
def mean_bound(exact, W, rows, ratio):
    """The header's bound of |mean - exact|: ``rows`` = R, the rows of the disc; ``ratio`` = sum_r w_r A_r / sum_r w_r n_r."""
    return 2.0 ** -24 * np.abs(exact) + 2.0 ** -149 + (3 * (W + 1) + 2 * rows + 8) * 2.0 ** -53 * ratio


def mean_exact(x, reach, half, weights, skip=None):
    """(exact, bound): the area-weighted mean over every disc of the float32 plane ``x`` in exact arithmetic, rounded once to float64 (NaN
    where the disc holds a non-finite value), and the header's bound at every point.  ``skip`` = ((j, i), (r, c)): the disc around (j, i)
    is summed without its point (r, c)."""
    x = np.asarray(x, np.float32)
    H, W = x.shape
    xd = x.astype(np.float64)
    finite = np.isfinite(xd)
    A = np.where(finite, np.abs(xd), 0.0).sum(axis=1)
    whole = [math.fsum(xd[r][finite[r]]) for r in range(H)]
    exact, bound = np.empty((H, W)), np.empty((H, W))
    wf = [Fraction(float(w)) for w in weights]
    for j in range(H):
        ds = [d for d in range(-reach, reach + 1) if half[j, reach + d] >= 0]
        for i in range(W):
            num, den, wa, bad = Fraction(0), Fraction(0), 0.0, False
            for d in ds:
                r, n = j + d, int(half[j, reach + d])
                if 2 * n + 1 >= W:
                    cols = np.arange(W)
                else:
                    cols = np.arange(i - n, i + n + 1) % W
                if skip is not None and skip[0] == (j, i) and skip[1][0] == r:
                    cols = cols[cols != skip[1][1]]
                    s = math.fsum(xd[r, cols][finite[r, cols]])
                elif cols.size == W:
                    s = whole[r]
                else:
                    s = math.fsum(xd[r, cols][finite[r, cols]])
                bad = bad or not finite[r, cols].all()
                num += wf[r] * Fraction(s)
                den += wf[r] * cols.size
                wa += float(weights[r]) * A[r]
            exact[j, i] = np.nan if bad else float(num / den)
            bound[j, i] = mean_bound(0.0 if bad else exact[j, i], W, len(ds), wa / float(den))
    return exact, bound


def case(M, C, H, W, seed=0, lo=1.0, hi=2.0):
    """(M, C, H, W) float32 in [lo, hi) with signs mixed on odd channels: no -0.0, |x| >= lo."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(lo, hi, (M, C, H, W)).astype(np.float32)
    x[:, 1::2] *= np.where(rng.random((M, len(range(1, C, 2)), H, W)) < 0.5, np.float32(-1), np.float32(1))
    return x
