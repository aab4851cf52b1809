"""numpy restatement of include/skyrim_point.h, written from the header: every product and every sum is a separate ``np.float32`` operation
in the header's order, so it is bit-equal to the kernel; a float64 evaluation of the same taps with the magnitude S of the header's bound;
and an independent float64 restatement of the station scores of ``points.PointForecast.verify`` with missing observations."""
from __future__ import annotations

import math

import numpy as np

U = 2.0 ** -24
TINY = 2.0 ** -126
REC = np.dtype([("row", "<i4"), ("col", "<i4"), ("nr", "<i4"), ("ncol", "<i4"), ("wr0", "<f4"), ("wr1", "<f4"), ("wc0", "<f4"), ("wc1", "<f4")])


def _taps(rec, H, W):
    """The header's clamps: (row, row1, col, col1, two rows?, two columns?)."""
    row = np.clip(rec["row"].astype(np.int64), 0, H - 1)
    col = np.mod(rec["col"].astype(np.int64), W)
    return row, np.minimum(row + 1, H - 1), col, np.mod(col + 1, W), rec["nr"] >= 2, rec["ncol"] >= 2


def gather(x, channels, rec):
    """x: (M, C, H, W) float32, rec: (P,) records -> (M, nc, P) float32, the operations of the header one by one."""
    x = np.asarray(x, np.float32)
    M, _, H, W = x.shape
    row, row1, col, col1, two_r, two_c = _taps(rec, H, W)
    wr0, wr1, wc0, wc1 = (rec[k].astype(np.float32) for k in ("wr0", "wr1", "wc0", "wc1"))
    out = np.empty((M, len(channels), rec.size), np.float32)
    with np.errstate(all="ignore"):
        for k, c in enumerate(channels):
            p = x[:, c]

            def v(cc):
                a = wr0 * p[:, row, cc]                                   # the accumulator starts as the first product
                b = wr1 * p[:, row1, cc]
                return np.where(two_r, (a + b).astype(np.float32), a)
            v0, v1 = v(col), v(col1)
            r = (wc0 * v0).astype(np.float32)
            t = (wc1 * v1).astype(np.float32)
            res = np.where(two_c, (r + t).astype(np.float32), r).astype(np.float32)
            # np.where keeps the bits of the branch it picks, NaN payloads included
            out[:, k] = res
    return out


def gather64(x, channels, rec):
    """(exact, S): the same taps in float64 (exact for fp32 inputs up to double rounding far below the bound) and S = sum |wc wr x|."""
    x = np.asarray(x, np.float32)
    M, _, H, W = x.shape
    row, row1, col, col1, two_r, two_c = _taps(rec, H, W)
    wr0, wr1, wc0, wc1 = (rec[k].astype(np.float64) for k in ("wr0", "wr1", "wc0", "wc1"))
    wr1, wc1 = np.where(two_r, wr1, 0.0), np.where(two_c, wc1, 0.0)
    at = lambda p, r, c: p[:, r, c].astype(np.float64)      # noqa: E731
    val = np.empty((M, len(channels), rec.size))
    S = np.empty_like(val)
    for k, c in enumerate(channels):
        p = x[:, c]
        terms = [wc0 * wr0 * at(p, row, col), wc0 * wr1 * np.where(two_r, at(p, row1, col), 0.0),
                 wc1 * wr0 * np.where(two_c, at(p, row, col1), 0.0), wc1 * wr1 * np.where(two_r & two_c, at(p, row1, col1), 0.0)]
        val[:, k] = terms[0] + terms[1] + terms[2] + terms[3]
        S[:, k] = sum(np.abs(t) for t in terms)
    return val, S


def bound(rec, S):
    """(nr + ncol + 1) u S + 2^-126 per point, broadcast over (M, nc, P)."""
    k = np.clip(rec["nr"], 1, 2).astype(np.float64) + np.clip(rec["ncol"], 1, 2) + 1
    return k * U * S + TINY


def station_scores(x, obs):
    """x: (M, T, C, P) member values, obs: (T, C, P) with NaN = missing -> dict of (T, C) arrays and rank_histogram (T, C, M + 1).
    Written point by point from the definitions: the error of the ensemble mean for bias / MAE / RMSE, the fair CRPS
    mean|x_m - y| - sum_{m, m'} |x_m - x_m'| / (2 M (M - 1)), the unbiased member variance for the spread, sqrt((M + 1) / M) spread / rmse,
    the rank = number of members below the observation; every valid point weighs the same."""
    x, obs = np.asarray(x, np.float64), np.asarray(obs, np.float64)
    M, T, C, P = x.shape
    out = {k: np.full((T, C), np.nan) for k in ("bias", "mae", "rmse", "crps", "spread", "ssr")}
    out["n"] = np.zeros((T, C), np.int64)
    out["rank_histogram"] = np.zeros((T, C, M + 1), np.int64)
    for t in range(T):
        for c in range(C):
            err, sq, ab, cr, var, n = [], [], [], [], [], 0
            for p in range(P):
                y = obs[t, c, p]
                if not np.isfinite(y):
                    continue
                xs = x[:, t, c, p]
                n += 1
                e = xs.mean() - y
                err.append(e), ab.append(abs(e)), sq.append(e * e)
                pair = sum(abs(a - b) for a in xs for b in xs)
                cr.append(np.abs(xs - y).mean() - (pair / (2 * M * (M - 1)) if M > 1 else 0.0))
                var.append(((xs - xs.mean()) ** 2).sum() / (M - 1) if M > 1 else 0.0)
                out["rank_histogram"][t, c, int((xs < y).sum())] += 1
            out["n"][t, c] = n
            if n:
                err, ab, sq, cr, var = (math.fsum(v) for v in (err, ab, sq, cr, var))      # sums over the points, exactly rounded
                out["bias"][t, c], out["mae"][t, c], out["rmse"][t, c], out["crps"][t, c] = err / n, ab / n, np.sqrt(sq / n), cr / n
                if M > 1:
                    out["spread"][t, c] = np.sqrt(var / n)
                    out["ssr"][t, c] = np.sqrt((M + 1) / M) * out["spread"][t, c] / out["rmse"][t, c]
    return out
