"""Float64 NumPy restatement of include/skyrim_score.h, written from the header's text: the per-point quantities, the area means, the
magnitudes S of the header's bounds, and ``area_weights`` (WeatherBench 2's cell-area weights)."""
from __future__ import annotations

import numpy as np

U = 2.0 ** -24
SLACK64 = 2.0 ** -40


def area_weights(lat):
    """w_j = sin(ub_j) - sin(lb_j): bounds midway between neighbours, the outer two half a spacing out, clipped to +-90 degrees."""
    lat = np.asarray(lat, np.float64)
    if lat.size == 1:
        return np.ones(1)
    lo, hi = np.empty_like(lat), np.empty_like(lat)
    for j in range(lat.size):
        before = lat[j - 1] if j > 0 else lat[0] - (lat[1] - lat[0])
        after = lat[j + 1] if j + 1 < lat.size else lat[-1] + (lat[-1] - lat[-2])
        a, b = (lat[j] + before) / 2, (lat[j] + after) / 2
        lo[j], hi[j] = max(min(a, b), -90.0), min(max(a, b), 90.0)
    return np.sin(np.deg2rad(hi)) - np.sin(np.deg2rad(lo))


def area_mean(t, w):
    """<t> = sum_j w_j sum_i t_ji / (W sum_j w_j) over the last two axes."""
    w = np.asarray(w, np.float64)
    return (t.sum(axis=-1) * w).sum(axis=-1) / (t.shape[-1] * w.sum())


def point_terms(x, y, c=None):
    """x: (M, ...) members, y: truth, c: climatology or None, float32 inputs -> dict of float64 per-point quantities."""
    x, y = np.asarray(x, np.float32).astype(np.float64), np.asarray(y, np.float32).astype(np.float64)
    M = x.shape[0]
    e = x - y
    t = dict(eb=e.sum(axis=0) / M, A=np.abs(e).sum(axis=0) / M)
    d = x - x[0]
    D = np.abs(d).sum(axis=0) / M
    t["v"] = ((d - d.sum(axis=0) / M) ** 2).sum(axis=0) / (M - 1) if M > 1 else np.zeros_like(y)
    t["Sv"] = ((np.abs(d) + D) ** 2).sum(axis=0) / (M - 1) if M > 1 else np.zeros_like(y)
    s = np.sort(x, axis=0)
    B = np.zeros_like(y)
    for i in range(M - 1):
        B += (i + 1) * (M - 1 - i) * (s[i + 1] - s[i])
    t["B"] = B / (M * (M - 1)) if M > 1 else B
    t["r"] = (np.asarray(x, np.float64) < y).sum(axis=0)
    if c is not None:
        t["a"] = y - np.asarray(c, np.float32).astype(np.float64)
        t["f"] = t["eb"] + t["a"]
    return t


def scores(x, y, w, c=None):
    """Per channel: x (M, C, H, W), y (C, H, W), w (H,) -> ({slot: (C,) float64}, {slot: (C,) bound}, counts (C, H, M + 1))."""
    t = point_terms(x, y, c)
    M = np.asarray(x).shape[0]
    m = lambda q: area_mean(q, w)      # noqa: E731
    A, B = m(t["A"]), m(t["B"])
    val = dict(bias=m(t["eb"]), mae=m(np.abs(t["eb"])), mse=m(t["eb"] ** 2), var=m(t["v"]), abs=A, pair=B, crps=A - B)
    S = dict(bias=A, mae=A, mse=m(t["A"] ** 2), var=m(t["Sv"]), abs=A, pair=B, crps=A + B)
    k = dict(bias=M + 1, mae=M + 1, mse=2 * M + 3, var=2 * M + 7, abs=M + 1, pair=M + 1, crps=M + 1)
    if c is not None:
        a, f, g = t["a"], t["f"], t["A"] + np.abs(t["a"])
        val.update(fa=m(f * a), ff=m(f * f), aa=m(a * a))
        S.update(fa=m(g * np.abs(a)), ff=m(g * g), aa=m(a * a))
        k.update(fa=M + 4, ff=2 * M + 5, aa=3)
    bound = {q: (k[q] * U + SLACK64) * S[q] for q in val}
    assert all(k[q] <= 64 + 2 * M for q in k)                        # the cap every bound of the header stays under
    r = t["r"]
    counts = np.stack([(r == q).sum(axis=-1) for q in range(M + 1)], axis=-1)
    return val, bound, counts


def table(val, M):
    """The host's metrics from the sums."""
    out = dict(bias=val["bias"], mae=val["mae"], rmse=np.sqrt(val["mse"]), crps=val["crps"])
    if "fa" in val:
        out["acc"] = val["fa"] / np.sqrt(val["ff"] * val["aa"])
    if M > 1:
        out["spread"] = np.sqrt(val["var"])
        out["ssr"] = np.sqrt((M + 1) / M) * out["spread"] / out["rmse"]
    return out


def rank_frequencies(counts, w, W):
    w = np.asarray(w, np.float64)
    return np.einsum("j,cjr->cr", w, counts.astype(np.float64)) / (W * w.sum())
