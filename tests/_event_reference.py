"""Event verification restated in numpy int64 / float64 from the definitions of include/skyrim_event.h and skyrim_amd/events.py, by other
means than the code under test: windows are loops of ``np.roll`` (no prefix sums), and every score is the area-weighted mean of its
per-point definition (no joint table)."""
from __future__ import annotations

import numpy as np


def point_counts(x, y, thr):
    """k (H, W) int64 = members above, o (H, W) int64 = truth above; x (M, H, W), y (H, W) float32.  A NaN compares false."""
    thr = np.float32(thr)
    with np.errstate(invalid="ignore"):
        return (np.asarray(x, np.float32) > thr).sum(axis=0).astype(np.int64), (np.asarray(y, np.float32) > thr).astype(np.int64)


def joint_counts(k, o, M):
    """counts[j][o][k] int64 (H, 2, M + 1)."""
    H = k.shape[0]
    out = np.zeros((H, 2, M + 1), np.int64)
    for j in range(H):
        np.add.at(out[j], (o[j], k[j]), 1)
    return out


def window_sums(k, o, hy, hx):
    """(Sf, So, n): the window sums of k and o (H, W) int64 and the window's points n (H,); hy rows, hx[j] columns either side, the
    columns periodic and hx clamped to (W - 1) // 2."""
    H, W = k.shape
    Sf, So, n = np.zeros_like(k), np.zeros_like(o), np.zeros(H, np.int64)
    for j in range(H):
        r0, r1 = max(j - hy, 0), min(j + hy, H - 1)
        h = int(min(max(int(hx[j]), 0), (W - 1) // 2))
        cf, co = k[r0:r1 + 1].sum(axis=0), o[r0:r1 + 1].sum(axis=0)
        for dx in range(-h, h + 1):
            Sf[j] += np.roll(cf, dx)
            So[j] += np.roll(co, dx)
        n[j] = (r1 - r0 + 1) * (2 * h + 1)
    return Sf, So, n


def row_sums(k, o, M, hy, hx):
    """sums[j] = (sum_i (Sf - M So)^2, sum_i Sf^2, sum_i (M So)^2) int64 (H, 3), and n (H,)."""
    Sf, So, n = window_sums(k, o, hy, hx)
    return np.stack([((Sf - M * So) ** 2).sum(axis=1), (Sf ** 2).sum(axis=1), ((M * So) ** 2).sum(axis=1)], axis=1), n


def wmean(field, w):
    """The area mean of a (H, W) field with the latitude weights w."""
    field, w = np.asarray(field, np.float64), np.asarray(w, np.float64)
    return float((w[:, None] * field).sum() / (field.shape[1] * w.sum()))


def scores(k, o, M, w):
    """Every point-wise score from its per-point definition."""
    f, ob = k / M, o.astype(np.float64)
    nan = float("nan")
    div = lambda a, b: a / b if b != 0 else nan      # noqa: E731
    s = dict(base_rate=wmean(ob, w), brier=wmean((f - ob) ** 2, w))
    base = s["base_rate"]
    rel = res = 0.0
    obs, weight = [], []
    for kk in range(M + 1):
        mask = k == kk
        n = wmean(mask, w)
        obar = div(wmean(mask * ob, w), n)
        obs.append(obar)
        weight.append(n)
        if n > 0:
            rel += n * (kk / M - obar) ** 2
            res += n * (obar - base) ** 2
    s.update(reliability=rel, resolution=res, uncertainty=base * (1 - base), observed_frequency=np.array(obs), weight=np.array(weight))
    pod = np.array([div(wmean((k >= i) * ob, w), base) for i in range(M + 2)])
    pofd = np.array([div(wmean((k >= i) * (1 - ob), w), wmean(1 - ob, w)) for i in range(M + 2)])
    area = 0.0                                       # the trapezoid rule from (0, 0) at i = M + 1 up to (1, 1) at i = 0
    for i in range(M + 1, 0, -1):
        area += (pofd[i - 1] - pofd[i]) * (pod[i - 1] + pod[i]) / 2
    s.update(pod_curve=pod, pofd_curve=pofd, auc=float(area))
    if M > 1:
        s["brier_fair"] = s["brier"] - wmean(k * (M - k) / (M * M * (M - 1)), w)
    else:
        a, b, c = wmean((k == 1) & (o == 1), w), wmean((k == 1) & (o == 0), w), wmean((k == 0) & (o == 1), w)
        chance = (a + b) * (a + c)
        s.update(pod=div(a, a + c), far=div(b, a + b), csi=div(a, a + b + c), ets=div(a - chance, a + b + c - chance),
                 frequency_bias=div(a + b, a + c))
    return s


def fss(k, o, M, hy, hx, w):
    Sf, So, n = window_sums(k, o, hy, hx)
    Pf, Po = Sf / (M * n[:, None]), So / n[:, None]
    den = wmean(Pf ** 2, w) + wmean(Po ** 2, w)
    return 1 - wmean((Pf - Po) ** 2, w) / den if den != 0 else float("nan")


def case(M, shape, seed, quantum=0.25):
    """Members (M, C, H, W) and a truth (C, H, W) float32 on a coarse lattice of values (multiples of ``quantum``), so that values EQUAL to
    a threshold on that lattice occur in members and truth; smooth in space plus noise, so that windows see structure."""
    C, H, W = shape
    rng = np.random.default_rng(seed)
    jj, ii = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    base = 2.0 * np.sin(2 * np.pi * ii / max(W, 2) * 3 + 0.3) * np.cos(np.pi * (jj + 0.5) / H)
    q = lambda a: (np.round(a / quantum) * quantum).astype(np.float32)      # noqa: E731
    y = q(base[None] + 0.5 * rng.standard_normal((C, H, W)))
    x = q(base[None, None] + 0.2 * rng.standard_normal((1, C, H, W)) + 0.7 * rng.standard_normal((M, C, H, W)))
    return x, y
