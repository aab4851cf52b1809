"""Numpy restatements of include/skyrim_gram.h and of the host algebra of skyrim_amd/scenarios.py, written from the definitions: the
Gram matrix and the bound's S in float64 from the members, the member combination in fp32 operation by operation, and centring, Ward's
clustering, EOFs and the energy score made DIRECTLY FROM THE MEMBERS' FIELDS, not from a Gram matrix."""
from __future__ import annotations

import numpy as np


def columns(i0, ni, W):
    return (i0 + np.arange(ni)) % W


def differences(members, truth, channel, region):
    """(M', nj, ni) float64 of the fp32 differences d_m = x_m - x_0 (and y - x_0) over the region."""
    j0, nj, i0, ni = region
    W = members[0].shape[-1]
    cols = columns(i0, ni, W)
    x = [np.asarray(m, np.float32)[channel, j0:j0 + nj][:, cols] for m in members]
    if truth is not None:
        x.append(np.asarray(truth, np.float32)[channel, j0:j0 + nj][:, cols])
    with np.errstate(invalid="ignore", over="ignore"):
        return np.stack([(v - x[0]).astype(np.float32) for v in x]).astype(np.float64)


def gram(members, truth, channels, region, weights):
    """(Gd, S): float64 (nc, M', M') of sum_j w_j sum_i d_m d_n and of sum_j |w_j| sum_i |d_m| |d_n|."""
    j0, nj, _, _ = region
    w = np.asarray(weights, np.float64)[j0:j0 + nj]
    G, S = [], []
    for c in channels:
        d = differences(members, truth, c, region)
        with np.errstate(invalid="ignore", over="ignore"):
            G.append(np.einsum("mji,nji,j->mn", d, d, w))
            S.append(np.einsum("mji,nji,j->mn", np.abs(d), np.abs(d), np.abs(w)))
    return np.stack(G), np.stack(S)


def combine(members, channels, coef, b):
    """float32 (K, nc, H, W): acc = b_k x_0; acc = acc + coef[k, m] (x_m - x_0) for m = 1 .. M - 1, every operation rounded to fp32."""
    coef, b = np.asarray(coef, np.float32), np.asarray(b, np.float32)
    K, M = coef.shape
    x = [np.asarray(m, np.float32)[list(channels)] for m in members]
    out = np.empty((K,) + x[0].shape, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(K):
            acc = (b[k] * x[0]).astype(np.float32)
            for m in range(1, M):
                d = (x[m] - x[0]).astype(np.float32)
                p = (coef[k, m] * d).astype(np.float32)
                acc = (acc + p).astype(np.float32)
            out[k] = acc
    return out


# ---- the host algebra from the members' fields ------------------------------------------------------------------------------------------ #
def anomalies(members, truth, channels, region, weights, normalise="spread", std=None):
    """(A, ay): the members' anomalies about the ensemble mean as float64 vectors (M, n) scaled so that a plain dot product is the
    area-mean, channel-normalised inner product, and the truth's anomaly about the same mean (or None)."""
    j0, nj, i0, ni = region
    W = members[0].shape[-1]
    cols = columns(i0, ni, W)
    w = np.asarray(weights, np.float64)[j0:j0 + nj]
    area = w.sum() * ni
    M = len(members)
    parts, yparts = [], []
    for k, c in enumerate(channels):
        x = np.stack([np.asarray(m, np.float32)[c, j0:j0 + nj][:, cols].astype(np.float64) for m in members])
        mean = x.mean(axis=0)
        a = (x - mean) * np.sqrt(w / area)[None, :, None]
        var = (a ** 2).sum() / (M - 1)
        scale = dict(spread=var if var > 0 else 1.0, none=1.0, std=None if std is None else float(std[k]) ** 2)[normalise]
        parts.append(a.reshape(M, -1) / np.sqrt(scale))
        if truth is not None:
            y = np.asarray(truth, np.float32)[c, j0:j0 + nj][:, cols].astype(np.float64)
            yparts.append(((y - mean) * np.sqrt(w / area)[:, None]).reshape(-1) / np.sqrt(scale))
    return np.concatenate(parts, axis=1), (np.concatenate(yparts) if truth is not None else None)


def ward(A, n_clusters, gaps=None):
    """Ward's clustering from the vectors: at every step the two clusters whose merge adds the least within-cluster sum of squares,
    n_i n_j / (n_i + n_j) |c_i - c_j|^2, are merged; labels by size descending, then lowest member.  ``gaps``: a list that receives, per
    merge, (second cheapest cost - cheapest cost) / the total sum of squares: how far each decision is from going the other way."""
    M = A.shape[0]
    total = ((A - A.mean(axis=0)) ** 2).sum()
    groups = [[m] for m in range(M)]
    while len(groups) > n_clusters:
        costs = []
        for x in range(len(groups)):
            for y in range(x + 1, len(groups)):
                ci, cj = A[groups[x]].mean(axis=0), A[groups[y]].mean(axis=0)
                ni, nj = len(groups[x]), len(groups[y])
                costs.append((ni * nj / (ni + nj) * ((ci - cj) ** 2).sum(), x, y))
        costs.sort(key=lambda t: t[0])                       # (stable: of equal costs the first pair in ascending (x, y))
        if gaps is not None and len(costs) > 1:
            gaps.append((costs[1][0] - costs[0][0]) / total)
        _, x, y = costs[0]
        groups[x] = sorted(groups[x] + groups[y])
        del groups[y]
        groups.sort(key=lambda g: g[0])
    groups.sort(key=lambda g: (-len(g), g[0]))
    labels = np.empty(M, np.int64)
    for c, g in enumerate(groups):
        labels[g] = c
    return labels


def representative_gap(A, labels):
    """The least (second smallest - smallest) squared distance to the centroid over the clusters of three or more members (the two members of a pair are always equally far), relative to the
    total sum of squares: how far each choice of a representative is from going the other way."""
    total = ((A - A.mean(axis=0)) ** 2).sum()
    gap = np.inf
    for c in range(int(labels.max()) + 1):
        idx = np.nonzero(labels == c)[0]
        if idx.size >= 3:
            d2 = np.sort(((A[idx] - A[idx].mean(axis=0)) ** 2).sum(axis=1))
            gap = min(gap, (d2[1] - d2[0]) / total)
    return gap


def summarise(A, labels):
    """Sizes, probabilities, representatives (the member nearest its cluster's centroid; distances within 1e-12 of the total sum of squares
    of the smallest are equal, and the lowest index wins) and the within / total / explained sums of squares."""
    M, n = A.shape[0], int(labels.max()) + 1
    sizes, reps, within = [], [], 0.0
    tie = 1e-12 * (A ** 2).sum()
    for c in range(n):
        idx = np.nonzero(labels == c)[0]
        d2 = ((A[idx] - A[idx].mean(axis=0)) ** 2).sum(axis=1)
        sizes.append(idx.size)
        reps.append(int(idx[int(np.nonzero(d2 <= d2.min() + tie)[0][0])]))
        within += d2.sum()
    total = (A ** 2).sum()
    return dict(sizes=np.asarray(sizes), probability=np.asarray(sizes) / M, representative=np.asarray(reps), within=within, total=total,
                explained=total - within)


def eofs(A, n):
    """SVD of the anomalies: variance fractions, PCs (M, n) with the largest-magnitude entry of each positive, patterns (n, points)."""
    M = A.shape[0]
    U, s, Vt = np.linalg.svd(A, full_matrices=False)
    lam = s ** 2 / (M - 1)
    frac = lam / lam.sum()
    pcs = U[:, :n] * s[:n]
    pat = Vt[:n].copy()
    for k in range(n):
        if pcs[int(np.argmax(np.abs(pcs[:, k]))), k] < 0:
            pcs[:, k], pat[k] = -pcs[:, k], -pat[k]
    return frac[:n], pcs, pat


def energy_score(A, ay):
    """The fair energy score by the pairwise-norm formula."""
    M = A.shape[0]
    first = np.mean([np.linalg.norm(A[m] - ay) for m in range(M)])
    second = sum(np.linalg.norm(A[m] - A[n]) for m in range(M) for n in range(M) if m != n) / (2.0 * M * (M - 1))
    return first - second


def nearest_cluster(A, ay, labels):
    return int(np.argmin([((A[labels == c].mean(axis=0) - ay) ** 2).sum() for c in range(int(labels.max()) + 1)]))
