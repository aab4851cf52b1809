"""NumPy restatements of include/skyrim_ens.h, written from the header's text: Philox4x32-10, the uniforms and Box-Muller pairs of
``skens_perturb`` in float64, and every statistic of ``skens_stats`` in float64."""
from __future__ import annotations

import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF


def philox4x32_10(ctr, key):
    """ctr: (..., 4) uint32, key: (2,) or (..., 2) uint32 -> (..., 4) uint32."""
    c = [np.asarray(ctr)[..., i].astype(np.uint64) for i in range(4)]
    key = np.asarray(key)
    k0, k1 = key[..., 0].astype(np.uint64), key[..., 1].astype(np.uint64)
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]
        hi0, lo0, hi1, lo1 = p0 >> 32, p0 & MASK, p1 >> 32, p1 & MASK
        c = [hi1 ^ c[1] ^ k0, lo1, hi0 ^ c[3] ^ k1, lo0]
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return np.stack(c, axis=-1).astype(np.uint32)


def uniform(r):
    return ((np.asarray(r, np.uint32) >> 8).astype(np.float64) + 0.5) * 2.0 ** -24


def normals(seed: int, member: int, n: int) -> np.ndarray:
    """z(seed, member, i) for i < n, float64."""
    g = np.arange((n + 3) // 4, dtype=np.uint64)
    ctr = np.zeros((g.size, 4), np.uint32)
    ctr[:, 0] = (g & MASK).astype(np.uint32)
    ctr[:, 1] = (g >> 32).astype(np.uint32)
    r = philox4x32_10(ctr, np.array([seed, member], np.uint32))
    u = uniform(r)
    z = np.empty((g.size, 4))
    for a, b, e in ((0, 1, 0), (2, 3, 2)):
        rad = np.sqrt(-2.0 * np.log(u[:, a]))
        z[:, e] = rad * np.cos(2.0 * np.pi * u[:, b])
        z[:, e + 1] = rad * np.sin(2.0 * np.pi * u[:, b])
    return z.reshape(-1)[:n]


def perturb(x0: np.ndarray, std: np.ndarray, chan_stride: int, scale: float, seed: int, member: int) -> np.ndarray:
    """Member ``member`` of the flat (L, C, H, W) state ``x0`` in float64 (member 0: x0 itself)."""
    x = np.asarray(x0, np.float64).reshape(-1)
    if member == 0:
        return x.copy()
    c = (np.arange(x.size) // chan_stride) % len(std)
    return x + float(scale) * np.asarray(std, np.float64)[c] * normals(seed, member, x.size)


def stats(x: np.ndarray, thresholds=(), levels=()):
    """x: (M, n) float32 member values -> dict of float64 statistics (exceed: (K, n), quant: (Q, n), order: sorted members)."""
    x32 = np.asarray(x, np.float32)
    x = x32.astype(np.float64)
    M = x.shape[0]
    mu = x.mean(axis=0)
    out = dict(mean=mu, spread=np.sqrt(((x - mu) ** 2).mean(axis=0)), min=x32.min(axis=0), max=x32.max(axis=0))
    out["exceed"] = np.stack([(x32 > np.float32(t)).sum(axis=0).astype(np.float32) / np.float32(M) for t in thresholds]) if len(thresholds) else None
    s = np.sort(x, axis=0)
    out["order"] = s
    q = []
    for lev in levels:
        h = (M - 1) * float(lev)
        k = min(int(np.floor(h)), M - 1)
        k1 = min(k + 1, M - 1)
        q.append((s[k] + (h - k) * (s[k1] - s[k]), np.maximum(np.abs(s[k]), np.abs(s[k1]))))
    out["quant"] = q
    return out


def mean_bound(x: np.ndarray, mu: np.ndarray) -> np.ndarray:
    """2u|mu| + M u D  with u = 2^-24, D = max_m |x_m - x_0|."""
    x = np.asarray(x, np.float64)
    u = 2.0 ** -24
    return 2 * u * np.abs(mu) + x.shape[0] * u * np.abs(x - x[0]).max(axis=0)


def spread_bound(x: np.ndarray, s: np.ndarray) -> np.ndarray:
    """4u D + M u s."""
    x = np.asarray(x, np.float64)
    u = 2.0 ** -24
    return 4 * u * np.abs(x - x[0]).max(axis=0) + x.shape[0] * u * s
