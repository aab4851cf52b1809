"""The numpy restatement of include/skyrim_breed.h and of ``breeding.factors``: what the kernels and the cycle are held to."""
from __future__ import annotations

import math

import numpy as np

U53 = 2.0 ** -53
SHAPES = [(2, 1, 1, 1), (3, 2, 5, 67), (5, 3, 9, 257), (64, 2, 4, 64), (2, 70, 3, 16)]       # (M, C, H, W)


def inputs(M, C, H, W, seed=0):
    """(y0 (C, H, W), members (M, C, H, W), weights (H,)): fields of size ~1 + 1e-2 noise per member, weights like cos(lat), all > 0."""
    rng = np.random.default_rng([seed, M, C, H, W])
    y0 = rng.standard_normal((C, H, W)).astype(np.float32)
    mem = (y0[None] + 1e-2 * rng.standard_normal((M, C, H, W))).astype(np.float32)
    w = np.cos(np.linspace(-1.4, 1.4, H)) + 0.01
    return y0, mem, w.astype(np.float64)


def norms(y0, members, w):
    """(S, T): S[m][c] = sum_j w_j sum_i d^2 with d one fp32 subtraction, the exact squares of a row summed with math.fsum and one float64
    product with w_j per row, the rows summed with math.fsum; T[m][c] = sum_j |w_j| sum_i d^2 the same way, the scale of the bound."""
    M, C, H, W = members.shape
    S, T = np.zeros((M, C)), np.zeros((M, C))
    for m in range(M):
        d = (members[m] - y0).astype(np.float32).astype(np.float64)             # fp32 subtraction, then exact in float64
        sq = d * d                                                              # 24 x 24 bits: exact
        for c in range(C):
            rows = [math.fsum(sq[c, j]) for j in range(H)]
            S[m, c] = math.fsum(w[j] * rows[j] for j in range(H))
            T[m, c] = math.fsum(abs(w[j]) * rows[j] for j in range(H))
    return S, T


def apply(x0, y0, members, f):
    """out[m] = x0 + f[m][c] * (members[m] - y0), three fp32 numpy operations each rounded on its own; a bit copy of x0 where f == 0."""
    out = np.empty_like(members)
    with np.errstate(all="ignore"):
        for m in range(members.shape[0]):
            t = (members[m] - y0).astype(np.float32)
            fm = f[m].astype(np.float32)[:, None, None]
            r = (fm * t).astype(np.float32)
            o = (x0 + r).astype(np.float32)
            out[m] = np.where(fm == 0, x0, o)
    return out


def factors(S, std, perturb_scale, norm, mask, weight_sum, n_lon):
    """``breeding.factors`` in numpy float64, rounded to fp32 once."""
    S = np.asarray(S, np.float64)
    std = np.asarray(std, np.float64).reshape(1, -1)
    on = std > 0
    if mask is not None:
        on = on & np.asarray(mask, bool).reshape(1, -1)
    A = S / (float(weight_sum) * float(n_lon))
    with np.errstate(all="ignore"):
        if norm == "channel":
            div = np.sqrt(A)
            f = np.where(on & (div != 0), perturb_scale * std / div, 0.0)
        else:
            rel = np.where(on, A / np.where(on, std * std, 1.0), 0.0)
            div = np.sqrt(rel.sum(axis=1, keepdims=True) / max(int(on.sum()), 1))
            f = np.where(on & (div != 0), np.broadcast_to(perturb_scale / div, A.shape), 0.0)
    return f.astype(np.float32)
