"""Two numpy restatements of include/skyrim_vert.h.

``fp32``: every operation on ``np.float32`` arrays in the header's order, with the header's ``sk_exp`` / ``sk_log`` (those of
tests/_thermo_reference.py): the kernel is compared with it bit for bit.
``f64``: the same algorithm in float64 with ``np.exp`` / ``np.log``: the yardstick the fp32 arithmetic is measured against
(tests/test_vert_cpu.py).  ``apply(..., consts=)`` hands it the fp32 host constants, so that it is exact arithmetic on the same inputs.

An op is a ``skyrim_amd.vertical.Op``; a state is (C, ...) with the columns on the trailing axes.
"""
from __future__ import annotations

import numpy as np

import _thermo_reference as TR

P, Z, Z_AGL, THETA, T = 1, 2, 3, 4, 5             # SKVERT_P ...
PLAIN, SPEED, THETA_F, PRESSURE = 1, 2, 3, 4      # SKVERT_PLAIN ...
NAN, NEAREST = 0, 1                               # SKVERT_NAN, SKVERT_NEAREST
NODE_NONE, NODE_ZS = -1, -2
NONE, LAYER, NODE_LAYER, LEVEL, NODE = 0, 1, 2, 3, 4      # where a result comes from
G = 9.80665


class Vert:
    def __init__(self, F):
        self.F, self.math = F, (TR.fp32 if F is np.float32 else TR.f64)
        self.KAPPA, self.LN1000 = F("0.2854"), self.math.log(F("1000"))

    def constants(self, pressures) -> tuple:
        """(lnp_k, ex_k)"""
        lnp = self.math.log(np.asarray(pressures, self.F))
        return lnp, self.math.exp(self.KAPPA * (self.LN1000 - lnp))

    @staticmethod
    def _crosses(a, b):
        return (((a >= 0) & (b <= 0)) | ((a <= 0) & (b >= 0))) & (a != b)

    def apply(self, op, state, zs=None, consts=None, info=None) -> dict:
        """{slot: plane} of one op.  ``info``: a dict that receives {(field, target): (mode, lower level, upper level)} -- the layer a
        result was taken from, for the comparison of the two precisions."""
        F = self.F
        state = np.asarray(state, F)
        L, shape = len(op.pressures), state.shape[1:]
        lnp, ex = consts if consts is not None else self.constants(op.pressures)
        lnp, ex = np.asarray(lnp, F), np.asarray(ex, F)
        agl = op.coord == Z_AGL
        masked = zs is not None and (op.coord != P or bool(op.mask))
        bad = np.zeros(shape, bool)
        zsv = np.zeros(shape, F)
        if masked or agl:
            zsv = np.asarray(zs, F)
            bad |= ~np.isfinite(zsv)
        nT = len(op.targets)
        tau = [zsv + F(t) if agl else np.full(shape, F(t), F) for t in op.targets]
        found = [np.zeros(shape, bool) for _ in range(nT)]
        frac = [np.zeros(shape, F) for _ in range(nT)]
        kl, ku = ([np.zeros(shape, np.int64) for _ in range(nT)] for _ in range(2))
        bestk = [np.full(shape, -1, np.int64) for _ in range(nT)]
        bestd = [np.zeros(shape, F) for _ in range(nT)]
        cu, klast, have = np.zeros(shape, F), np.zeros(shape, np.int64), np.zeros(shape, bool)
        with np.errstate(all="ignore"):
            for k in range(L - 1, -1, -1):
                if op.coord == P:
                    c = np.full(shape, lnp[k], F)
                else:
                    raw = state[op.c[k]]
                    bad |= ~np.isfinite(raw)
                    c = raw * ex[k] if op.coord == THETA else raw
                z = c
                if masked and op.coord not in (Z, Z_AGL):
                    z = state[op.z[k]]
                    bad |= ~np.isfinite(z)
                ok = ~(z < zsv) if masked else np.ones(shape, bool)
                for t in range(nT):
                    a, b = c - tau[t], cu - tau[t]
                    hit = ok & have & ~found[t] & self._crosses(a, b)
                    frac[t] = np.where(hit, a / (a - b), frac[t])
                    kl[t], ku[t] = np.where(hit, k, kl[t]), np.where(hit, klast, ku[t])
                    found[t] |= hit
                    d = np.abs(a)
                    near = ok & ((bestk[t] < 0) | (d <= bestd[t]))
                    bestd[t], bestk[t] = np.where(near, d, bestd[t]), np.where(near, k, bestk[t])
                cu, klast = np.where(ok, c, cu), np.where(ok, k, klast)
                have |= ok
            results = {}
            for f, fd in enumerate(op.fields):
                if not any(s >= 0 for s in fd.outputs):
                    continue
                node = fd.node[0] != NODE_NONE
                na = nb = np.zeros(shape, F)
                if node:
                    na = zsv if fd.node[0] == NODE_ZS else state[fd.node[0]]
                    if fd.kind == SPEED:
                        nb = zsv if fd.node[1] == NODE_ZS else state[fd.node[1]]
                    bad |= ~np.isfinite(na) | ~np.isfinite(nb)
                for t, slot in enumerate(fd.outputs):
                    if slot < 0:
                        continue
                    mode = np.where(found[t], LAYER, NONE)
                    kL, kU, fr = kl[t].copy(), ku[t].copy(), frac[t].copy()
                    p, q = (zsv + F(fd.gh)) - tau[t], cu - tau[t]
                    take = node & ~found[t] & have & self._crosses(p, q)
                    mode = np.where(take, NODE_LAYER, mode)
                    fr = np.where(take, p / (p - q), fr)
                    kU = np.where(take, klast, kU)
                    if op.outside == NEAREST:
                        near = (mode == NONE) & have
                        mode = np.where(near, np.where(node & (np.abs(p) <= bestd[t]), NODE, LEVEL), mode)
                        kL = np.where(near, bestk[t], kL)
                    kL, kU = np.clip(kL, 0, L - 1), np.clip(kU, 0, L - 1)
                    layer, from_node = (mode == LAYER) | (mode == NODE_LAYER), (mode == NODE_LAYER) | (mode == NODE)
                    if info is not None:
                        info[(f, t)] = (mode, kL, kU)
                    pick = lambda planes, k: np.take_along_axis(planes, k[None], 0)[0]      # noqa: E731
                    if fd.kind == PRESSURE:
                        col = np.broadcast_to(lnp.reshape((L,) + (1,) * len(shape)), (L,) + shape)
                        lL, lU = pick(col, kL), pick(col, kU)
                        res = np.where(mode == LAYER, self.math.exp(lL + (lU - lL) * fr), self.math.exp(lL))
                    else:
                        vals = []
                        for comp, chans in enumerate((fd.a, fd.b) if fd.kind == SPEED else (fd.a,)):
                            planes = state[list(chans)]
                            vl, vu = pick(planes, kL), pick(planes, kU)
                            bad |= (((mode == LAYER) | (mode == LEVEL)) & ~np.isfinite(vl)) | (layer & ~np.isfinite(vu))
                            if fd.kind == THETA_F:
                                col = np.broadcast_to(ex.reshape((L,) + (1,) * len(shape)), (L,) + shape)
                                vl, vu = vl * pick(col, kL), vu * pick(col, kU)
                            lower = np.where(from_node, nb if comp else na, vl)
                            vals.append(np.where(layer, lower + (vu - lower) * fr, lower))
                        if fd.kind == SPEED:
                            uu, vv = vals[0] * vals[0], vals[1] * vals[1]
                            res = np.sqrt(uu + vv)
                        else:
                            res = vals[0]
                    results[slot] = np.where(mode == NONE, F("nan"), res).astype(F)
        return {s: np.where(bad, F("nan"), v).astype(F) for s, v in results.items()}


fp32 = Vert(np.float32)
f64 = Vert(np.float64)

LEVELS = TR.LEVELS                                 # {2: ..., 13: Pangu's, 16: ...}: hPa, bottom-up
# the targets the planted columns are built around, in user units: metres, metres above the ground, K, degrees C, hPa
Z_M, AGL_M, THETA_K, T_C, P_HPA = (1500.0, 5000.0), (100.0, 5.0, 1500.0), (320.0, 300.0), (-10.0, 0.0), (700.0, 875.0, 1100.0, 30.0)
GZ = np.float32(G * Z_M[0])                        # the fp32 target of 1500 m
TM10 = np.float32(273.15 + T_C[0])                 # and of -10 C
PLANTED = ("target on an interior level", "target on the top level", "target above every level", "target below every level",
           "theta crosses three times", "two adjacent levels with the coordinate of the target", "one level masked", "several levels masked",
           "all levels masked", "target between the node and the lowest level", "the same with the lowest level masked", "-0.0 values",
           "NaN in a coordinate plane", "Inf in a field plane", "NaN in zs", "-Inf in t")


def layout(L) -> dict:
    """The channels of ``planted``'s states: t, u, v, q, z of level k at k, L + k ...; then u10m, v10m, t2m"""
    lay = {x: tuple(range(i * L, (i + 1) * L)) for i, x in enumerate("tuvqz")}
    lay.update(u10m=5 * L, v10m=5 * L + 1, t2m=5 * L + 2, C=5 * L + 3)
    return lay


def columns(seed, n, levels):
    """Random columns for the levels (hPa, bottom-up), float64: t, u, v, q, z (L, n) with z strictly increasing and theta increasing with
    height, continuous and well separated, and zs (n,) below the lowest level in most columns and above some levels in the others."""
    rng = np.random.default_rng(seed)
    p = np.asarray(levels, np.float64)
    L = p.size
    zh = -8000.0 * np.log(p / 1000.0)
    ts = rng.uniform(265.0, 305.0, n)
    lapse = rng.uniform(4.0, 7.5, n) / 1000.0
    t = np.maximum(ts[None] - lapse[None] * zh[:, None] + rng.normal(0, 0.5, (L, n)), 195.0)
    ex = (1000.0 / p) ** 0.2854
    for k in range(1, L):                                   # well separated: t falls and theta rises by half a kelvin a level at the least
        t[k] = np.clip(t[k], (t[k - 1] * ex[k - 1] + 0.5) / ex[k], t[k - 1] - 0.5)
    z = G * (zh[:, None] * rng.uniform(0.9, 1.1, n)[None] + rng.uniform(30.0, 300.0, n)[None])
    z += G * np.cumsum(rng.uniform(5.0, 40.0, (L, n)), axis=0)
    u, v = rng.normal(0, 12.0, (L, n)) + 0.002 * zh[:, None], rng.normal(0, 9.0, (L, n))
    q = np.abs(rng.normal(0, 4e-3, (L, n))) * (p[:, None] / 1000.0) ** 3
    zs = np.where(rng.random(n) < 0.35, rng.uniform(0.0, 40000.0, n), z[0] - G * rng.uniform(20.0, 400.0, n))
    return t, u, v, q, z, zs


def planted(seed, H, W, levels):
    """(state (5 L + 3, H, W) float32 in the ``layout``; zs (H, W)): random columns, the first sixteen replaced by the corner cases
    ``PLANTED`` in that order.  The corners are built around the targets ``Z_M[0]`` (and ``AGL_M``), ``THETA_K[0]`` and ``T_C[0]``."""
    L, n = len(levels), H * W
    assert n >= len(PLANTED)
    t, u, v, q, z, zs = columns(seed, n, levels)
    p = np.asarray(levels, np.float64)
    ex = (1000.0 / p) ** 0.2854
    down = np.arange(L - 1, -1, -1.0)                               # levels below the top
    mid = L // 2
    z[:, 0] = float(GZ) + 6000.0 * (np.arange(L) - mid)             # 0: c_mid = tau exactly (interior when L > 2): frac = 0, the level's value
    t[:, 0] = float(TM10) - 4.0 * (np.arange(L) - mid)
    z[:, 1], t[:, 1] = float(GZ) - 3000.0 * down, float(TM10) + 5.0 * down      # 1: the top level has the target: reproduced to rounding only
    z[:, 2], t[:, 2] = 1000.0 + 100.0 * np.arange(L), 300.0 - np.arange(L)      # 2: every z below 1500 m, every t above 0 C
    z[:, 3], t[:, 3] = 60000.0 + 5000.0 * np.arange(L), 200.0 - np.arange(L)    # 3: every z above 5000 m, every t below -10 C
    wave = np.where(np.arange(L) % 2 == 0, 310.0, 330.0) + np.arange(L)
    if L > 3:
        wave[4:] = 340.0 + np.arange(L - 4)                                     # 4: theta 310, 331, 312, 333, 340 ...: 320 K is crossed three times
    t[:, 4] = wave / ex
    if L > 3:                                                                    # 5: c_1 = c_2 = tau: that layer has a = b and is skipped
        z[:, 5] = float(GZ) + 5000.0 * (np.arange(L) - 1.5)
        z[1, 5] = z[2, 5] = float(GZ)
        t[:, 5] = float(TM10) - 5.0 * (np.arange(L) - 1.5)
        t[1, 5] = t[2, 5] = float(TM10)
    zs[6] = 0.5 * (z[0, 6] + z[1, 6])                                            # 6: one level masked
    zs[7] = 0.5 * (z[2, 7] + z[3, 7]) if L > 3 else 0.5 * (z[0, 7] + z[1, 7])    # 7: several
    zs[8] = 1e9                                                                  # 8: all
    zs[9] = z[0, 9] - G * 300.0                                                  # 9: 100 m above the ground lies between the 10-m node and level 0; 5 m lies below the node
    zs[10] = z[1, 10] - G * 300.0                                                # 10: the same above a masked level 0
    z[0, 10] = z[1, 10] - G * 700.0
    u[:, 11], q[:, 11] = -0.0, -0.0                                              # 11: -0.0
    state = np.concatenate([t, u, v, q, z, 0.7 * u[:1], 0.7 * v[:1], t[:1] + 1.0]).astype(np.float32)
    zs = zs.astype(np.float32)
    lay = layout(L)
    state[lay["z"][min(2, L - 1)], 12] = np.nan                                  # 12: NaN in a coordinate plane of the Z kinds
    state[lay["u"][mid], 13] = np.inf                                            # 13: Inf in a field plane: it counts where a result reads it
    zs[14] = np.nan                                                              # 14
    state[lay["t"][1], 15] = -np.inf                                             # 15
    state[lay["u10m"], 11] = -0.0
    return state.reshape(lay["C"], H, W), zs.reshape(H, W)
