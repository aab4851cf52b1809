"""NumPy restatements of include/skyrim_stoch.h, written from the header's text: the coefficients of draw number ``draw`` (the
restatement of ``_noise_reference`` with counter word 3 = 1 + draw), the autoregressive step and the SPPT / additive step with the fused
multiply-add emulated in float64, and the shared cases of the tests."""
from __future__ import annotations

import math
from fractions import Fraction

import numpy as np

import _ens_reference as R
import _noise_reference as NR

fma32_is_exact = NR.fma32_is_exact


def normals4(seed: int, member: int, l, p, f, draw: int) -> np.ndarray:
    """(..., 4) float64 normals of the Philox block (l, p, f, 1 + draw) under key (seed, member)."""
    l, p, f = np.broadcast_arrays(np.asarray(l), np.asarray(p), np.asarray(f))
    ctr = np.stack([l, p, f, np.full_like(l, 1 + draw)], axis=-1).astype(np.uint32)
    u = R.uniform(R.philox4x32_10(ctr, np.array([seed, member], np.uint32)))
    z = np.empty(u.shape)
    for a, b in ((0, 1), (2, 3)):
        rad = np.sqrt(-2.0 * np.log(u[..., a]))
        z[..., a] = rad * np.cos(2.0 * np.pi * u[..., b])
        z[..., b] = rad * np.sin(2.0 * np.pi * u[..., b])
    return z


def coefficients(seed: int, member: int, fields, lmax: int, table, draw: int) -> tuple[np.ndarray, np.ndarray]:
    """``_noise_reference.coefficients`` for draw number ``draw``: (a, bound), a [lmax][lmax][2][F] float64, bound the stated
    t (3.7e-6 + 3 u |z|) (1 + 2^-20) of skyrim_noise.h per element, 0 where a is a structural zero."""
    fields = np.asarray(fields, np.int64)
    table = np.asarray(table, np.float64)
    l = np.arange(lmax, dtype=np.int64)[:, None, None]
    m = np.arange(lmax, dtype=np.int64)[None, :, None]
    z4 = normals4(seed, member, l, m >> 1, fields[None, None, :], draw)          # [l][m][F][4]
    odd = (np.arange(lmax) & 1).astype(bool)[None, :, None]
    z = np.stack([np.where(odd, z4[..., 2], z4[..., 0]), np.where(odd, z4[..., 3], z4[..., 1])], axis=2)     # [l][m][2][F]
    t = np.where(m == 0, 1.0, math.sqrt(0.5)) * table[:, None, None]            # [l][m][1]
    live = ((m <= l) & (l > 0))[:, :, None, :] & np.ones((1, 1, 2, 1), bool)
    live[:, 0, 1, :] = False                                                    # the zonal coefficient is real
    a = np.where(live, t[:, :, None, :] * z, 0.0)
    bound = np.where(live, t[:, :, None, :] * (NR.EPS_Z + 3 * NR.U * np.abs(z)) * (1 + 2.0 ** -20), 0.0)
    return a, bound


def live_mask(lmax: int) -> np.ndarray:
    """bool [lmax][lmax][2]: the coefficients that are not structural zeros."""
    l, m = np.arange(lmax)[:, None], np.arange(lmax)[None, :]
    live = np.repeat(((m <= l) & (l > 0))[:, :, None], 2, axis=2)
    live[:, 0, 1] = False
    return live


def fma32(a, b, c) -> np.ndarray:
    """fmaf on float32 arrays, correctly rounded for every finite input: ``_noise_reference.fma32`` (the exact product plus c, rounded to
    float64 and then to float32), with the elements where that double rounding could differ -- an inexact float64 sum that is a float32
    tie -- recomputed in exact rational arithmetic."""
    a, b, c = np.broadcast_arrays(np.asarray(a, np.float32), np.asarray(b, np.float32), np.asarray(c, np.float32))
    if a.ndim == 0:
        return fma32(a[None], b[None], c[None])[0]
    with np.errstate(all="ignore"):
        out = NR.fma32(a, b, c).copy()
        p = a.astype(np.float64) * b.astype(np.float64)
        x = c.astype(np.float64)
        hi = p + x
        bb = hi - p
        lo = (p - (hi - bb)) + (x - bb)
        near = hi.astype(np.float32)
        up = np.nextafter(near, np.float32(np.inf)).astype(np.float64)
        dn = np.nextafter(near, np.float32(-np.inf)).astype(np.float64)
        n64 = near.astype(np.float64)
        doubt = np.isfinite(hi) & (lo != 0) & ((hi == 0.5 * (n64 + up)) | (hi == 0.5 * (n64 + dn)))
    for i in zip(*np.nonzero(doubt)):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        cands = [float(dn[i]), float(n64[i]), float(up[i])]
        out[i] = np.float32(min(cands, key=lambda v: abs(Fraction(v) - exact)))      # (an exact tie cannot occur here: lo != 0)
    return out


def evolve(p, fresh, phi, psi) -> np.ndarray:
    """p' = fmaf(phi, p, fl32(psi * fresh)) on float32 arrays."""
    fresh = np.asarray(fresh, np.float32)
    return fma32(np.float32(phi), np.asarray(p, np.float32), np.float32(psi) * fresh)


def apply(xp, xn, r, y, gs, ga, lim, C: int, hw: int) -> np.ndarray:
    """skstoch_apply on flat float32 arrays; ``r`` with ``gs``, or ``y`` with ``ga``, may be None."""
    xn = np.asarray(xn, np.float32)
    i = np.arange(xn.size)
    c, q = (i // hw) % C, i % hw
    lim = np.float32(lim)
    t = xn.copy()
    with np.errstate(all="ignore"):
        if r is not None:
            g = np.asarray(gs, np.float32)[c]
            d = xn - np.asarray(xp, np.float32)
            w = np.fmin(np.fmax(g * np.asarray(r, np.float32)[q], -lim), lim)
            t = np.where(g == 0, xn, fma32(w, d, xn))
        if y is not None:
            g = np.asarray(ga, np.float32)[c]
            t = np.where(g == 0, t, fma32(g, np.asarray(y, np.float32), t))
    return t.astype(np.float32)


# ---- shared cases ---------------------------------------------------------------------------------------------------------------------- #
COEFF_SHAPES = ((1, 1), (1, 2), (3, 5), (7, 9), (5, 33))                       # (F, lmax)
DRAWS = (1, 2, 2 ** 32 - 2)
# (L, C, hw): hw a multiple of 4 (the pattern's 16-byte loads); hw odd with planes that end inside a group of four, n % 4 != 0, several
# workgroups; a tiny odd case; hw = 1
APPLY_SHAPES = ((1, 3, 1000), (2, 3, 515), (2, 5, 7), (1, 1, 3), (1, 3, 1))
LIM = 0.9


def apply_inputs(L: int, C: int, hw: int):
    """(xp, xn, r, y, gs, ga) float32: a temperature-like state and its step, a pattern and fields in the synthesis' scaled units
    (2^4 times unit variance), amplitudes such that fl32(gs r) has standard deviation 0.6 -- so that the clip at 0.9 is active on both
    sides for about 6.7 % of the points each (P(z > 1.5)) -- and, when there are three channels or more, channel 1 switched off in both
    terms and channel 2 in the SPPT term alone."""
    rng = np.random.default_rng(100 * C + hw + 7 * L)
    n = L * C * hw
    xp = (250.0 + 30.0 * rng.normal(size=n)).astype(np.float32)
    xn = (xp + 2.0 * rng.normal(size=n)).astype(np.float32)
    r = (16.0 * rng.normal(size=hw)).astype(np.float32)
    y = (16.0 * rng.normal(size=n)).astype(np.float32)
    gs = np.full(C, 0.6 / 16.0, np.float32)
    ga = (1e-3 * rng.uniform(0.5, 20.0, size=C) / 16.0).astype(np.float32)
    if C >= 3:
        gs[1] = ga[1] = 0.0
        gs[2] = 0.0
    return xp, xn, r, y, gs, ga
