"""NumPy restatements of include/skyrim_noise.h, written from the header's text: the spectrum, the coefficients of one
(seed, member, field) from Philox and the float64 normals of ``_ens_reference``, the float64 synthesis with its error bound u (k S + Q),
the covariance function of the field, and the quantiles the statistical tests take their bars from."""
from __future__ import annotations

import math

import numpy as np

import _ens_reference as R

U = 2.0 ** -24
EPS_Z = 3.7e-6                     # |device normal - float64 normal| (tests/test_ens_kernels_gpu.py)
Z6 = 4.753424308822899             # the standard normal's upper 1e-6 quantile


def spectrum(lmax: int, length_scale_km: float = 500.0, alpha: float = 2.0) -> np.ndarray:
    l = np.arange(lmax, dtype=np.float64)
    s = ((6371.0 / length_scale_km) ** 2 + l * (l + 1)) ** (-alpha / 2)
    s[0] = 0.0
    return s / math.sqrt(np.sum((2 * l + 1) * s * s) / (4 * math.pi))


def normals4(seed: int, member: int, l, p, f) -> np.ndarray:
    """(..., 4) float64 normals of the Philox block (l, p, f, 1) under key (seed, member)."""
    l, p, f = np.broadcast_arrays(np.asarray(l), np.asarray(p), np.asarray(f))
    ctr = np.stack([l, p, f, np.ones_like(l)], axis=-1).astype(np.uint32)
    u = R.uniform(R.philox4x32_10(ctr, np.array([seed, member], np.uint32)))
    z = np.empty(u.shape)
    for a, b in ((0, 1), (2, 3)):
        rad = np.sqrt(-2.0 * np.log(u[..., a]))
        z[..., a] = rad * np.cos(2.0 * np.pi * u[..., b])
        z[..., b] = rad * np.sin(2.0 * np.pi * u[..., b])
    return z


def coefficients(seed: int, member: int, fields, lmax: int, table) -> tuple[np.ndarray, np.ndarray]:
    """(a, bound): a [lmax][lmax][2][F] float64 = table[l] (sqrt(1/2)) z, exactly 0 for l = 0 and m > l; bound: the header's
    t (3.7e-6 + 3 u |z|) (1 + 2^-20) per element (0 where a is an exact zero).  ``table``: [lmax] (sigma_l 2^e as the device holds it)."""
    fields = np.asarray(fields)
    table = np.asarray(table, np.float64)
    l = np.arange(lmax)[:, None, None]
    m = np.arange(lmax)[None, :, None]
    z4 = normals4(seed, member, l, m >> 1, fields[None, None, :])               # [l][m][F][4]
    odd = (np.arange(lmax) & 1).astype(bool)[None, :, None]
    z = np.stack([np.where(odd, z4[..., 2], z4[..., 0]), np.where(odd, z4[..., 3], z4[..., 1])], axis=2)     # [l][m][2][F]
    t = np.where(m == 0, 1.0, math.sqrt(0.5)) * table[:, None, None]            # [l][m][1]
    live = ((m <= l) & (l > 0))[:, :, None, :] & np.ones((1, 1, 2, 1), bool)
    live[:, 0, 1, :] = False                                                    # the zonal coefficient is real
    a = np.where(live, t[:, :, None, :] * z, 0.0)
    bound = np.where(live, t[:, :, None, :] * (EPS_Z + 3 * U * np.abs(z)) * (1 + 2.0 ** -20), 0.0)
    return a, bound


def legendre(lmax: int, n_lat_full: int, n_lat: int) -> np.ndarray:
    """[m][l][k] float64 Pbar_l^m(cos theta_k) on the first n_lat rows of the n_lat_full-row equiangular grid (sht.py's recurrence)."""
    from skyrim_amd.sfno.sht import colatitudes_and_weights, legendre_functions
    theta, _ = colatitudes_and_weights(n_lat_full, "equiangular")
    return legendre_functions(lmax, lmax, theta[:n_lat])


def synthesize(a: np.ndarray, P: np.ndarray, n_lon: int):
    """(y, S, Q) [F][lat][lon] float64 of coefficients a [l][m][2][F]: the field of the header, its sum of absolute addends, and the
    quantisation floor of the fp16 planes."""
    lmax = a.shape[0]
    F = a.shape[-1]
    n_lat = P.shape[-1]
    cm = np.where(np.arange(lmax) == 0, 1.0, 2.0)
    ang = 2.0 * np.pi * np.outer(np.arange(lmax), np.arange(n_lon)) / n_lon
    cos, sin = np.cos(ang) * cm[:, None], np.sin(ang) * cm[:, None]             # [m][j], c_m folded in
    are, aim = a[:, :, 0, :], a[:, :, 1, :]                                      # [l][m][F]
    leg = lambda p, x: np.einsum("mlk,lmf->mkf", p, x, optimize=True)            # noqa: E731
    tre, tim = leg(P, are), leg(P, aim)
    Pa = np.abs(P)
    sre, sim = leg(Pa, np.abs(are)), leg(Pa, np.abs(aim))

    def lon(tc, ts, c, s):                                                       # sum_m tc[m,k,f] c[m,j] + ts[m,k,f] s[m,j] -> [f][k][j]
        out = tc.reshape(lmax, -1).T @ c + ts.reshape(lmax, -1).T @ s
        return out.reshape(n_lat, F, n_lon).transpose(1, 0, 2)
    y = lon(tre, tim, cos, -sin)
    S = lon(sre, sim, np.abs(cos), np.abs(sin))
    q_a = np.einsum("m,lmf->f", cm, np.abs(are) + np.abs(aim))                   # [F]
    q_p = 2.0 * np.einsum("m,mlk->k", cm, Pa)                                    # [lat]
    q_t = (sre + sim).sum(axis=0).T                                              # [F][lat]
    Q = 0.5 * (q_a[:, None] + q_p[None, :] + q_t + 4.0 * lmax)
    return y, S, np.broadcast_to(Q[:, :, None], y.shape)


def k_bound(lmax: int) -> float:
    return 18.0 * lmax + 32.0


def covariance(sigma: np.ndarray, cos_gamma) -> np.ndarray:
    """C(gamma) = sum_l sigma_l^2 (2 l + 1) / (4 pi) P_l(cos gamma)."""
    l = np.arange(sigma.size)
    return np.polynomial.legendre.legval(np.asarray(cos_gamma, np.float64), sigma ** 2 * (2 * l + 1) / (4 * math.pi))


def area_weights(n_lat_full: int, n_lat: int) -> np.ndarray:
    """Row weights (Clenshaw-Curtis, the transform's own) of the first n_lat rows, normalised to sum 1."""
    from skyrim_amd.sfno.sht import colatitudes_and_weights
    wq = colatitudes_and_weights(n_lat_full, "equiangular")[1][:n_lat]
    return wq / wq.sum()


def square_mean_variance(sigma: np.ndarray, n_lat_full: int, n_lat: int, n_lon: int) -> float:
    """sum_pq w_p w_q C(gamma_pq)^2 over all pairs of grid points (w_p = row weight / n_lon): half the variance of the area mean of y^2
    for a unit Gaussian field y (Isserlis), so its inverse is the field's effective count of independent points.  Longitudes are uniform,
    so the pair sum runs over (row, row, longitude difference)."""
    theta = np.pi * np.arange(n_lat) / (n_lat_full - 1)
    w = area_weights(n_lat_full, n_lat)
    dphi = 2 * np.pi * np.arange(n_lon) / n_lon
    cg = (np.cos(theta)[:, None, None] * np.cos(theta)[None, :, None]
          + np.sin(theta)[:, None, None] * np.sin(theta)[None, :, None] * np.cos(dphi)[None, None, :])
    C = covariance(sigma, np.clip(cg, -1.0, 1.0))
    return float(np.einsum("a,b,abj->", w, w, C * C) / n_lon)


def chi2_quantiles(nu: float, z: float = Z6) -> tuple[float, float]:
    """(lower, upper) quantiles of chi^2_nu / nu at the two-sided normal quantile z (Wilson-Hilferty; nu in the hundreds and above)."""
    h = 2.0 / (9.0 * nu)
    return (1 - h - z * math.sqrt(h)) ** 3, (1 - h + z * math.sqrt(h)) ** 3


def fisher_bar(n: int, z: float = Z6) -> float:
    """Half-width of atanh(r) for n independent pairs."""
    return z / math.sqrt(n - 3)


def fma32(g, y, x) -> np.ndarray:
    """fmaf in float32: the product of two fp32 numbers is exact in float64; the sum is rounded to float64 and then to float32.  Exact
    (no double rounding) whenever the float64 sum is itself exact or not a float32 tie -- ``fma32_is_exact`` checks the test's values."""
    return (np.asarray(g, np.float32).astype(np.float64) * np.asarray(y, np.float32).astype(np.float64)
            + np.asarray(x, np.float32).astype(np.float64)).astype(np.float32)


def fma32_is_exact(g, y, x) -> bool:
    """True when the float64 emulation of every element is the correctly rounded fma: the exact sum, carried as a (hi, lo) two-sum pair,
    is either exact in float64 (lo == 0) or hi is not half-way between two float32 numbers (then no second rounding can move it)."""
    p = np.asarray(g, np.float32).astype(np.float64) * np.asarray(y, np.float32).astype(np.float64)
    x = np.asarray(x, np.float32).astype(np.float64)
    hi = p + x
    bb = hi - p
    lo = (p - (hi - bb)) + (x - bb)
    near = hi.astype(np.float32).astype(np.float64)
    up = np.nextafter(hi.astype(np.float32), np.float32(np.inf)).astype(np.float64)
    dn = np.nextafter(hi.astype(np.float32), np.float32(-np.inf)).astype(np.float64)
    tie = (hi == 0.5 * (near + up)) | (hi == 0.5 * (near + dn))
    return bool(np.all((lo == 0) | ~tie))


# ---- shared cases ---------------------------------------------------------------------------------------------------------------------- #
APPLY_SHAPES = ((1, 3, 1000), (2, 5, 7), (1, 1, 3), (1, 3, 1))


def apply_inputs(L: int, C: int, hw: int):
    """(x0, y, g) float32 of the apply test: a temperature-like state, a field in the synthesis' scaled units, amplitudes with one
    channel switched off when there is more than one."""
    rng = np.random.default_rng(1000 * L + 10 * C + hw)
    x0 = (250.0 + 30.0 * rng.normal(size=L * C * hw)).astype(np.float32)
    y = (40.0 * rng.normal(size=L * C * hw)).astype(np.float32)
    g = (1e-3 * rng.uniform(0.5, 20.0, size=C) * 2.0 ** -4).astype(np.float32)
    if C > 1:
        g[1] = 0.0
    return x0, y, g


# 64 members x 8 fields at 33 x 64, lmax 32: 512 independent samples per grid point.  Seed 2024 was the first one tried.
STAT = dict(seed=2024, members=64, F=8, n_lat=33, n_lon=64, lmax=32)
ROW_PAIRS = ((16, 17), (16, 19), (10, 20), (0, 3), (5, 28), (31, 32))


def statistics_fields_float64() -> np.ndarray:
    """[members * F][n_lat][n_lon]: the float64 restatement of the fields of ``STAT`` (members 1 .. 64; member 0 is the control)."""
    s = STAT
    sigma = spectrum(s["lmax"])
    P = legendre(s["lmax"], s["n_lat"], s["n_lat"])
    out = []
    for mem in range(1, s["members"] + 1):
        a, _ = coefficients(s["seed"], mem, np.arange(s["F"]), s["lmax"], sigma)
        out.append(synthesize(a, P, s["n_lon"])[0])
    return np.concatenate(out)


def statistics_check(y: np.ndarray) -> dict:
    """Holds N = 512 unit-variance samples per point (y: [N][n_lat][n_lon], in units of the field's sigma) to bars at 1e-6 per comparison:
    * the area-weighted mean of the sample second moment: T = sum_p w_p mean_n y_np^2 has E T = 1 and, the field being Gaussian,
      Var T = (2 / N) sum_pq w_p w_q C(gamma_pq)^2 (Isserlis), so T is held to chi^2_nu / nu with nu = N / sum_pq w_p w_q C_pq^2 -- the
      effective sample count of the field times N, counted from the exact covariance on this grid;
    * every point's second moment to chi^2_N / N;
    * per longitude, the sample correlation of two rows to C(theta_2 - theta_1) within the Fisher-z bar z / sqrt(N - 3).
    Returns the worst use of each bar (1 = at the bar)."""
    s = STAT
    N = y.shape[0]
    assert y.shape == (s["members"] * s["F"], s["n_lat"], s["n_lon"])
    sigma = spectrum(s["lmax"])
    theta = np.pi * np.arange(s["n_lat"]) / (s["n_lat"] - 1)
    w = np.repeat(area_weights(s["n_lat"], s["n_lat"]) / s["n_lon"], s["n_lon"])
    assert abs(float(covariance(sigma, 1.0)) - 1) < 1e-12
    nu = N / square_mean_variance(sigma, s["n_lat"], s["n_lat"], s["n_lon"])
    v = (y.astype(np.float64) ** 2).mean(axis=0)
    T = float((w * v.reshape(-1)).sum())
    lo, hi = chi2_quantiles(nu)
    worst = {"area mean": max((T - 1) / (hi - 1), (1 - T) / (1 - lo))}
    assert lo <= T <= hi, (T, lo, hi, nu)
    lo, hi = chi2_quantiles(N)
    worst["worst point"] = max((v.max() - 1) / (hi - 1), (1 - v.min()) / (1 - lo))
    assert lo <= v.min() and v.max() <= hi, (v.min(), v.max(), lo, hi)
    bar, use = fisher_bar(N), 0.0
    for k1, k2 in ROW_PAIRS:
        rho = float(covariance(sigma, np.cos(theta[k2] - theta[k1])))
        a, b = y[:, k1, :].astype(np.float64), y[:, k2, :].astype(np.float64)
        a, b = a - a.mean(axis=0), b - b.mean(axis=0)
        r = (a * b).sum(axis=0) / np.sqrt((a * a).sum(axis=0) * (b * b).sum(axis=0))
        dz = np.abs(np.arctanh(r) - np.arctanh(rho))
        use = max(use, float(dz.max()) / bar)
        assert dz.max() <= bar, (k1, k2, rho, float(dz.max()), bar)
    worst["row correlation"] = use
    return worst
