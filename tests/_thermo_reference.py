"""Two numpy restatements of include/skyrim_thermo.h.

``fp32``: every operation on ``np.float32`` arrays in the header's order, with the header's ``sk_exp`` / ``sk_log`` (``np.rint``,
``np.ldexp``, ``np.frexp``) and the header's branches: the kernel is compared with it bit for bit.
``f64``: the same algorithm in float64 with ``np.exp`` / ``np.log`` and the moist-adiabat solve iterated to convergence: the yardstick the
fp32 arithmetic is measured against (tests/test_thermo_cpu.py).

Columns are the last axis: a plane is (N,) or (H, W), a column input (L, ...) bottom-up.
"""
from __future__ import annotations

import numpy as np

Q, R = 0, 1                                       # SKTHERMO_Q, SKTHERMO_R
SRC_LOWEST, SRC_MAX_THETAE = 0, 1                 # SKTHERMO_SRC_*
NSUB, NITER = 8, 3                                # SKTHERMO_NSUB, SKTHERMO_NITER
CONVERGED = 40                                    # secant updates of the float64 yardstick (it stops moving long before)


class Thermo:
    def __init__(self, F):
        self.F, self.single = F, F is np.float32
        f = F
        self.EPS, self.ONE_M_EPS, self.KAPPA, self.RD = f("0.622"), f("0.378"), f("0.2854"), f("287.04")
        self.T0, self.E_MIN, self.LN1000 = f("273.15"), f("1e-10"), self.log(f("1000"))
        self.niter = NITER if self.single else CONVERGED

    # ---- sk_exp, sk_log, sk_pow --------------------------------------------------------------------------------------------------------- #
    def exp(self, x):
        if not self.single:
            return np.exp(x)
        f = np.float32
        x = np.asarray(x, f)
        x = np.where(x < f("-87"), f("-87"), x)
        x = np.where(x > f("88"), f("88"), x)
        n = np.rint(x * f("1.44269504"))
        r = (x - n * f("0.693359375")) - n * f("-2.12194440e-4")
        p = f("1.98412698e-4")
        for c in ("1.38888889e-3", "8.33333333e-3", "4.16666667e-2", "1.66666667e-1", "0.5"):
            p = p * r + f(c)
        p = ((p * r) * r + r) + f(1)
        with np.errstate(invalid="ignore"):
            return np.ldexp(p, np.where(np.isfinite(n), n, 0).astype(np.int32)).astype(f)

    def log(self, x):
        if not self.single:
            return np.log(x)
        f = np.float32
        m, e = np.frexp(np.asarray(x, f))
        lo = m < f("0.70710678")
        m = np.where(lo, m + m, m)
        e = (e - lo).astype(f)
        s = (m - f(1)) / (m + f(1))
        z = s * s
        p = f("0.181818182")
        for c in ("0.222222222", "0.285714286", "0.4", "0.666666667", "2"):
            p = p * z + f(c)
        return (e * f("-2.12194440e-4") + s * p) + e * f("0.693359375")

    def pow(self, a, b):
        return self.exp(b * self.log(a))

    # ---- the formulas --------------------------------------------------------------------------------------------------------------------- #
    def es(self, T):
        f = self.F
        return f("6.112") * self.exp((f("17.67") * (T - self.T0)) / (T - f("29.65")))

    def vapour(self, kind, m, T, p):
        f = self.F
        e = (m * p) / (self.EPS + self.ONE_M_EPS * m) if kind == Q else (m / f(100)) * self.es(T)
        return np.where(e < self.E_MIN, self.E_MIN, e)

    def mixr(self, e, p):
        h = self.F("0.5") * p
        e = np.where(e > h, h, e)
        return (self.EPS * e) / (p - e)

    def tv(self, T, w):
        return (T * (self.F(1) + w / self.EPS)) / (self.F(1) + w)

    def dewpoint(self, e):
        f = self.F
        le = self.log(e / f("6.112"))
        return (f("243.5") * le) / (f("17.67") - le) + self.T0

    def tlcl(self, T, td):
        f = self.F
        return f(1) / (f(1) / (td - f(56)) + self.log(T / td) / f(800)) + f(56)

    def thetae(self, T, TL, lq, w):
        """Bolton (43) with lq = ln(1000 / p)"""
        f = self.F
        a = self.exp((self.KAPPA * (f(1) - f("0.28") * w)) * lq)
        b = self.exp(((f("3.376") / TL - f("0.00254")) * (w * f(1000))) * (f(1) + f("0.81") * w))
        return (T * a) * b

    def thetae_sat(self, T, pp, lq):
        return self.thetae(T, T, lq, self.mixr(self.es(T), pp))

    # ---- the ops -------------------------------------------------------------------------------------------------------------------------- #
    def _nan_where(self, bad, *outs):
        return tuple(np.where(bad, self.F("nan"), o).astype(self.F) for o in outs)

    def moist(self, t, m, p, kind, theta_only=False):
        """(td, other humidity, thetae, theta) of one level; p in hPa.  ``theta_only``: the moisture plane is not read, so a non-finite
        value in it does not reach theta"""
        f = self.F
        t, m, p = np.asarray(t, f), np.asarray(m, f), f(p)
        with np.errstate(all="ignore"):
            lq = self.LN1000 - self.log(p)
            e = self.vapour(kind, m, t, p)
            td = self.dewpoint(e)
            other = (f(100) * e) / self.es(t) if kind == Q else (self.EPS * e) / (p - self.ONE_M_EPS * e)
            the = self.thetae(t, self.tlcl(t, td), lq, self.mixr(e, p))
            th = t * self.exp(self.KAPPA * lq)
        bad = ~(np.isfinite(t) & np.isfinite(m))
        return self._nan_where(bad, td, other, the) + self._nan_where(~np.isfinite(t) if theta_only else bad, th)

    def index(self, t850, t700, t500, m850, m700, kind):
        """(kx, tt)"""
        f = self.F
        a = [np.asarray(x, f) for x in (t850, t700, t500, m850, m700)]
        t850, t700, t500, m850, m700 = a
        with np.errstate(all="ignore"):
            td850 = self.dewpoint(self.vapour(kind, m850, t850, f(850)))
            td700 = self.dewpoint(self.vapour(kind, m700, t700, f(700)))
            kx = ((t850 - t500) + (td850 - self.T0)) - (t700 - td700)
            tt = (t850 - t500) + (td850 - t500)
        bad = ~np.all([np.isfinite(x) for x in a], axis=0)
        return self._nan_where(bad, kx, tt)

    def freeze(self, t, z, zs=None):
        f = self.F
        t, z = np.asarray(t, f), np.asarray(z, f)
        L = t.shape[0]
        bad = ~(np.all(np.isfinite(t), 0) & np.all(np.isfinite(z), 0))
        shape = t.shape[1:]
        if zs is not None:
            zs = np.asarray(zs, f)
            bad |= ~np.isfinite(zs)
        res = np.zeros(shape, f)
        found, have = np.zeros(shape, bool), np.zeros(shape, bool)
        tu, zu = np.zeros(shape, f), np.zeros(shape, f)
        with np.errstate(all="ignore"):
            for k in range(L - 1, -1, -1):
                ok = np.ones(shape, bool) if zs is None else ~(z[k] < zs)
                a, b = t[k] - self.T0, tu - self.T0
                cross = (((a >= 0) & (b <= 0)) | ((a <= 0) & (b >= 0))) & (a != b)
                hit = ok & have & ~found & cross
                zc = z[k] + (zu - z[k]) * (a / (a - b))
                res = np.where(hit, zc, res)
                found |= hit
                res = np.where(ok & ~found, z[k], res)
                tu, zu = np.where(ok, t[k], tu), np.where(ok, z[k], zu)
                have |= ok
        return self._nan_where(bad | ~have, res)[0]

    def nodes(self, p):
        """The host constants of the ascent: lnp (L,), per layer k and node s = 1 .. NSUB: pp, lq, ex; h (L - 1,); exlev (L,)."""
        f = self.F
        p = np.asarray(p, f)
        L = p.size
        lnp = self.log(p)
        pp, lq, ex = (np.zeros((L - 1, NSUB), f) for _ in range(3))
        h = np.zeros(L - 1, f)
        exlev = self.exp(self.KAPPA * (lnp - self.LN1000))
        for k in range(L - 1):
            h[k] = (lnp[k] - lnp[k + 1]) / f(NSUB)
            for s in range(1, NSUB + 1):
                lp = lnp[k] + (f(s) / f(NSUB)) * (lnp[k + 1] - lnp[k])
                pp[k, s - 1] = self.exp(lp)
                lq[k, s - 1] = self.LN1000 - lp
                ex[k, s - 1] = self.exp(self.KAPPA * (lp - self.LN1000))
        return lnp, pp, lq, ex, h, exlev

    def parcel(self, t, m, p, kind, source=SRC_LOWEST, p_src_min=700.0, p_top=100.0, z=None, zs=None, force_src=None, trace=None):
        """(cape, li, p_src); li is NaN-filled when no level is 500 hPa.  ``force_src``: a level index that replaces the selection (the
        fp32-against-f64 comparison forces the same source in both); ``trace``: a dict that receives the parcel's node temperatures."""
        f = self.F
        t, m, p = np.asarray(t, f), np.asarray(m, f), np.asarray(p, f)
        L, shape = t.shape[0], t.shape[1:]
        lnp, npp, nlq, nex, h, exlev = self.nodes(p)
        ktop = max(k for k in range(L) if p[k] >= f(p_top))
        k500 = next((k for k in range(L) if p[k] == f(500)), -1)
        bad = ~(np.all(np.isfinite(t), 0) & np.all(np.isfinite(m), 0))
        masked = np.zeros((L,) + shape, bool)
        if zs is not None:
            z, zs = np.asarray(z, f), np.asarray(zs, f)
            bad |= ~(np.all(np.isfinite(z), 0) & np.isfinite(zs))
            masked = z < zs
        with np.errstate(all="ignore"):
            e = np.stack([self.vapour(kind, m[k], t[k], p[k]) for k in range(L)])
            w = np.stack([self.mixr(e[k], p[k]) for k in range(L)])
            tve = self.tv(t, w)
            # the source: the lowest unmasked level, or the largest thetae among the unmasked levels with p >= p_src_min (ties: the lower)
            src = np.full(shape, -1, np.int32)
            best = np.zeros(shape, f)
            for k in range(L):
                ok = ~masked[k]
                if source == SRC_MAX_THETAE and p[k] >= f(p_src_min):
                    lqk = self.LN1000 - lnp[k]
                    the = self.thetae(t[k], self.tlcl(t[k], self.dewpoint(e[k])), lqk, w[k])
                    take = ok & ((src < 0) | (the > best))
                    best = np.where(take, the, best)
                else:
                    take = ok & (src < 0)
                src = np.where(take, k, src)
            if force_src is not None:
                src = np.where(src >= 0, np.int32(force_src), src)
            none = src < 0
            s0 = np.where(none, 0, src)
            pick = lambda a: np.take_along_axis(a, s0[None], 0)[0]      # noqa: E731
            T0, e0, w0 = pick(t), pick(e), pick(w)
            lnp_s = lnp[s0]
            p_s = p[s0]
            lq_s = self.LN1000 - lnp_s
            TL = self.tlcl(T0, self.dewpoint(e0))
            the = self.thetae(T0, TL, lq_s, w0)
            th0 = T0 / exlev[s0]
            lq_lcl = lq_s - self.log(TL / T0) / self.KAPPA
            tot, prevB, Tprev = np.zeros(shape, f), np.zeros(shape, f), T0.copy()
            stopped = np.zeros(shape, bool)
            li = np.where(src == k500, f(0), f("nan")).astype(f) if k500 >= 0 else np.full(shape, f("nan"), f)
            for k in range(min(ktop, L - 1)):
                run = src <= k
                act = run & ~stopped & ~masked[k + 1]
                stopped |= run & masked[k + 1]
                exprev = exlev[k]
                for s in range(NSUB):
                    pp, lq, ex = npp[k, s], nlq[k, s], nex[k, s]
                    tenv = tve[k] + (f(s + 1) / f(NSUB)) * (tve[k + 1] - tve[k])
                    Tdry = th0 * ex
                    Ta, Tb = Tprev, (Tprev / exprev) * ex
                    Fa = self.thetae_sat(Ta, pp, lq) - the
                    for _ in range(self.niter):
                        Fb = self.thetae_sat(Tb, pp, lq) - the
                        d = Fb - Fa
                        step = np.where(d != 0, (Fb * (Tb - Ta)) / np.where(d != 0, d, f(1)), f(0))
                        Ta, Fa = Tb, Fb
                        Tb = Tb - step
                    sat = lq > lq_lcl
                    Tpar = np.where(sat, Tb, Tdry)
                    wp = np.where(sat, self.mixr(self.es(Tpar), pp), w0)
                    B = self.tv(Tpar, wp) - tenv
                    B = np.where(B > 0, B, f(0))
                    tot = np.where(act, tot + (f("0.5") * (B + prevB)) * h[k], tot)
                    prevB = np.where(act, B, prevB)
                    Tprev = np.where(act, Tpar, Tprev)
                    if trace is not None:
                        trace[(k, s)] = (Tpar.copy(), act.copy(), sat.copy())
                    exprev = ex
                if k + 1 == k500:
                    li = np.where(act, t[k + 1] - Tprev, li)
            cape = self.RD * tot
        return self._nan_where(bad | none, cape, li, p_s)


fp32 = Thermo(np.float32)
f64 = Thermo(np.float64)


PANGU_LEVELS = (1000, 925, 850, 700, 600, 500, 400, 300, 250, 200, 150, 100, 50)


def columns(seed, n, levels=PANGU_LEVELS):
    """Random columns for the levels (hPa, bottom-up): float32 t (strictly decreasing with height), q, r (percent), z (geopotential,
    m2/s2) of shape (L, n), and a surface geopotential zs (n,) that masks the lowest levels of some columns."""
    rng = np.random.default_rng(seed)
    p = np.asarray(levels, np.float64)
    L = p.size
    zh = -8000.0 * np.log(p / 1000.0)
    ts = rng.uniform(255.0, 308.0, n)
    lapse = rng.uniform(4.5, 9.0, n) / 1000.0
    t = ts[None] - lapse[None] * zh[:, None] + rng.normal(0, 0.7, (L, n))
    t = np.maximum(t, 190.0)
    for k in range(1, L):                                   # strictly decreasing with height: one 0 C crossing at the most
        t[k] = np.minimum(t[k], t[k - 1] - 0.05)
    rh = rng.uniform(0.02, 1.05, (L, n)) * np.where(rng.random(n) < 0.3, 1.0, rng.uniform(0.3, 1.0, n))[None]
    es = 6.112 * np.exp(17.67 * (t - 273.15) / (t - 29.65))
    e = np.minimum(rh * es, 0.3 * p[:, None])
    q = 0.622 * e / (p[:, None] - 0.378 * e)
    z = 9.80665 * (zh[:, None] * (t.mean(0) / 255.0)[None] + rng.normal(0, 20.0, (L, n)))
    zs = np.where(rng.random(n) < 0.4, rng.uniform(-500.0, 30000.0, n), -1000.0)
    f = np.float32
    return t.astype(f), q.astype(f), (100.0 * rh).astype(f), z.astype(f), zs.astype(f)


LEVELS = {2: (850, 500), 13: PANGU_LEVELS, 16: (1000, 975, 950, 925, 900, 850, 800, 700, 600, 500, 400, 300, 250, 200, 150, 100)}
PLANTED = ("dry", "r130", "saturated", "source second from top", "lcl above top", "all masked", "one unmasked", "t = 273.15 at a level",
           "no crossing")


def planted(seed, H, W, levels):
    """(state (4 L, H, W) float32 with the channels t, q, r, z of level k at k, L + k, 2 L + k, 3 L + k; zs (H, W)): random columns,
    the first nine replaced by the corner cases ``PLANTED`` in that order."""
    L, n = len(levels), H * W
    t, q, r, z, zs = (a.astype(np.float64) for a in columns(seed, n, levels))
    p = np.asarray(levels, np.float64)

    def q_of(rh, col):
        e = np.minimum(rh / 100.0 * 6.112 * np.exp(17.67 * (t[:, col] - 273.15) / (t[:, col] - 29.65)), 0.45 * p)
        return 0.622 * e / (p - 0.378 * e)
    q[:, 0], r[:, 0] = 0.0, 0.0
    r[:, 1] = 130.0
    q[:, 1] = q_of(130.0, 1)
    r[:, 2] = 100.0
    q[:, 2] = q_of(100.0, 2)
    zs[3] = 0.5 * (z[L - 3, 3] + z[L - 2, 3]) if L > 2 else z[0, 3] - 10.0
    q[:, 4], r[:, 4] = 1e-8, 1e-3
    zs[4] = -1e5
    zs[5] = 1e9
    zs[6] = 0.5 * (z[L - 2, 6] + z[L - 1, 6])
    k = min(3, L - 1)
    t[:, 7] = 273.15 + 6.0 * (k - np.arange(L))
    t[k, 7] = float(np.float32("273.15"))
    t[:, 8] = np.minimum(t[:, 8], 272.0 - np.arange(L))
    zs[7], zs[8] = -1e5, -1e5
    state = np.concatenate([t, q, r, z]).astype(np.float32).reshape(4 * L, H, W)
    return state, zs.astype(np.float32).reshape(H, W)
