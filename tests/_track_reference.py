"""Float64 restatement of cyclone detection and linking (include/skyrim_track.h, skyrim_amd/tracks.py) on the same fp32 inputs.

Nothing here reads the product's window tables: a window is the brute-force set {q : haversine(c, q) <= R} over the grid's own
latitudes and longitudes.  ``detect`` returns every centre with its criterion values, the header's error bound of each value and the
relative distance of each value to its threshold; ``radius_margin`` the closest any pair distance comes to a radius.
"""
from __future__ import annotations

import numpy as np

A_KM = 6371.0
U = 2.0 ** -24


def haversine_km(lat1, lon1, lat2, lon2):
    p1, p2, dl = np.radians(lat1), np.radians(lat2), np.radians(np.asarray(lon2, np.float64) - lon1)
    s = np.sin((p2 - p1) / 2) ** 2 + np.cos(p1) * np.cos(p2) * np.sin(dl / 2) ** 2
    return 2 * A_KM * np.arcsin(np.sqrt(np.clip(s, 0.0, 1.0)))


def band(lat, lat_max):
    rows = np.nonzero(np.abs(np.asarray(lat, np.float64)) <= lat_max)[0]
    return int(rows[0]), int(rows[-1]) + 1


def _near_rows(lat, j, radius, extra=0):
    """Rows whose meridian distance to row j is within the radius (a superset of the window's rows), ``extra`` more on either side."""
    lat = np.asarray(lat, np.float64)
    rows = np.nonzero(A_KM * np.abs(np.radians(lat - lat[j])) <= radius * (1 + 1e-6))[0]
    return np.arange(max(rows[0] - extra, 0), min(rows[-1] + extra, lat.size - 1) + 1)


def window(lat, lon, j, i, radius):
    """(rows, mask): mask[r, c] says whether point (rows[r], c) is within ``radius`` km of (j, i)."""
    lat, lon = np.asarray(lat, np.float64), np.asarray(lon, np.float64)
    rows = _near_rows(lat, j, radius)
    return rows, haversine_km(lat[j], lon[i], lat[rows][:, None], lon[None, :]) <= radius


def mask_half_widths(lat, lon, j, radius):
    """{row: half-width} of the window of (j, 0), counted from the brute-force mask; its points must be |di| <= half-width exactly."""
    rows, m = window(lat, lon, j, 0, radius)
    W = len(lon)
    out = {}
    for r, row in zip(rows, m):
        if row.any():
            k = int(row[:W // 2 + 1].sum()) - 1
            want = np.zeros(W, bool)
            want[:k + 1] = True
            if k > 0:
                want[-k:] = True
            assert np.array_equal(row, want), "a window row is not a symmetric run around the centre"
            out[int(r)] = k
    return out


def radius_margin(lat, lon, lat_max, radii):
    """The least |d - R| / R over every pair (band row centre, grid point) that could be in a window, for each radius."""
    lat, lon = np.asarray(lat, np.float64), np.asarray(lon, np.float64)
    j0, j1 = band(lat, lat_max)
    worst = np.inf
    for radius in sorted(set(radii)):
        for j in range(j0, j1):
            rows = _near_rows(lat, j, radius, extra=1)
            d = haversine_km(lat[j], lon[0], lat[rows][:, None], lon[None, :])
            worst = min(worst, float(np.abs(d - radius).min() / radius))
    return worst


def row_coefficients(lat, lon):
    """float32 (H, 4): A, B+, B-, sgn(lat), as the header defines them; made in float64."""
    phi = np.radians(np.asarray(lat, np.float64))
    dlam = np.radians(360.0 / len(lon))
    a = A_KM * 1e3
    out = np.zeros((phi.size, 4), np.float64)
    for j in range(1, phi.size - 1):
        c = np.cos(phi[j])
        dphi = phi[j + 1] - phi[j - 1]
        out[j] = (1.0 / (2 * a * c * dlam), np.cos(phi[j + 1]) / (a * c * dphi), np.cos(phi[j - 1]) / (a * c * dphi), np.sign(phi[j]))
    return out.astype(np.float32)


def _lex_min_3x3(p):
    """Points that are the strict lexicographic minimum of their 3 x 3 neighbourhood (rows 1 .. H - 2); NaN compares false."""
    H, W = p.shape
    idx = np.arange(H * W, dtype=np.int64).reshape(H, W)
    ok = np.zeros((H, W), bool)
    ok[1:-1] = True
    with np.errstate(invalid="ignore"):
        for dj in (-1, 0, 1):
            for di in (-1, 0, 1):
                if dj == 0 and di == 0:
                    continue
                q = np.roll(np.roll(p, -dj, axis=0), -di, axis=1)
                iq = np.roll(np.roll(idx, -dj, axis=0), -di, axis=1)
                ok &= (p < q) | ((p == q) & (idx < iq))
    ok[0] = ok[-1] = False
    return ok


def _margin(value, thr):
    if not np.isfinite(thr):
        return np.inf
    return abs(value - thr) / max(abs(thr), 1e-300) if thr != 0 else (np.inf if value != 0 else 0.0)


def detect(state, lat, lon, ch, radii, thr, lat_max):
    """Centres of one fp32 (C, H, W) state.  ``ch``: dict msl, u10, v10, u850, v850 and optionally z_up, z_lo (channel indices);
    ``radii`` = (msl, vort, wind, core) in km; ``thr`` = dict msl, vort, wind, core.  Returns (centres, undecided): centres sorted by
    (j, i), each a dict j, i, msl, vort, wind, core, and b_vort, b_wind, b_core (the header's bounds); ``undecided``: the least
    relative distance of any evaluated criterion value to its threshold (0 for a zero threshold only when the value is exactly 0)."""
    state = np.asarray(state)
    assert state.dtype == np.float32
    lat, lon = np.asarray(lat, np.float64), np.asarray(lon, np.float64)
    H, W = state.shape[1:]
    j0, j1 = band(lat, lat_max)
    rc = row_coefficients(lat, lon).astype(np.float64)
    p32 = state[ch["msl"]]
    p = p32.astype(np.float64)
    u8, v8 = state[ch["u850"]].astype(np.float64), state[ch["v850"]].astype(np.float64)
    t1 = rc[:, 0:1] * (np.roll(v8, -1, axis=1) - np.roll(v8, 1, axis=1))
    t2 = rc[:, 1:2] * np.roll(u8, -1, axis=0)
    t3 = rc[:, 2:3] * np.roll(u8, 1, axis=0)
    zeta = (t1 - (t2 - t3)) * rc[:, 3:4]
    s_vort = np.abs(rc[:, 0:1]) * (np.abs(np.roll(v8, -1, axis=1)) + np.abs(np.roll(v8, 1, axis=1))) + np.abs(t2) + np.abs(t3)
    speed = np.sqrt(state[ch["u10"]].astype(np.float64) ** 2 + state[ch["v10"]].astype(np.float64) ** 2)
    core_on = ch.get("z_up", -1) >= 0
    tau = state[ch["z_up"]].astype(np.float64) - state[ch["z_lo"]].astype(np.float64) if core_on else None
    survivors = _lex_min_3x3(p)
    centres, undecided = [], np.inf
    with np.errstate(invalid="ignore"):
        for j, i in zip(*np.nonzero(survivors[j0:j1])):
            j = int(j) + j0
            i = int(i)
            pc, idx_c = p[j, i], j * W + i
            if not pc <= thr.get("msl", np.inf):
                continue
            undecided = min(undecided, _margin(pc, thr.get("msl", np.inf)))
            rows, m = window(lat, lon, j, i, radii[0])
            assert 0 < j - rows[0] and m[j - rows[0] - 1:j - rows[0] + 2][:, [(i - 1) % W, i, (i + 1) % W]].all(), "3 x 3 outside the msl window"
            pq = p[rows][m]
            iq = (rows[:, None] * W + np.arange(W)[None, :])[m]
            other = iq != idx_c
            if not np.all(((pc < pq) | ((pc == pq) & (idx_c < iq)))[other]):
                continue
            rows, m = window(lat, lon, j, i, radii[1])
            assert rows[0] >= 1 and rows[-1] <= H - 2
            zq = zeta[rows][m]
            vort = np.max(zq[~np.isnan(zq)], initial=-np.inf)
            b_vort = 4 * U * np.max(s_vort[rows][m])
            undecided = min(undecided, _margin(vort, thr["vort"]))
            if not vort >= thr["vort"]:
                continue
            rows, m = window(lat, lon, j, i, radii[2])
            sq = speed[rows][m]
            wind = np.max(sq[~np.isnan(sq)], initial=-np.inf)
            undecided = min(undecided, _margin(wind, thr["wind"]))
            if not wind >= thr["wind"]:
                continue
            core = b_core = 0.0
            if core_on:
                rows, m = window(lat, lon, j, i, radii[3])
                tq = tau[rows][m]
                d = tq - tau[j, i]
                dn = d[~np.isnan(d)]
                core = (np.max(dn, initial=-np.inf) - d.sum() / d.size) if d.size else np.nan
                b_core = (12 * U + 2.0 ** -40) * np.max(np.abs(tq))
                undecided = min(undecided, _margin(core, thr["core"]))
                if not core >= thr["core"]:
                    continue
            centres.append(dict(j=j, i=i, msl=p32[j, i], vort=float(vort), wind=float(wind), core=float(core), b_vort=float(b_vort),
                                b_wind=float(4 * U * wind), b_core=float(b_core)))
    return centres, float(undecided)


# ---- linking and strike probability ----------------------------------------------------------------------------------------------------- #
def link(times, candidates, max_speed_kmh=90.0, min_points=2):
    """The linker restated with a distance matrix: ``candidates[t]`` is a list of (lat, lon) of one member in (j, i) order.  Returns
    the tracks as lists of (t, candidate index), in the order they started, those shorter than ``min_points`` dropped."""
    tracks, live = [], []
    for t, cands in enumerate(candidates):
        free = list(range(len(cands)))
        still = []
        if live and cands:
            hours = (np.datetime64(times[t], "s") - np.datetime64(times[t - 1], "s")) / np.timedelta64(3600, "s")
            dist = np.full((len(live), len(cands)), np.inf)
            for a, tid in enumerate(live):
                pts = [candidates[tt][kk] for tt, kk in tracks[tid]]
                lat, lon = pts[-1]
                if len(pts) > 1:
                    lat = float(np.clip(2 * pts[-1][0] - pts[-2][0], -90, 90))
                    lon = (pts[-1][1] + ((pts[-1][1] - pts[-2][1] + 180) % 360 - 180)) % 360
                for k, (clat, clon) in enumerate(cands):
                    dist[a, k] = haversine_km(lat, lon, clat, clon)
            dist[dist > max_speed_kmh * float(hours)] = np.inf
            while np.isfinite(dist).any():
                a, k = np.unravel_index(np.argmin(dist), dist.shape)          # the first minimum in (track, candidate) order
                tracks[live[a]].append((t, int(k)))
                still.append(live[a])
                free.remove(int(k))
                dist[a, :] = np.inf
                dist[:, k] = np.inf
        for k in free:
            tracks.append([(t, k)])
            still.append(len(tracks) - 1)
        live = sorted(still)
    return [tr for tr in tracks if len(tr) >= min_points]


def strike_probability(points_by_member, n_members, lat, lon, radius_km=120.0):
    """(H, W) fraction of members with a track point within the radius: every grid point against every track point."""
    lat, lon = np.asarray(lat, np.float64), np.asarray(lon, np.float64)
    hit = np.zeros((n_members, lat.size, lon.size), bool)
    for m, pts in points_by_member.items():
        for plat, plon in pts:
            hit[m] |= haversine_km(plat, plon, lat[:, None], lon[None, :]) <= radius_km
    return hit.sum(axis=0) / float(n_members)
