"""``torch.ops.skyrim_hip.track_detect`` against the float64 restatement (tests/_track_reference.py) on planted vortices, white noise
and one full-size field: the sets of centres are identical, msl is bit-equal, vort / wind / core lie within the header's bounds."""
from __future__ import annotations

import datetime

import numpy as np
import pytest
import torch

import _track_reference as R
from skyrim_amd import ensemble as E
from skyrim_amd import tracks as T

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CH = dict(msl=0, u10=1, v10=2, u850=3, v850=4, z_up=5, z_lo=6)
TOY33 = dict(lat_max=60.0, r_msl_km=2500.0, r_vort_km=1500.0, r_wind_km=1900.0, r_core_km=2100.0, thr_vort=3e-5, thr_wind=8.0, thr_core=50.0)
TOY49 = dict(lat_max=60.0, r_msl_km=1700.0, r_vort_km=1000.0, r_wind_km=1300.0, r_core_km=1100.0, thr_vort=3e-5, thr_wind=8.0, thr_core=50.0)
# (lat, lon, depth in Pa, +1 cyclonic / -1 anticyclonic winds): the seam, the last band row (-56.25) and just outside the band
# (61.875), both hemispheres, a low with anticyclonic winds, two lows closer than r_msl (the deeper survives)
VORTICES = [(28.0, 358.0, 3000.0, 1), (-56.25, 200.0, 2500.0, 1), (61.875, 60.0, 2800.0, 1), (-22.0, 70.0, 2000.0, 1),
            (39.0, 250.0, 2600.0, -1), (17.0, 130.0, 3200.0, 1), (17.0, 141.0, 1500.0, 1)]


def grid(n_lat, n_lon, rows=None, ascending=False):
    lat = np.linspace(90.0, -90.0, n_lat)[:rows]
    return (lat[::-1].copy() if ascending else lat), np.arange(n_lon) * (360.0 / n_lon)


def planted(lat, lon, vortices, sigma_km, shift=0.0, ripple=0.0, strength=0.5e-4):
    """A (7, H, W) float32 state: a smooth background plus Gaussian lows with winds from a stream function (so that pressure, vorticity
    and wind belong together) and a warm thickness anomaly over every low."""
    la, lo = np.radians(lat)[:, None], np.radians(lon)[None, :]
    a = R.A_KM * 1e3
    msl = 101000.0 + 300.0 * np.sin(la) + 80.0 * np.cos(2 * lo) * np.cos(la) + ripple * np.sin(9 * lo) * np.cos(7 * la)
    psi = 2.0e6 * np.sin(la) * np.cos(lo)
    tau = 1.0e5 + 4000.0 * np.cos(la) ** 2 + 0 * lo
    for vlat, vlon, depth, cyc in vortices:
        g = np.exp(-0.5 * (R.haversine_km(vlat, vlon + shift, lat[:, None], lon[None, :]) / sigma_km) ** 2)
        msl = msl - depth * g
        psi = psi - np.sign(vlat) * cyc * (depth / 3000.0) * strength * (sigma_km * 1e3) ** 2 * g
        tau = tau + 0.3 * depth * g
    dlat = np.gradient(np.radians(lat))[:, None]
    dlon = np.radians(lon[1] - lon[0])
    u = -np.gradient(psi, axis=0) / (a * dlat)
    v = (np.roll(psi, -1, axis=1) - np.roll(psi, 1, axis=1)) / (2 * a * np.cos(la).clip(1e-3) * dlon)
    z_lo = 14000.0 + 500.0 * np.cos(la) + 0 * lo
    return np.stack([msl, 0.8 * u, 0.8 * v, u, v, z_lo + tau, z_lo]).astype(np.float32)


def run_op(states, lat, lon, cfg, warm_core=True, capacity=None, misalign=False):
    """(count, records written (sorted), the whole record buffer as bytes) of one track_detect on the device."""
    geo = T.geometry(lat, lon, cfg, warm_core)
    M, (C, H, W) = len(states), states[0].shape
    members = []
    for s in states:
        if misalign:
            flat = torch.empty(s.size + 1, dtype=torch.float32, device=DEV)
            t = flat[1:].view(C, H, W)
            assert t.data_ptr() % 16 == 4
        else:
            t = torch.empty((C, H, W), dtype=torch.float32, device=DEV)
        t.copy_(torch.from_numpy(s))
        members.append(t)
    table = E.member_table(members)
    capacity = 64 * M if capacity is None else capacity
    records = torch.full((capacity * 32,), 0xAB, dtype=torch.uint8, device=DEV)
    count = torch.full((1,), -7, dtype=torch.int32, device=DEV)
    ws = torch.empty(T.workspace_bytes(M, geo.j1 - geo.j0, W), dtype=torch.uint8, device=DEV)
    h = {k: torch.from_numpy(v).to(DEV) for k, v in geo.h.items()}
    channels = [CH[k] for k in ("msl", "u10", "v10", "u850", "v850")] + ([CH["z_up"], CH["z_lo"]] if warm_core else [-1, -1])
    torch.ops.skyrim_hip.track_detect(members, table, channels, [geo.j0, geo.j1], [cfg.thr_msl, cfg.thr_vort, cfg.thr_wind, cfg.thr_core],
                                      h["msl"], h["vort"], h["wind"], h.get("core"), torch.from_numpy(geo.rowc).to(DEV), records, count, ws)
    n = int(count.item())
    raw = records.cpu().numpy()
    written = min(n, capacity)
    assert np.all(raw[written * 32:] == 0xAB), "bytes beyond the written records were touched"
    rec = np.sort(raw[:written * 32].view(T.RECORD), order=("member", "j", "i"))
    assert np.all(rec["pad"] == 0)
    return n, rec


def reference(states, lat, lon, cfg, warm_core=True):
    ch = CH if warm_core else {k: v for k, v in CH.items() if not k.startswith("z_")}
    thr = dict(msl=cfg.thr_msl, vort=cfg.thr_vort, wind=cfg.thr_wind, core=cfg.thr_core)
    out, undecided = [], np.inf
    for m, s in enumerate(states):
        centres, und = R.detect(s, lat, lon, ch, cfg.radii(), thr, cfg.lat_max)
        undecided = min(undecided, und)
        out += [dict(member=m, **c) for c in centres]
    return out, undecided


def compare(what, states, lat, lon, cfg, warm_core=True, **kw):
    assert R.radius_margin(lat, lon, cfg.lat_max, cfg.radii()[:4 if warm_core else 3]) > 1e-9
    ref, undecided = reference(states, lat, lon, cfg, warm_core)
    assert undecided > 1e-4, f"{what}: a criterion value lies within {undecided:.2e} of its threshold"
    n, rec = run_op(states, lat, lon, cfg, warm_core, **kw)
    assert n == len(ref) == len(rec), (what, n, len(ref))
    assert [(r["member"], r["j"], r["i"]) for r in rec] == [(c["member"], c["j"], c["i"]) for c in ref], what
    share = dict(vort=0.0, wind=0.0, core=0.0)
    for r, c in zip(rec, ref):
        assert r["msl"].tobytes() == np.float32(c["msl"]).tobytes()
        for k in share:
            err = abs(float(r[k]) - c[k])
            if k == "core" and not warm_core:
                assert r[k] == 0.0
                continue
            share[k] = max(share[k], err / c["b_" + k] if c["b_" + k] > 0 else (0.0 if err == 0 else np.inf))
    print(f"{what}: {n} centres, worst share of the bound vort {share['vort']:.3f} wind {share['wind']:.3f} core {share['core']:.3f}")
    assert max(share.values()) <= 1, (what, share)
    return ref, rec


GRIDS = {"33x64": (grid(33, 64), TOY33, 800.0), "49x192": (grid(49, 192), TOY49, 600.0),
         "32of33x64": (grid(33, 64, rows=32), TOY33, 800.0), "ascending": (grid(33, 64, ascending=True), TOY33, 800.0)}


@pytest.mark.parametrize("case", list(GRIDS))
@pytest.mark.parametrize("M", [1, 2, 9, 50])
def test_planted_vortices(case, M):
    (lat, lon), kw, sigma = GRIDS[case]
    cfg = T.TrackerConfig(**kw)
    states = [planted(lat, lon, VORTICES, sigma, shift=3.0 * m) for m in range(M)]
    ref, _ = compare(f"{case} M={M}", states, lat, lon, cfg, misalign=(M == 2))
    first = [(c["j"], c["i"]) for c in ref if c["member"] == 0]
    jl = lambda v: int(np.argmin(np.abs(lat - v)))                         # noqa: E731
    rows = {j for j, _ in first}
    assert jl(-56.25) in rows and jl(61.875) not in rows and jl(39.0) not in rows          # last band row in, outside and anticyclonic out
    assert any(i in (0, len(lon) - 1) for _, i in first)                                  # the low on the seam
    assert sum(j == jl(17.0) for j, _ in first) == 1                                      # of the two close lows, one


def test_ties_constant_field_and_no_warm_core():
    (lat, lon), kw, sigma = GRIDS["33x64"]
    cfg = T.TrackerConfig(**kw)
    s = planted(lat, lon, VORTICES[:1] + VORTICES[3:4], sigma)
    j = int(np.argmin(np.abs(lat - 28.0)))
    low = np.float32(s[0].min() - 100.0)
    s[0, j, 62] = s[0, j, 0] = low                              # bit-equal minima two columns apart, across the seam: index j W + 0 wins
    s[0, j + 1, 63] = low                                       # and a third one on the next row, a neighbour of both
    ref, rec = compare("bit-equal minima", [s], lat, lon, cfg)
    assert (j, 0) in [(c["j"], c["i"]) for c in ref] and not any(c["j"] in (j, j + 1) and c["i"] in (62, 63) for c in ref)
    flat = s.copy()
    flat[0] = np.float32(101325.0)
    ref, _ = compare("constant msl", [flat, s], lat, lon, cfg)
    assert all(c["member"] == 1 for c in ref) and len(ref) >= 1
    nan = s.copy()
    nan[0, j - 1, 1] = np.nan                                   # a NaN inside the window of (j, 0): no centre there
    ref, _ = compare("a NaN in a window", [nan], lat, lon, cfg)
    assert (j, 0) not in [(c["j"], c["i"]) for c in ref]
    ref_core, _ = compare("with the warm core", [s], lat, lon, cfg)
    ref_none, _ = compare("without the warm core", [s], lat, lon, cfg, warm_core=False)
    assert len(ref_none) >= len(ref_core) >= 1


def test_white_noise_survivors_in_the_thousands():
    (lat, lon), kw, _ = GRIDS["49x192"]
    cfg = T.TrackerConfig(**dict(kw, thr_vort=2e-5, thr_wind=12.0, thr_core=300.0))
    rng = np.random.default_rng(5)
    states = []
    for m in range(3):
        s = planted(lat, lon, [], 600.0)
        s[0] += rng.normal(0, 300.0, s[0].shape).astype(np.float32)
        s[1:5] += rng.normal(0, 6.0, s[1:5].shape).astype(np.float32)
        s[5] += rng.normal(0, 150.0, s[5].shape).astype(np.float32)
        states.append(s)
    j0, j1 = R.band(lat, cfg.lat_max)
    survivors = sum(int(R._lex_min_3x3(s[0].astype(np.float64))[j0:j1].sum()) for s in states)
    assert survivors >= 1500, survivors
    ref, _ = compare(f"white noise, {survivors} prefilter survivors", states, lat, lon, cfg, capacity=4096)
    assert len(ref) >= 10


def test_full_size_default_radii():
    lat, lon = grid(721, 1440)
    cfg = T.TrackerConfig()
    lows = [(25.0, 359.9, 3000.0, 1), (-60.0, 100.0, 2500.0, 1), (60.25, 30.0, 2500.0, 1), (-15.0, 200.0, 2000.0, 1), (35.0, 280.0, 2500.0, -1),
            (12.0, 140.0, 3200.0, 1), (12.0, 142.5, 1500.0, 1)]
    s = planted(lat, lon, lows, 150.0, ripple=40.0, strength=2e-4)
    ref, _ = compare("721 x 1440", [s], lat, lon, cfg)
    assert len(ref) >= 4


def test_capacity_below_the_count():
    (lat, lon), kw, sigma = GRIDS["33x64"]
    cfg = T.TrackerConfig(**kw)
    states = [planted(lat, lon, VORTICES, sigma, shift=3.0 * m) for m in range(2)]
    ref, _ = reference(states, lat, lon, cfg)
    assert len(ref) >= 6
    n, rec = run_op(states, lat, lon, cfg, capacity=3)          # (run_op checks that nothing beyond three records was written)
    assert n == len(ref) and len(rec) == 3
    want = {(c["member"], c["j"], c["i"]): c for c in ref}
    for r in rec:
        c = want[(int(r["member"]), int(r["j"]), int(r["i"]))]
        assert r["msl"].tobytes() == np.float32(c["msl"]).tobytes()
    n0, rec0 = run_op(states, lat, lon, cfg, capacity=0)
    assert n0 == len(ref) and len(rec0) == 0
    names = ["msl", "u10m", "v10m", "u850", "v850", "z200", "z850"]
    tracker = T.LeadTracker("toy", names, lat, lon, 2, dict(kw, capacity=1), DEV)
    members = [torch.from_numpy(s).to(DEV) for s in states]
    with pytest.raises(RuntimeError, match=rf"{len(ref)} candidates.*holds 2"):
        tracker.add(datetime.datetime(2024, 5, 13), members)
    ok = T.LeadTracker("toy", names, lat, lon, 2, kw, DEV)
    ok.add(datetime.datetime(2024, 5, 13), members)
    assert [(r["member"], r["j"], r["i"]) for r in ok.records[0]] == [(c["member"], c["j"], c["i"]) for c in ref]
