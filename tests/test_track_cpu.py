"""Cyclone tracking without a GPU: the window tables against brute-force haversine masks, the geometry refusals, the C ABI of
include/skyrim_track.h (exports, argument errors), the channel plan, the linker on hand-written candidates, the strike probability
and the JSON file."""
from __future__ import annotations

import datetime
import re
from pathlib import Path

import numpy as np
import pytest

import _track_reference as R
from skyrim_amd import tracks as T

HEADER = Path(__file__).resolve().parent.parent / "include" / "skyrim_track.h"
T0 = datetime.datetime(2024, 5, 13, 18, 0)


def grid(n_lat, n_lon, rows=None, ascending=False):
    lat = np.linspace(90.0, -90.0, n_lat)[:rows]
    return (lat[::-1].copy() if ascending else lat), np.arange(n_lon) * (360.0 / n_lon)


# ---- 1. geometry ------------------------------------------------------------------------------------------------------------------------ #
TOY = dict(lat_max=60.0, r_msl_km=2500.0, r_vort_km=1500.0, r_wind_km=1900.0, r_core_km=2100.0)
GRIDS = {"33x64": (grid(33, 64), TOY),
         "49x192": (grid(49, 192), dict(lat_max=60.0, r_msl_km=1700.0, r_vort_km=1000.0, r_wind_km=1300.0, r_core_km=1100.0)),
         "32of33x64": (grid(33, 64, rows=32), TOY),
         "ascending": (grid(33, 64, ascending=True), TOY)}


def _check_rows(lat, lon, geo, cfg, rows):
    for name, radius in zip(T.CRITERIA, cfg.radii()):
        table, D = geo.h[name], geo.d[name]
        for j in rows:
            want = R.mask_half_widths(lat, lon, j, radius)
            got = {j + dj: int(table[j - geo.j0, dj + D]) for dj in range(-D, D + 1) if table[j - geo.j0, dj + D] >= 0}
            assert got == want, (name, j)


@pytest.mark.parametrize("case", list(GRIDS))
def test_tables_equal_brute_force_masks(case):
    (lat, lon), kw = GRIDS[case]
    cfg = T.TrackerConfig(**kw)
    geo = T.geometry(lat, lon, cfg)
    assert (geo.j0, geo.j1) == R.band(lat, cfg.lat_max) and T.geometry(lat, lon, cfg) is geo                 # cached
    assert R.radius_margin(lat, lon, cfg.lat_max, cfg.radii()) > 1e-9
    _check_rows(lat, lon, geo, cfg, range(geo.j0, geo.j1))
    assert geo.rowc.dtype == np.float32 and np.array_equal(geo.rowc, R.row_coefficients(lat, lon))
    assert np.all(geo.rowc[[0, -1]] == 0) and set(np.unique(geo.rowc[1:-1, 3])) <= {-1.0, 0.0, 1.0}


def test_tables_at_full_size_default_radii():
    lat, lon = grid(721, 1440)
    cfg = T.TrackerConfig()
    geo = T.geometry(lat, lon, cfg)
    assert (geo.j0, geo.j1) == (120, 601) and geo.d == dict(msl=16, vort=10, wind=10, core=10)
    assert geo.h["vort"].max() == 20 and geo.h["msl"].max() == 32                  # 278 km at 60 degrees: 41 points; 445 km: 65
    _check_rows(lat, lon, geo, cfg, (120, 121, 240, 359, 360, 361, 483, 599, 600))
    lat720 = lat[:720]
    g720 = T.geometry(lat720, lon, cfg)
    assert np.array_equal(g720.h["msl"], geo.h["msl"]) and np.array_equal(g720.rowc[:719], geo.rowc[:719])


def test_geometry_refusals():
    lat, lon = grid(33, 64)
    with pytest.raises(ValueError, match="points wide on a circle"):
        T.geometry(lat, lon, T.TrackerConfig(**dict(TOY, lat_max=75.0, r_msl_km=5300.0)))
    with pytest.raises(ValueError, match="pole row"):
        T.geometry(lat, lon, T.TrackerConfig(**dict(TOY, lat_max=80.0, r_msl_km=1300.0)))
    with pytest.raises(ValueError, match="3 x 3 neighbourhood"):
        T.geometry(lat, lon, T.TrackerConfig(**dict(TOY, r_msl_km=700.0)))            # a grid step is 625 km, more at the diagonal
    with pytest.raises(ValueError, match="3 x 3 neighbourhood"):
        T.geometry(lat, lon, T.TrackerConfig(**dict(TOY, r_msl_km=400.0)))            # not even the next row
    with pytest.raises(ValueError, match="uniform longitudes"):
        T.geometry(lat, lon[:40], T.TrackerConfig(**TOY))


# ---- 2. ABI ------------------------------------------------------------------------------------------------------------------------------ #
def test_library_exports_every_declared_symbol():
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    syms = sorted(set(re.findall(r"\b(sktrack_[a-z0-9_]+)\s*\(", text)))
    lib = T.load_library()
    assert syms == sorted(T.EXPORTS) and len(syms) == 3
    for s in syms:
        assert hasattr(lib, s)
    assert lib.sktrack_abi_version() == T.ABI_VERSION == int(re.search(r"SKTRACK_ABI_VERSION (\d+)", text).group(1))
    assert T.SPEC.env == "SKYRIM_TRACK_LIB" and int(re.search(r"SKTRACK_MAX_MEMBERS (\d+)", text).group(1)) == T.MAX_MEMBERS
    assert T.RECORD.itemsize == 32 and T.RECORD.names == ("member", "j", "i", "msl", "vort", "wind", "core", "pad")
    from skyrim_amd import ops
    assert "track_detect" in ops.OP_NAMES


def _desc():
    fake = 4096                                                # never dereferenced: the argument checks come first
    d = T.TrackDesc()
    d.members, d.M, d.C, d.H, d.W = fake, 4, 7, 33, 64
    d.ch_msl, d.ch_u10, d.ch_v10, d.ch_u850, d.ch_v850, d.ch_zup, d.ch_zlo = 0, 1, 2, 3, 4, 5, 6
    d.j0, d.j1 = 6, 27
    d.thr_msl, d.thr_vort, d.thr_wind, d.thr_core = np.inf, 1e-5, 5.0, 0.0
    d.h_msl = d.h_vort = d.h_wind = d.h_core = d.rowc = d.records = d.count = d.workspace = fake
    d.d_msl, d.d_vort, d.d_wind, d.d_core = 4, 2, 3, 3
    d.capacity, d.workspace_bytes = 16, 16 + 8 * 4 * 11 * 32
    return d


def test_argument_errors_need_no_gpu():
    import ctypes
    lib = T.load_library()
    assert lib.sktrack_workspace_bytes(4, 21, 64) == 16 + 8 * 4 * 11 * 32
    assert lib.sktrack_workspace_bytes(50, 481, 1440) == 16 + 8 * 50 * 241 * 720
    for bad in ((0, 21, 64), (65, 21, 64), (4, 0, 64), (4, 21, 2)):
        assert lib.sktrack_workspace_bytes(*bad) == 0
    assert lib.sktrack_detect(None, None) == -1
    changes = [("members", None), ("M", 0), ("M", 65), ("W", 2), ("ch_msl", 7), ("ch_u850", -1), ("ch_zlo", -1), ("ch_zup", 9), ("j0", 27),
               ("j1", 34), ("j0", 4), ("d_msl", 6), ("d_vort", -1), ("j1", 32), ("h_msl", None), ("h_core", None), ("h_wind", 4098),
               ("rowc", None), ("rowc", 4100), ("records", None), ("capacity", -1), ("count", None), ("count", 4098), ("workspace", None),
               ("workspace", 4100), ("workspace_bytes", 16 + 8 * 4 * 11 * 32 - 1), ("C", 1 << 20)]
    for field, value in changes:
        d = _desc()
        setattr(d, field, value)
        assert lib.sktrack_detect(ctypes.byref(d), None) == -1, (field, value)


# ---- 3. channels ----------------------------------------------------------------------------------------------------------------------- #
def test_channel_plan():
    from skyrim_amd.dlwp.spec import CHANNELS as DLWP
    from skyrim_amd.fcn.spec import CHANNELS as FCN
    from skyrim_amd.pangu.spec import CHANNELS as PANGU
    p = T.channel_plan(PANGU, None, "pangu")
    assert p.warm_core and [PANGU[k] for k in (p.msl, p.u10, p.v10, p.u850, p.v850, p.z_up, p.z_lo)] == \
        ["msl", "u10m", "v10m", "u850", "v850", "z200", "z850"]
    with pytest.raises(ValueError, match=r"dlwp.*'msl'"):
        T.channel_plan(DLWP, None, "dlwp")
    f = T.channel_plan(FCN, None, "fourcastnet")
    assert not f.warm_core and (f.z_up, f.z_lo) == (-1, -1) and "dropped" in f.note and "z200" in f.note
    with pytest.raises(ValueError, match="z300"):
        T.channel_plan(FCN, T.TrackerConfig(core_levels=("z300", "z850")), "fourcastnet")
    assert T.channel_plan(FCN, T.TrackerConfig(core_levels=("z500", "z850")), "fourcastnet").warm_core
    assert not T.channel_plan(PANGU, dict(core_levels=None), "pangu").warm_core
    with pytest.raises(ValueError, match="dlwp"):                      # the whole request, before any device
        T.check_request("dlwp", DLWP, *grid(33, 64), 1, TOY)
    with pytest.raises(ValueError, match="1 to 64"):
        T.check_request("pangu", PANGU, *grid(33, 64), 65, TOY)


# ---- 4. the linker ---------------------------------------------------------------------------------------------------------------------- #
def _cands(points):
    return [dict(lat=la, lon=lo % 360.0, msl=1e5, wind=10.0, vort=1e-4, core=1.0) for la, lo in points]


def _times(n, hours=6):
    return [T0 + datetime.timedelta(hours=hours * k) for k in range(n)]


def _both(times, steps, **kw):
    got = T.link(times, [_cands(s) for s in steps], **kw)
    ref = R.link(times, [[(la, lo % 360.0) for la, lo in s] for s in steps], **kw)
    assert [list(zip(tr["lat"], tr["lon"])) for tr in got] == [[(steps[t][k][0], steps[t][k][1] % 360.0) for t, k in tr] for tr in ref]
    return got


def test_linker_crossing_paths():
    # two storms moving towards each other along a parallel: 2 degrees per step each, they swap sides between steps 2 and 3;
    # the displacement prediction keeps each on its course
    a = [(20.0, 100.0 + 2.0 * k) for k in range(6)]
    b = [(20.5, 111.0 - 2.0 * k) for k in range(6)]
    steps = [sorted([a[k], b[k]], key=lambda p: (-p[0], p[1])) for k in range(6)]
    got = _both(_times(6), steps)
    assert len(got) == 2
    lons = sorted(tuple(tr["lon"]) for tr in got)
    assert lons == sorted([tuple(p[1] for p in a), tuple(p[1] for p in b)])


def test_linker_across_the_seam_and_speed_limit():
    seam = [[(15.0, 357.0 + 1.5 * k)] for k in range(5)]                                 # 357, 358.5, 0, 1.5, 3
    got = _both(_times(5), seam)
    assert len(got) == 1 and got[0]["lon"] == [357.0, 358.5, 0.0, 1.5, 3.0]
    # 6 degrees of longitude on the equator beyond the predicted 14: 667 km > 90 km/h x 6 h = 540 km -> the track ends, a new one starts
    fast = [[(0.0, 10.0)], [(0.0, 12.0)], [(0.0, 20.0)], [(0.0, 22.0)]]
    got = _both(_times(4), fast)
    assert [tr["lon"] for tr in got] == [[10.0, 12.0], [20.0, 22.0]]
    assert len(_both(_times(4), fast, max_speed_kmh=150.0)) == 1


def test_linker_min_points_and_ties():
    steps = [[(10.0, 50.0), (-30.0, 200.0)], [(10.5, 51.0)], [(11.0, 52.0)]]
    assert [len(tr["times"]) for tr in _both(_times(3), steps)] == [3]
    assert [len(tr["times"]) for tr in _both(_times(3), steps, min_points=1)] == [3, 1]
    assert _both(_times(3), steps, min_points=4) == []
    # a distance tie: two tracks at equal distance from one candidate -> the lower track id takes it; then one track at equal distance
    # from two candidates -> the lower candidate index
    tie = [[(0.0, 100.0), (0.0, 104.0)], [(0.0, 102.0)]]
    got = _both(_times(2), tie, min_points=1)
    assert [tr["lon"] for tr in got] == [[100.0, 102.0], [104.0]]
    tie2 = [[(0.0, 102.0)], [(0.0, 100.0), (0.0, 104.0)]]
    got = _both(_times(2), tie2, min_points=1)
    assert [tr["lon"] for tr in got] == [[102.0, 100.0], [104.0]]


# ---- 5. the result ---------------------------------------------------------------------------------------------------------------------- #
def _some_tracks():
    lat, lon = grid(49, 192)
    times = _times(3)
    trs = [dict(member=0, times=times, lat=[30.0, 31.0, 33.0], lon=[358.0, 359.5, 1.0], msl=[99000.0, 98500.0, 98000.0],
                wind=[20.0, 25.0, 30.0], vort=[1e-4, 2e-4, 3e-4], core=[5.0, 6.0, float("nan")]),
           dict(member=2, times=times[1:], lat=[-41.25, -45.0], lon=[120.0, 123.75], msl=[97000.0, 96000.0], wind=[18.0, 19.0],
                vort=[9e-5, 8e-5], core=[1.0, 2.0])]
    crit = dict(T.asdict(T.TrackerConfig()), band=(8, 41), warm_core=True, note="")
    return T.Tracks("pangu", 4, times, lat, lon, trs, crit, "abc")


def test_strike_probability_against_brute_force():
    tr = _some_tracks()
    for radius in (120.0, 500.0, 1500.0):
        sp = tr.strike_probability(radius)
        pts = {0: list(zip(tr.tracks[0]["lat"], tr.tracks[0]["lon"])), 2: list(zip(tr.tracks[1]["lat"], tr.tracks[1]["lon"]))}
        ref = R.strike_probability(pts, 4, tr.lat, tr.lon, radius)
        assert sp.dims == ("lat", "lon") and np.array_equal(sp.values, ref)
    assert set(np.unique(tr.strike_probability(1500.0).values)) == {0.0, 0.25} and tr.strike_probability(120.0).values[36, 66] == 0.25


def test_json_round_trip(tmp_path):
    tr = _some_tracks()
    path = tr.save(tmp_path)
    assert Path(path) == tmp_path / "abc" / "pangu-ens4-tracks.json"
    back = T.Tracks.load(path)
    assert back.model_name == "pangu" and back.n_members == 4 and back.times == tr.times and back.forecast_id == "abc"
    assert back.criteria == tr.criteria and np.array_equal(back.lat, tr.lat) and np.array_equal(back.lon, tr.lon)
    assert len(back) == 2
    for a, b in zip(back, tr):
        assert a["member"] == b["member"] and a["times"] == b["times"]
        for f in T.FIELDS:
            assert np.array_equal(a[f], b[f], equal_nan=True)
    assert T.Tracks("fuxi", 1, [], tr.lat, tr.lon, [], {}).file_name() == "fuxi-tracks.json"


def test_command_line_options():
    from click.testing import CliRunner
    from skyrim_amd import track_cli
    res = CliRunner().invoke(track_cli.track, ["--help"])
    assert res.exit_code == 0 and track_cli.track.name == "track"
    for opt in ("--model_name", "--lead_time", "--members", "--thr_wind", "--output_dir"):
        assert opt in res.output
