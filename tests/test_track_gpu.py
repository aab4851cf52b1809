"""Cyclone tracking end to end on the MI355X with the Pangu toy model (49 x 192): ``ensemble_forecast(tracks=True)`` against the float64
restatement and the reference linker on the kept members, ``tracks=False`` unchanged, ``track_cyclones`` against ``track_prediction``
on the files of the same rollout, and the refusal for a model without the channels."""
from __future__ import annotations

import datetime
from types import SimpleNamespace

import numpy as np
import pytest

import _track_reference as R
from skyrim_amd import tracks as T

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T0 = datetime.datetime(2024, 5, 13, 18, 0)
# thresholds far below anything a field holds: every minimum of an msl window is a candidate, and no value is near a threshold
CFG = dict(lat_max=60.0, r_msl_km=1700.0, r_vort_km=1000.0, r_wind_km=1300.0, r_core_km=1100.0, thr_vort=-1e30, thr_wind=0.0, thr_core=-1e30,
           max_speed_kmh=400.0, min_points=1, capacity=512)


@pytest.fixture(scope="module")
def pangu(toy):
    from skyrim_amd.core.models.pangu import PanguModel
    g, params, _ = toy
    return PanguModel(ic_source="gfs", geom=g, params=params)


def _reference_tracks(members, times, names, lat, lon, cfg):
    """(tracks as lists of (time index, lat, lon, msl bits) per member in start order, candidates at step 0, worst share of a bound)."""
    ch = dict(msl=names.index("msl"), u10=names.index("u10m"), v10=names.index("v10m"), u850=names.index("u850"), v850=names.index("v850"),
              z_up=names.index("z200"), z_lo=names.index("z850"))
    thr = dict(msl=cfg.thr_msl, vort=cfg.thr_vort, wind=cfg.thr_wind, core=cfg.thr_core)
    out, first = [], 0
    for m in range(members.shape[0]):
        cands = [R.detect(np.ascontiguousarray(members[m, t]), lat, lon, ch, cfg.radii(), thr, cfg.lat_max)[0] for t in range(len(times))]
        first += len(cands[0])
        pts = [[(float(lat[c["j"]]), float(lon[c["i"]])) for c in step] for step in cands]
        for tr in R.link(times, pts, cfg.max_speed_kmh, cfg.min_points):
            out.append((m, [(t, cands[t][k]) for t, k in tr]))
    return out, first


def test_ensemble_tracks_equal_the_restatement_on_the_members(pangu):
    kw = dict(n_steps=2, n_members=3, keep_members=True, products=("mean", "spread"), perturb_scale=0.05)
    plain = pangu.ensemble_forecast(T0, **kw)
    ens = pangu.ensemble_forecast(T0, tracks=True, track_config=CFG, **kw)
    assert plain.tracks is None and isinstance(ens.tracks, T.Tracks)
    for p in ("mean", "spread", "members"):
        assert np.array_equal(getattr(plain, p).values, getattr(ens, p).values)
    cfg = T.as_config(CFG)
    names = ens.members.channel.values.tolist()
    lat, lon = np.asarray(pangu.model.grid.lat, np.float64), np.asarray(pangu.model.grid.lon, np.float64)
    times = list(ens.tracks.times)
    assert len(times) == 3 and ens.tracks.n_members == 3 and ens.tracks.criteria["warm_core"] and ens.tracks.criteria["thr_wind"] == 0.0
    ref, first = _reference_tracks(np.asarray(ens.members.values), times, names, lat, lon, cfg)
    assert first >= 1, "the restatement finds no candidate at step 0"
    assert len(ens.tracks) == len(ref) >= 1
    worst = 0.0
    for got, (m, pts) in zip(ens.tracks, ref):
        assert got["member"] == m and got["times"] == [times[t] for t, _ in pts]
        assert got["lat"] == [float(lat[c["j"]]) for _, c in pts] and got["lon"] == [float(lon[c["i"]]) for _, c in pts]
        assert np.asarray(got["msl"], np.float32).tobytes() == np.asarray([c["msl"] for _, c in pts], np.float32).tobytes()
        for k in ("vort", "wind", "core"):
            for v, (_, c) in zip(got[k], pts):
                worst = max(worst, abs(v - c[k]) / c["b_" + k] if c["b_" + k] > 0 else (0.0 if v == c[k] else np.inf))
    print(f"ensemble tracks: {len(ref)} tracks, {first} candidates at step 0, worst share of a bound {worst:.3f}")
    assert worst <= 1
    sp = ens.tracks.strike_probability(500.0)
    pts = {}
    for tr in ens.tracks:
        pts.setdefault(tr["member"], []).extend(zip(tr["lat"], tr["lon"]))
    assert np.array_equal(sp.values, R.strike_probability(pts, 3, lat, lon, 500.0)) and sp.values.max() > 0


def test_track_cyclones_equals_track_prediction_on_saved_files(pangu, tmp_path):
    cfg = {"output_dir": str(tmp_path)}
    live = pangu.track_cyclones(T0, n_steps=2, config=CFG, save=True, save_config=cfg)
    assert len(live) >= 1 and live.n_members == 1 and len(live.times) == 3
    assert T.Tracks.load(live.path).criteria == live.criteria and live.path.endswith("pangu-tracks.json")
    _, paths = pangu.rollout(T0, n_steps=2, save=True, save_config={"output_dir": str(tmp_path / "files")})
    disk = T.track_prediction(list(paths), config=CFG, device=DEV)
    assert [np.datetime64(t, "s") for t in disk.times] == [np.datetime64(t, "s") for t in live.times] and len(disk) == len(live)
    for a, b in zip(disk, live):
        assert a["lat"] == b["lat"] and a["lon"] == b["lon"] and len(a["times"]) == len(b["times"])
        for k in ("msl", "vort", "wind", "core"):
            assert np.allclose(a[k], b[k], rtol=1e-4, atol=0)


def test_dlwp_is_refused_before_the_device_is_touched():
    from skyrim_amd.core import Skyrim
    from skyrim_amd.core.models.dlwp import DLWPModel
    from skyrim_amd.dlwp.spec import CHANNELS

    class NoDevice:
        out_channel_names = list(CHANNELS)
        grid = SimpleNamespace(lat=np.linspace(90, -90, 721), lon=np.arange(1440) * 0.25)

        def __getattr__(self, name):                            # the device, the generator: nothing of it may be asked for
            raise AssertionError(f"model.{name} was read before the refusal")

    gm = object.__new__(DLWPModel)
    gm.model_name, gm.model = "dlwp", NoDevice()
    s = object.__new__(Skyrim)
    s.model = gm
    with pytest.raises(ValueError, match=r"dlwp cannot be tracked.*'msl'"):
        s.track_cyclones(T0)
    with pytest.raises(ValueError, match=r"dlwp cannot be tracked"):
        T.LeadTracker("dlwp", CHANNELS, NoDevice.grid.lat, NoDevice.grid.lon, 4, None, DEV)
