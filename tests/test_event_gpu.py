"""Event verification end to end on the MI355X with the Pangu toy model (49 x 192): ``ensemble_forecast(scores=True, events=...)`` for a
raw channel and a derived field, and on a target grid, against the numpy restatement on the kept members (integers exact, scores to
1e-12); ``verify(events=...)`` at M = 1 against the restatement on ``forecast()`` output; ``score_prediction`` on saved files; the same
requests without ``events``; and the ``verify`` command with ``--event``."""
from __future__ import annotations

import datetime
import json
from pathlib import Path

import numpy as np
import pytest

import _event_reference as R
from skyrim_amd import events as E
from skyrim_amd import verify as V

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T0 = datetime.datetime(2024, 5, 13, 18, 0)
TARGET = (np.linspace(90.0, -90.0, 13), np.arange(48) * 7.5)
RADII = (0.0, 500.0, 1500.0)
KW = dict(n_steps=2, n_members=5, keep_members=True, products=(), perturb_scale=0.05)


@pytest.fixture(scope="module")
def pangu(toy):
    from skyrim_amd.core.models.pangu import PanguModel
    g, params, _ = toy
    return PanguModel(ic_source="gfs", geom=g, params=params)


@pytest.fixture(scope="module")
def plain(pangu):
    """The ensemble without scores: its members give the truth (the control run) and the thresholds.  Computed once, left unchanged."""
    return pangu.ensemble_forecast(T0, derived=["ws10m"], **KW)


@pytest.fixture(scope="module")
def truth(pangu, plain):
    from skyrim_amd.labeled import DataArray
    lat, lon = np.asarray(pangu.model.grid.lat), np.asarray(pangu.model.grid.lon)
    return DataArray(np.asarray(plain.members.values)[0], ["time", "channel", "lat", "lon"],
                     dict(time=list(plain.members.time.values), channel=plain.members.channel.values.tolist(), lat=lat, lon=lon))


def _quantiles(values, levels):
    return [float(np.float32(v)) for v in np.quantile(np.asarray(values, np.float64), levels)]


def _against_restatement(ev, members, truth, lat, lon, what):
    """``ev`` (EventScores) against the restatement: members {channel: (M, T, H, W)}, truth {channel: (T, H, W)}."""
    M = ev.n_members
    w = V.area_weights(lat)
    assert ev.neighbourhoods_km == [float(r) for r in RADII][:len(ev.neighbourhoods_km)]
    win = [E.windows(lat, lon, r) for r in ev.neighbourhoods_km]
    worst, rates = 0.0, []
    for t in range(len(ev.times)):
        for e, c in enumerate(ev.channels):
            for i, thr in enumerate(ev.thresholds[c]):
                k, o = R.point_counts(members[c][:, t], truth[c][t], thr)
                assert np.array_equal(ev.counts.values[t, e, i], R.joint_counts(k, o, M).sum(axis=0)), (what, t, c, thr)
                ref = R.scores(k, o, M, w)
                for name in ev.names:
                    got = ev.fss.values[t, e, i] if name == "fss" else getattr(ev, name).values[t, e, i]
                    want = np.array([R.fss(k, o, M, hy, hx, w) for hy, hx in win]) if name == "fss" else ref[name]
                    assert np.allclose(got, want, rtol=0, atol=1e-12, equal_nan=True), (what, name, t, c, thr, got, want)
                    worst = max(worst, float(np.nan_to_num(np.abs(np.asarray(got) - want)).max()))
                rates.append(ref["base_rate"])
            assert np.isnan(ev.brier.values[t, e, len(ev.thresholds[c]):]).all()
    print(f"{what}: worst difference from the restatement {worst:.2e}; base rates {min(rates):.3f} .. {max(rates):.3f}")
    assert 0 < max(rates) < 1, what                                  # the thresholds cut through the values


def test_ensemble_events_of_a_raw_and_a_derived_channel(pangu, plain, truth):
    names = plain.members.channel.values.tolist()
    lat, lon = np.asarray(pangu.model.grid.lat), np.asarray(pangu.model.grid.lon)
    k2 = names.index("t2m")
    events = {"t2m": _quantiles(plain.members.values[:, :, k2], [0.5, 0.9]), "ws10m": _quantiles(plain.derived.members.values[:, :, 0], [0.3, 0.7, 0.95])}
    kw = dict(KW, derived=["ws10m"], scores=True, truth=truth)
    ens = pangu.ensemble_forecast(T0, events=events, neighbourhoods_km=RADII, **kw)
    assert np.array_equal(ens.members.values, plain.members.values) and np.array_equal(ens.derived.members.values, plain.derived.members.values)
    ev, dev = ens.scores.events, ens.derived.scores.events
    assert ev.channels == ["t2m"] and dev.channels == ["ws10m"] and ev.n_members == 5 and "brier_fair" in ev.names and "fss" in ev.names
    assert ev.fss.shape == (3, 1, 4, 3) and ev.brier.dims == ("time", "channel", "threshold")
    m = np.asarray(ens.members.values)[:, :, k2]
    _against_restatement(ev, {"t2m": m}, {"t2m": m[0]}, lat, lon, "raw t2m")
    dm = np.asarray(ens.derived.members.values)[:, :, 0]
    _against_restatement(dev, {"ws10m": dm}, {"ws10m": dm[0]}, lat, lon, "derived ws10m")      # the derived truth is the derived control
    # the same request without events: no events, and the scores bit for bit
    none = pangu.ensemble_forecast(T0, **kw)
    assert none.scores.events is None and none.derived.scores.events is None and '"events"' not in none.scores.to_json()
    assert np.array_equal(none.scores.sums.values, ens.scores.sums.values) and np.array_equal(none.scores.rank_counts.values, ens.scores.rank_counts.values)
    assert np.array_equal(none.derived.scores.sums.values, ens.derived.scores.sums.values)
    back = V.Scores.from_json(ens.scores.to_json())
    assert np.array_equal(back.events.counts.values, ev.counts.values) and np.array_equal(back.events.fss.values, ev.fss.values, equal_nan=True)
    # events=True: the thresholds of exceed
    same = pangu.ensemble_forecast(T0, exceed={"t2m": events["t2m"]}, events=True, **dict(kw, keep_members=False))
    assert same.scores.events.thresholds == {"t2m": events["t2m"]} and same.scores.events.fss is None
    assert np.array_equal(same.scores.events.counts.values, ev.counts.values)


def test_ensemble_events_on_a_target_grid(pangu, plain, truth):
    names = plain.members.channel.values.tolist()
    lat, lon = np.asarray(pangu.model.grid.lat), np.asarray(pangu.model.grid.lon)
    k2 = names.index("t2m")
    events = {"t2m": _quantiles(plain.members.values[:, :, k2], [0.6])}
    ens = pangu.ensemble_forecast(T0, grid=TARGET, scores=True, truth=truth, events=events, neighbourhoods_km=RADII[:2], **KW)
    m = np.asarray(ens.members.values)[:, :, k2]
    _against_restatement(ens.scores.events, {"t2m": m}, {"t2m": m[0]}, lat, lon, "raw t2m next to a grid")
    rm = np.asarray(ens.regridded.members.values)[:, :, k2]
    rev = ens.regridded.scores.events
    assert rev.fss.shape == (3, 1, 4, 2) and ens.regridded.scores.grid == "13x48"
    _against_restatement(rev, {"t2m": rm}, {"t2m": rm[0]}, *TARGET, "regridded t2m")           # the regridded truth is the regridded control
    region = dict(region=(-30.0, 30.0, 340.0, 20.0), res=7.5)
    with pytest.raises(ValueError, match="still available"):        # a regional target has no periodic windows ...
        pangu.ensemble_forecast(T0, grid=region, scores=True, truth=truth, events=events, neighbourhoods_km=(500.0,), **KW)


def test_verify_and_score_prediction_at_one_member(pangu, tmp_path):
    m = pangu
    names = list(m.out_channel_names)
    lat, lon = np.asarray(m.model.grid.lat), np.asarray(m.model.grid.lon)
    before = m.forecast(T0, n_steps=2)
    vals = np.array(before.values)                                  # (T, C, H, W)
    src = m.data_source
    order = [list(src.channel_names).index(n) for n in names]
    chans = ["t2m", "u10m"]
    events = {c: _quantiles(vals[:, names.index(c)], [0.5, 0.9]) for c in chans}
    s = m.verify(T0, n_steps=2, events=events, neighbourhoods_km=RADII)
    ev = s.events
    assert ev.n_members == 1 and ev.channels == chans and {"pod", "far", "csi", "ets", "frequency_bias"} <= set(ev.names) and "brier_fair" not in ev.names
    truth = {c: np.stack([np.asarray(src[t])[order][names.index(c)] for t in s.times]).astype(np.float32) for c in chans}
    _against_restatement(ev, {c: vals[None, :, names.index(c)] for c in chans}, truth, lat, lon, "verify at M = 1")
    assert np.all(ev.pod.values[0, :, :2] == 1) and np.all(ev.far.values[0, :, :2] == 0) and np.all(ev.fss.values[0, :, :2] == 1)      # lead 0
    plain = m.verify(T0, n_steps=2)
    assert plain.events is None and np.array_equal(plain.sums.values, s.sums.values) and '"events"' not in plain.to_json()
    assert np.array_equal(np.asarray(m.forecast(T0, n_steps=2).values), vals)          # forecast() after verify(): the bits it gave before
    cfg = {"output_dir": str(tmp_path), "file_type": "netcdf"}
    _, paths = m.rollout(T0, n_steps=2, save=True, save_config=cfg)
    sp = V.score_prediction(list(paths), src, device=DEV, events=events, neighbourhoods_km=RADII)
    assert sp.times == s.times and np.array_equal(sp.events.counts.values, ev.counts.values)
    for name in ev.names:
        assert np.array_equal(getattr(sp.events, name).values, getattr(ev, name).values, equal_nan=True), name
    assert V.score_prediction(list(paths), src, device=DEV).events is None


def test_verify_command_line_writes_the_events(tmp_path):
    from click.testing import CliRunner
    from skyrim_amd.verify_cli import verify
    for extra, name in (([], "pangu-scores.json"),):               # (the ensemble route hands the same keywords on: tested above)
        res = CliRunner().invoke(verify, ["-m", "pangu", "-l", "6", "-o", str(tmp_path), "-d", "20240513", "-t", "1800", "--event", "t2m:270,285",
                                          "--event", "u10m:5", "--neighbourhood_km", "0", "--neighbourhood_km", "500"] + extra)
        assert res.exit_code == 0, res.output + repr(res.exception)
        path = [ln for ln in res.output.splitlines() if ln.endswith(".json")]
        assert len(path) == 1 and Path(path[0]).name == name
        doc = json.loads(Path(path[0]).read_text())["events"]
        assert doc["channels"] == ["t2m", "u10m"] and doc["thresholds"] == {"t2m": [270.0, 285.0], "u10m": [5.0]} and doc["neighbourhoods_km"] == [0.0, 500.0]
        assert np.asarray(doc["counts"]).shape == (2, 2, 4, 2, 2 if not extra else 4) and "fss" in doc["scores"] and "brier" in doc["scores"]
        assert sum(">" in ln and ln.startswith("+") for ln in res.output.splitlines()) == 2 * 3          # two lead times x three events
        ev = V.Scores.load(path[0]).events
        assert ev.n_members == (3 if extra else 1)
        points = ev.counts.values[:, 0, :2].sum(axis=(-1, -2))
        assert points.min() == points.max() > 0 and np.all(ev.counts.values[:, 1, 1:] == 0)      # every point once; no second u10m threshold
