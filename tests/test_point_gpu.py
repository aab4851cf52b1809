"""Point forecasts end to end on the MI355X with the Pangu toy model (49 x 192): ``ensemble_forecast(points=...)`` against the float32
restatement of include/skyrim_point.h applied to the kept members -- raw channels, derived fields and closed aggregate windows, bit for
bit -- with every other product unchanged, the statistics and station scores of the sampled values, ``point_forecast`` against
``extract_prediction`` on the files of the same rollout, the command line, and the refusals that come before the device."""
from __future__ import annotations

import csv
import datetime

import numpy as np
import pytest

import _ens_reference as ER
import _point_reference as R
from skyrim_amd import points as P

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T0 = datetime.datetime(2024, 5, 13, 18, 0)
H6 = datetime.timedelta(hours=6)
KW = dict(n_steps=5, n_members=3, keep_members=True, products=("mean", "spread"), perturb_scale=0.05, derived=["ws10m"],
          aggregates=["ws10m:max:12h"])
PLACES = {"node": (45.0, 30.0), "Istanbul": (41.01, 28.98), "west of Greenwich": (51.48, -0.4), "north pole": (90.0, 10.0),
          "south pole": (-90.0, 359.0), "Quito": (-0.18, 281.53), "date line": (-17.7, 179.99), "on a row": (-7.5, 100.3)}
CHANNELS = ["t2m", "ws10m", "msl", "u10m"]                                    # raw and derived, in the order asked for


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def pangu(toy):
    from skyrim_amd.core.models.pangu import PanguModel
    g, params, _ = toy
    return PanguModel(ic_source="gfs", geom=g, params=params)


@pytest.fixture(scope="module")
def plain(pangu):
    """The ensemble without points: computed once, shared, left unchanged."""
    return pangu.ensemble_forecast(T0, **KW)


@pytest.fixture(scope="module")
def ens(pangu):
    return pangu.ensemble_forecast(T0, points=PLACES, point_channels=CHANNELS, **KW)


def test_without_points_nothing_changes(plain, ens):
    assert plain.points is None and plain.aggregated["12h"].points is None
    for p in ("mean", "spread", "members"):                                    # bit for bit what they were
        assert not np.any(bits(getattr(plain, p).values) != bits(getattr(ens, p).values)), p
        assert not np.any(bits(getattr(plain.derived, p).values) != bits(getattr(ens.derived, p).values)), p
        assert not np.any(bits(getattr(plain.aggregated["12h"], p).values) != bits(getattr(ens.aggregated["12h"], p).values)), p


def test_sampled_members_equal_the_restatement_on_the_kept_members(pangu, ens):
    lat, lon = np.asarray(pangu.model.grid.lat), np.asarray(pangu.model.grid.lon)
    pf = ens.points
    v = pf.values
    assert v.dims == ("member", "time", "channel", "point") and v.shape == (3, 6, 4, len(PLACES)) and v.values.dtype == np.float32
    assert pf.channels == CHANNELS and pf.names == list(PLACES) and str(v.method.values) == "bilinear"
    assert [np.datetime64(t, "s") for t in v.time.values] == [np.datetime64(T0 + k * H6, "s") for k in range(6)]
    assert np.allclose(v.lat.values, [p[0] for p in PLACES.values()]) and np.allclose(v.lon.values, [p[1] % 360 for p in PLACES.values()])
    rec = P.records(PLACES, lat, lon)
    assert set(rec["nr"].tolist()) == {1, 2} and set(rec["ncol"].tolist()) == {1, 2} and rec["col"].max() == 191
    names = ens.members.channel.values.tolist()
    raw, der = np.asarray(ens.members.values), np.asarray(ens.derived.members.values)
    for t in range(6):
        both = np.ascontiguousarray(np.concatenate([raw[:, t], der[:, t]], axis=1))
        want = R.gather(both, [(names + ["ws10m"]).index(c) for c in CHANNELS], rec)
        assert not np.any(bits(v.values[:, t]) != bits(want)), t
    # the closed 12-h windows, sampled from the accumulator: window ends as time axis
    a = ens.aggregated["12h"]
    ap = a.points
    assert ap.channels == ["ws10m_max_12h"] and ap.names == list(PLACES) and ap.values.shape == (3, 2, 1, len(PLACES))
    assert [np.datetime64(t, "s") for t in ap.values.time.values] == [np.datetime64(T0 + 2 * H6, "s"), np.datetime64(T0 + 4 * H6, "s")]
    am = np.asarray(a.members.values)
    for w in range(2):
        assert not np.any(bits(ap.values.values[:, w]) != bits(R.gather(np.ascontiguousarray(am[:, w]), [0], rec))), w


def test_a_node_with_nearest_is_that_cell(pangu, ens):
    lat, lon = np.asarray(pangu.model.grid.lat), np.asarray(pangu.model.grid.lon)
    j, i = 12, 16
    assert (lat[j], lon[i]) == (45.0, 30.0)
    near = pangu.ensemble_forecast(T0, points={"node": (45.0, 30.0), "close": (44.0, 30.5)}, point_channels=["msl", "ws10m"], point_method="nearest",
                                   **KW).points
    raw, der = np.asarray(ens.members.values), np.asarray(ens.derived.members.values)
    k = ens.members.channel.values.tolist().index("msl")
    for p in range(2):
        assert not np.any(bits(near.values.values[:, :, 0, p]) != bits(raw[:, :, k, j, i]))
        assert not np.any(bits(near.values.values[:, :, 1, p]) != bits(der[:, :, 0, j, i]))
    # bilinear on the node: one tap of weight 1, the same cell
    assert not np.any(bits(ens.points.values.values[:, :, 2, 0]) != bits(raw[:, :, k, j, i]))


def test_statistics_and_station_scores_of_the_sampled_values(ens):
    pf = ens.points
    x = np.asarray(pf.values.values)
    r = ER.stats(x.reshape(3, -1), levels=[0.25, 0.5])
    assert np.array_equal(pf.mean().values.reshape(-1), r["mean"])
    np.testing.assert_allclose(pf.spread().values.reshape(-1), r["spread"], rtol=1e-13)
    q = pf.quantile([0.25, 0.5]).values
    for i in range(2):
        np.testing.assert_allclose(q[i].reshape(-1), r["quant"][i][0], rtol=1e-14)
    # observations taken from the control member: member 0 alone has RMSE 0, the ensemble does not
    obs = {c: x[0, :, k].astype(np.float64) for k, c in enumerate(pf.channels)}
    control = P.PointForecast(pf.values.isel(member=[0]), pf.model_name)
    s0 = control.verify(obs)
    assert np.all(s0["rmse"] == 0) and np.all(s0["crps"] == 0) and np.all(s0["n"] == len(PLACES))
    s = pf.verify(obs)
    assert np.all(s["rmse"][1:] > 0) and np.all(s["rmse"][0, [0, 2, 3]] > 0) and s["channels"] == CHANNELS
    want = R.station_scores(x, np.stack([obs[c] for c in CHANNELS], axis=1))
    for k in ("bias", "mae", "rmse", "crps", "spread", "ssr"):
        np.testing.assert_allclose(s[k], want[k], rtol=1e-12, atol=0, equal_nan=True, err_msg=k)
    assert np.array_equal(s["rank_histogram"], want["rank_histogram"])


def test_point_forecast_equals_extract_prediction_on_saved_files(pangu, tmp_path):
    raw = ["t2m", "msl", "u10m"]
    live = pangu.point_forecast(T0, 3, points=PLACES, channels=raw + ["ws10m"], derived=["ws10m"])
    assert live.values.shape == (1, 4, 4, len(PLACES)) and live.channels == raw + ["ws10m"] and np.isfinite(live.values.values).all()
    _, paths = pangu.rollout(T0, n_steps=3, save=True, save_config={"output_dir": str(tmp_path)})
    disk = P.extract_prediction(list(paths), PLACES, channels=raw, device=DEV)
    assert disk.channels == raw and disk.times == live.times and disk.n_members == 1
    assert not np.any(bits(disk.values.values) != bits(live.values.values[:, :, :3]))
    near = P.extract_prediction(list(paths), PLACES, channels=["msl"], method="nearest", device=DEV)
    assert str(near.values.method.values) == "nearest" and not np.array_equal(near.values.values, disk.values.values[:, :, 1:2])
    from skyrim_amd.core import Skyrim
    s = object.__new__(Skyrim)
    s.model = pangu
    again = s.point_forecast(T0, 3, points=PLACES, channels=raw + ["ws10m"], derived=["ws10m"], save=True, save_config={"output_dir": str(tmp_path)})
    assert np.array_equal(again.values.values, live.values.values) and again.path.endswith("pangu-points.json")


def test_command_line_writes_the_same_values(pangu, tmp_path, monkeypatch):
    from click.testing import CliRunner
    import skyrim_amd.core as core
    from skyrim_amd.point_cli import point
    s = object.__new__(core.Skyrim)
    s.model = pangu
    monkeypatch.setattr(core, "Skyrim", lambda name, ic_source=None: s)          # the command line on the toy model
    out = tmp_path / "values.csv"
    obs = tmp_path / "obs.csv"
    live = pangu.point_forecast(T0, 2, points={"Istanbul": PLACES["Istanbul"], "Quito": PLACES["Quito"]}, channels=["t2m", "msl"])
    with open(obs, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["time", "channel", "point", "value"])
        for ti, t in enumerate(live.times):
            w.writerow([t.isoformat(), "t2m", "Istanbul", repr(float(live.values.values[0, ti, 0, 0]))])      # (the float32 as a double, digit for digit)
    res = CliRunner().invoke(point, ["-m", "pangu", "-d", "20240513", "-t", "1800", "--n_steps", "2", "--point", "Istanbul:41.01,28.98",
                                     "--point", "Quito:-0.18,281.53", "--channel", "t2m", "--channel", "msl", "--output", str(out),
                                     "--observations", str(obs)])
    assert res.exit_code == 0, res.output + repr(res.exception)
    rows = list(csv.reader(open(out)))
    assert rows[0] == ["time", "member", "channel", "point", "value"] and len(rows) == 1 + 3 * 2 * 2
    got = np.array([np.float32(r[4]) for r in rows[1:]]).reshape(3, 1, 2, 2).transpose(1, 0, 2, 3)
    assert not np.any(bits(got) != bits(live.values.values))
    score = [ln for ln in res.output.splitlines() if ln.startswith("score ")]
    assert len(score) == 3 * 2 and all("t2m: n=1 " in ln and "rmse=0" in ln for ln in score[0::2]) and all(ln.endswith("msl: n=0 ") for ln in score[1::2])
    assert res.output.splitlines()[-1] == str(out)


def test_refusals_come_before_the_device(pangu, monkeypatch):
    import skyrim_amd.datasource as ds
    monkeypatch.setattr(ds, "get_initial_condition_for_model", lambda *a, **k: pytest.fail("the device was reached"))
    import skyrim_amd.ensemble as E
    with pytest.raises(ValueError, match="tp06"):
        pangu.ensemble_forecast(T0, points=PLACES, point_channels=["t2m", "tp06"], n_steps=1, n_members=2)
    with pytest.raises(ValueError, match="tp06"):
        pangu.point_forecast(T0, 1, points=PLACES, channels=["tp06"])
    with pytest.raises(ValueError, match="ws10m"):
        pangu.point_forecast(T0, 1, points=PLACES, channels=["ws10m"])         # a derived field that derived= does not name
    half = pangu.model.grid.lat[:40]                                             # a source without its southern rows
    with pytest.raises(ValueError, match="'south pole'.*outside the source latitudes"):
        P.check_request(pangu.model.out_channel_names, half, pangu.model.grid.lon, 3, PLACES, ["t2m"])
    with pytest.raises(ValueError, match="twice"):
        pangu.ensemble_forecast(T0, points=[("a", 1, 2), ("a", 3, 4)], n_steps=1, n_members=2)
    with pytest.raises(ValueError, match="unknown method"):
        pangu.ensemble_forecast(T0, points=PLACES, point_method="cubic", n_steps=1, n_members=2)
    with pytest.raises(ValueError, match="points"):
        pangu.point_forecast(T0, 1)
    assert E.EnsembleForecast("m", 1, 0, 0.0).points is None
