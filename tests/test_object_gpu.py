"""Weather objects end to end on the MI355X with the Pangu toy model (49 x 192): ``ensemble_forecast(objects=...)`` against the numpy
restatement on the kept members, the probability planes against the exceedance fractions, the truth's objects, ``object_forecast``
against ``objects_prediction`` on the files of the same rollout, the JSON file and the command line."""
from __future__ import annotations

import datetime
import json

import numpy as np
import pytest

import _object_reference as R
from skyrim_amd import objects as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T0 = datetime.datetime(2024, 5, 13, 18, 0)
M = 4
KW = dict(n_steps=2, n_members=M, keep_members=True, products=("mean", "spread"), perturb_scale=0.05, derived=["ws10m"])


@pytest.fixture(scope="module")
def pangu(toy):
    from skyrim_amd.core.models.pangu import PanguModel
    g, params, _ = toy
    return PanguModel(ic_source="gfs", geom=g, params=params)


@pytest.fixture(scope="module")
def plain(pangu):
    """The ensemble without objects, with its members kept: where the thresholds come from and what ``objects=`` must not change."""
    return pangu.ensemble_forecast(T0, **KW)


def off_the_values(values, q, lowest):
    """A threshold that every lead time has objects beyond -- the lowest (``lowest``) or highest over the lead times of the q-quantile of
    ``values`` (member, time, lat, lon) -- moved between two neighbouring values, so that none equals it (>= and > then select the
    same points); exact in fp32."""
    per_lead = [float(np.quantile(values[:, t], q)) for t in range(values.shape[1])]
    v = np.unique(np.asarray(values, np.float32))
    k = int(np.searchsorted(v, min(per_lead) if lowest else max(per_lead)))
    k = min(max(k, 1), v.size - 1)
    while k < v.size - 1 and np.float32((np.float64(v[k - 1]) + np.float64(v[k])) / 2) in (v[k - 1], v[k]):
        k += 1                                                  # neighbours in fp32: move on to a pair with room between them
    thr = np.float32((np.float64(v[k - 1]) + np.float64(v[k])) / 2)
    assert not np.any(v == thr)
    return float(thr)


@pytest.fixture(scope="module")
def request_(plain):
    names = plain.members.channel.values.tolist()
    ws = np.asarray(plain.derived.members.values)[:, :, 0]
    msl = np.asarray(plain.members.values)[:, :, names.index("msl")]
    return {"ws10m": {"above": [off_the_values(ws, 0.9, True)]}, "msl": {"below": [off_the_values(msl, 0.08, False)], "min_area_km2": 1e5},
            "connectivity": 8, "min_pixels": 1, "capacity": 2048}


@pytest.fixture(scope="module")
def ens(pangu, request_):
    thr, thr2 = request_["ws10m"]["above"][0], request_["msl"]["below"][0]
    return pangu.ensemble_forecast(T0, objects=request_, scores=True, exceed={"ws10m": [thr], "msl": [thr2]}, **KW)


def test_objects_equal_the_restatement_on_the_members(pangu, plain, ens, request_):
    obj = ens.objects
    assert plain.objects is None and isinstance(obj, O.Objects) and obj.n_members == M and len(obj.times) == 3
    for p in ("mean", "spread", "members"):
        assert np.array_equal(getattr(plain, p).values, getattr(ens, p).values)
    assert obj.planes == [f"ws10m>={request_['ws10m']['above'][0]:g}", f"msl<={request_['msl']['below'][0]:g}"]
    names = ens.members.channel.values.tolist()
    lat, lon = np.asarray(pangu.model.grid.lat, np.float64), np.asarray(pangu.model.grid.lon, np.float64)
    g = O.tables(lat, lon)
    assert g.periodic
    raw, der = np.asarray(ens.members.values), np.asarray(ens.derived.members.values)
    found = 0
    for t in range(3):
        ids_all = np.zeros((M, 2) + g.row.shape[1:] + g.col.shape[1:], np.int32)
        keep = np.zeros((M, 2, obj.request.capacity + 1), np.uint8)
        for m in range(M):
            for p, plane in enumerate(obj.request.planes):
                v = der[m, t, 0] if plane.name == "ws10m" else raw[m, t, names.index("msl")]
                labels = R.flood_labels(R.mask_of(v, plane.threshold, plane.direction), 8, True)
                ids, n, _ = R.number(labels, obj.request.min_pixels, obj.request.capacity)
                rec = R.records(v, ids, g.row, g.col, plane.direction, plane.value_scale, m, 0)
                want = O.properties(rec, lat, lon, plane.value_scale)
                want["keep"] = O.keep_mask(want, plane)
                got = obj.objects[t][m][p]
                assert obj.n_found[t, m, p] == n == len(got) >= 1
                for k in O.PROPS.names:
                    np.testing.assert_array_equal(got[k], want[k], err_msg=f"lead {t} member {m} plane {plane.label} {k}")
                ref = R.host_properties(rec, lat, lon, plane.value_scale)
                for k in ("area_km2", "lat", "lon", "mean"):
                    np.testing.assert_allclose(got[k], ref[k], rtol=1e-12, atol=1e-9)
                ids_all[m, p], keep[m, p, 1:n + 1] = ids, want["keep"]
                found += n
        counts = R.probability_counts(ids_all, keep)
        for p in range(2):
            np.testing.assert_array_equal(obj.counts[t][p], counts[p])
    assert not obj.truncated.any() and found >= 3 * M * 2


def test_probability_is_a_count_below_the_exceedance_fraction(ens, request_):
    obj = ens.objects
    for p, (ch, above) in enumerate((("ws10m", True), ("msl", False))):
        prob = np.asarray(obj.probability(p).values)
        assert prob.shape == (3, 49, 192) and np.array_equal(prob * M, np.rint(prob * M)) and prob.max() > 0
        ex = np.asarray((ens.derived if above else ens).exceedance[ch].values)[:, 0]      # the fraction of members strictly above
        beyond = ex if above else 1.0 - ex
        assert np.all(prob * M <= np.rint(beyond * M))          # an object's points are beyond the threshold; small ones were dropped
    assert np.array_equal(np.asarray(obj.probability(obj.planes[0]).values), np.asarray(obj.probability(0).values))
    assert obj.count(0).shape == (3, M) and obj.count(0).min() >= 1


def test_truth_objects_come_from_the_same_kernels(ens):
    rows = ens.objects.verify(max_km=1000.0)
    assert len(rows) == 3 * 2 and {r["plane"] for r in rows} == set(ens.objects.planes)
    for r in rows:
        assert r["n_truth"] >= 1 and 0.0 <= r["hit_rate"] <= 1.0 and 0.0 <= r["probability"] <= 1.0
    first = [r for r in rows if r["time"] == ens.objects.times[0]]
    # at the initial time member 0 is the unperturbed analysis: it holds every object of the truth where the truth has it
    assert all(r["hit_rate"] >= 1.0 / M and r["probability"] >= 1.0 / M for r in first)


def test_a_forecast_verified_against_itself(pangu, request_):
    da = pangu.forecast(T0, n_steps=2)
    obj = O.objects_prediction(da, request_, derived=["ws10m"], truth=da, device=DEV, model_name="pangu")
    rows = obj.verify()
    assert len(rows) == 3 * 2
    for r in rows:
        assert r["hit_rate"] == 1.0 and r["centroid_error_km"] == 0.0 and r["false_alarm_ratio"] == 0.0 and r["area_ratio"] == 1.0
        assert r["probability"] == 1.0 and r["n_truth"] == r["n_forecast"] >= 1


def test_object_forecast_equals_objects_prediction_on_saved_files(pangu, request_, tmp_path):
    cfg = {"output_dir": str(tmp_path)}
    live = pangu.object_forecast(T0, n_steps=2, objects=request_, derived=["ws10m"], save=True, save_config=cfg)
    assert live.n_members == 1 and len(live.times) == 3 and live.path.endswith("pangu-objects.json") and live.truth is None
    back = O.Objects.load(live.path)
    assert back.to_json() == live.to_json()                     # the JSON round trip
    for t in range(3):
        for p in range(2):
            np.testing.assert_array_equal(back.counts[t][p], live.counts[t][p])
    _, paths = pangu.rollout(T0, n_steps=2, save=True, save_config={"output_dir": str(tmp_path / "files")})
    disk = O.objects_prediction(list(paths), request_, derived=["ws10m"], device=DEV)
    assert [np.datetime64(t, "s") for t in disk.times] == [np.datetime64(t, "s") for t in live.times]
    np.testing.assert_array_equal(disk.n_found, live.n_found)
    for t in range(3):
        for p in range(2):
            np.testing.assert_array_equal(disk.counts[t][p], live.counts[t][p])
            a, b = disk.objects[t][0][p], live.objects[t][0][p]
            for k in ("n_pixels", "area_km2", "lat", "lon", "keep"):
                np.testing.assert_array_equal(a[k], b[k])
            np.testing.assert_allclose(a["mean"], b["mean"], rtol=1e-4)


def test_command_line_writes_the_same_file(pangu, request_, tmp_path, monkeypatch):
    from click.testing import CliRunner
    import skyrim_amd.core as core
    from skyrim_amd.object_cli import objects as command
    s = object.__new__(core.Skyrim)
    s.model = pangu
    monkeypatch.setattr(core, "Skyrim", lambda name, ic_source=None: s)          # the command line on the toy model
    live = pangu.object_forecast(T0, n_steps=2, objects=request_, derived=["ws10m"])
    res = CliRunner().invoke(command, ["-m", "pangu", "-d", "20240513", "-t", "1800", "-l", "12", "-o", str(tmp_path), "--derived", "ws10m",
                                       "--object", f"ws10m:above:{request_['ws10m']['above'][0]!r}",
                                       "--object", f"msl:below:{request_['msl']['below'][0]!r}", "--min_pixels", "1", "--capacity", "2048"])
    assert res.exit_code == 0, res.output + repr(res.exception)
    path = res.output.splitlines()[-1]
    assert path.endswith("pangu-objects.json") and path.startswith(str(tmp_path))
    # the command line's filters apply to every channel: here none, so only the msl plane's min_area_km2 differs
    want = json.loads(live.to_json())
    got = json.loads(open(path).read())
    assert got["n_found"] == want["n_found"] and got["times"] == want["times"]
    for t in range(3):
        assert got["objects"][t][0][0] == want["objects"][t][0][0]                 # the ws10m plane: the same request, the same file
        for k in O.PROPS.names:
            if k != "keep":
                assert got["objects"][t][0][1][k] == want["objects"][t][0][1][k]
    assert any(ln.startswith("+12h msl<=") for ln in res.output.splitlines())


def test_refusals_come_before_the_device(pangu):
    with pytest.raises(ValueError, match="neither output channels"):
        pangu.object_forecast(T0, n_steps=1, objects={"ivt": {"above": [250.0]}})
    with pytest.raises(ValueError, match="9 planes"):
        pangu.ensemble_forecast(T0, n_steps=1, n_members=2, objects={"msl": {"above": list(range(9))}})
