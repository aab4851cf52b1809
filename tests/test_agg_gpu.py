"""Time-window aggregates end to end on the MI355X with the Pangu toy model (49 x 192): ``ensemble_forecast(aggregates=[...])`` against
the float32 restatement of include/skyrim_agg.h applied to the kept members over time (bit for bit), its statistics and scores against
the restatements of skyrim_ens.h and skyrim_score.h on the aggregated members, the window ends as time axis, ``aggregate_forecast``
against ``aggregate_prediction`` on the files of the same rollout, and the command line."""
from __future__ import annotations

import datetime

import numpy as np
import pytest

import _agg_reference as R
import _ens_reference as ER
import _score_reference as SR
from skyrim_amd import aggregate as A
from skyrim_amd import verify as V

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T0 = datetime.datetime(2024, 5, 13, 18, 0)
H6 = datetime.timedelta(hours=6)
AGGS = ["ws10m:max:12h", "t2m:mean:12h", "ws10m:hours_above@8:all", "msl:when_min:all"]
KW = dict(n_steps=5, n_members=3, keep_members=True, products=("mean", "spread"), perturb_scale=0.05)


@pytest.fixture(scope="module")
def pangu(toy):
    from skyrim_amd.core.models.pangu import PanguModel
    g, params, _ = toy
    return PanguModel(ic_source="gfs", geom=g, params=params)


@pytest.fixture(scope="module")
def plain(pangu):
    """The same ensemble without aggregates: computed once, shared, left unchanged.  Its control member is the truth."""
    return pangu.ensemble_forecast(T0, derived=["ws10m"], **KW)


def restate(raw, derived, names, requests, n_steps):
    """{label: (fields, (M, windows, fields, H, W))} of the restatement applied over time to members (M, T, C, H, W) and their derived
    planes (M, T, D, H, W); hidden slots are dropped."""
    plan = A.plan(names, requests, H6, n_steps)
    M, _, _, H, W = raw.shape
    acc = np.frombuffer(b"\xab" * (4 * M * plan.D * H * W), np.float32).reshape(M, plan.D, H, W).copy()
    out = {g.label: (g.fields, []) for g in plan.groups}
    for k in range(1, n_steps + 1):
        x = np.ascontiguousarray(np.concatenate([raw[:, k], derived[:, k]], axis=1))
        R.update(x, acc, plan.ops_at(k), 6.0 * k)
        for g, _ in plan.closing(k):
            out[g.label][1].append(acc[:, g.slots].copy())
    return {label: (fields, np.stack(wins, axis=1)) for label, (fields, wins) in out.items()}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_ensemble_aggregates_equal_the_restatement_on_the_members(pangu, plain):
    from skyrim_amd.labeled import DataArray
    lat, lon = np.asarray(pangu.model.grid.lat), np.asarray(pangu.model.grid.lon)
    names = plain.members.channel.values.tolist()
    times = list(plain.mean.time.values)
    truth = DataArray(np.asarray(plain.members.values)[0], ["time", "channel", "lat", "lon"], dict(time=times, channel=names, lat=lat, lon=lon))
    ens = pangu.ensemble_forecast(T0, derived=["ws10m"], aggregates=AGGS, scores=True, truth=truth, exceed={"ws10m_max_12h": [12.0]}, **KW)
    for p in ("mean", "spread", "members"):                                    # the raw and derived products: bit for bit what they were
        assert np.array_equal(getattr(plain, p).values, getattr(ens, p).values), p
        assert np.array_equal(getattr(plain.derived, p).values, getattr(ens.derived, p).values), p
    assert plain.aggregated == {} and list(ens.aggregated) == ["12h", "all"] and ens.exceedance == {} and ens.derived.exceedance == {}
    raw, dm = np.asarray(ens.members.values), np.asarray(ens.derived.members.values)
    want = restate(raw, dm, names + ["ws10m"], AGGS, 5)
    w = V.area_weights(lat)
    ends = {"12h": [T0 + 2 * H6, T0 + 4 * H6], "all": [T0 + 5 * H6]}
    starts = {"12h": [T0, T0 + 2 * H6], "all": [T0]}
    for label, a in ens.aggregated.items():
        fields, ref = want[label]
        assert a.label == label and a.fields == fields and a.members.dims == ("member", "time", "channel", "lat", "lon")
        assert a.fields == {"12h": ["ws10m_max_12h", "t2m_mean_12h"], "all": ["ws10m_hours_above@8_all", "msl_when_min_all"]}[label]
        got = np.asarray(a.members.values)
        assert got.shape == ref.shape and not np.any(bits(got) != bits(ref)), label          # bit for bit
        for da in (a.mean, a.spread, a.members):                                             # the window ends, and where each began
            assert [np.datetime64(t, "s") for t in da.time.values] == [np.datetime64(t, "s") for t in ends[label]]
            assert [np.datetime64(t, "s") for t in da._coords["window_start"]] == [np.datetime64(t, "s") for t in starts[label]]
        assert a.mean.channel.values.tolist() == fields and a.min is None
        for t in range(got.shape[1]):
            x = got[:, t].reshape(3, -1)
            r = ER.stats(x)
            em = np.abs(a.mean.values[t].reshape(-1).astype(np.float64) - r["mean"]) / np.maximum(ER.mean_bound(x, r["mean"]), 1e-300)
            es = np.abs(a.spread.values[t].reshape(-1).astype(np.float64) - r["spread"]) / np.maximum(ER.spread_bound(x, r["spread"]), 1e-300)
            print(f"aggregated {label} window {t}: mean {em.max():.3f} of its bound, spread {es.max():.3f} of its bound")
            assert em.max() <= 1 and es.max() <= 1
        # the scores: the aggregated truth is the aggregated control member (the truth is the control run)
        s = a.scores
        assert s.channels == fields and s.n_members == 3 and a.dropped == {}
        assert [np.datetime64(t, "s") for t in s.times] == [np.datetime64(t, "s") for t in ends[label]]
        slots = s.sums.slot.values.tolist()
        worst = 0.0
        for t in range(got.shape[1]):
            val, bound, counts = SR.scores(got[:, t], got[0, t], w)
            for k, name in enumerate(slots):
                err = np.abs(s.sums.values[k, t] - val[name])
                worst = max(worst, float(np.where(bound[name] > 0, err / np.where(bound[name] > 0, bound[name], 1), np.where(err == 0, 0, np.inf)).max()))
            assert np.array_equal(s.rank_counts.values[t], counts.sum(axis=1))
            table = SR.table({n: s.sums.values[k, t] for k, n in enumerate(slots)}, 3)
            for name in ("crps", "rmse"):
                assert np.array_equal(s.metric(name)[t], table[name], equal_nan=True), name
        print(f"aggregated {label} scores: worst share of the bound {worst:.3f}")
        assert worst <= 1
    a = ens.aggregated["12h"]
    assert a.incomplete == (5, 5) and ens.aggregated["all"].incomplete is None                # step 5 opens a 12-h window that stays open
    assert set(a.exceedance) == {"ws10m_max_12h"} and ens.aggregated["all"].exceedance == {}
    for t in range(2):
        r = ER.stats(np.asarray(a.members.values)[:, t, 0].reshape(3, -1), thresholds=[12.0])
        assert np.array_equal(a.exceedance["ws10m_max_12h"].values[t].reshape(1, -1), r["exceed"])
    # what the aggregates mean: a maximum is at least every step's value, the hours lie in [0, 30], the time of the minimum is a lead time
    assert np.all(np.asarray(a.members.values)[:, 0, 0] >= dm[:, 1, 0]) and np.all(np.asarray(a.members.values)[:, 0, 0] >= dm[:, 2, 0])
    hrs, when = (np.asarray(ens.aggregated["all"].members.values)[:, 0, k] for k in (0, 1))
    assert set(np.unique(hrs)) <= {0.0, 6.0, 12.0, 18.0, 24.0, 30.0} and set(np.unique(when)) <= {6.0, 12.0, 18.0, 24.0, 30.0}


def test_aggregate_forecast_equals_aggregate_prediction_on_saved_files(pangu, tmp_path):
    aggs = AGGS + ["t2m:min:12h", "ws10m:when_max:12h", "msl:sum:6h"]
    live = pangu.aggregate_forecast(T0, 5, aggs, derived=["ws10m"])
    assert list(live) == ["12h", "all", "6h"]
    assert live["12h"].channel.values.tolist() == ["ws10m_max_12h", "t2m_mean_12h", "t2m_min_12h", "ws10m_when_max_12h"]
    assert live["12h"].shape[:2] == (2, 4) and live["all"].shape[:2] == (1, 2) and live["6h"].shape[:2] == (5, 1)
    assert live["12h"].incomplete == {"12h": (5, 5)} and all(np.isfinite(da.values).all() for da in live.values())
    _, paths = pangu.rollout(T0, n_steps=5, save=True, save_config={"output_dir": str(tmp_path)})
    disk = A.aggregate_prediction(list(paths), aggs, derived=["ws10m"], device=DEV)
    for label, da in live.items():
        assert [np.datetime64(t, "s") for t in disk[label].time.values] == [np.datetime64(t, "s") for t in da.time.values]
        assert not np.any(bits(disk[label].values) != bits(da.values)), label
    # the one forecast is the unperturbed control: its sum over one step is the step
    from skyrim_amd.core import Skyrim
    s = object.__new__(Skyrim)
    s.model = pangu
    again = s.aggregate_forecast(T0, 5, aggs, derived=["ws10m"])
    assert all(np.array_equal(again[k].values, live[k].values) for k in live)


def test_command_line_writes_the_same_arrays(pangu, tmp_path, monkeypatch):
    from click.testing import CliRunner
    import skyrim_amd.core as core
    from skyrim_amd.aggregate_cli import aggregate
    from skyrim_amd.labeled import open_dataarray
    s = object.__new__(core.Skyrim)
    s.model = pangu
    monkeypatch.setattr(core, "Skyrim", lambda name, ic_source=None: s)          # the command line on the toy model
    res = CliRunner().invoke(aggregate, ["-m", "pangu", "-l", "24", "-o", str(tmp_path), "-d", "20240513", "-t", "1800", "--derived", "ws10m",
                                         "--aggregate", "ws10m:max:12h", "--aggregate", "t2m:mean:12h", "--aggregate", "msl:when_min:all"])
    assert res.exit_code == 0, res.output + repr(res.exception)
    live = pangu.aggregate_forecast(T0, 4, ["ws10m:max:12h", "t2m:mean:12h", "msl:when_min:all"], derived=["ws10m"])
    files = [ln for ln in res.output.splitlines() if ln.endswith(".nc")]
    assert len(files) == 2 and sum(ln.startswith("(") for ln in res.output.splitlines()) == 2 * 2 + 1
    for path, label in zip(files, ("12h", "all")):
        assert f"-agg{label}__" in path
        da = open_dataarray(path)
        assert da.channel.values.tolist() == live[label].channel.values.tolist()
        assert np.array_equal(np.asarray(da.values, np.float32), live[label].values), label
