"""Neighbourhood fields end to end on the MI355X with the Pangu toy model (49 x 192): ``ensemble_forecast(neighbourhood=[...])`` against
the restatement of include/skyrim_nbr.h applied to the kept members, its statistics, scores and points against the restatements of
skyrim_ens.h and skyrim_score.h and ``LeadPoints`` on the restated members, ``neighbourhood_forecast`` against
``neighbourhood_prediction`` on the files of the same rollout, a request without ``neighbourhood=``, and the replay of an archive."""
from __future__ import annotations

import datetime

import numpy as np
import pytest

import _ens_reference as ER
import _nbr_reference as R
import _score_reference as SR
from skyrim_amd import neighbourhood as N
from skyrim_amd import verify as V

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T0 = datetime.datetime(2024, 5, 13, 18, 0)
H6 = datetime.timedelta(hours=6)
NBRS = ["ws10m:max:500km", "t2m:frac_above@285:1200km", "t2m:min:500km", "msl:mean:1200km"]
FIELDS = ["ws10m_max_500km", "t2m_frac_above@285_1200km", "t2m_min_500km", "msl_mean_1200km"]
KW = dict(n_steps=2, n_members=3, keep_members=True, products=("mean", "spread"), perturb_scale=0.05)
POINTS = {"node": (45.0, 30.0), "Istanbul": (41.01, 28.98)}


@pytest.fixture(scope="module")
def pangu(toy):
    from skyrim_amd.core.models.pangu import PanguModel
    g, params, _ = toy
    return PanguModel(ic_source="gfs", geom=g, params=params)


@pytest.fixture(scope="module")
def plain(pangu):
    """The same ensemble without neighbourhood fields: computed once, shared, left unchanged.  Its control member is the truth."""
    return pangu.ensemble_forecast(T0, derived=["ws10m"], **KW)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def restate(x, plan):
    """(M, T, D, H, W) exact fields and, for the MEAN slots, the exact mean and its bound, from members x (M, T, C, H, W)."""
    M, T, _, H, W = x.shape
    tables = list(zip(plan.reach, plan.half))
    out = np.zeros((M, T, plan.D, H, W), np.float32)
    means = {}
    for t in range(T):
        out[:, t] = R.fields(np.ascontiguousarray(x[:, t]), plan.ops, tables, out[:, t])
        for op in plan.ops:
            if op.kind == N.MEAN:
                for m in range(M):
                    means[(m, t, op.out)] = R.mean_exact(x[m, t, op.channel], *tables[op.radius], plan.weights)
    return out, means


def test_ensemble_fields_equal_the_restatement_on_the_members(pangu, plain):
    import torch
    from skyrim_amd import points as pointing
    from skyrim_amd.ensemble import member_table
    from skyrim_amd.labeled import DataArray
    lat, lon = np.asarray(pangu.model.grid.lat), np.asarray(pangu.model.grid.lon)
    names = plain.members.channel.values.tolist()
    times = list(plain.mean.time.values)
    truth = DataArray(np.asarray(plain.members.values)[0], ["time", "channel", "lat", "lon"], dict(time=times, channel=names, lat=lat, lon=lon))
    ens = pangu.ensemble_forecast(T0, derived=["ws10m"], neighbourhood=NBRS, scores=True, truth=truth, exceed={"ws10m_max_500km": [8.0, 12.0]},
                                  quantiles={"t2m_min_500km": [0.5]}, points=POINTS, **KW)
    for p in ("mean", "spread", "members"):                                    # the raw and derived products: bit for bit what they were
        assert np.array_equal(getattr(plain, p).values, getattr(ens, p).values), p
        assert np.array_equal(getattr(plain.derived, p).values, getattr(ens.derived, p).values), p
    assert plain.neighbourhood is None and ens.exceedance == {} and ens.derived.exceedance == {}
    nb = ens.neighbourhood
    assert nb.fields == FIELDS and nb.members.dims == ("member", "time", "channel", "lat", "lon") and nb.dropped == {}
    assert nb.mean.channel.values.tolist() == FIELDS and nb.min is None and list(nb.mean.time.values) == times
    x = np.concatenate([np.asarray(ens.members.values), np.asarray(ens.derived.members.values)], axis=2)
    plan = N.check_request(names, NBRS, lat, lon, 3, ["ws10m"])
    want, means = restate(x, plan)
    got = np.asarray(nb.members.values)
    exact = [k for k, op in enumerate(plan.ops) if op.kind != N.MEAN]
    assert got.shape == want.shape and not np.any(bits(got[:, :, exact]) != bits(want[:, :, exact]))      # bit for bit
    worst = 0.0
    for (m, t, slot), (ex, bound) in means.items():
        worst = max(worst, float((np.abs(got[m, t, slot].astype(np.float64) - ex) / bound).max()))
    print(f"neighbourhood mean on the toy forecast: largest error / bound = {worst:.3f}")
    assert worst <= 1
    # the statistics are ens_stats over the fields' members
    for t in range(got.shape[1]):
        xs = got[:, t].reshape(3, -1)
        r = ER.stats(xs)
        em = np.abs(nb.mean.values[t].reshape(-1).astype(np.float64) - r["mean"]) / np.maximum(ER.mean_bound(xs, r["mean"]), 1e-300)
        es = np.abs(nb.spread.values[t].reshape(-1).astype(np.float64) - r["spread"]) / np.maximum(ER.spread_bound(xs, r["spread"]), 1e-300)
        assert em.max() <= 1 and es.max() <= 1
        r = ER.stats(got[:, t, 0].reshape(3, -1), thresholds=[8.0, 12.0])
        assert np.array_equal(nb.exceedance["ws10m_max_500km"].values[t].reshape(2, -1), r["exceed"])
    assert set(nb.exceedance) == {"ws10m_max_500km"} and set(nb.quantile) == {"t2m_min_500km"}
    assert nb.quantile["t2m_min_500km"].shape == (3, 1, 49, 192)
    # the point-wise exceedance is never above the neighbourhood's: the maximum within 500 km is at least the value at the node
    ws = np.asarray(ens.derived.members.values)[:, :, 0]
    assert np.all(got[:, :, 0] >= ws) and np.all((got[:, :, 1] >= 0) & (got[:, :, 1] <= 1))
    # the scores: the truth's fields are the control member's fields (the truth is the control run)
    s, w = nb.scores, V.area_weights(lat)
    assert s.channels == FIELDS and s.n_members == 3
    slots = s.sums.slot.values.tolist()
    worst = 0.0
    for t in range(got.shape[1]):
        val, bound, counts = SR.scores(got[:, t], got[0, t], w)
        for k, name in enumerate(slots):
            err = np.abs(s.sums.values[k, t] - val[name])
            worst = max(worst, float(np.where(bound[name] > 0, err / np.where(bound[name] > 0, bound[name], 1), np.where(err == 0, 0, np.inf)).max()))
        assert np.array_equal(s.rank_counts.values[t], counts.sum(axis=1))
    print(f"neighbourhood scores: worst share of the bound {worst:.3f}")
    assert worst <= 1
    # the points: LeadPoints on the same planes
    lp = pointing.LeadPoints(FIELDS, lat, lon, 3, POINTS, None, "bilinear", DEV, (), got.shape[1])
    for t in range(got.shape[1]):
        st = [torch.from_numpy(np.ascontiguousarray(got[m, t])).to(DEV) for m in range(3)]
        lp.add(times[t], st, member_table(st))
    assert np.array_equal(bits(np.asarray(nb.points.values.values)), bits(np.asarray(lp.result().values.values)))


def test_neighbourhood_forecast_equals_neighbourhood_prediction_on_saved_files(pangu, tmp_path):
    live = pangu.neighbourhood_forecast(T0, 2, NBRS, derived=["ws10m"])
    assert live.channel.values.tolist() == FIELDS and live.shape == (3, 4, 49, 192) and np.isfinite(live.values).all()
    _, paths = pangu.rollout(T0, n_steps=2, save=True, save_config={"output_dir": str(tmp_path)})
    disk = N.neighbourhood_prediction(list(paths), NBRS, derived=["ws10m"], device=DEV)
    assert [np.datetime64(t, "s") for t in disk.time.values] == [np.datetime64(t, "s") for t in live.time.values]
    assert not np.any(bits(disk.values) != bits(live.values))
    from skyrim_amd.core import Skyrim
    s = object.__new__(Skyrim)
    s.model = pangu
    assert np.array_equal(s.neighbourhood_forecast(T0, 2, NBRS, derived=["ws10m"]).values, live.values)
    # the one forecast is the unperturbed control of an ensemble
    ens = pangu.ensemble_forecast(T0, derived=["ws10m"], neighbourhood=NBRS, **KW)
    assert not np.any(bits(np.asarray(ens.neighbourhood.members.values)[0]) != bits(live.values))


def test_a_request_without_neighbourhood_launches_what_it_launched(pangu, monkeypatch):
    import json
    from test_ens_gpu import LAUNCH_GOLDEN, LAUNCH_REQUESTS, launch_sequence
    assert launch_sequence(monkeypatch, pangu, **LAUNCH_REQUESTS["A"]) == json.loads(LAUNCH_GOLDEN.read_text())["A"]
    with_it = launch_sequence(monkeypatch, pangu, **dict(LAUNCH_REQUESTS["A"], neighbourhood=["t2m:max:500km", "ws10m:max:500km"]))
    # scored, so at every one of the five leads: the ops on the states, those on the deriver's buffer, and the truth's fields (M = 1)
    assert with_it.count("sknbr_run") == 3 * 5 and "sknbr_run" not in json.loads(LAUNCH_GOLDEN.read_text())["A"]
    assert with_it.index("sknbr_run") > with_it.index("skderive_run")                                       # after the deriver's stage


def test_replay_of_an_archive_equals_the_live_run(pangu, tmp_path):
    kw = dict(products=("mean", "spread"), keep_members=True, derived=["ws10m"], neighbourhood=NBRS, exceed={"ws10m_max_500km": [8.0]})
    live = pangu.ensemble_forecast(T0, n_steps=2, n_members=3, perturb_scale=0.05, archive=dict(packing="float32", dir=str(tmp_path)), **kw)
    rep = live.archive.replay(**kw)
    for p in ("mean", "spread", "members"):
        assert not np.any(bits(getattr(rep.neighbourhood, p).values) != bits(getattr(live.neighbourhood, p).values)), p
    assert np.array_equal(rep.neighbourhood.exceedance["ws10m_max_500km"].values, live.neighbourhood.exceedance["ws10m_max_500km"].values)
