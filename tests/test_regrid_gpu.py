"""Regridding end to end on the MI355X with the Pangu toy model (49 x 192 -> 13 x 48): ``ensemble_forecast(grid=...)`` against the float64
restatements on the kept members with the raw products unchanged, the scores on the target grid, ``verify(grid=...)`` against
``score_prediction`` of ``regrid_forecast``, ``regrid_forecast`` against ``regrid_prediction`` on the files of the same rollout, and a
``GlobalEnsemble`` over members on different latitude axes."""
from __future__ import annotations

import datetime

import numpy as np
import pytest

import _ens_reference as ER
import _regrid_reference as R
import _score_reference as SR
from skyrim_amd import regrid as G
from skyrim_amd import verify as V

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T0 = datetime.datetime(2024, 5, 13, 18, 0)
TARGET = (np.linspace(90.0, -90.0, 13), np.arange(48) * 7.5)
KW = dict(n_steps=2, n_members=3, keep_members=True, products=("mean", "spread"), perturb_scale=0.05)


@pytest.fixture(scope="module")
def pangu(toy):
    from skyrim_amd.core.models.pangu import PanguModel
    g, params, _ = toy
    return PanguModel(ic_source="gfs", geom=g, params=params)


@pytest.fixture(scope="module")
def plain(pangu):
    """The same ensemble without a grid: computed once, shared, left unchanged."""
    return pangu.ensemble_forecast(T0, **KW)


@pytest.fixture(scope="module")
def tabs(pangu):
    t = G.tables(pangu.model.grid.lat, pangu.model.grid.lon, *TARGET, "conservative")
    return (t.rows.start, t.rows.count, t.rows.weight), (t.cols.start, t.cols.count, t.cols.weight)


def _thresholds(values, rel=1e-4):
    """Two thresholds (fp32) among the values such that no value lies within ``rel`` relative of either; the margin is asserted."""
    flat = np.sort(np.asarray(values, np.float64).reshape(-1))
    picks = []
    for lo, hi in ((0.80, 0.90), (0.90, 0.99)):                # the widest gap of each range
        a, b = int(lo * flat.size), int(hi * flat.size)
        j = a + int(np.argmax(np.diff(flat[a:b + 1])))
        picks.append(float(np.float32((flat[j] + flat[j + 1]) / 2)))
    margin = min(float(np.abs(flat - t).min()) / abs(t) for t in picks)
    assert margin > rel, f"a member value lies within {margin:.2e} (relative) of a threshold"
    return picks


def test_ensemble_products_on_the_target_grid(pangu, plain, tabs):
    probe = pangu.ensemble_forecast(T0, grid=TARGET, **KW)                      # the regridded members, to choose thresholds from
    names = plain.members.channel.values.tolist()
    k2 = names.index("t2m")
    thr = _thresholds(probe.regridded.members.values[:, :, k2])
    ens = pangu.ensemble_forecast(T0, grid=TARGET, exceed={"t2m": thr}, quantiles={"t2m": [0.5]}, **KW)
    assert plain.regridded is None
    for p in ("mean", "spread", "members"):                                    # the raw products: bit for bit what they were
        assert np.array_equal(getattr(plain, p).values, getattr(ens, p).values), p
    r = ens.regridded
    assert r.method == "conservative" and np.array_equal(r.lat, TARGET[0]) and np.array_equal(r.lon, TARGET[1])
    assert r.members.dims == ("member", "time", "channel", "lat", "lon") and r.members.shape == (3, 3, len(names), 13, 48)
    assert r.mean.shape == (3, len(names), 13, 48) and r.min is None and r.scores is None and set(r.exceedance) == {"t2m"}
    assert np.array_equal(probe.regridded.members.values, r.members.values)
    raw, rm = np.asarray(ens.members.values), np.asarray(r.members.values)
    worst = 0.0
    for m in range(3):
        for t in range(3):
            for k in range(len(names)):
                exact, bound = R.apply(raw[m, t, k], *tabs)
                worst = max(worst, float((np.abs(rm[m, t, k].astype(np.float64) - exact) / bound).max()))
    print(f"regridded members: worst share of the bound {worst:.3f}")
    assert worst <= 1
    # the statistics of the regridded members: the restatement of skyrim_ens.h under the tolerances of tests/test_ens_gpu.py
    fractions = []
    for t in range(3):
        x = rm[:, t].reshape(3, -1)
        ref = ER.stats(x)
        em = np.abs(r.mean.values[t].reshape(-1).astype(np.float64) - ref["mean"]) / np.maximum(ER.mean_bound(x, ref["mean"]), 1e-300)
        es = np.abs(r.spread.values[t].reshape(-1).astype(np.float64) - ref["spread"]) / np.maximum(ER.spread_bound(x, ref["spread"]), 1e-300)
        print(f"regridded lead {t}: mean {em.max():.3f} of its bound, spread {es.max():.3f} of its bound")
        assert em.max() <= 1 and es.max() <= 1
        e = ER.stats(rm[:, t, k2].reshape(3, -1), thresholds=thr)
        assert np.array_equal(r.exceedance["t2m"].values[t].reshape(2, -1), e["exceed"])
        fractions.append(float(e["exceed"].mean()))
        (q, big), = ER.stats(rm[:, t, k2].reshape(3, -1), levels=[0.5])["quant"]
        assert np.all(np.abs(r.quantile["t2m"].values[t, 0].reshape(-1).astype(np.float64) - q) <= 2 * np.spacing(big.astype(np.float32)))
    assert 0 < max(fractions) < 1                                               # the thresholds cut through the members' values
    only = pangu.ensemble_forecast(T0, grid=TARGET, **dict(KW, keep_members="regridded"))
    assert only.members is None and np.array_equal(only.regridded.members.values, rm)


def test_scores_on_the_target_grid(pangu, plain, tabs):
    from skyrim_amd.labeled import DataArray
    lat, lon = np.asarray(pangu.model.grid.lat), np.asarray(pangu.model.grid.lon)
    names = plain.members.channel.values.tolist()
    control = np.asarray(plain.members.values)[0]                               # (T, C, H, W): the truth is the control member
    times = list(plain.mean.time.values)
    truth = DataArray(control, ["time", "channel", "lat", "lon"], dict(time=times, channel=names, lat=lat, lon=lon))
    ens = pangu.ensemble_forecast(T0, grid=TARGET, scores=True, truth=truth, **KW)
    assert np.array_equal(plain.members.values, ens.members.values)
    rs = ens.regridded.scores
    assert rs.channels == names and rs.n_members == 3 and ens.scores.channels == names and rs.grid == "13x48" and ens.scores.grid == ""
    assert '"grid": "13x48"' in rs.to_json() and '"grid"' not in ens.scores.to_json() and V.Scores.from_json(rs.to_json()).grid == "13x48"
    rm = np.asarray(ens.regridded.members.values)
    w = V.area_weights(TARGET[0])
    slots = rs.sums.slot.values.tolist()
    worst = 0.0
    for t in range(3):
        val, bound, counts = SR.scores(rm[:, t], rm[0, t], w)                  # the regridded truth is the regridded control member
        for k, name in enumerate(slots):
            err = np.abs(rs.sums.values[k, t] - val[name])
            worst = max(worst, float(np.where(bound[name] > 0, err / np.where(bound[name] > 0, bound[name], 1), np.where(err == 0, 0, np.inf)).max()))
        assert np.array_equal(rs.rank_counts.values[t], counts.sum(axis=1))
        ref = SR.table({n: rs.sums.values[k, t] for k, n in enumerate(slots)}, 3)
        for name in ("crps", "rmse"):
            assert np.array_equal(rs.metric(name)[t], ref[name], equal_nan=True), name
    print(f"regridded scores: worst share of the bound {worst:.3f}")
    assert worst <= 1 and float(rs.metric("rmse")[1:].min()) > 0


def test_verify_on_a_grid_agrees_with_scoring_the_regridded_forecast(pangu, plain):
    from skyrim_amd.labeled import DataArray
    lat, lon = np.asarray(pangu.model.grid.lat), np.asarray(pangu.model.grid.lon)
    names = plain.members.channel.values.tolist()
    times = list(plain.mean.time.values)
    member = np.asarray(plain.members.values)[1]                                # a perturbed member as the truth: the errors are not zero
    truth = DataArray(member, ["time", "channel", "lat", "lon"], dict(time=times, channel=names, lat=lat, lon=lon))
    scores = pangu.verify(T0, n_steps=2, truth=truth, grid=TARGET)
    assert scores.grid == "13x48" and scores.channels == names
    fc = pangu.regrid_forecast(T0, 2, TARGET, "conservative")
    assert fc.shape == (3, len(names), 13, 48) and np.array_equal(fc._coords["lat"], TARGET[0])
    rtruth = G.regrid_prediction(truth, TARGET, "conservative", device=DEV)
    ref = V.score_prediction(fc, rtruth, device=DEV)
    assert np.array_equal(scores.sums.values, ref.sums.values) and np.array_equal(scores.table.values, ref.table.values, equal_nan=True)
    assert float(scores.metric("rmse")[1:].min()) > 0
    native = pangu.verify(T0, n_steps=2, truth=truth)                           # without a grid: what it was, and no label
    assert native.grid == "" and native.sums.values.shape == scores.sums.values.shape and not np.array_equal(native.sums.values, scores.sums.values)


def test_regrid_forecast_equals_regrid_prediction_on_saved_files(pangu, tmp_path):
    spec = dict(region=(-15.0, 15.0, 341.0, 18.0))
    for grid, method in ((TARGET, "conservative"), (spec, "nearest"), ("7.5deg", "bilinear")):
        live = pangu.regrid_forecast(T0, 2, grid, method)
        assert live.dims == ("time", "channel", "lat", "lon") and np.isfinite(live.values).all()
        if method == "conservative":
            _, paths = pangu.rollout(T0, n_steps=2, save=True, save_config={"output_dir": str(tmp_path)})
        disk = G.regrid_prediction(list(paths), grid, method, device=DEV)
        assert [np.datetime64(t, "s") for t in disk.time.values] == [np.datetime64(t, "s") for t in live.time.values]
        assert np.array_equal(disk.values.view(np.uint32), live.values.view(np.uint32)), method
    assert live.shape[2:] == (25, 48)
    from skyrim_amd.core import Skyrim
    s = object.__new__(Skyrim)
    s.model = pangu
    assert np.array_equal(s.regrid_forecast(T0, 2, "7.5deg", "bilinear").values, live.values)
    sub = pangu.regrid_forecast(T0, 1, TARGET, channels=["t2m", "z500"])
    assert sub.channel.values.tolist() == ["t2m", "z500"] and sub.shape == (2, 2, 13, 48)


def test_global_ensemble_averages_members_on_different_latitude_axes(pangu):
    from skyrim_amd.core.models.ensemble import GlobalEnsemble
    a = pangu.forecast(T0, n_steps=1)
    b = a.isel(lat=slice(0, 48))                                                # the same forecast without its south-pole row
    assert a.shape[2] == 49 and b.shape[2] == 48
    with pytest.raises(ValueError, match="ensemble members are on different lat axes"):
        GlobalEnsemble(["pangu", "fourcastnet"])._ensemble_predictions([a, b])
    ens = GlobalEnsemble(["pangu", "fourcastnet"], grid=TARGET)
    mean = ens._ensemble_predictions([a, b])
    ra, rb = (G.regrid_prediction(p, TARGET, "conservative", device=DEV).values.astype(np.float64) for p in (a, b))
    assert mean.shape == ra.shape == (a.shape[0], a.shape[1], 13, 48)
    want = (ra + rb) / 2
    assert np.all(np.abs(mean.values - want) <= 2.0 ** -23 * np.abs(want))
    assert np.array_equal(ra[:, :, :12], rb[:, :, :12]) and not np.array_equal(ra[:, :, 12], rb[:, :, 12])      # only the last cell misses a row
