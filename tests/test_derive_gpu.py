"""Derived fields end to end on the MI355X with the Pangu toy model (49 x 192): ``ensemble_forecast(derived=[...])`` against the float64
restatements on the kept members, the raw products unchanged, derived scores against the derived control run, ``derive_fields`` against
``derive_prediction`` on the files of the same rollout, and the refusal for a model without specific humidity."""
from __future__ import annotations

import datetime
from types import SimpleNamespace

import numpy as np
import pytest

import _derive_reference as R
import _ens_reference as ER
import _score_reference as SR
from skyrim_amd import derived as D
from skyrim_amd import verify as V

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T0 = datetime.datetime(2024, 5, 13, 18, 0)
FIELDS = ["ws10m", "ivt", "vo850", "thk500_1000"]
LEVELS = [300, 400, 500, 600, 700, 850, 925, 1000]
KW = dict(n_steps=2, n_members=3, keep_members=True, products=("mean", "spread"), perturb_scale=0.05)


@pytest.fixture(scope="module")
def pangu(toy):
    from skyrim_amd.core.models.pangu import PanguModel
    g, params, _ = toy
    return PanguModel(ic_source="gfs", geom=g, params=params)


@pytest.fixture(scope="module")
def plain(pangu):
    """The same ensemble without derived fields: computed once, shared, left unchanged."""
    return pangu.ensemble_forecast(T0, **KW)


def _restate(state, names, lat, lon):
    """{field: (value, bound)} of FIELDS for one (C, H, W) state."""
    ch = names.index
    rowc, e0, e1 = R.row_table(lat, lon)
    v, S = R.speed(state[ch("u10m")], state[ch("v10m")])
    out = {"ws10m": (v, R.bound(R.K_SPEED, S, R.TINY_SPEED))}
    w = R.column_weights(LEVELS).astype(np.float32)
    v, S, k, tiny = R.column(*(state[[ch(f"{x}{l}") for l in LEVELS]] for x in "quv"), w)["ivt"]
    out["ivt"] = (v, R.bound(k, S, tiny))
    out["vo850"] = R.vortdiv(state[ch("u850")], state[ch("v850")], rowc, e0, e1)["vo"]
    v, S = R.diff(state[ch("z500")], state[ch("z1000")])
    out["thk500_1000"] = (v, R.bound(R.K_DIFF, S, R.TINY_DIFF))
    return out


def _thresholds(values, rel=1e-4):
    """Two thresholds (fp32) among the values such that no value lies within ``rel`` relative of either; the margin is asserted."""
    flat = np.sort(np.asarray(values, np.float64).reshape(-1))
    picks = []
    for lo, hi in ((0.90, 0.97), (0.97, 0.9995)):               # the upper tail, where the values lie far apart: the widest gap of each range
        a, b = int(lo * flat.size), int(hi * flat.size)
        j = a + int(np.argmax(np.diff(flat[a:b + 1])))
        picks.append(float(np.float32((flat[j] + flat[j + 1]) / 2)))
    margin = min(float(np.abs(flat - t).min()) / abs(t) for t in picks)
    assert margin > rel, f"a member value lies within {margin:.2e} (relative) of a threshold"
    return picks


def test_ensemble_derived_products_equal_the_restatements_on_the_members(pangu, plain):
    probe = pangu.ensemble_forecast(T0, derived=["ws10m"], **KW)               # the members' wind speed, to choose thresholds from
    thr = _thresholds(probe.derived.members.values)
    ens = pangu.ensemble_forecast(T0, derived=FIELDS, exceed={"ws10m": thr, "t2m": [280.0]}, quantiles={"ivt": [0.5]}, **KW)
    assert plain.derived is None
    for p in ("mean", "spread", "members"):                                    # the raw products: bit for bit what they were
        assert np.array_equal(getattr(plain, p).values, getattr(ens, p).values), p
    assert set(ens.exceedance) == {"t2m"} and set(ens.derived.exceedance) == {"ws10m"} and set(ens.derived.quantile) == {"ivt"}
    d = ens.derived
    assert d.fields == FIELDS and d.mean.channel.values.tolist() == FIELDS and d.members.dims == ("member", "time", "channel", "lat", "lon")
    assert d.members.shape == (3, 3, 4) + ens.mean.shape[2:] and d.min is None and d.scores is None
    assert np.array_equal(probe.derived.members.values[:, :, 0], d.members.values[:, :, 0])
    names = ens.members.channel.values.tolist()
    lat, lon = np.asarray(pangu.model.grid.lat, np.float64), np.asarray(pangu.model.grid.lon, np.float64)
    raw, dm = np.asarray(ens.members.values), np.asarray(d.members.values)
    worst = dict.fromkeys(FIELDS, 0.0)
    for m in range(3):
        for t in range(3):
            ref = _restate(raw[m, t], names, lat, lon)
            for k, name in enumerate(FIELDS):
                val, bnd = ref[name]
                err = np.abs(dm[m, t, k].astype(np.float64) - val)
                worst[name] = max(worst[name], float(np.where(bnd > 0, err / np.where(bnd > 0, bnd, 1), np.where(err == 0, 0, np.inf)).max()))
    print("derived members: worst share of the bound " + " ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert max(worst.values()) <= 1
    # the statistics of the derived members: the restatement of skyrim_ens.h under the tolerances of tests/test_ens_gpu.py
    fractions = []
    for t in range(3):
        x = dm[:, t].reshape(3, -1)
        ref = ER.stats(x)
        em = np.abs(d.mean.values[t].reshape(-1).astype(np.float64) - ref["mean"]) / np.maximum(ER.mean_bound(x, ref["mean"]), 1e-300)
        es = np.abs(d.spread.values[t].reshape(-1).astype(np.float64) - ref["spread"]) / np.maximum(ER.spread_bound(x, ref["spread"]), 1e-300)
        print(f"derived lead {t}: mean {em.max():.3f} of its bound, spread {es.max():.3f} of its bound")
        assert em.max() <= 1 and es.max() <= 1
        r = ER.stats(dm[:, t, 0].reshape(3, -1), thresholds=thr)
        assert np.array_equal(d.exceedance["ws10m"].values[t].reshape(2, -1), r["exceed"])
        fractions.append(float(r["exceed"].mean()))
        (q, big), = ER.stats(dm[:, t, 1].reshape(3, -1), levels=[0.5])["quant"]
        assert np.all(np.abs(d.quantile["ivt"].values[t, 0].reshape(-1).astype(np.float64) - q) <= 2 * np.spacing(big.astype(np.float32)))
    assert 0 < max(fractions) < 1                                               # the thresholds cut through the members' values


def test_derived_scores_against_the_derived_control_run(pangu, plain):
    from skyrim_amd.labeled import DataArray
    lat, lon = np.asarray(pangu.model.grid.lat), np.asarray(pangu.model.grid.lon)
    names = plain.members.channel.values.tolist()
    control = np.asarray(plain.members.values)[0]                               # (T, C, H, W)
    times = list(plain.mean.time.values)
    truth = DataArray(control, ["time", "channel", "lat", "lon"], dict(time=times, channel=names, lat=lat, lon=lon))
    ens = pangu.ensemble_forecast(T0, derived=FIELDS, scores=True, truth=truth, **KW)
    assert np.array_equal(plain.members.values, ens.members.values)
    ds = ens.derived.scores
    assert ds.channels == FIELDS and ds.n_members == 3 and ens.derived.dropped == {} and ens.scores.channels == names
    dm = np.asarray(ens.derived.members.values)
    w = V.area_weights(lat)
    slots = ds.sums.slot.values.tolist()
    worst = 0.0
    for t in range(3):
        val, bound, counts = SR.scores(dm[:, t], dm[0, t], w)                  # the derived truth is the derived control member
        for k, name in enumerate(slots):
            err = np.abs(ds.sums.values[k, t] - val[name])
            worst = max(worst, float(np.where(bound[name] > 0, err / np.where(bound[name] > 0, bound[name], 1), np.where(err == 0, 0, np.inf)).max()))
        assert np.array_equal(ds.rank_counts.values[t], counts.sum(axis=1))
        ref = SR.table({n: ds.sums.values[k, t] for k, n in enumerate(slots)}, 3)
        for name in ("crps", "rmse"):
            assert np.array_equal(ds.metric(name)[t], ref[name], equal_nan=True), name
    print(f"derived scores: worst share of the bound {worst:.3f}")
    assert worst <= 1 and float(ds.metric("rmse")[1:].min()) > 0
    # a truth without humidity: ivt is dropped from the scores and reported, the others are scored
    dry = DataArray(control[:, [names.index(c) for c in names if not c.startswith("q")]], ["time", "channel", "lat", "lon"],
                    dict(time=times, channel=[c for c in names if not c.startswith("q")], lat=lat, lon=lon))
    part = pangu.ensemble_forecast(T0, derived=FIELDS, scores=True, truth=dry, **dict(KW, keep_members=False))
    assert part.derived.scores.channels == ["ws10m", "vo850", "thk500_1000"] and list(part.derived.dropped) == ["ivt"]
    assert part.derived.dropped["ivt"][0] == "q300"
    keep = [FIELDS.index(c) for c in part.derived.scores.channels]
    assert np.allclose(part.derived.scores.sums.values, ds.sums.values[:, :, keep], rtol=1e-10, atol=0)


def test_derive_fields_equals_derive_prediction_on_saved_files(pangu, tmp_path):
    fields = FIELDS + ["div850", "iwv"]
    live = pangu.derive_fields(T0, 2, fields)
    assert live.dims == ("time", "channel", "lat", "lon") and live.channel.values.tolist() == fields and live.shape[:2] == (3, 6)
    assert np.isfinite(live.values).all()
    _, paths = pangu.rollout(T0, n_steps=2, save=True, save_config={"output_dir": str(tmp_path)})
    disk = D.derive_prediction(list(paths), fields, device=DEV)
    assert [np.datetime64(t, "s") for t in disk.time.values] == [np.datetime64(t, "s") for t in live.time.values]
    assert np.array_equal(disk.values, live.values)
    from skyrim_amd.core import Skyrim
    s = object.__new__(Skyrim)
    s.model = pangu
    assert np.array_equal(s.derive_fields(T0, 2, fields).values, live.values)


def test_a_model_without_humidity_is_refused_before_any_launch():
    from skyrim_amd.core import Skyrim
    from skyrim_amd.core.models.fourcastnet import FourcastnetModel
    from skyrim_amd.fcn.spec import CHANNELS

    class NoDevice:
        out_channel_names = list(CHANNELS)
        in_channel_names = list(CHANNELS)
        grid = SimpleNamespace(lat=np.linspace(90, -90, 721)[:720], lon=np.arange(1440) * 0.25)

        def __getattr__(self, name):                            # the device, the generator: nothing of it may be asked for
            raise AssertionError(f"model.{name} was read before the refusal")

    gm = object.__new__(FourcastnetModel)
    gm.model_name, gm.model = "fourcastnet", NoDevice()
    s = object.__new__(Skyrim)
    s.model = gm
    with pytest.raises(ValueError, match="specific humidity"):
        s.ensemble_forecast(T0, n_members=3, derived=["ivt"])
    with pytest.raises(ValueError, match="specific humidity"):
        s.derive_fields(T0, 2, ["ivt"])
    with pytest.raises(ValueError, match="specific humidity"):
        D.LeadDeriver(CHANNELS, NoDevice.grid.lat, NoDevice.grid.lon, 3, ["ivt"], DEV)
