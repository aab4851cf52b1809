"""Fields on chosen surfaces end to end on the MI355X with the Pangu toy model of tests/conftest.py (the ``toy`` fixture: 49 x 192, 13
levels): ``ensemble_forecast(derived=["ws@100magl", "t@1500m", ...])`` against the numpy float32 restatement on the kept members (bit for
bit), with exceedance, scores and points; the truth through the same ops; ``derive_fields`` against ``derive_prediction`` on saved
files; and a request without ``@`` names, which loads and launches nothing new."""
from __future__ import annotations

import datetime

import numpy as np
import pytest

import _ens_reference as ER
import _score_reference as SR
import _vert_reference as R
from skyrim_amd import derived as D
from skyrim_amd import verify as VF
from skyrim_amd import vertical as V

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T0 = datetime.datetime(2024, 5, 13, 18, 0)
KW = dict(n_steps=2, n_members=3, keep_members=True, products=("mean",), perturb_scale=0.05)


@pytest.fixture(scope="module")
def pangu(toy):
    from skyrim_amd.core.models.pangu import PanguModel
    g, params, _ = toy
    return PanguModel(ic_source="gfs", geom=g, params=params)


@pytest.fixture(scope="module")
def ground(pangu):
    """a surface some 200 m below sea level with a plateau of 1 km: the lowest levels of the plateau's columns lie below it"""
    zs = np.full((len(pangu.model.grid.lat), len(pangu.model.grid.lon)), -2000.0, np.float32)
    zs[10:20, 30:90] = 1e4
    return zs


def same_bits(got, want, what):
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), what
    diff = (got.view(np.uint32) != want.view(np.uint32)) & ~nan
    assert not diff.any(), (what, int(diff.sum()), got[diff][:4], want[diff][:4])


def restate(state, names, fields, zs=None, vertical=None):
    """{field: plane} of one (C, H, W) state: the plan's own ops through the float32 restatement"""
    lat, lon = np.linspace(90.0, -90.0, state.shape[1]), np.arange(state.shape[2]) * (360.0 / state.shape[2])
    plan = D.plan(names, fields, lat, lon, surface=zs is not None, vertical=vertical)
    out = {}
    for op in plan.vert_ops:
        for slot, plane in R.fp32.apply(op, state, zs).items():
            out[fields[slot]] = plane
    return out


def test_ensemble_fields_on_surfaces_equal_the_restatement_on_the_members(pangu, ground, monkeypatch):
    from skyrim_amd.labeled import DataArray
    fields = ["ws@100magl", "t@1500m", "ws10m"]
    lat, lon = np.asarray(pangu.model.grid.lat), np.asarray(pangu.model.grid.lon)
    j, i = 12, 16
    places = {"node": (float(lat[j]), float(lon[i])), "plateau": (float(lat[15]), float(lon[60]))}
    plain = pangu.ensemble_forecast(T0, derived=["ws10m"], **KW)
    names = plain.members.channel.values.tolist()
    truth = DataArray(np.asarray(plain.members.values)[0], ["time", "channel", "lat", "lon"],
                      dict(time=list(plain.mean.time.values), channel=names, lat=lat, lon=lon))
    opts = {"outside": "nearest"}                                              # (a value in every column: the statistics and scores below are of finite fields)
    ens = pangu.ensemble_forecast(T0, derived=fields, derived_surface=ground, vertical=opts, exceed={"ws@100magl": [8.0]}, scores=True, truth=truth,
                                  points=places, point_channels=["t@1500m"], point_method="nearest", **KW)
    assert np.array_equal(plain.members.values, ens.members.values)            # the raw products are what they were
    d = ens.derived
    assert d.fields == fields and d.members.shape[:3] == (3, 3, 3) and set(d.exceedance) == {"ws@100magl"}
    # ws10m beside the fields on surfaces has the bits it has alone: the derive launch is the same, the vert launch writes other slots
    assert np.array_equal(np.asarray(plain.derived.members.values)[:, :, 0], np.asarray(d.members.values)[:, :, 2])
    raw, dm = np.asarray(ens.members.values), np.asarray(d.members.values)
    for m in range(3):
        for t in range(3):
            ref = restate(raw[m, t], names, fields[:2], ground, opts)
            nans = restate(raw[m, t], names, fields[:2], ground)              # the same with NaN outside: where there is a crossing, the same values
            for k, f in enumerate(fields[:2]):
                same_bits(dm[m, t, k], ref[f], (f, m, t))
                there = ~np.isnan(nans[f])
                assert there.mean() > 0.5 and np.array_equal(nans[f][there].view(np.uint32), ref[f][there].view(np.uint32))
    assert np.isfinite(dm).all()
    print(f"ws@100magl of the synthetic members: {float(dm[:, :, 0].min()):.2f} .. {float(dm[:, :, 0].max()):.2f} m/s; "
          f"t@1500m {float(dm[:, :, 1].min()):.1f} .. {float(dm[:, :, 1].max()):.1f} K")
    fractions = []
    for t in range(3):
        r = ER.stats(dm[:, t, 0].reshape(3, -1), thresholds=[8.0])
        assert np.array_equal(d.exceedance["ws@100magl"].values[t].reshape(1, -1), r["exceed"])
        fractions.append(float(r["exceed"].mean()))
    assert 0 < max(fractions) < 1                                              # the threshold cuts through the members' values
    # the points: the nearest cell of the derived plane
    pv = ens.points.values.values
    assert ens.points.channels == ["t@1500m"] and pv.shape == (3, 3, 1, 2)
    assert np.array_equal(pv[:, :, 0, 0].view(np.uint32), dm[:, :, 1, j, i].view(np.uint32))
    assert np.array_equal(pv[:, :, 0, 1].view(np.uint32), dm[:, :, 1, 15, 60].view(np.uint32))
    # the scores: the truth is the control member and goes through the same ops, so its derived truth is the control's derived planes
    ds = d.scores
    assert ds.channels == fields and d.dropped == {} and ds.n_members == 3
    w = VF.area_weights(lat)
    slots = ds.sums.slot.values.tolist()
    for t in range(3):
        val, bound, _ = SR.scores(dm[:, t], dm[0, t], w)
        for k, name in enumerate(slots):
            err = np.abs(ds.sums.values[k, t] - val[name])
            assert np.all(np.where(bound[name] > 0, err <= bound[name], err == 0)), (t, name)
    crps = ds.metric("crps")
    assert np.isfinite(crps).all() and crps.shape[0] == 3 and float(crps[1:, :2].min()) > 0
    # a request without @ names never loads the library, launches what it launched before and gives what it gave
    def boom(*a, **k):
        raise AssertionError("libskyrim_vert used without an @ name")
    monkeypatch.setattr(V, "load_library", boom)
    monkeypatch.setattr(V, "run", boom)
    again = pangu.ensemble_forecast(T0, derived=["ws10m"], vertical={"outside": "nearest"}, **KW)
    assert np.array_equal(again.derived.members.values, plain.derived.members.values) and np.array_equal(again.mean.values, plain.mean.values)


def test_derive_fields_equals_derive_prediction_and_the_restatement(pangu, ground, tmp_path):
    fields = ["u@320K", "p@320K", "z@-10C", "ws@875hPa", "theta@875hPa", "ws@150magl", "z@100magl", "q@3000m", "thk500_1000", "zdeg0"]
    opts = {"outside": "nearest"}
    live = pangu.derive_fields(T0, 2, fields, derived_surface=ground, vertical=opts)
    assert live.channel.values.tolist() == fields and live.shape[:2] == (3, len(fields))
    _, paths = pangu.rollout(T0, n_steps=2, save=True, save_config={"output_dir": str(tmp_path)})
    disk = D.derive_prediction(list(paths), fields, device=DEV, surface=ground, vertical=opts)
    assert np.array_equal(disk.values.view(np.uint32), live.values.view(np.uint32))
    one = D.derive_prediction(list(paths), ["u@320K"], device=DEV)             # alone, without a surface, with NaN outside
    from skyrim_amd.leads import open_saved
    saved = open_saved(list(paths), "test_vert_gpu")
    seen = 0
    for t, (_, _, state) in enumerate(saved.states(DEV)):
        host = state.cpu().numpy()
        ref = restate(host, list(saved.names), fields[:-2], ground, opts)
        for k, f in enumerate(fields[:-2]):
            same_bits(disk.values[t, k], ref[f], (f, t))
        same_bits(one.values[t, 0], restate(host, list(saved.names), ["u@320K"])["u@320K"], ("u@320K alone", t))
        seen += 1
    assert seen == 3
    # z@0C is zdeg0 wherever the isotherm crosses the column (zdeg0 falls back to the lowest level elsewhere)
    iso = pangu.derive_fields(T0, 1, ["z@0C", "zdeg0"], derived_surface=ground)
    crossed = ~np.isnan(iso.values[:, 0])
    assert crossed.any() and np.array_equal(iso.values[:, 0][crossed].view(np.uint32), iso.values[:, 1][crossed].view(np.uint32))


def test_replay_and_aggregates_take_at_names(pangu, ground, tmp_path):
    """``aggregates="ws@100magl:max:12h"`` in the forecast, and the same fields from the archive's files"""
    fields = ["ws@100magl", "t@1500m"]
    kw = dict(n_steps=2, n_members=2, keep_members=True, products=("mean",), perturb_scale=0.05)
    ens = pangu.ensemble_forecast(T0, derived=fields, derived_surface=ground, aggregates=["ws@100magl:max:12h"],
                                  archive={"packing": "float32", "dir": str(tmp_path / "arch")}, **kw)
    dm = np.asarray(ens.derived.members.values)
    a = ens.aggregated["12h"]
    assert a.fields == ["ws@100magl_max_12h"] and np.array_equal(np.asarray(a.members.values)[:, 0, 0], dm[:, 1:, 0].max(axis=1))
    again = ens.archive.replay(derived=fields, derived_surface=ground, vertical={"outside": "nan"}, keep_members=True, products=("mean",))
    assert np.array_equal(np.asarray(again.derived.members.values).view(np.uint32), dm.view(np.uint32))
