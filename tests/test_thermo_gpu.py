"""Column thermodynamics end to end on the MI355X with the Pangu toy model of tests/conftest.py (the ``toy`` fixture: 49 x 192, 13 levels): ``ensemble_forecast(derived=["mucape", ...])``
against the numpy float32 restatement on the kept members (bit for bit), with exceedance and scores; a request without thermodynamic
names unchanged; ``derive_fields`` against ``derive_prediction``; a model that carries relative humidity through ``LeadDeriver``; and
the surface mask, which changes the columns it masks and no others, in the forecast and in the truth of its scores, window aggregates included."""
from __future__ import annotations

import datetime

import numpy as np
import pytest

import _ens_reference as ER
import _score_reference as SR
import _thermo_reference as R
from skyrim_amd import derived as D
from skyrim_amd import thermo as T
from skyrim_amd import verify as V

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T0 = datetime.datetime(2024, 5, 13, 18, 0)
LEVELS = list(R.PANGU_LEVELS)
KW = dict(n_steps=2, n_members=3, keep_members=True, products=("mean",), perturb_scale=0.05)


@pytest.fixture(scope="module")
def pangu(toy):
    from skyrim_amd.core.models.pangu import PanguModel
    g, params, _ = toy
    return PanguModel(ic_source="gfs", geom=g, params=params)


def same_bits(got, want, what):
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), what
    diff = (got.view(np.uint32) != want.view(np.uint32)) & ~nan
    assert not diff.any(), (what, int(diff.sum()), got[diff][:4], want[diff][:4])


def restate(state, names, fields, zs=None, letter="q"):
    """{field: plane} of one (C, H, W) state by the float32 restatement"""
    kind = R.Q if letter == "q" else R.R
    col = lambda x: state[[names.index(f"{x}{l}") for l in LEVELS]]           # noqa: E731
    ch = lambda n: state[names.index(n)]                                       # noqa: E731
    out = {}
    for f in fields:
        if f in ("mucape", "muli", "mucape_src", "sbcape", "sbli"):
            src = R.SRC_MAX_THETAE if f.startswith("mu") else R.SRC_LOWEST
            res = R.fp32.parcel(col("t"), col(letter), LEVELS, kind, src, z=col("z") if zs is not None else None, zs=zs)
            out[f] = res[{"cape": 0, "li": 1, "_src": 2}[f[2:] if f != "mucape_src" else "_src"]]
        elif f in ("kx", "tt"):
            out[f] = R.fp32.index(ch("t850"), ch("t700"), ch("t500"), ch(f"{letter}850"), ch(f"{letter}700"), kind)[f == "tt"]
        elif f == "zdeg0":
            out[f] = R.fp32.freeze(col("t"), col("z"), zs)
        elif f[:2] in ("td", "rh", "th") or f[0] == "q":
            what = f.rstrip("0123456789")
            lev = int(f[len(what):])
            out[f] = R.fp32.moist(ch(f"t{lev}"), ch(f"{letter}{lev}"), lev, kind, theta_only=False)[{"td": 0, "rh": 1, "q": 1, "thetae": 2, "theta": 3}[what]]
    return out


def test_ensemble_thermo_fields_equal_the_restatement_on_the_members(pangu, monkeypatch):
    from skyrim_amd.labeled import DataArray
    fields = ["mucape", "thetae850", "ws10m"]
    plain = pangu.ensemble_forecast(T0, derived=["ws10m"], **KW)
    names = plain.members.channel.values.tolist()
    lat, lon = np.asarray(pangu.model.grid.lat), np.asarray(pangu.model.grid.lon)
    truth = DataArray(np.asarray(plain.members.values)[0], ["time", "channel", "lat", "lon"],
                      dict(time=list(plain.mean.time.values), channel=names, lat=lat, lon=lon))
    ens = pangu.ensemble_forecast(T0, derived=fields, exceed={"mucape": [500.0]}, scores=True, truth=truth, **KW)
    assert np.array_equal(plain.members.values, ens.members.values)            # the raw products are what they were
    d = ens.derived
    assert d.fields == fields and d.members.shape[:3] == (3, 3, 3) and set(d.exceedance) == {"mucape"}
    # ws10m beside the thermodynamic fields has the bits it has alone: the derive launch is the same, the thermo launch writes other slots
    assert np.array_equal(np.asarray(plain.derived.members.values)[:, :, 0], np.asarray(d.members.values)[:, :, 2])
    raw, dm = np.asarray(ens.members.values), np.asarray(d.members.values)
    for m in range(3):
        for t in range(3):
            ref = restate(raw[m, t], names, fields[:2])
            for k, f in enumerate(fields[:2]):
                same_bits(dm[m, t, k], ref[f], (f, m, t))
    assert np.isfinite(dm).all()
    print(f"mucape of the synthetic members: max {float(dm[:, :, 0].max()):.1f} J/kg, {float((dm[:, :, 0] > 0).mean()):.3f} of the columns unstable")
    fractions = []
    for t in range(3):
        r = ER.stats(dm[:, t, 0].reshape(3, -1), thresholds=[500.0])
        assert np.array_equal(d.exceedance["mucape"].values[t].reshape(1, -1), r["exceed"])
        fractions.append(float(r["exceed"].mean()))
    assert float(dm[:, :, 0].max()) > 500.0 and 0 < max(fractions) < 1      # the threshold cuts through the members' values
    # the scores: the truth is the control member, so its derived truth is the control's derived planes -- member 0 has no error at all
    ds = d.scores
    assert ds.channels == fields and d.dropped == {} and ds.n_members == 3
    rmse = ds.metric("rmse")
    assert np.isfinite(rmse).all() and rmse.shape[0] == 3 and float(rmse[1:, 1:].min()) > 0
    # a request without thermodynamic names never loads the thermo library
    def boom():
        raise AssertionError("thermo.load_library called")
    monkeypatch.setattr(T, "load_library", boom)
    again = pangu.ensemble_forecast(T0, derived=["ws10m"], **KW)
    assert np.array_equal(again.derived.members.values, plain.derived.members.values) and np.array_equal(again.mean.values, plain.mean.values)


def test_derive_fields_equals_derive_prediction_and_the_restatement(pangu, tmp_path):
    fields = ["sbcape", "sbli", "mucape", "muli", "mucape_src", "td850", "rh850", "thetae850", "theta500", "kx", "tt", "zdeg0", "thk500_1000"]
    live = pangu.derive_fields(T0, 2, fields)
    assert live.channel.values.tolist() == fields and live.shape[:2] == (3, len(fields))
    _, paths = pangu.rollout(T0, n_steps=2, save=True, save_config={"output_dir": str(tmp_path)})
    disk = D.derive_prediction(list(paths), fields, device=DEV)
    assert np.array_equal(disk.values.view(np.uint32), live.values.view(np.uint32))
    from skyrim_amd.leads import open_saved
    saved = open_saved(list(paths), "test_thermo_gpu")
    seen = 0
    for t, (_, _, state) in enumerate(saved.states(DEV)):
        ref = restate(state.cpu().numpy(), list(saved.names), fields[:-1])
        for k, f in enumerate(fields[:-1]):
            same_bits(disk.values[t, k], ref[f], (f, t))
        seen += 1
    assert seen == 3


def test_relative_humidity_channels_and_a_surface_through_the_lead_deriver():
    import torch
    H, W, M = 9, 20, 2
    names = [f"{x}{l}" for x in "tqrz" for l in LEVELS]
    made = [R.planted(60 + m, H, W, LEVELS) for m in range(M)]
    zs = made[0][1]
    keep = [i for i, n in enumerate(names) if n[0] != "q"]                     # a model with t, r and z: no specific humidity
    rnames = [names[i] for i in keep]
    lat, lon = np.linspace(80.0, -80.0, H), np.arange(W) * (360.0 / W)
    fields = ["mucape", "q850", "kx", "zdeg0", "sbli", "td700", "mucape_src"]
    deriver = D.LeadDeriver(rnames, lat, lon, M, fields, device=DEV, surface=zs)
    assert deriver.plan.moisture == "r" and not deriver.plan.ops
    states = [torch.from_numpy(np.ascontiguousarray(s[keep])).to(DEV) for s, _ in made]
    out, _ = deriver.add(states)
    for m in range(M):
        ref = restate(made[m][0][keep], rnames, fields, zs=zs, letter="r")
        got = out[m].cpu().numpy()
        for k, f in enumerate(fields):
            same_bits(got[k], ref[f], (f, m))


def test_a_surface_changes_only_the_columns_it_masks(pangu):
    fields = ["mucape", "mucape_src", "sbcape", "zdeg0", "thetae850", "kx"]
    free = pangu.derive_fields(T0, 1, fields)
    lat, lon = np.asarray(pangu.model.grid.lat), np.asarray(pangu.model.grid.lon)
    zs = np.full((lat.size, lon.size), -1e6, np.float32)
    zs[10:20, 30:90] = 1e4                                                      # a plateau of ~1 km: the lowest levels of its columns lie below it
    masked = pangu.derive_fields(T0, 1, fields, derived_surface=zs)
    same = np.ones(zs.shape, bool)
    same[10:20, 30:90] = False
    for k, f in enumerate(fields):
        assert np.array_equal(masked.values[:, k][:, same].view(np.uint32), free.values[:, k][:, same].view(np.uint32)), f
    src_free, src_masked = free.values[:, 1][:, ~same], masked.values[:, 1][:, ~same]
    assert np.all(src_masked <= src_free) and np.any(src_masked < src_free)    # the source moves up where the ground is higher
    for k in (4, 5):                                                            # fields of fixed levels do not read the surface
        assert np.array_equal(masked.values[:, k].view(np.uint32), free.values[:, k].view(np.uint32))
    # the same surface through the ensemble: the control member is the deterministic forecast, and the truth is masked as the forecast is
    ens = pangu.ensemble_forecast(T0, n_steps=1, n_members=2, keep_members=True, products=("mean",), perturb_scale=0.05, derived=["mucape_src", "zdeg0"],
                                  derived_surface=zs, scores=True)
    got = np.asarray(ens.derived.members.values)
    assert np.array_equal(got[0, :, 0].view(np.uint32), masked.values[:, 1].view(np.uint32))
    assert np.array_equal(got[0, :, 1].view(np.uint32), masked.values[:, 3].view(np.uint32))
    assert ens.derived.scores.channels == ["mucape_src", "zdeg0"] and ens.derived.dropped == {}
    assert np.isfinite(ens.derived.scores.metric("rmse")).all()



def test_window_aggregates_of_masked_fields_are_scored_against_a_masked_truth(pangu):
    """``aggregates=`` with ``derived_surface=`` and ``scores=True``: the truth is the control run, so the aggregated truth must be the
    aggregated control member -- which it is only when the truth is derived under the same surface as the forecast"""
    from skyrim_amd.labeled import DataArray
    kw = dict(n_steps=2, n_members=3, keep_members=True, products=("mean",), perturb_scale=0.05)
    fields = ["mucape_src", "zdeg0"]
    lat, lon = np.asarray(pangu.model.grid.lat), np.asarray(pangu.model.grid.lon)
    zs = np.full((lat.size, lon.size), -1e6, np.float32)
    zs[10:20, 30:90] = 1e4
    plain = pangu.ensemble_forecast(T0, **kw)
    names = plain.members.channel.values.tolist()
    truth = DataArray(np.asarray(plain.members.values)[0], ["time", "channel", "lat", "lon"],
                      dict(time=list(plain.mean.time.values), channel=names, lat=lat, lon=lon))
    ens = pangu.ensemble_forecast(T0, derived=fields, derived_surface=zs, aggregates=["mucape_src:min:12h", "zdeg0:max:12h"], scores=True,
                                  truth=truth, **kw)
    a = ens.aggregated["12h"]
    assert a.fields == ["mucape_src_min_12h", "zdeg0_max_12h"] and a.dropped == {} and a.scores.channels == a.fields
    got, dm = np.asarray(a.members.values), np.asarray(ens.derived.members.values)
    assert got.shape[:3] == (3, 1, 2)
    assert np.array_equal(got[:, 0, 0], dm[:, 1:, 0].min(axis=1)) and np.array_equal(got[:, 0, 1], dm[:, 1:, 1].max(axis=1))
    free = pangu.derive_fields(T0, 2, fields)                                  # without the surface the plateau's columns are others
    assert np.any(free.values[1:, 0].min(axis=0)[10:20, 30:90] != got[0, 0, 0][10:20, 30:90])
    w = V.area_weights(lat)
    s = a.scores
    slots = s.sums.slot.values.tolist()
    val, bound, counts = SR.scores(got[:, 0], got[0, 0], w)                     # the truth: member 0's own aggregates
    worst = 0.0
    for k, name in enumerate(slots):
        err = np.abs(s.sums.values[k, 0] - val[name])
        worst = max(worst, float(np.where(bound[name] > 0, err / np.where(bound[name] > 0, bound[name], 1), np.where(err == 0, 0, np.inf)).max()))
    print(f"aggregated masked scores: worst share of the bound {worst:.3f}")
    assert worst <= 1 and np.array_equal(s.rank_counts.values[0], counts.sum(axis=1))
    # and the lead-time scores of the same run: the derived truth is the control's derived planes
    ds = ens.derived.scores
    slots = ds.sums.slot.values.tolist()
    for t in range(3):
        val, bound, _ = SR.scores(dm[:, t], dm[0, t], w)
        for k, name in enumerate(slots):
            err = np.abs(ds.sums.values[k, t] - val[name])
            assert np.all(np.where(bound[name] > 0, err <= bound[name], err == 0)), (t, name)
