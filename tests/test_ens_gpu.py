"""``ensemble_forecast`` end to end on the MI355X: Pangu at 49 x 192 and FuXi at its toy size (two history levels, the cascade),
the control member against ``forecast``, every product against the float64 statistic of the kept members, seeds, files and the
``ensemble`` command."""
from __future__ import annotations

import datetime
from pathlib import Path

import numpy as np
import pytest
import torch

import _ens_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T0 = datetime.datetime(2024, 5, 13, 18, 0)
FUXI_TOY = dict(n_lat=73, n_lon=144, channels=6, embed=128, heads=2, depth=2, window=(3, 6))


@pytest.fixture(scope="module")
def pangu(toy):
    from skyrim_amd.core.models.pangu import PanguModel
    g, params, _ = toy
    return PanguModel(ic_source="gfs", geom=g, params=params)


@pytest.fixture(scope="module")
def fuxi():
    from skyrim_amd.core.models.fuxi import FuxiModel
    from skyrim_amd.fuxi.spec import FuxiConfig, init_synthetic
    cfg = FuxiConfig(**FUXI_TOY, cascade_steps=(1, 2))
    return FuxiModel(ic_source="synthetic", cfg=cfg, params=init_synthetic(cfg, 11), device=DEV)


def _products_match_members(ens, exceed, quantiles):
    mem = np.asarray(ens.members.values)                       # (M, T, C, H, W)
    M, T, C = mem.shape[:3]
    names = ens.members.channel.values.tolist()
    for t in range(T):
        x = mem[:, t].reshape(M, -1)
        ref = R.stats(x)
        assert np.array_equal(ens.min.values[t].reshape(-1), ref["min"]) and np.array_equal(ens.max.values[t].reshape(-1), ref["max"])
        em = np.abs(ens.mean.values[t].reshape(-1).astype(np.float64) - ref["mean"]) / np.maximum(R.mean_bound(x, ref["mean"]), 1e-300)
        es = np.abs(ens.spread.values[t].reshape(-1).astype(np.float64) - ref["spread"]) / np.maximum(R.spread_bound(x, ref["spread"]), 1e-300)
        print(f"{ens.model_name} lead {t}: mean {em.max():.3f} of its bound, spread {es.max():.3f} of its bound")
        assert em.max() <= 1 and es.max() <= 1
        for ch, thr in exceed.items():
            r = R.stats(mem[:, t, names.index(ch)].reshape(M, -1), thresholds=thr)
            assert np.array_equal(ens.exceedance[ch].values[t].reshape(len(thr), -1), r["exceed"])
        for ch, lev in quantiles.items():
            r = R.stats(mem[:, t, names.index(ch)].reshape(M, -1), levels=lev)
            for k, (q, big) in enumerate(r["quant"]):
                got = ens.quantile[ch].values[t, k].reshape(-1).astype(np.float64)
                assert np.all(np.abs(got - q) <= 2 * np.spacing(big.astype(np.float32)))


def _end_to_end(m, exceed, quantiles):
    before = m.forecast(T0, n_steps=3)
    before_vals = np.array(before.values)
    kw = dict(n_steps=3, n_members=5, keep_members=True, products=("mean", "spread", "min", "max"), exceed=exceed, quantiles=quantiles)
    ens = m.ensemble_forecast(T0, seed=0, **kw)
    assert ens.n_members == 5 and ens.seed == 0 and ens.perturb_scale == 1e-3 and ens.paths == []
    assert ens.mean.dims == ("time", "channel", "lat", "lon") and ens.mean.shape == before.shape
    assert ens.members.dims == ("member", "time", "channel", "lat", "lon") and ens.members.shape == (5,) + before.shape
    assert np.array_equal(ens.mean.time.values, before.time.values)
    for ch, v in exceed.items():
        assert ens.exceedance[ch].dims == ("time", "threshold", "lat", "lon") and ens.exceedance[ch].shape[1] == len(v)
    for ch, v in quantiles.items():
        assert ens.quantile[ch].dims == ("time", "quantile", "lat", "lon") and ens.quantile[ch].shape[1] == len(v)
    mem = np.asarray(ens.members.values)
    assert np.array_equal(mem[0], before_vals)                               # the control member: forecast, bit for bit
    assert all(not np.array_equal(mem[k], mem[0]) for k in range(1, 5))
    assert float(np.asarray(ens.spread.values)[1:].max()) > 0
    _products_match_members(ens, exceed, quantiles)
    again = m.ensemble_forecast(T0, seed=0, **kw)
    assert np.array_equal(np.asarray(again.members.values), mem) and np.array_equal(again.spread.values, ens.spread.values)
    other = np.asarray(m.ensemble_forecast(T0, seed=1, **kw).members.values)
    assert np.array_equal(other[0], mem[0]) and all(not np.array_equal(other[k], mem[k]) for k in range(1, 5))
    one = m.ensemble_forecast(T0, n_steps=3, n_members=1)
    assert np.array_equal(one.mean.values, before_vals) and np.all(one.spread.values == 0)
    from skyrim_amd.core.models.base import GlobalPrediction
    name = ens.mean.channel.values.tolist()[0]
    assert GlobalPrediction(ens.mean).point(float(ens.mean.lat.values[3]), float(ens.mean.lon.values[5]), name, n_step=1) == ens.mean.values[1, 0, 3, 5].item()
    after = m.forecast(T0, n_steps=3)                                        # an ordinary call on the same object: the bits it gave before
    assert np.array_equal(np.asarray(after.values), before_vals)
    return ens


def test_pangu_toy_end_to_end(pangu):
    _end_to_end(pangu, {"t2m": [273.15, 303.15]}, {"t2m": [0.1, 0.5, 0.9]})
    pred, _ = pangu.rollout(T0, n_steps=2, save=False)
    ref = pangu.forecast(T0, n_steps=2)
    assert np.array_equal(np.asarray(pred.values)[-1], np.asarray(ref.values)[-1])


def test_fuxi_toy_end_to_end_and_cascade(fuxi):
    names = fuxi.out_channel_names
    _end_to_end(fuxi, {names[0]: [0.0, 1.0]}, {names[-1]: [0.0, 0.5, 1.0]})
    # every member switches stage at the same step: the step count belongs to the generator, not to the loop object
    calls, real = [], fuxi.model.engine.call

    def spy(older, newer, time, stage):
        calls.append(stage)
        return real(older, newer, time, stage)
    fuxi.model.engine.call = spy
    try:
        fuxi.ensemble_forecast(T0, n_steps=3, n_members=4)
    finally:
        del fuxi.model.engine.call
    assert calls == ["short"] * 4 + ["medium"] * 4 + ["long"] * 4


def test_non_finite_member_is_named(fuxi):
    real = fuxi.model.engine.call
    count = [0]

    def poison(older, newer, time, stage):
        out = real(older, newer, time, stage)
        count[0] += 1
        if count[0] == 5:                                    # 3 members: the 5th call is member 1's second step
            out = out.clone()
            out[0, 0, 0] = float("nan")
        return out
    fuxi.model.engine.call = poison
    try:
        with pytest.raises(FloatingPointError, match=r"member(\(s\))? \[?1\]?.*step 2"):
            fuxi.ensemble_forecast(T0, n_steps=3, n_members=3)
    finally:
        del fuxi.model.engine.call
    assert np.isfinite(fuxi.forecast(T0, n_steps=1).values).all()


@pytest.mark.parametrize("file_type", ["netcdf", "zarr"])
def test_save_writes_product_files(pangu, tmp_path, file_type):
    from skyrim_amd.labeled import open_dataarray
    cfg = {"output_dir": str(tmp_path), "file_type": file_type}
    ens = pangu.ensemble_forecast(T0, n_steps=2, n_members=3, products=("mean", "spread"), save=True, save_config=cfg)
    fid = cfg["forecast_id"]
    assert ens.forecast_id == fid and len(ens.paths) == 4
    if file_type == "netcdf":
        want = [f"pangu-ens3-{p}__{src}__{a}__{b}.nc" for (src, a, b) in (("synthetic", "20240513_18:00", "20240514_00:00"),
                                                                          ("file", "20240514_00:00", "20240514_06:00")) for p in ("mean", "spread")]
        assert [Path(p).name for p in ens.paths] == want
        for p in ens.paths:
            assert Path(p).parent == tmp_path / fid and Path(p).exists()
            assert len(Path(p).stem.split("__")) == 4
        for step in (1, 2):
            back = open_dataarray(ens.paths[2 * (step - 1)])
            assert back.shape == (2, 69, 49, 192)
            assert np.array_equal(back.isel(time=-1).values, ens.mean.values[step])
            assert np.array_equal(open_dataarray(ens.paths[2 * (step - 1) + 1]).isel(time=-1).values, ens.spread.values[step])
    else:
        assert set(ens.paths) == {str(tmp_path / fid / "pangu-ens3-mean"), str(tmp_path / fid / "pangu-ens3-spread")}
        back = open_dataarray(tmp_path / fid / "pangu-ens3-mean")
        assert back.shape[0] == 4                                             # two appends of two time entries each
        assert np.array_equal(back.isel(time=-1).values, ens.mean.values[2])


def _stats_launches(monkeypatch, gm, **kw):
    """[[(offset, n, names of the outputs given)] per step] of one ``ensemble_forecast``: every ``skyrim_amd.ensemble.stats`` call, still
    made.  A step opens where the driver builds the member table of the raw states."""
    from skyrim_amd import ensemble as E
    real_stats, real_table = E.stats, E.member_table
    state = len(gm.model.out_channel_names) * len(gm.model.grid.lat) * len(gm.model.grid.lon)
    steps = []

    def table(members):
        if len(members) == kw["n_members"] and members[0].numel() == state:
            steps.append([])
        return real_table(members)

    def spy(members, table, offset, n, mean=None, spread=None, min=None, max=None, exceed=None, thresholds=(), quant=None, levels=()):
        out = dict(mean=mean, spread=spread, min=min, max=max, exceed=exceed, quant=quant)
        steps[-1].append((offset, n, tuple(sorted(k for k, v in out.items() if v is not None))))
        return real_stats(members, table, offset, n, thresholds=thresholds, levels=levels, **out)
    monkeypatch.setattr(E, "member_table", table)
    monkeypatch.setattr(E, "stats", spy)
    gm.ensemble_forecast(T0, **kw)
    monkeypatch.undo()
    return steps


def _expected_launches(n_steps, products, raw, stored):
    """DESIGN.md 17, the launch rule.  Every step: one all-field launch for the raw set ``raw`` = (fields, hw, stored steps, exceed,
    quantiles); it carries the mean and, at a stored step, the products.  Per stored entry of each set of ``stored`` (the same tuples):
    one all-field launch when ``products`` is not empty, one per exceed channel and one per quantile channel; the raw set's all-field
    launch is the one it has anyway."""
    steps = []
    for k in range(n_steps + 1):
        fields, hw, at, _, _ = raw
        step = [(0, len(fields) * hw, tuple(sorted(set(products if k in at else ()) | {"mean"})))]
        for own, (fields, hw, at, exceed, quantiles) in enumerate([raw] + list(stored)):
            if k not in at:
                continue
            if products and own:
                step.append((0, len(fields) * hw, tuple(sorted(products))))
            step += [(fields.index(ch) * hw, hw, ("exceed",)) for ch in exceed] + [(fields.index(ch) * hw, hw, ("quant",)) for ch in quantiles]
        steps.append(sorted(step))
    return steps


def test_stats_launches_per_step(pangu, monkeypatch):
    """How many ``skens_stats`` launches a lead time costs, pinned as multisets per step: 4 steps, every second one stored, a 12-hour
    window that closes at steps 2 and 4."""
    names = list(pangu.model.out_channel_names)
    hw, rhw = 49 * 192, 13 * 24
    kw = dict(n_steps=4, n_members=3, save_every=2, products=("mean", "spread"))
    ex, qu = {"t2m": [280.0]}, {"msl": [0.5]}
    saved, closes = (0, 2, 4), (2, 4)
    cases = {
        "A": (dict(kw, derived=["ws10m"], aggregates=["t2m:max:12h"], exceed=dict(ex, ws10m=[8.0], t2m_max_12h=[285.0]), quantiles=qu),
              [(["ws10m"], hw, saved, ["ws10m"], []), (["t2m_max_12h"], hw, closes, ["t2m_max_12h"], [])]),
        "B": (dict(kw, grid="15deg", exceed=ex, quantiles=qu), [(names, rhw, saved, list(ex), list(qu))]),
        "C": (dict(kw, products=(), exceed=ex), []),
    }
    for case, (args, stored) in cases.items():
        got = _stats_launches(monkeypatch, pangu, **args)
        raw = (names, hw, saved, list(args["exceed"].keys() & set(names)), list(args.get("quantiles", {})))
        want = _expected_launches(4, args["products"], raw, stored)
        assert [sorted(s) for s in got] == want, case


LAUNCH_KW = dict(n_members=3, n_steps=4, save_every=2, products=("mean", "spread"))
LAUNCH_REQUESTS = {
    # everything that combines: every family but the regridded one, every per-lead consumer
    "A": dict(LAUNCH_KW, exceed={"t2m": [280.0], "ws10m": [8.0], "t2m_max_12h": [285.0]}, quantiles={"msl": [0.5]}, derived=["ws10m"],
              aggregates=["t2m:max:12h"], scores=True, events=True, neighbourhoods_km=[500.0], tracks=True,
              track_config=dict(lat_max=60.0, r_msl_km=1700.0, r_vort_km=1000.0, r_wind_km=1300.0, r_core_km=1100.0),   # radii for 3.75 degrees
              points={"node": (45.0, 30.0), "Istanbul": (41.01, 28.98)}, scenarios={"channels": ["z500"], "n_clusters": 2, "n_eofs": 2},
              spectra={"channels": ["t2m", "ws10m"]}, objects={"msl": {"below": [101000.0]}, "ws10m": {"above": [8.0]}}),
    # the regridded family, scored, its members kept
    "B": dict(LAUNCH_KW, grid="15deg", scores=True, keep_members="regridded", exceed={"t2m": [280.0]}, quantiles={"msl": [0.5]}),
    # members held as states: bred seeds, every step perturbed
    "C": dict(LAUNCH_KW, breeding={"cycles": 2}, stochastic={"kind": "both"}),
}
LAUNCH_GOLDEN = Path(__file__).parent / "golden" / "ens_launch_sequence.json"


def launch_sequence(monkeypatch, gm, **kw) -> list:
    """The ``what`` of every C-ABI call of one ``ensemble_forecast``, in order: every binding reports its return code through
    ``skyrim_amd.native.check``, the model's own steps included.  The request runs once before the recorded run, so that the tables a
    process makes once (transform twiddles, prepared spectral weights) exist whatever ran before."""
    from skyrim_amd import native
    real, seen = native.check, []

    def spy(code, what, lib=None):
        seen.append(what)
        return real(code, what, lib)
    gm.ensemble_forecast(T0, **kw)
    monkeypatch.setattr(native, "check", spy)
    gm.ensemble_forecast(T0, **kw)
    monkeypatch.undo()
    return seen


@pytest.mark.parametrize("case", sorted(LAUNCH_REQUESTS))
def test_launch_sequence_is_the_recorded_one(pangu, monkeypatch, case):
    """The driver is host code around fixed launches: which entry points it calls, and in which order, is
    ``golden/ens_launch_sequence.json``, recorded with ``launch_sequence`` before the driver was rebuilt around its plan, member source,
    families and consumers.  A reordering of consumers, a launch made twice or one left out shows here by name."""
    import json
    want = json.loads(LAUNCH_GOLDEN.read_text())[case]
    got = launch_sequence(monkeypatch, pangu, **LAUNCH_REQUESTS[case])
    first = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
    assert got == want, f"request {case}: {len(got)} calls for {len(want)} recorded; first difference at call {first}: {got[first:first + 3]} for {want[first:first + 3]}"


def test_ensemble_command_line(tmp_path):
    from click.testing import CliRunner
    from skyrim_amd.ensemble_cli import ensemble
    res = CliRunner().invoke(ensemble, ["-m", "pangu", "-n", "3", "-l", "12", "-o", str(tmp_path), "-d", "20240513", "-t", "1800"])
    assert res.exit_code == 0, res.output + repr(res.exception)
    paths = [ln for ln in res.output.splitlines() if ln.endswith(".nc")]
    assert len(paths) == 4 and all(Path(p).exists() for p in paths)
    names = sorted(Path(p).name.split("__")[0] for p in paths)
    assert names == ["pangu-ens3-mean"] * 2 + ["pangu-ens3-spread"] * 2
