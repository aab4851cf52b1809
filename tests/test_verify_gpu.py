"""Forecast verification end to end on the MI355X: ``verify`` on Pangu at 49 x 192 and on FuXi at its toy size (two history levels,
the cascade), ``ensemble_forecast(scores=True)`` against the float64 restatement on the kept members, ``score_prediction`` on saved
files, the refusals that name the other route, and the ``verify`` command."""
from __future__ import annotations

import datetime
import json
from pathlib import Path

import numpy as np
import pytest

import _score_reference as R
from skyrim_amd import verify as V

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


def _against_restatement(scores, members, truth_at, clim_at, what, lat):
    """scores.sums against R.scores on ``members`` (M, T, C, H, W) and truth_at(time) / clim_at(time) (C, H, W): every slot within the
    header's bound; the table is the host's formula of the sums; rank counts exact."""
    M, T = members.shape[:2]
    w = V.area_weights(lat)
    slots = scores.sums.slot.values.tolist()
    worst = 0.0
    for t, time in enumerate(scores.times):
        y = np.asarray(truth_at(time), np.float32)
        c = None if clim_at is None else np.asarray(clim_at(time), np.float32)
        val, bound, counts = R.scores(members[:, t], y, w, c)
        for k, name in enumerate(slots):
            err = np.abs(scores.sums.values[k, t] - val[name])
            share = np.where(bound[name] > 0, err / np.where(bound[name] > 0, bound[name], 1), np.where(err == 0, 0, np.inf))
            worst = max(worst, float(share.max()))
        if M > 1:
            assert np.array_equal(scores.rank_counts.values[t], counts.sum(axis=1))
            assert np.allclose(scores.rank_histogram.values[t], R.rank_frequencies(counts, w, members.shape[-1]), rtol=0, atol=1e-14)
            assert np.all(np.abs(scores.rank_histogram.values[t].sum(axis=-1) - 1) <= 1e-12)
        ref = R.table({n: scores.sums.values[k, t] for k, n in enumerate(slots)}, M)
        for name in scores.table.metric.values.tolist():
            assert np.array_equal(scores.metric(name)[t], ref[name], equal_nan=True), name
    print(f"{what}: worst share of the bound {worst:.3f}")
    assert worst <= 1, what


def _end_to_end(m, tmp_path):
    names = list(m.out_channel_names)
    lat = np.asarray(m.model.grid.lat)
    before = m.forecast(T0, n_steps=3)
    vals = np.array(before.values)
    src = m.data_source
    order = [list(src.channel_names).index(n) for n in names]
    truth_at = lambda time: np.asarray(src[time])[order]       # noqa: E731
    s = m.verify(T0, n_steps=3)
    assert s.n_members == 1 and s.channels == names and len(s.times) == 4 \
        and [np.datetime64(t, "s") for t in s.times] == list(np.asarray(before.time.values).astype("datetime64[s]"))
    assert s.table.metric.values.tolist() == ["bias", "mae", "rmse", "crps"] and s.rank_histogram is None
    assert np.all(s.sums.values[:, 0] == 0)                                            # lead 0: the truth source is the IC source
    assert np.array_equal(s.metric("crps"), s.metric("mae")) and np.all(s.metric("rmse")[1:] > 0)
    _against_restatement(s, vals[None], truth_at, None, f"{m.model_name} verify", lat)
    assert np.array_equal(np.asarray(m.forecast(T0, n_steps=3).values), vals)          # forecast() after verify(): the bits it gave before
    # the forecast's own DataArray as the truth: exactly 0; a climatology = truth + a constant: ACC defined
    own = m.verify(T0, n_steps=3, truth=before)
    assert np.all(own.metric("rmse") == 0) and np.all(own.metric("crps") == 0)
    clim = before.copy()
    clim.values = clim.values - np.float32(2.0)
    sc = m.verify(T0, n_steps=3, climatology=clim, channels=names[:2])
    assert sc.channels == names[:2] and "acc" in sc.table.metric.values.tolist() and np.isfinite(sc.metric("acc")).all()
    _against_restatement(sc, vals[None][:, :, :2], lambda t: truth_at(t)[:2],
                         lambda t: clim.values[list(sc.times).index(t), :2], f"{m.model_name} verify with a climatology", lat)
    # the ensemble: scores=False changes nothing; scores=True matches the restatement on the kept members
    kw = dict(n_steps=3, n_members=5, keep_members=True, products=("mean", "spread"))
    plain = m.ensemble_forecast(T0, **kw)
    ens = m.ensemble_forecast(T0, scores=True, **kw)
    assert plain.scores is None and np.array_equal(plain.mean.values, ens.mean.values) and np.array_equal(plain.spread.values, ens.spread.values)
    es = ens.scores
    assert es.n_members == 5 and set(es.table.metric.values.tolist()) == {"bias", "mae", "rmse", "crps", "spread", "ssr"}
    assert es.rank_histogram.dims == ("time", "channel", "rank") and es.rank_histogram.shape == (4, len(names), 6)
    _against_restatement(es, np.asarray(ens.members.values), truth_at, None, f"{m.model_name} ensemble scores", lat)
    assert np.array_equal(np.asarray(m.forecast(T0, n_steps=3).values), vals)
    # forecasts already on disk: the table verify gave
    for file_type in ("netcdf", "zarr"):
        cfg = {"output_dir": str(tmp_path / file_type), "file_type": file_type}
        _, paths = m.rollout(T0, n_steps=3, save=True, save_config=cfg)
        sp = V.score_prediction([paths[-1]] if file_type == "zarr" else list(paths), src, device=DEV)
        assert sp.times == s.times and sp.channels == names
        _against_restatement(sp, vals[None], truth_at, None, f"{m.model_name} score_prediction on {file_type}", lat)
        assert np.allclose(sp.table.values, s.table.values, rtol=1e-5, atol=0, equal_nan=True)


def test_pangu_toy_end_to_end(pangu, tmp_path):
    _end_to_end(pangu, tmp_path)


def test_fuxi_toy_end_to_end(fuxi, tmp_path):
    _end_to_end(fuxi, tmp_path)


def test_graphcast_names_the_other_route():
    from skyrim_amd.core.models.graphcast import GraphcastModel
    with pytest.raises(NotImplementedError, match="score_prediction"):
        GraphcastModel.verify(object.__new__(GraphcastModel), T0)


def test_verify_command_line(tmp_path):
    from click.testing import CliRunner
    from skyrim_amd.verify_cli import verify
    for extra, name in (([], "pangu-scores.json"), (["-n", "3"], "pangu-ens3-scores.json")):
        res = CliRunner().invoke(verify, ["-m", "pangu", "-l", "12", "-o", str(tmp_path), "-d", "20240513", "-t", "1800"] + extra)
        assert res.exit_code == 0, res.output + repr(res.exception)
        path = [ln for ln in res.output.splitlines() if ln.endswith(".json")]
        assert len(path) == 1 and Path(path[0]).name == name and Path(path[0]).exists()
        doc = json.loads(Path(path[0]).read_text())
        assert len(doc["times"]) == 3 and np.asarray(doc["table"]).shape[1] == 3           # n_steps + 1 lead times
        assert sum(ln.startswith("+") for ln in res.output.splitlines()) == 3 * 4           # z500, t850, t2m, u10m at three lead times
