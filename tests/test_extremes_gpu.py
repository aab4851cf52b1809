"""Climate-relative extremes end to end on the MI355X with the Pangu toy model (49 x 192): ``ensemble_forecast(extremes={...})`` against
the stand-alone op on the kept members (bit for bit, each lead with the climate slice of its valid time, each window with that of its
end), the same request without ``extremes=``, ``extremes_forecast`` against ``extremes_prediction`` on the files of the same rollout,
the command line's ``build`` then ``apply``, and the files of ``save=True``."""
from __future__ import annotations

import datetime

import numpy as np
import pytest
import torch

from skyrim_amd import climate as K
from skyrim_amd import extremes as X
from skyrim_amd.members import member_table
from skyrim_amd.ops import hip

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T0 = datetime.datetime(2024, 5, 13, 18, 0)
H6 = datetime.timedelta(hours=6)
LEVELS = [0.0, 0.01, 0.05, 0.1, 0.25, 0.5, 0.75, 0.9, 0.95, 0.99, 1.0]
FIELDS = ["t2m", "ws10m", "ws10m_max_12h"]
KW = dict(n_steps=5, n_members=3, keep_members=True, products=("mean", "spread"), perturb_scale=0.05, derived=["ws10m"],
          aggregates=["ws10m:max:12h"])
ASK = dict(fields=FIELDS, efi=True, sot=[0.9, 0.1], above=[0.95], below=[0.05], floor={"ws10m": 0.5})


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def pangu(toy):
    from skyrim_amd.core.models.pangu import PanguModel
    g, params, _ = toy
    return PanguModel(ic_source="gfs", geom=g, params=params)


@pytest.fixture(scope="module")
def plain(pangu):
    """The request without ``extremes=``: computed once, shared, left unchanged."""
    return pangu.ensemble_forecast(T0, **KW)


@pytest.fixture(scope="module")
def clim(pangu, plain):
    """A climate of synthetic planes around the forecast's own first state, one slice per (day, hour) of the rollout, each shifted by its
    own amount so that a wrong slice shows."""
    lat, lon = np.asarray(pangu.model.grid.lat), np.asarray(pangu.model.grid.lon)
    names = plain.mean.channel.values.tolist()
    base = np.stack([np.asarray(plain.mean.values)[0, names.index("t2m")], np.asarray(plain.derived.mean.values)[0, 0],
                     np.asarray(plain.derived.mean.values)[0, 0]])
    z = np.array([-3.0, -2.3, -1.6, -1.3, -0.7, 0.0, 0.7, 1.3, 1.6, 2.3, 3.0], np.float32)
    scale = np.array([1.5, 1.0, 1.0], np.float32)
    slices = {}
    for n, (day, hour) in enumerate([(13, 18), (14, 0), (14, 6), (14, 12), (14, 18), (15, 0)]):
        slices[(5, day, hour)] = (base[None] + z[:, None, None, None] * scale[None, :, None, None] + np.float32(0.05 * n)).astype(np.float32)
    return K.Climate(LEVELS, FIELDS, lat, lon, slices, n_samples=0, half_window_days=0)


def standalone(members, channel, plane, M=3, floor=-np.inf):
    """The op on host members (M, H, W) of one field against one climate plane set (Q, H, W): dict of arrays."""
    st = [torch.from_numpy(np.ascontiguousarray(members[m][None])).to(DEV) for m in range(M)]
    H, W = members.shape[1:]
    cl = torch.from_numpy(np.ascontiguousarray(plane[None])).to(DEV)
    sot = [K.sot_request(LEVELS, q, M) for q in ASK["sot"]] if M > 1 else []
    prob = [(K.level_index(LEVELS, 0.95, "t"), False), (K.level_index(LEVELS, 0.05, "t"), True)]
    efi, so, pr = (torch.empty(s, device=DEV) for s in ((1, H, W), (len(sot), 1, H, W), (2, 1, H, W)))
    hip.clim_extremes(st, member_table(st), [0], cl, LEVELS, [float(floor)], [r[0] for r in sot], [float(r[1]) for r in sot],
                      [r[2] for r in sot], [r[3] for r in sot], [r[0] for r in prob], [r[1] for r in prob], efi, so if sot else None, pr)
    return dict(efi=efi[0].cpu().numpy(), sot=so[:, 0].cpu().numpy(), prob=pr[:, 0].cpu().numpy())


def check_family(ex, members, field, fi, times, clim, floor=-np.inf):
    """``ex`` (an Extremes) at field index ``fi`` equals the stand-alone op on ``members`` (M, T, H, W), each time with its own slice."""
    for ti, t in enumerate(times):
        key, arr = clim.at(t)
        assert ex.keys[ti] == key
        want = standalone(members[:, ti], field, arr[:, clim.fields.index(field)], floor=floor)
        assert np.array_equal(bits(ex.efi.values[ti, fi]), bits(want["efi"])), (field, ti)
        for s, q in enumerate(ASK["sot"]):
            assert np.array_equal(bits(ex.sot[q].values[ti, fi]), bits(want["sot"][s])), (field, ti, q)
        assert np.array_equal(bits(ex.probability(field, "above", 0.95).values[ti]), bits(want["prob"][0]))
        assert np.array_equal(bits(ex.probability(field, "below", 0.05).values[ti]), bits(want["prob"][1]))


def test_ensemble_extremes_equal_the_op_on_the_members(pangu, plain, clim):
    ens = pangu.ensemble_forecast(T0, extremes=dict(ASK, climate=clim), **KW)
    # every existing product: bit for bit what it was
    for p in ("mean", "spread", "members"):
        assert np.array_equal(bits(getattr(plain, p).values), bits(getattr(ens, p).values)), p
        assert np.array_equal(bits(getattr(plain.derived, p).values), bits(getattr(ens.derived, p).values)), p
        assert np.array_equal(bits(getattr(plain.aggregated["12h"], p).values), bits(getattr(ens.aggregated["12h"], p).values)), p
    assert plain.extremes is None and plain.aggregated["12h"].extremes is None
    names = ens.members.channel.values.tolist()
    times = [T0 + k * H6 for k in range(6)]
    ex = ens.extremes
    assert ex.fields == ["t2m", "ws10m"] and ex.efi.shape == (6, 2, 49, 192)
    assert ex.keys == [(5, 13, 18), (5, 14, 0), (5, 14, 6), (5, 14, 12), (5, 14, 18), (5, 15, 0)]
    check_family(ex, np.asarray(ens.members.values)[:, :, names.index("t2m")], "t2m", 0, times, clim)
    check_family(ex, np.asarray(ens.derived.members.values)[:, :, 0], "ws10m", 1, times, clim, floor=0.5)
    ag = ens.aggregated["12h"]
    ends = [T0 + 2 * H6, T0 + 4 * H6]                                   # the windows' ends choose the slices
    assert ag.extremes.fields == ["ws10m_max_12h"] and ag.extremes.keys == [(5, 14, 6), (5, 14, 18)]
    check_family(ag.extremes, np.asarray(ag.members.values)[:, :, 0], "ws10m_max_12h", 0, ends, clim)
    assert np.isfinite(ex.efi.values).all() and np.abs(ex.efi.values).max() <= 1


def test_extremes_add_only_their_own_launches(pangu, clim, monkeypatch):
    from skyrim_amd import native
    kw = dict(KW, n_steps=2)

    def sequence(**more):
        real, seen = native.check, []
        monkeypatch.setattr(native, "check", lambda code, what, lib=None: (seen.append(what), real(code, what, lib))[1])
        pangu.ensemble_forecast(T0, **kw, **more)
        monkeypatch.undo()
        return seen
    without, with_x = sequence(), sequence(extremes=dict(ASK, climate=clim))
    assert "skclim_extremes" not in without and with_x.count("skclim_extremes") == 3 + 3 + 1      # raw and derived at 3 leads, one window
    assert [w for w in with_x if w != "skclim_extremes"] == without


def test_extremes_forecast_equals_extremes_prediction_on_saved_files(pangu, clim, tmp_path):
    ask = dict(climate=clim, fields=["t2m", "ws10m"], above=[0.95], below=[0.05], floor={"ws10m": 0.5})
    live = pangu.extremes_forecast(T0, 3, ask, derived=["ws10m"])
    assert live.fields == ["t2m", "ws10m"] and live.efi.shape == (4, 2, 49, 192) and live.sot == {}
    assert set(np.unique(live.probability("t2m", "above", 0.95).values).tolist()) <= {0.0, 1.0}
    with pytest.raises(ValueError, match="one state has none"):
        pangu.extremes_forecast(T0, 1, dict(ask, sot=[0.9]), derived=["ws10m"])
    _, paths = pangu.rollout(T0, n_steps=3, save=True, save_config={"output_dir": str(tmp_path)})
    disk = X.extremes_prediction(list(paths), ask, derived=["ws10m"], device=DEV)
    assert disk.keys == live.keys
    for stem, da in live.arrays().items():
        assert np.array_equal(bits(disk.arrays()[stem].values), bits(da.values)), stem


def test_command_line_build_then_apply(pangu, tmp_path):
    from click.testing import CliRunner
    from skyrim_amd.extremes_cli import extremes
    from skyrim_amd.labeled import open_dataarray
    _, paths = pangu.rollout(T0, n_steps=3, save=True, save_config={"output_dir": str(tmp_path / "fc")})
    cdir, odir = str(tmp_path / "clim"), str(tmp_path / "out")
    res = CliRunner().invoke(extremes, ["build", *paths, "-f", "t2m", "-f", "ws10m", "--derived", "ws10m", "--half_window_days", "2",
                                        "--levels", "11", "-o", cdir])
    assert res.exit_code == 0, res.output + repr(res.exception)
    c = K.Climate.open(cdir)
    assert c.fields == ["t2m", "ws10m"] and c.levels.size == 11 and sorted(c.slices) == [(5, 13, None), (5, 14, None)] and c.n_samples == 4
    res = CliRunner().invoke(extremes, ["apply", *paths, "--climate", cdir, "--derived", "ws10m", "--above", "0.9", "-o", odir])
    assert res.exit_code == 0, res.output + repr(res.exception)
    files = [ln for ln in res.output.splitlines() if ln.endswith(".nc")]
    assert len(files) == 2
    want = X.extremes_prediction(list(paths), dict(climate=c, above=[0.9]), derived=["ws10m"], device=DEV)
    for f, stem in zip(files, ("efi", "pabove0.9")):
        assert f.endswith(f"{stem}.nc")
        assert np.array_equal(bits(open_dataarray(f).values), bits(want.arrays()[stem].values)), stem
    assert np.isfinite(want.efi.values).all() and np.abs(want.efi.values).max() <= 1


def test_ensemble_save_writes_the_extremes_under_the_forecast_id(pangu, clim, tmp_path):
    """``save=True``: the results go where ``objects`` and ``points`` write theirs, ``{output_dir}/{forecast id}/``, the saved leads' and
    each window group's (two windows here, whose ``window_start`` coordinate is not a dimension of the file)."""
    from pathlib import Path
    from skyrim_amd.labeled import open_dataarray
    ens = pangu.ensemble_forecast(T0, extremes=dict(ASK, climate=clim), save=True, save_config={"output_dir": str(tmp_path)}, **dict(KW, n_steps=4))
    d = tmp_path / ens.forecast_id / "extremes"
    assert ens.paths.count(str(d)) == 2 and ens.extremes.path == str(d) == ens.aggregated["12h"].extremes.path
    stems = ["efi", "sot0.9", "sot0.1", "pabove0.95", "pbelow0.05"]
    assert sorted(p.name for p in d.iterdir()) == sorted([f"pangu-ens3-{s}.nc" for s in stems] + [f"pangu-ens3-agg12h-{s}.nc" for s in stems])
    for label, ex in (("pangu-ens3", ens.extremes), ("pangu-ens3-agg12h", ens.aggregated["12h"].extremes)):
        for stem, da in ex.arrays().items():
            back = open_dataarray(d / f"{label}-{stem}.nc")
            assert tuple(back.dims) == ("time", "field", "lat", "lon") and back._coords["field"].tolist() == ex.fields
            assert np.array_equal(bits(back.values), bits(da.values)), (label, stem)
    assert ens.aggregated["12h"].extremes.efi.shape[0] == 2 and all(Path(p).exists() for p in ens.paths)
