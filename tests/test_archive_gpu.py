"""Member archives end to end on the MI355X with the Pangu toy model (49 x 192, 3 members, 3 steps): ``ensemble_forecast(archive={...})``
leaves every product as it was; a ``float32`` archive holds the live members bit for bit and replays to bit-equal products; an ``int16``
archive holds the bytes the numpy restatement makes of the live members, and its replay works on exactly their decoded values; the
``channels=`` subset; the command line; and no ``.part`` file after a stage raises."""
from __future__ import annotations

import datetime
import json
from pathlib import Path

import numpy as np
import pytest
import torch

import _pack_reference as R
from skyrim_amd import archive as A
from skyrim_amd.members import member_table
from skyrim_amd.ops import hip

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T0 = datetime.datetime(2024, 5, 13, 18, 0)
H6 = datetime.timedelta(hours=6)
POINTS = {"reykjavik": (64.1, 338.1), "quito": (-0.2, 281.5)}
KW = dict(n_steps=3, n_members=3, keep_members=True, products=("mean", "spread"), perturb_scale=0.05, exceed={"t2m": [280.0]},
          quantiles={"t2m": [0.5]}, derived=["ws10m"], points=POINTS, aggregates=["t2m:max:12h"])
SUBSET = ["msl", "t2m", "u10m", "v10m"]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(a, b):
    return np.array_equal(bits(a.values), bits(b.values))


@pytest.fixture(scope="module")
def pangu(toy):
    from skyrim_amd.core.models.pangu import PanguModel
    g, params, _ = toy
    return PanguModel(ic_source="gfs", geom=g, params=params)


@pytest.fixture(scope="module")
def plain(pangu):
    """The request without ``archive=``: computed once, shared, left unchanged."""
    return pangu.ensemble_forecast(T0, **KW)


@pytest.fixture(scope="module")
def lossless(pangu, tmp_path_factory):
    d = tmp_path_factory.mktemp("f32")
    return pangu.ensemble_forecast(T0, archive=dict(packing="float32", dir=str(d)), **KW), d


@pytest.fixture(scope="module")
def packed(pangu, tmp_path_factory):
    out = tmp_path_factory.mktemp("i16")
    cfg = dict(output_dir=str(out))
    return pangu.ensemble_forecast(T0, archive=dict(packing="int16"), save=True, save_config=cfg, **KW), out, cfg


def products_equal(a, b):
    for p in ("mean", "spread", "members"):
        assert same(getattr(a, p), getattr(b, p)), p
        assert same(getattr(a.derived, p), getattr(b.derived, p)), p
        assert same(getattr(a.aggregated["12h"], p), getattr(b.aggregated["12h"], p)), p
    assert same(a.exceedance["t2m"], b.exceedance["t2m"]) and same(a.quantile["t2m"], b.quantile["t2m"])
    assert same(a.points.values, b.points.values)


def test_every_product_is_what_it_was_without_the_archive(plain, lossless, packed):
    assert plain.archive is None
    for ens in (lossless[0], packed[0]):
        products_equal(plain, ens)
        assert isinstance(ens.archive, A.MemberArchive) and set(ens.archive.paths) <= set(ens.paths)


def test_float32_files_hold_the_live_members_bit_for_bit(plain, lossless, pangu):
    ens, d = lossless
    arch = ens.archive
    names = plain.members.channel.values.tolist()
    assert arch.dir == Path(d) and arch.packing == "float32" and arch.channels == names and arch.leads == [0, 1, 2, 3] and arch.M == 3
    assert sorted(p.name for p in Path(d).iterdir()) == sorted([A.MANIFEST] + [Path(p).name for p in arch.paths]) and len(arch.paths) == 12
    assert Path(arch.path(2, 1)).name == f"pangu-ens3-m002__{pangu.source_label}__{T0:%Y%m%d_%H:%M}__{T0 + H6:%Y%m%d_%H:%M}.nc"
    manifest = json.loads((Path(d) / A.MANIFEST).read_text())
    assert manifest["seed"] == 0 and manifest["perturbation"] == "white" and manifest["n_bad"] is None and manifest["time_step_s"] == 21600.0
    live = np.asarray(plain.members.values)
    for k in range(4):
        for m in range(3):
            da = arch.member(m, k)
            assert da.time.values[0] == np.datetime64(T0 + k * H6) and np.array_equal(bits(da.values[0]), bits(live[m, k]))
        time, states = arch.states(k, DEV)
        assert time == T0 + k * H6 and all(np.array_equal(bits(s.cpu().numpy()), bits(live[m, k])) for m, s in enumerate(states))


def test_float32_replay_is_bit_equal(plain, lossless, pangu):
    truth = plain.members.isel(member=0)
    again = pangu.ensemble_forecast(T0, scores=True, truth=truth, **KW)
    rep = lossless[0].archive.replay(scores=True, truth=truth, **{k: v for k, v in KW.items() if k not in ("n_steps", "n_members", "perturb_scale")})
    products_equal(again, rep)
    assert np.array_equal(np.asarray(again.scores.sums.values), np.asarray(rep.scores.sums.values))
    assert np.array_equal(np.asarray(again.derived.scores.sums.values), np.asarray(rep.derived.scores.sums.values))
    assert rep.n_members == 3 and rep.model_name == "pangu" and rep.archive is None


def test_replay_runs_the_stages_that_need_every_lead(lossless, pangu):
    """Tracks (every lead from 0) and spectra from the archive equal those of the live forecast: the stand-in for the model carries all
    the stages read of one."""
    extra = dict(tracks=True, track_config=dict(lat_max=60.0, r_msl_km=1700.0, r_vort_km=1000.0, r_wind_km=1300.0, r_core_km=1100.0),      # radii for 3.75 degrees
                 spectra={"channels": ["z500"]})
    live = pangu.ensemble_forecast(T0, n_steps=3, n_members=3, perturb_scale=0.05, products=("mean",), **extra)
    rep = lossless[0].archive.replay(products=("mean",), **extra)
    assert same(live.mean, rep.mean) and len(live.tracks) == len(rep.tracks)
    assert np.array_equal(np.asarray(live.spectra.power.values), np.asarray(rep.spectra.power.values), equal_nan=True)


def test_int16_files_equal_the_reference_and_replay_works_on_their_decoded_values(plain, packed):
    ens, out, cfg = packed
    arch = ens.archive
    names = plain.members.channel.values.tolist()
    assert arch.dir == Path(out) / cfg["forecast_id"] / "members" and arch.packing == "int16" and arch.channels == names
    live = np.asarray(plain.members.values)                 # (member, time, channel, lat, lon)
    C, H, W = live.shape[2:]
    manifest, decoded = arch.manifest, np.empty_like(live)
    for k in range(4):
        states = [live[m, k] for m in range(3)]
        tab = R.table(states, range(C))
        for m, img in enumerate(R.quantize(states, range(C), tab)):
            raw = Path(arch.path(m, k)).read_bytes()
            assert img in raw and len(raw) < len(img) + 16384
            assert manifest["n_bad"][k][m] == [0] * C
            decoded[m, k] = R.unpack(img, tab[m], (C, H, W))
            assert np.array_equal(bits(arch.member(m, k).values[0]), bits(decoded[m, k]))
            err = np.abs(decoded[m, k].astype(np.float64) - live[m, k].astype(np.float64))
            assert all((err[c] <= R.bound(err[c], tab[m, c])).all() for c in range(C))      # the header's bound, on a real state
    assert not list(arch.dir.glob("*.part"))
    rep = arch.replay(keep_members=True, products=("mean",))
    assert np.array_equal(bits(rep.members.values), bits(decoded))
    st = [torch.from_numpy(decoded[m, 2]).to(DEV) for m in range(3)]
    mean = torch.empty_like(st[0])
    hip.ens_stats(st, member_table(st), 0, st[0].numel(), mean, None, None, None, None, [], None, [])
    assert np.array_equal(bits(rep.mean.values[2]), bits(mean.cpu().numpy()))


def test_channel_subset_and_the_refusal_of_a_product_outside_it(plain, pangu, tmp_path):
    ens = pangu.ensemble_forecast(T0, n_steps=1, n_members=3, perturb_scale=0.05, products=("mean",),
                                  archive=dict(packing="int16", channels=SUBSET, dir=str(tmp_path)))
    arch = A.open(tmp_path)
    names = plain.members.channel.values.tolist()
    assert arch.channels == SUBSET and arch.leads == [0, 1] and ens.archive.paths == arch.paths and ens.paths == arch.paths      # (no save=: nothing else)
    live = np.asarray(plain.members.values)[:, :2][:, :, [names.index(c) for c in SUBSET]]
    for k in range(2):
        states = [live[m, k] for m in range(3)]
        tab = R.table(states, range(len(SUBSET)))
        for m, img in enumerate(R.quantize(states, range(len(SUBSET)), tab)):
            assert img in Path(arch.path(m, k)).read_bytes()
    rep = arch.replay(derived=["ws10m"], exceed={"t2m": [280.0]}, channels=["t2m"])
    assert rep.mean.channel.values.tolist() == ["t2m"] and rep.derived.mean.shape == (2, 1, 49, 192) and rep.exceedance["t2m"].shape == (2, 1, 49, 192)
    with pytest.raises(ValueError, match="'z500' is not an output channel"):
        arch.replay(exceed={"z500": [5500.0]})
    with pytest.raises(ValueError, match="packing = 'int12'"):
        pangu.ensemble_forecast(T0, n_steps=1, n_members=2, archive=dict(packing="int12", dir=str(tmp_path)))


def test_info_and_replay_from_the_command_line(packed, tmp_path):
    from click.testing import CliRunner
    from skyrim_amd import archive_cli
    arch = packed[0].archive
    res = CliRunner().invoke(archive_cli.archive, ["info", str(arch.dir)])
    assert res.exit_code == 0, res.output
    info = json.loads(res.output)
    assert info["packing"] == "int16" and info["n_members"] == 3 and info["leads"] == [0, 1, 2, 3] and info["n_bad"] == 0
    res = CliRunner().invoke(archive_cli.archive, ["replay", str(arch.dir), "-p", "mean", "-x", "t2m=280", "-o", str(tmp_path)])
    assert res.exit_code == 0, res.output
    files = res.output.split()
    assert len(files) == 3 and all(Path(f).exists() and "pangu-ens3-mean" in f for f in files)
    res = CliRunner().invoke(archive_cli.archive, ["replay", str(arch.dir), "-x", "nope=1"])
    assert res.exit_code == 2 and "not an output channel" in res.output


def test_no_part_file_is_left_after_a_stage_raises(pangu, tmp_path, monkeypatch):
    """A host stage behind the archive raises at the second lead, while files are being written: the error comes out, the save threads
    end, and the directory holds whole files only."""
    from skyrim_amd import points as P

    calls = []

    def failing(self, *a, **k):
        calls.append(1)
        if len(calls) == 2:
            raise RuntimeError("the station list went away")
    monkeypatch.setattr(P.LeadPoints, "add", failing)
    with pytest.raises(RuntimeError, match="station list"):
        pangu.ensemble_forecast(T0, n_steps=3, n_members=3, perturb_scale=0.05, points=POINTS, archive=dict(packing="int16", dir=str(tmp_path)))
    left = sorted(p.name for p in tmp_path.iterdir())
    assert len(left) == 6 and all(n.endswith(".nc") for n in left)      # the two leads that were packed, no manifest, no .part
    import threading
    assert not [t for t in threading.enumerate() if t.name.startswith("skyrim-archive")]
