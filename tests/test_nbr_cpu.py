"""Neighbourhood fields without a GPU (skyrim_amd/neighbourhood.py, include/skyrim_nbr.h): the disc tables against a brute-force builder that
tests every pair of nodes, their symmetry and the whole sphere, the grammar and every refusal of the request, where the fields' names
route in the ensemble's plan, the build entries, the descriptor's layout against the header, and every argument error of the library."""
from __future__ import annotations

import ctypes
import inspect
import re
import shutil
import subprocess
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

import _nbr_reference as R
from skyrim_amd import ensemble, native
from skyrim_amd import neighbourhood as N
from skyrim_amd.tracks import EARTH_RADIUS_KM

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "skyrim_nbr.h"
GRIDS = [(9, 12, True), (7, 15, True), (33, 64, True), (32, 64, False)]


def radii_of(lat, lon):
    """Below the smallest step between two nodes off the poles, about 1.5 and about 4 row steps, and the whole sphere."""
    dphi = np.deg2rad(abs(lat[1] - lat[0])) * EARTH_RADIUS_KM
    off_pole = np.abs(lat) < 90
    dlam = EARTH_RADIUS_KM * np.cos(np.deg2rad(lat[off_pole])).min() * np.deg2rad(360.0 / lon.size)
    return [0.5 * min(dphi, dlam), 1.53 * dphi, 4.07 * dphi, 25000.0]


# ---- 1. the disc ------------------------------------------------------------------------------------------------------------------------ #
@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: f"{g[0]}x{g[1]}")
def test_discs_are_the_brute_force_sets(grid):
    H, W, south = grid
    lat, lon = R.grid(H, W, south)
    dist = R.pair_distances(lat, lon)
    for k, radius in enumerate(radii_of(lat, lon)):
        assert not (np.abs(dist - radius) <= 1e-9 * radius).any(), "a pair of nodes lies on the rim: the comparison would test rounding"
        reach, half = N.discs(lat, lon, radius)
        assert half.dtype == np.int32 and half.shape == (H, 2 * reach + 1) and half.max() <= W // 2
        assert (half[:, 0] >= 0).any() or (half[:, -1] >= 0).any(), "reach is the largest |d| used"
        S = R.table_sets(reach, half, W)
        assert np.array_equal(S, dist <= radius), f"radius {radius:.1f} km"
        assert np.array_equal(S, S.transpose(2, 3, 0, 1)), "(r, c) in S(j, i) <=> (j, i) in S(r, c)"
        assert np.array_equal(N.disc_points(half, W), S.reshape(H, W, -1).sum(axis=2)[:, 0])
        pole = np.abs(lat) == 90
        if k == 0:                                               # the point itself; on a pole row the whole row, which is one place
            own = np.zeros((H, W, H, W), bool)
            for j in range(H):
                for i in range(W):
                    own[j, i, j, :] = True if pole[j] else (np.arange(W) == i)
            assert reach == 0 and np.array_equal(S, own)
        if k == 3:                                               # the whole sphere: every node once in every disc
            assert S.all() and (N.disc_points(half, W) == H * W).all() and reach == H - 1


def test_discs_refuse_what_is_no_global_grid():
    lat, lon = R.grid(9, 12)
    for bad_lon, why in ((lon[:-1], "closes the circle"), (lon * np.linspace(1, 1.01, 12), "closes the circle"), (np.zeros(12), "closes the circle")):
        with pytest.raises(ValueError, match=why):
            N.discs(lat, bad_lon, 500.0)
    for bad_lat in (np.array([90, 45, 45, 0.0]), np.array([0, 45, 30.0]), np.array([95, 0.0])):
        with pytest.raises(ValueError, match="monotonic|within"):
            N.discs(bad_lat, lon, 500.0)
    for bad_r in (0.0, -5.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="finite and positive"):
            N.discs(lat, lon, bad_r)


# ---- 2. requests ------------------------------------------------------------------------------------------------------------------------ #
def test_request_grammar_and_names():
    r = N.parse_request("ws10m:max:100km")
    assert r == N.Request("ws10m", "max", "100km") and r.name == "ws10m_max_100km" and r.km == 100
    assert N.parse_request(" t2m : frac_above@303.15 : 50km ").name == "t2m_frac_above@303.15_50km"
    assert N.parse_request(SimpleNamespace(channel="msl", stat="mean", radius="200km")) == N.Request("msl", "mean", "200km")
    assert N.parse_request("t2m:frac_above@inf:5km") and N.parse_request("t2m:frac_above@-inf:5km")
    assert N.op_of(N.parse_request("t2m:frac_above@303.15:50km"), 2, 5, 1) == N.Op(N.FRAC_ABOVE, 2, 5, 1, float(np.float32(303.15)))
    assert N.op_of(N.parse_request("t2m:min:50km"), 2, 5, 1) == N.Op(N.MIN, 2, 5, 1, 0.0)
    for bad, why in (("ws10m:max", "channel:stat:radius"), ("ws10m:max:100km:x", "channel:stat:radius"), (":max:100km", "empty"),
                     ("t2m:median:100km", "unknown statistic"), ("t2m:gauss:100km", "Gaussian"), ("t2m:frac_above@nan:100km", "needs a number"),
                     ("t2m:frac_above@:100km", "needs a number"), ("t2m:max:100", "<N>km"), ("t2m:max:0km", "<N>km"), ("t2m:max:1.5km", "<N>km"),
                     ("t2m:max:-3km", "<N>km"), (42, "a string")):
        with pytest.raises(ValueError, match=why):
            N.parse_request(bad)


def test_encode_decode_round_trip():
    ops = [N.Op(N.MAX, 3, 0, 2), N.Op(N.FRAC_ABOVE, 0, 2, 1, float("-inf")), N.Op(N.MEAN, 1, 1), N.Op(N.MIN, 2, 3, 3)]
    assert N.decode(*N.encode(ops)) == ops
    for ints, floats in (([1, 0, 0], [0.0]), ([1, 0, 0, 0], []), ([9, 0, 0, 0], [0.0])):
        with pytest.raises(ValueError, match="nbr_fields"):
            N.decode(ints, floats)


def test_check_request_refuses_before_the_device():
    lat, lon = R.grid(33, 64)
    names = ["u10m", "v10m", "t2m"]
    p = N.check_request(names, ["ws10m:max:700km", "t2m:frac_above@300:700km", "t2m:mean:2000km"], lat, lon, 3, ["ws10m"])
    assert p.fields == ["ws10m_max_700km", "t2m_frac_above@300_700km", "t2m_mean_2000km"] and p.radii == [700, 2000] and p.D == 3
    assert p.ops == [N.Op(N.MAX, 3, 0, 0), N.Op(N.FRAC_ABOVE, 2, 1, 0, 300.0), N.Op(N.MEAN, 2, 2, 1)]
    assert [h.shape for h in p.half] == [(33, 2 * r + 1) for r in p.reach] and p.weights.shape == (33,) and p.weights.dtype == np.float64
    ok = ["t2m:max:700km"]
    for reqs, why in (("t2m:max:700km", "a list of requests"), ([], "at least one"), (["t2m:max:700km", "t2m:max:700km"], "requested twice"),
                      (["ws10m:max:700km"], "not an output channel"), ([f"t2m:frac_above@{k}:700km" for k in range(17)], "17 ops"),
                      ([f"t2m:max:{k}km" for k in (600, 700, 800, 900, 1000)], "5 distinct radii")):
        with pytest.raises(ValueError, match=why):
            N.check_request(names, reqs, lat, lon, 3)
    with pytest.raises(ValueError, match="already channels"):
        N.check_request(names + ["t2m_max_700km"], ok, lat, lon, 3)
    with pytest.raises(ValueError, match="already channels"):
        N.check_request(names, ok, lat, lon, 3, ["t2m_max_700km"])
    with pytest.raises(ValueError, match="already channels"):
        N.check_request(names, ok, lat, lon, 3, (), ["t2m_max_700km"])
    with pytest.raises(ValueError, match="aggregates as input"):
        N.check_request(names, ["t2m_max_24h:max:700km"], lat, lon, 3, (), ["t2m_max_24h"])
    for m in (0, 65):
        with pytest.raises(ValueError, match="1 to 64 members"):
            N.check_request(names, ok, lat, lon, m)
    with pytest.raises(ValueError, match="closes the circle"):
        N.check_request(names, ok, lat, lon[:40], 3)
    with pytest.raises(ValueError, match="closes the circle"):
        N.check_request(names, ok, lat, np.sort(np.random.default_rng(0).uniform(0, 360, 64)), 3)
    with pytest.raises(ValueError, match="strictly monotonic"):
        N.check_request(names, ok, np.r_[lat[:5], lat[4:]], lon, 3)
    wide = np.arange(N.MAX_W + 2) * (360.0 / (N.MAX_W + 2))
    with pytest.raises(ValueError, match="SKNBR_MAX_W"):
        N.check_request(names, ok, lat, wide, 3)
    tall = np.linspace(90, -90, 721)
    with pytest.raises(ValueError, match="SKNBR_MAX_REACH"):
        N.check_request(names, ["t2m:max:5000km"], tall, lon, 3)
    assert N.MAX_W >= 1440 and N.MAX_REACH >= 64 and N.check_request(names, ["t2m:max:25000km"], lat, lon, 1).reach == [32]


class _Loop:
    import datetime as _dt
    import torch as _torch
    from test_ens_cpu import GEOM as _GEOM
    n_history_levels = 1
    time_step = _dt.timedelta(hours=6)
    device = _torch.device("cpu")
    in_channel_names = out_channel_names = ["u10m", "v10m", "t2m"]
    geom = grid = _GEOM
    channel_std = _torch.ones(3)


def _plan(**kw):
    args = dict(n_steps=4, n_members=3, seed=0, products=("mean",), exceed=None, quantiles=None, channels=None, save_every=1, keep_members=False)
    args.update(kw)
    return ensemble.plan_request(_Loop(), **args)


def test_the_fields_route_to_their_family_in_the_plan():
    reqs = ["ws10m:max:1500km", "t2m:frac_above@300:1500km"]
    p = _plan(derived=["ws10m"], neighbourhood=reqs, exceed={"ws10m_max_1500km": [25.0], "t2m": [300.0], "ws10m": [20.0]},
              quantiles={"t2m_frac_above@300_1500km": [0.5]}, events={"ws10m_max_1500km": [25.0]}, scores=True)
    assert p.neighbourhood.fields == ["ws10m_max_1500km", "t2m_frac_above@300_1500km"]
    assert p.exceed == {"derived": {"ws10m": [20.0]}, "nbr": {"ws10m_max_1500km": [25.0]}, "raw": {"t2m": [300.0]}}
    assert p.quantiles["nbr"] == {"t2m_frac_above@300_1500km": [0.5]} and p.events["nbr"] == {"ws10m_max_1500km": [25.0]}
    assert _plan().neighbourhood is None and "nbr" not in _plan(exceed={"t2m": [300.0]}).exceed
    with pytest.raises(ValueError, match="or one of the neighbourhood fields"):
        _plan(neighbourhood=reqs[1:], exceed={"t2m_max_1500km": [1.0]})
    with pytest.raises(ValueError, match="not an output channel"):
        _plan(neighbourhood=reqs)                                  # ws10m without derived=
    with pytest.raises(ValueError, match="aggregates as input"):
        _plan(neighbourhood=["t2m_max_24h:max:1500km"], aggregates=["t2m:max:24h"])
    # out of scope, refused by name
    with pytest.raises(ValueError, match="input to aggregates= are out of scope"):
        _plan(neighbourhood=reqs[1:], aggregates=["t2m_frac_above@300_1500km:max:24h"])
    with pytest.raises(ValueError, match="input to spectra= are out of scope"):
        _plan(neighbourhood=reqs[1:], spectra={"channels": ["t2m_frac_above@300_1500km"]})
    with pytest.raises(ValueError, match="input to scenarios= are out of scope"):
        _plan(neighbourhood=reqs[1:], scenarios={"channels": ["t2m_frac_above@300_1500km"]})
    with pytest.raises(ValueError, match="input to objects= are out of scope"):
        _plan(neighbourhood=reqs[1:], objects={"t2m_frac_above@300_1500km": {"above": [0.5]}})
    with pytest.raises(ValueError, match="input to extremes= are out of scope"):
        _plan(neighbourhood=reqs[1:], extremes={"climate": None, "fields": ["t2m_frac_above@300_1500km"]})
    with pytest.raises(ValueError, match="together with grid="):
        _plan(neighbourhood=reqs[1:], grid="5deg")


def test_signatures_keep_their_order():
    from skyrim_amd.core.models.base import GlobalModel
    tail = "derived grid regrid_method perturbation length_scale_km alpha lmax perturb_channels".split()
    for fn in (ensemble.run, ensemble.validate, ensemble.plan_request, GlobalModel.ensemble_forecast):
        params = inspect.signature(fn).parameters
        names = list(params)
        assert names[names.index("aggregates") + 1] == "neighbourhood" and params["neighbourhood"].default is None, fn.__name__
        if fn is not ensemble.plan_request:
            assert names[-len(tail):] == tail, fn.__name__
    from skyrim_amd import archive
    assert "neighbourhood" in archive.REPLAY_ARGS
    assert "neighbourhood" in [f.name for f in ensemble.Plan.__dataclass_fields__.values()]


def test_wrappers_that_cannot_do_it_say_what_to_do():
    import datetime
    from skyrim_amd.core.models.ensemble import GlobalEnsemble
    from skyrim_amd.core.models.graphcast import GraphcastModel
    t0 = datetime.datetime(2024, 5, 13, 18)
    with pytest.raises(NotImplementedError, match="neighbourhood_prediction"):
        GraphcastModel.neighbourhood_forecast(object.__new__(GraphcastModel), t0, 4, ["t2m:max:100km"])
    with pytest.raises(ValueError, match="neighbourhood_prediction"):
        ge = object.__new__(GlobalEnsemble)
        ge.model_names = ["pangu", "fuxi"]
        ge.neighbourhood_forecast(t0, 4, ["t2m:max:100km"])


# ---- 3. the build and the ABI ----------------------------------------------------------------------------------------------------------- #
def test_build_entries_and_exports():
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    syms = set(re.findall(r"\b(sknbr_[a-z0-9_]+)\s*\(", text))
    assert syms == set(N.EXPORTS) == {"sknbr_abi_version", "sknbr_check", "sknbr_run"}
    lib = N.load_library()
    assert all(hasattr(lib, s) for s in syms)
    assert lib.sknbr_abi_version() == N.ABI_VERSION == int(re.search(r"#define SKNBR_ABI_VERSION (\d+)", text).group(1))
    assert N.SPEC.stem == "skyrim_nbr" and N.SPEC.prefix == "sknbr" and N.SPEC.env == "SKYRIM_NBR_LIB"
    for name, val in (("MEMBERS", N.MAX_MEMBERS), ("OPS", N.MAX_OPS), ("RADII", N.MAX_RADII), ("W", N.MAX_W), ("REACH", N.MAX_REACH)):
        assert int(re.search(rf"SKNBR_MAX_{name} (\d+)", text).group(1)) == val
    for k, kind in enumerate(("MAX", "MIN", "MEAN", "FRAC_ABOVE"), 1):
        assert re.search(rf"#define SKNBR_{kind} {k}\b", text) and getattr(N, kind) == k
    make = (ROOT / "skyrim_amd/csrc/Makefile").read_text()
    assert re.search(r"^\$\(LIB_NBR\): nbr_ops\.hip fields\.h \.\./\.\./include/skyrim_nbr\.h program\.h\n.*\n\t\$\(HIPCC\) \$\(CXXFLAGS\) -ffp-contract=off -shared", make, re.M)
    assert all("$(LIB_NBR)" in line for line in make.splitlines() if line.startswith("all:") or line.startswith("\trm -rf"))
    assert ",nbr," in make.splitlines()[0] and "event}" in make and ",nbr," in native.__doc__ and "event}" in native.__doc__
    assert "sknbr_abi_version() == 1" in (ROOT / "__graft_entry__.py").read_text()
    from skyrim_amd import ops
    assert "nbr_fields" in ops.OP_NAMES


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not installed")
def test_descriptor_layout_matches_the_header(tmp_path):
    parts = [("sknbr_desc", N.NbrDesc), ("sknbr_op", N.OpDesc), ("sknbr_radius", N.RadiusDesc)]
    lines = []
    for cname, cls in parts:
        lines.append(f'  printf(" %zu", sizeof({cname}));\n')
        lines += [f'  printf(" %zu", offsetof({cname}, {"in" if f == "in_" else f}));\n' for f, _ in cls._fields_]
    src = tmp_path / "layout.cpp"
    src.write_text('#include <cstdio>\n#include <cstddef>\n#include "skyrim_nbr.h"\nint main() {\n' + "".join(lines) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    r = subprocess.run(["hipcc", "-x", "c++", "-std=c++17", f"-I{ROOT / 'include'}", str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    want = []
    for _, cls in parts:
        want += [ctypes.sizeof(cls)] + [getattr(cls, f).offset for f, _ in cls._fields_]
    assert got == want


def _desc(M=4):
    fake = 4096                                                # never dereferenced: the argument checks come first
    d = N.describe([N.Op(N.MAX, 0, 0, 0), N.Op(N.FRAC_ABOVE, 2, 1, 1, 0.5), N.Op(N.MEAN, 1, 3, 0)], M, 3, 5, 8, 4, 4 * 5 * 8, [1, 2])
    d.members, d.out, d.weights = fake, fake, fake
    d.radii[0].half = d.radii[1].half = fake
    return d


def test_argument_errors_need_no_gpu():
    lib = N.load_library()
    check = lambda d: lib.sknbr_check(ctypes.byref(d))         # noqa: E731
    assert check(_desc()) == 0 and check(_desc(1)) == 0 and check(_desc(64)) == 0
    assert lib.sknbr_check(None) == -1 and lib.sknbr_run(None, None) == -1

    def bad(change, M=4):
        d = _desc(M)
        change(d)
        assert check(d) == -1
        assert lib.sknbr_run(ctypes.byref(d), None) == -1       # the same refusal, before any launch

    bad(lambda d: None, M=0)
    bad(lambda d: None, M=65)
    bad(lambda d: setattr(d.ops[1], "out", 0))                 # a slot named twice
    bad(lambda d: setattr(d.ops[0], "in_", 3))                 # channel
    bad(lambda d: setattr(d.ops[0], "in_", -1))
    bad(lambda d: setattr(d.ops[0], "out", 4))                 # slot
    bad(lambda d: setattr(d.ops[0], "out", -1))
    bad(lambda d: setattr(d.ops[0], "kind", 0))                # kind
    bad(lambda d: setattr(d.ops[0], "kind", 5))
    bad(lambda d: setattr(d.ops[0], "radius", 2))              # radius index
    bad(lambda d: setattr(d.ops[0], "radius", -1))
    bad(lambda d: setattr(d.ops[1], "thr", float("nan")))
    bad(lambda d: setattr(d, "W", N.MAX_W + 1))                # W beyond the limit (member_stride would be too small as well)
    bad(lambda d: (setattr(d, "W", N.MAX_W + 1), setattr(d, "member_stride", 4 * 5 * (N.MAX_W + 1))))
    bad(lambda d: setattr(d.radii[1], "reach", N.MAX_REACH + 1))
    bad(lambda d: setattr(d.radii[1], "reach", -1))
    bad(lambda d: setattr(d, "n_radii", 0))
    bad(lambda d: setattr(d, "n_radii", 5))
    bad(lambda d: setattr(d, "n_ops", 0))
    bad(lambda d: setattr(d, "n_ops", 17))
    bad(lambda d: setattr(d, "member_align", 8))
    bad(lambda d: setattr(d, "member_stride", 4 * 5 * 8 - 1))
    bad(lambda d: setattr(d, "D", 0))
    bad(lambda d: setattr(d, "members", 4100))                 # misaligned table
    bad(lambda d: setattr(d, "weights", 4100))
    bad(lambda d: setattr(d, "out", 4098))
    bad(lambda d: setattr(d.radii[0], "half", 4098))
    for ptr in ("members", "out", "weights"):                  # null pointers
        bad(lambda d, ptr=ptr: setattr(d, ptr, None))
    bad(lambda d: setattr(d.radii[1], "half", None))


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not installed")
def test_kernel_uses_no_scratch():
    r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "--cuda-device-only", "-c", "nbr_ops.hip",
                        "-o", "/dev/null", "-Rpass-analysis=kernel-resource-usage"], cwd=ROOT / "skyrim_amd" / "csrc", capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    lds = [int(v) for v in re.findall(r"LDS Size \[bytes/block\]: (\d+)", r.stderr)]
    assert len(scratch) == 1 and scratch == [0] and 0 < lds[0] <= 64 * 1024


# ---- 4. the restatement on a hand-made case --------------------------------------------------------------------------------------------- #
def test_reference_restates_the_header():
    lat, lon = R.grid(5, 16)
    reach, half = N.discs(lat, lon, 0.75 * np.deg2rad(45.0) * EARTH_RADIUS_KM)      # on the equator the neighbours east and west, no other row
    assert reach == 0 and half[2, 0] == 1
    x = np.arange(80, dtype=np.float32).reshape(5, 16)             # the equator: 32 ... 47
    x[2, 3] = np.nan
    mx = R.one(x, N.MAX, reach, half)
    assert np.isnan(mx[2, 2:5]).all() and mx[2, 0] == 47.0 and mx[2, 15] == 47.0 and mx[2, 14] == 47.0 and mx[2, 13] == 46.0
    assert R.one(x, N.MIN, reach, half)[2, 0] == 32.0
    fr = R.one(x, N.FRAC_ABOVE, reach, half, 32.5)
    assert fr[2, 0] == np.float32(2 / 3) and fr[2, 1] == np.float32(2 / 3) and np.isnan(fr[2, 4]) and fr[2, 6] == 1.0
    w = np.ones(5)
    exact, bound = R.mean_exact(x, reach, half, w)
    assert exact[2, 0] == (47 + 32 + 33) / 3 and np.isnan(exact[2, 3]) and exact[2, 14] == 46.0 and (bound[2] > 0).all()
    less, _ = R.mean_exact(x, reach, half, w, skip=((2, 14), (2, 15)))
    assert less[2, 14] == 45.5 and less[2, 0] == exact[2, 0]


# ---- 5. the command line and the forecasts that need no device --------------------------------------------------------------------------- #
def test_command_line_options():
    from click.testing import CliRunner
    from skyrim_amd import neighbourhood_cli
    from skyrim_amd.labeled import DataArray
    res = CliRunner().invoke(neighbourhood_cli.neighbourhood, ["--help"])
    assert res.exit_code == 0 and "--neighbourhood" in res.output and "--derived" in res.output and "--members" in res.output
    v = {p.name: p for p in neighbourhood_cli.neighbourhood.params}
    assert v["requests"].multiple and v["members"].default == 1
    res = CliRunner().invoke(neighbourhood_cli.neighbourhood, ["-m", "pangu"])
    assert res.exit_code != 0 and "at least one --neighbourhood" in res.output
    res = CliRunner().invoke(neighbourhood_cli.neighbourhood, ["-m", "pangu", "--neighbourhood", "t2m:median:100km"])
    assert res.exit_code != 0 and "unknown statistic" in repr(res.exception)
    import datetime
    t0 = datetime.datetime(2024, 5, 13, 18)
    da = DataArray(np.arange(8, dtype=np.float32).reshape(2, 1, 2, 2), ["time", "channel", "lat", "lon"],
                   dict(time=[t0, t0 + datetime.timedelta(hours=6)], channel=["t2m_max_100km"], lat=[1.0, 0.0], lon=[0.0, 180.0]))
    assert neighbourhood_cli.lines(da) == ["+0h t2m_max_100km: min=0 mean=1.5 max=3", "+6h t2m_max_100km: min=4 mean=5.5 max=7"]


def test_forecasts_check_before_the_device():
    import datetime
    from test_ens_cpu import _Model
    from skyrim_amd.labeled import DataArray
    m, t0 = _Model(), datetime.datetime(2024, 5, 13, 18)
    with pytest.raises(ValueError, match="not an output channel"):
        m.neighbourhood_forecast(t0, 2, ["msl:max:500km"])
    with pytest.raises(ValueError, match="<N>km"):
        m.neighbourhood_forecast(t0, 2, ["t2m:max:500"])
    with pytest.raises(RuntimeError, match="GPU"):
        m.neighbourhood_forecast(t0, 2, ["t2m:max:500km"])
    with pytest.raises(ValueError, match="not an output channel"):
        m.ensemble_forecast(t0, n_steps=2, n_members=3, neighbourhood=["msl:max:500km"])
    lat, lon = np.linspace(60, -60, 5), np.arange(8) * 45.0
    da = DataArray(np.zeros((2, 1, 5, 8), np.float32), ["time", "channel", "lat", "lon"],
                   dict(time=[t0, t0 + datetime.timedelta(hours=6)], channel=["t2m"], lat=lat, lon=lon))
    with pytest.raises(ValueError, match="unknown statistic"):
        N.neighbourhood_prediction(da, ["t2m:p90:500km"])
    with pytest.raises(ValueError, match="closes the circle"):
        N.neighbourhood_prediction(da.isel(lon=slice(0, 5)), ["t2m:max:500km"])
