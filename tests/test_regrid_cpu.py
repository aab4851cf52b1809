"""Regridding without a GPU: the C ABI of include/skyrim_regrid.h (exports, argument errors of skregrid_run and skregrid_validate), the
weights of ``regrid.tables`` against the restatement's overlap integrals, their normalisation, conservation of the area mean, the fixed
points of the three methods, and the refusals of the Python layer."""
from __future__ import annotations

import ctypes
import inspect
import re
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

import _regrid_reference as R
from skyrim_amd import regrid as G

HEADER = Path(__file__).resolve().parent.parent / "include" / "skyrim_regrid.h"


def grid(n_lat, n_lon, rows=None, ascending=False):
    lat = np.linspace(90.0, -90.0, n_lat)[:rows]
    return (lat[::-1].copy() if ascending else lat), np.arange(n_lon) * (360.0 / n_lon)


def cases():
    """(name, source grid, target grid, methods): the four grid pairs the weights are compared on."""
    lat, lon = grid(49, 192)
    fcn = grid(49, 192, rows=48)
    asc = grid(49, 192, ascending=True)
    inner = (np.linspace(75.0, -75.0, 11), np.arange(48) * 7.5 + 1.0)                      # inside the 48 rows: bilinear may reach it
    return [("49x192 -> 13x48", (lat, lon), grid(13, 48), G.METHODS),
            ("48x192 -> 13x48", fcn, grid(13, 48), ("conservative", "nearest")),
            ("48x192 inner", fcn, inner, ("bilinear",)),
            ("ascending", asc, grid(13, 48, ascending=True), G.METHODS),
            ("date line", (lat, lon), G.target_grid(dict(region=(-30.0, 30.0, 340.0, 20.0), res=7.5), lat, lon), G.METHODS),
            ("date line crop", (lat, lon), G.target_grid(dict(region=(-30.0, 0.0, 350.0, 12.0)), lat, lon), G.METHODS)]


# ---- 1. ABI ------------------------------------------------------------------------------------------------------------------------------ #
def test_library_exports_every_declared_symbol():
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    syms = sorted(set(re.findall(r"\b(skregrid_[a-z0-9_]+)\s*\(", text)))
    lib = G.load_library()
    assert syms == sorted(G.EXPORTS) and len(syms) == 3
    for s in syms:
        assert hasattr(lib, s)
    const = lambda name: int(re.search(rf"SKREGRID_{name} \(?(-?\d+)", text).group(1))      # noqa: E731
    assert lib.skregrid_abi_version() == G.ABI_VERSION == const("ABI_VERSION")
    assert G.SPEC.env == "SKYRIM_REGRID_LIB"
    assert (const("MAX_MEMBERS"), const("MAX_CHANNELS"), const("MAX_TAPS"), const("MAX_W")) == (G.MAX_MEMBERS, G.MAX_CHANNELS, G.MAX_TAPS, G.MAX_W)
    assert (G.MAX_MEMBERS, G.MAX_CHANNELS, G.MAX_TAPS, G.MAX_W) == (64, 256, 32, 8192) and (const("E_ARG"), const("E_HIP")) == (-1, -2)
    assert ctypes.sizeof(G.TableDesc) == 24 and ctypes.sizeof(G.RegridDesc) == 8 + 4 * 8 + 4 * 256 + 48 + 16
    from skyrim_amd import ops
    assert "regrid" in ops.OP_NAMES


def _desc(channels=(0, 3, 1), C=4, H=49, W=192, Ho=13, Wo=24, M=3):
    fake = 4096                                                # never dereferenced: the argument checks come first
    d = G.describe(M, C, H, W, Ho, Wo, channels, len(channels) * Ho * Wo)
    d.members = d.out = fake
    for t in (d.rows, d.cols):
        t.start = t.count = t.weight = fake
    return d


def test_run_refuses_bad_descriptors_without_a_gpu():
    lib = G.load_library()
    assert lib.skregrid_run(None, None) == -1
    changes = [("members", None), ("members", 4100), ("out", None), ("out", 4098), ("M", 0), ("M", 65), ("member_align", 8), ("nc", 0), ("nc", 257),
               ("W", 8196), ("W", 3), ("H", 1), ("Ho", 0), ("Wo", 0), ("C", 3), ("C", 1 << 20), ("member_stride", 3 * 13 * 24 - 1),
               ("Ho", 1 << 20)]
    for name, value in changes:
        d = _desc()
        setattr(d, name, value)
        assert lib.skregrid_run(ctypes.byref(d), None) == -1, (name, value)
    for table in ("rows", "cols"):
        for part in ("start", "count", "weight"):
            for value in (None, 4100):                         # NULL, and 4-byte but not 16-byte aligned
                d = _desc()
                setattr(getattr(d, table), part, value)
                assert lib.skregrid_run(ctypes.byref(d), None) == -1, (table, part, value)
    for bad in ((0, 4), (-1, 0), (0, 1, 1 << 30)):             # a channel >= C, a negative one
        assert lib.skregrid_run(ctypes.byref(_desc(channels=bad)), None) == -1, bad
    d = _desc(C=1 << 10, H=1 << 10, W=(1 << 10) + 4)           # C H W > 2^30
    assert lib.skregrid_run(ctypes.byref(d), None) == -1


def _validate(start, count, weight, n_src, periodic):
    start, count = np.asarray(start, np.int32), np.asarray(count, np.int32)
    w = np.zeros((start.size, G.MAX_TAPS), np.float32)
    for o, row in enumerate(weight):
        w[o, :len(row)] = row
    return G.load_library().skregrid_validate(start.ctypes.data, count.ctypes.data, w.ctypes.data, start.size, n_src, int(periodic))


def test_validate_refuses_bad_tables():
    lib = G.load_library()
    good = ([0, 5], [2, 3], [[0.5, 0.5], [0.25, 0.5, 0.25]])
    assert _validate(*good, 8, False) == 0 and _validate(*good, 8, True) == 0
    assert _validate([0, 6], [2, 3], good[2], 8, True) == 0                            # a periodic axis wraps
    assert _validate([0, 6], [2, 3], good[2], 8, False) == -1                          # start + count > n_src
    assert _validate([0, 5], [0, 3], [[], good[2][1]], 8, False) == -1                 # count 0
    assert _validate([0], [33], [[1.0] * 32], 64, False) == -1                         # count 33
    assert _validate([0, 8], [2, 3], good[2], 8, True) == -1 and _validate([-1, 5], [2, 3], good[2], 8, True) == -1
    assert _validate([0], [5], [[0.2] * 5], 4, True) == -1                             # more taps than source points
    for bad in (np.nan, np.inf, -np.inf, 0.0):
        assert _validate([0, 5], [2, 3], [[0.5, 0.5], [0.25, bad, 0.25]], 8, False) == -1, bad
    assert _validate([0, 5], [2, 2], [[0.5, 0.5], [0.25, 0.5, np.nan]], 8, False) == 0  # beyond count: padding, not read
    z = np.zeros(4, np.int32)
    assert lib.skregrid_validate(None, z.ctypes.data, z.ctypes.data, 1, 8, 0) == -1 and lib.skregrid_validate(z.ctypes.data, z.ctypes.data, None, 1, 8, 0) == -1
    assert _validate([0], [1], [[1.0]], 0, False) == -1
    ax = G.Axis(np.zeros(2, np.int32), np.array([1, 0], np.int32), np.ones((2, 32), np.float32), 8, False)
    with pytest.raises(ValueError, match="skregrid_validate"):
        G.validate_axis(ax)


# ---- 2. the weights ------------------------------------------------------------------------------------------------------------------------ #
def test_weights_match_the_restatement():
    for name, src, dst, methods in cases():
        for method in methods:
            t = G.tables(*src, *dst, method)
            rows, cols = R.matrices(*src, *dst, method)
            assert t.rows.dense().shape == rows.shape and t.cols.dense().shape == cols.shape, (name, method)
            # float64 weights rounded once to fp32: 2^-24 relative, on weights <= 1
            assert np.abs(t.rows.dense() - rows).max() <= 2.0 ** -24, (name, method, "rows")
            assert np.abs(t.cols.dense() - cols).max() <= 2.0 ** -24, (name, method, "cols")
            for ax in (t.rows, t.cols):                        # no zero weight is emitted, the padding is zero
                for o in range(ax.start.size):
                    assert np.all(ax.weight[o, :ax.count[o]] != 0) and np.all(ax.weight[o, ax.count[o]:] == 0)
            assert G.tables(*src, *dst, method) is t           # cached
    lat, lon = grid(721, 1440)
    t = G.tables(lat, lon, *G.target_grid("1.5deg", lat, lon), "conservative")
    assert t.rows.start.size == 121 and t.cols.start.size == 240 and t.rows.count.max() == 7 and t.cols.count.max() == 7
    assert t.rows.count[0] == 4 and t.cols.start[0] == 1437                             # the pole cell; the first column wraps


def test_conservative_weights_are_normalised():
    for name, src, dst, methods in cases():
        if "conservative" not in methods:
            continue
        t = G.tables(*src, *dst, "conservative")
        for ax in (t.rows, t.cols):
            assert np.abs(ax.weight.astype(np.float64).sum(axis=1) - 1.0).max() <= 2.0 ** -22, name
    fcn = grid(49, 192, rows=48)
    cov = R.conservative_rows(fcn[0], G.target_grid("15deg", *fcn)[0])[1]
    assert 0.9 < cov[-1] < 1.0 and np.all(np.abs(cov[:-1] - 1.0) < 1e-12)               # the last cell misses the south-pole row


def test_area_mean_is_conserved():
    rng = np.random.default_rng(3)
    for (n_lat, n_lon), res in (((49, 192), grid(13, 48)), ((721, 1440), "1.5deg")):
        lat, lon = grid(n_lat, n_lon)
        dlat, dlon = G.target_grid(res, lat, lon)
        x = 280.0 + 30.0 * np.cos(np.radians(lat))[:, None] + rng.normal(0, 5.0, (n_lat, n_lon))
        rows, cols = R.matrices(lat, lon, dlat, dlon, "conservative")                  # the restatement alone conserves it ...
        want = R.area_mean(x, lat)
        assert abs(R.area_mean(rows @ x @ cols.T, dlat) - want) <= 1e-12 * abs(want)
        t = G.tables(lat, lon, dlat, dlon, "conservative")                              # ... and the fp32-rounded weights to 1e-6
        from skyrim_amd.verify import area_weights
        y = t.rows.dense() @ x @ t.cols.dense().T
        ws, wd = area_weights(lat), area_weights(dlat)
        got, ref = (wd[:, None] * y).sum() / (wd.sum() * dlon.size), (ws[:, None] * x).sum() / (ws.sum() * n_lon)
        print(f"area mean {n_lat}x{n_lon} -> {dlat.size}x{dlon.size}: relative difference {abs(got - ref) / abs(ref):.2e}")
        assert abs(got - ref) <= 1e-6 * abs(ref)
        assert abs(ref - want) <= 1e-12 * abs(want)


def test_fixed_points():
    lat, lon = grid(49, 192)
    for name, src, dst, methods in cases():
        for method in methods:                                 # a constant maps to the constant
            t = G.tables(*src, *dst, method)
            y = t.rows.dense() @ np.full((src[0].size, src[1].size), 7.25) @ t.cols.dense().T
            assert np.abs(y - 7.25).max() <= 7.25 * 2.0 ** -21, (name, method)
    # bilinear reproduces a field that is linear in latitude; made from the float64 weights of the restatement it is exact to round-off
    dlat, dlon = np.linspace(88.0, -88.0, 31), np.arange(40) * 9.0 + 0.7
    x = (3.0 + 0.5 * lat)[:, None] * np.ones(192)
    rows, cols = R.matrices(lat, lon, dlat, dlon, "bilinear")
    assert np.abs(rows @ x @ cols.T - (3.0 + 0.5 * dlat)[:, None]).max() <= 1e-12
    t = G.tables(lat, lon, dlat, dlon, "bilinear")
    assert np.abs(t.rows.dense() @ x @ t.cols.dense().T - (3.0 + 0.5 * dlat)[:, None]).max() <= 48.0 * 2.0 ** -22
    assert set(t.rows.count.tolist()) <= {1, 2} and set(t.cols.count.tolist()) == {2}
    for asc in (False, True):                                  # the identity: one tap of weight 1 everywhere, for every method
        la, lo = grid(49, 192, ascending=asc)
        for method in G.METHODS:
            t = G.tables(la, lo, la, lo, method)
            for ax, n in ((t.rows, 49), (t.cols, 192)):
                assert np.array_equal(ax.start, np.arange(n)) and np.all(ax.count == 1) and np.all(ax.weight[:, 0] == 1.0), (asc, method)
    # a region at the source's resolution is the source's own points: nearest is a crop
    rl, ro = G.target_grid(dict(region=(-30.0, 0.0, 350.0, 12.0)), lat, lon)
    t = G.tables(lat, lon, rl, ro, "nearest")
    assert np.array_equal(lat[t.rows.start], rl) and np.array_equal(lon[t.cols.start], ro) and ro[0] > ro[-1]
    assert np.all(np.diff(t.rows.start) == 1) and np.array_equal(t.cols.start, (t.cols.start[0] + np.arange(ro.size)) % 192)
    a = G.tables(lat, lon, np.array([45.0 + 3.75 / 2]), np.array([1.875 / 2]), "nearest")      # ties go to the lower index
    assert a.rows.start[0] == 11 and a.cols.start[0] == 0 and lat[11] == 48.75


# ---- 3. the refusals of the Python layer ----------------------------------------------------------------------------------------------------- #
def test_target_grid():
    lat, lon = grid(721, 1440)
    la, lo = G.target_grid("1.5deg", lat, lon)
    assert la.size == 121 and lo.size == 240 and la[0] == 90.0 and la[-1] == -90.0 and lo[1] == 1.5
    assert np.array_equal(G.target_grid(1.5, lat[::-1], lon)[0], la[::-1])             # oriented like the source
    assert G.grid_label("1.5deg") == "1.5deg" and G.grid_label(dict(region=(0, 10, 350, 10), res=0.5)) == "region0_10_350_10@0.5deg"
    for bad in ("1.7deg", 0.7, "7deg"):
        with pytest.raises(ValueError, match="is not an integer"):
            G.target_grid(bad, lat, lon)
    for bad in ("fine", -1.0, dict(res=1.0), dict(region=(10, 0, 0, 10)), 3 + 2j):
        with pytest.raises(ValueError):
            G.target_grid(bad, lat, lon)
    bl, bo = G.target_grid(dict(region=(30.0, 60.0, 350.0, 10.0), res=5.0), lat, lon)
    assert bl.tolist() == [60, 55, 50, 45, 40, 35, 30] and bo.tolist() == [350, 355, 0, 5, 10]


def test_tables_refuse_what_they_cannot_serve():
    lat, lon = grid(721, 1440)
    with pytest.raises(ValueError, match=r"reads 4\d source rows.*at most 32.*coarsest.*7.5 degrees"):
        G.tables(lat, lon, *G.target_grid("10deg", lat, lon), "conservative")
    with pytest.raises(ValueError, match="unknown method 'cubic'"):
        G.tables(lat, lon, *G.target_grid("1.5deg", lat, lon), "cubic")
    fcn = grid(49, 192, rows=48)
    with pytest.raises(ValueError, match=r"target row 12 \(latitude -90\) lies outside the source latitudes"):
        G.tables(*fcn, *G.target_grid("15deg", *fcn), "bilinear")
    half = grid(49, 192, rows=25)                              # the northern hemisphere only
    with pytest.raises(ValueError, match=r"target row 7 \(latitude -15\) is less than half covered"):
        G.tables(*half, *G.target_grid("15deg", *half), "conservative")
    G.tables(*half, np.linspace(90.0, 0.0, 7), np.arange(24) * 15.0, "conservative")    # (its own half is served)


def test_validate_and_the_entry_points_refuse_before_the_device():
    from skyrim_amd import ensemble as E
    from skyrim_amd.core.models.base import GlobalModel
    from skyrim_amd.core.models.ensemble import GlobalEnsemble, _on_grid_of
    from skyrim_amd.labeled import DataArray
    from skyrim_amd.pangu.spec import CHANNELS
    lat, lon = grid(49, 192)
    model = SimpleNamespace(out_channel_names=list(CHANNELS), in_channel_names=list(CHANNELS), grid=SimpleNamespace(lat=lat, lon=lon))
    args, tail = (model, 2, 3, 0, ("mean",), None, None), (None, 1, False)
    assert E.validate(*args, *tail, grid="15deg")[3] == [0, 1, 2]
    with pytest.raises(ValueError, match="grid= together with derived="):
        E.validate(*args, *tail, derived=["ws10m"], grid="15deg")
    with pytest.raises(ValueError, match="unknown method 'spline'"):
        E.validate(*args, *tail, grid="15deg", regrid_method="spline")
    with pytest.raises(ValueError, match="is not an integer"):
        E.validate(*args, *tail, grid="7deg")
    with pytest.raises(ValueError, match='"regridded"'):
        E.validate(*args, None, 1, "regridded")
    big = SimpleNamespace(out_channel_names=list(CHANNELS), in_channel_names=list(CHANNELS), grid=SimpleNamespace(lat=grid(721, 1440)[0], lon=grid(721, 1440)[1]))
    with pytest.raises(ValueError, match="keep_members=True would hold"):
        E.validate(big, 4, 50, 0, ("mean",), None, None, None, 1, True, grid="1.5deg")
    assert E.validate(big, 4, 50, 0, ("mean",), None, None, None, 1, "regridded", grid="1.5deg")[3] == [0, 1, 2, 3, 4]      # 2 GB: fits
    # the pinned tail of the signatures, and where the new keywords stand
    new = ["perturbation", "length_scale_km", "alpha", "lmax", "perturb_channels"]
    for fn in (E.run, GlobalModel.ensemble_forecast, E.validate):
        names = list(inspect.signature(fn).parameters)
        assert names[-5:] == new and names[-8:-5] == ["derived", "grid", "regrid_method"], fn
        d = inspect.signature(fn).parameters
        assert d["grid"].default is None and d["regrid_method"].default == "conservative"
    assert E.EnsembleForecast("pangu", 3, 0, 1e-3).regridded is None
    # GlobalEnsemble without a grid refuses members on different latitude axes exactly as before
    a = DataArray(np.zeros((1, 1, 49, 192), np.float32), ["time", "channel", "lat", "lon"], dict(time=[0], channel=["t2m"], lat=lat, lon=lon))
    b = DataArray(np.zeros((1, 1, 48, 192), np.float32), ["time", "channel", "lat", "lon"], dict(time=[0], channel=["t2m"], lat=lat[:48], lon=lon))
    with pytest.raises(ValueError, match="ensemble members are on different lat axes"):
        _on_grid_of(a, b)
    ens = GlobalEnsemble(["pangu", "fourcastnet"])
    assert ens.grid is None and ens.regrid_method == "conservative"
    with pytest.raises(ValueError, match="ensemble members are on different lat axes"):
        ens._ensemble_predictions([a, b])
    with pytest.raises(ValueError, match="unknown method"):
        GlobalEnsemble(["pangu", "fourcastnet"], grid="1.5deg", regrid_method="spline")


def test_commands_list_the_grid_options():
    from click.testing import CliRunner
    from skyrim_amd import regrid_cli, verify_cli
    res = CliRunner().invoke(verify_cli.verify, ["--help"])
    assert res.exit_code == 0 and "--grid" in res.output and "--regrid_method" in res.output
    v = {p.name: p for p in verify_cli.verify.params}
    assert v["grid"].default is None and v["regrid_method"].default == "conservative"
    res = CliRunner().invoke(regrid_cli.regrid, ["--help"])
    assert res.exit_code == 0 and "--region" in res.output and "[conservative|bilinear|nearest]" in res.output
    assert regrid_cli.parse_grid("1.5deg", None, None) == "1.5deg"
    assert regrid_cli.parse_grid("1.5deg", "30,60,350,10", "0.5") == dict(region=(30.0, 60.0, 350.0, 10.0), res="0.5")
    assert regrid_cli.output_name(Path("pangu__gfs__20240101_00:00__20240102_00:00.nc")) == "pangu-regrid__gfs__20240101_00:00__20240102_00:00.nc"
