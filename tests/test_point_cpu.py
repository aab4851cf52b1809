"""Point forecasts without a GPU: the exports and argument checks of libskyrim_point.so, ``skpoint_validate``, the records against the
tables of ``regrid.tables``, ``Points`` parsing, the float32 restatement against its float64 twin within the header's bound, the station
scores against an independent restatement and against tests/_score_reference.py, the host limit and the command line's options."""
from __future__ import annotations

import ctypes
import datetime
import re
from pathlib import Path

import numpy as np
import pytest

import _point_reference as R
import _score_reference as SR
from skyrim_amd import points as P
from skyrim_amd import regrid as G

ROOT = Path(__file__).resolve().parents[1]
E_ARG = -1


def grid(n_lat, n_lon, rows=None):
    return np.linspace(90.0, -90.0, n_lat)[:rows], np.arange(n_lon) * (360.0 / n_lon)


# ---- the library ------------------------------------------------------------------------------------------------------------------------ #
def test_library_exports_every_symbol_of_the_header_and_the_abi_matches():
    text = (ROOT / "include" / "skyrim_point.h").read_text()
    declared = re.findall(r"^(?:int|void)\s+(skpoint_\w+)\s*\(", text, re.M)
    assert sorted(declared) == sorted(P.EXPORTS) == ["skpoint_abi_version", "skpoint_gather", "skpoint_validate"]
    lib = P.load_library()
    for name in declared:
        assert hasattr(lib, name)
    assert lib.skpoint_abi_version() == P.ABI_VERSION == int(re.search(r"#define SKPOINT_ABI_VERSION (\d+)", text).group(1))
    for macro, value in (("MAX_MEMBERS", P.MAX_MEMBERS), ("MAX_CHANNELS", P.MAX_CHANNELS), ("CHUNK", P.CHUNK)):
        assert int(re.search(rf"#define SKPOINT_{macro} (\d+)", text).group(1)) == value
    assert P.MAX_POINTS == 1 << 20 and "#define SKPOINT_MAX_POINTS (1 << 20)" in text
    assert P.REC.itemsize == 32 and P.REC == R.REC
    assert ctypes.sizeof(P.PointDesc) == 8 + 5 * 4 + 4 * 256 + 4 + 8 + 4 + 4 + 8 + 8          # (with the padding before each pointer)


def good_desc():
    d = P.describe(3, 6, 33, 64, [0, 5, 2], 100, 300)
    d.members, d.records, d.out = 0x1000, 0x2000, 0x3000                       # never dereferenced: every call below is refused first
    return d


def test_gather_refuses_bad_arguments_without_a_gpu():
    lib = P.load_library()
    assert lib.skpoint_gather(None, None) == E_ARG

    def refused(**kw):
        d = good_desc()
        for k, v in kw.items():
            setattr(d, k, v)
        return lib.skpoint_gather(ctypes.byref(d), None) == E_ARG
    assert refused(members=None) and refused(records=None) and refused(out=None)
    assert refused(M=0) and refused(M=65) and refused(nc=0) and refused(nc=257) and refused(P=0) and refused(P=(1 << 20) + 1)
    assert refused(member_stride=299)                                          # shorter than nc P
    assert refused(records=0x2010 - 8) and refused(records=0x2004)             # not 16-byte aligned
    assert refused(out=0x3002) and refused(members=0x1004)
    assert refused(H=0) and refused(W=1) and refused(C=0)
    assert refused(C=69, H=4096, W=4096)                                       # C H W > 2^30
    for bad in (-1, 6):
        d = good_desc()
        d.channels[1] = bad
        assert lib.skpoint_gather(ctypes.byref(d), None) == E_ARG
    assert P.MAX_CHANNELS * P.MAX_POINTS <= 2 ** 30                           # nc P <= 2^30 follows from the two limits


def test_validate_accepts_good_records_and_refuses_each_bad_kind():
    lib = P.load_library()
    H, W = 5, 8
    good = np.zeros(4, P.REC)
    good[0] = (0, 0, 1, 1, 1.0, 0.0, 1.0, 0.0)
    good[1] = (3, 7, 2, 2, 0.25, 0.75, 0.5, 0.5)                               # row H - 2 with two taps, the last column with two
    good[2] = (4, 7, 1, 2, -2.0, np.nan, 1e-20, 3.0)                           # row H - 1 with one tap; an unused weight may be anything
    good[3] = (2, 3, 2, 1, 1.0, 1.0, 1.0, 0.0)
    call = lambda r, n=None, h=H, w=W: lib.skpoint_validate(r.ctypes.data, r.size if n is None else n, h, w)      # noqa: E731
    assert call(good) == 0
    P.validate_records(good, H, W)
    assert lib.skpoint_validate(None, 1, H, W) == E_ARG and call(good, n=0) == E_ARG and call(good, h=0) == E_ARG and call(good, w=1) == E_ARG
    for field, value in (("row", -1), ("row", H), ("col", -1), ("col", W), ("nr", 0), ("nr", 3), ("ncol", 0), ("ncol", 3),
                         ("wr0", 0.0), ("wr0", np.inf), ("wc0", np.nan), ("wc0", 0.0), ("wr1", 0.0), ("wr1", np.nan), ("wc1", -np.inf),
                         ("wc1", 0.0)):
        bad = good.copy()
        bad[field][1] = value
        assert call(bad) == E_ARG, (field, value)
        with pytest.raises(ValueError, match="skpoint_validate"):
            P.validate_records(bad, H, W)
    bad = good.copy()
    bad["row"][1] = H - 1                                                      # two row taps from the last row
    assert call(bad) == E_ARG
    with pytest.raises(ValueError):
        P.validate_records(good.astype([("row", "<i4")] + P.REC.descr[1:-1] + [("wc1", "<f8")]), H, W)


# ---- the records ------------------------------------------------------------------------------------------------------------------------ #
def test_records_on_nodes_across_the_date_line_and_at_the_poles():
    lat, lon = grid(721, 1440)
    r = P.records({"node": (12.25, 45.5), "west": (10.1, -0.1), "east": (10.1, 359.9), "np": (90.0, 0.0), "sp": (-90.0, 10.0)}, lat, lon)
    assert tuple(r[0]) == (311, 182, 1, 1, 1.0, 0.0, 1.0, 0.0)                 # a source point hit exactly: one tap of weight 1
    assert r[1] == r[2] and r["col"][1] == 1439 and r["ncol"][1] == 2          # the taps are W - 1 and (W - 1 + 1) mod W = 0
    assert np.float32(r["wc0"][1]) + np.float32(r["wc1"][1]) == 1 and abs(r["wc1"][1] - 0.6) < 1e-6
    assert (r["row"][3], r["nr"][3], r["wr0"][3]) == (0, 1, 1.0)
    assert (r["row"][4], r["nr"][4], r["wr0"][4]) == (720, 1, 1.0)             # the south pole is the last row, one tap
    assert P.records({"node": (12.25, 45.5), "west": (10.1, -0.1), "east": (10.1, 359.9), "np": (90.0, 0.0), "sp": (-90.0, 10.0)}, lat, lon) is r
    n = P.records({"tie": (12.125, 45.625), "near": (12.2, 45.7)}, lat, lon, "nearest")
    assert tuple(n[0]) == (311, 182, 1, 1, 1.0, 0.0, 1.0, 0.0)                 # ties go to the lower index on both axes
    assert tuple(n[1])[:4] == (311, 183, 1, 1)
    with pytest.raises(ValueError, match="unknown method"):
        P.records({"a": (0, 0)}, lat, lon, "cubic")


def test_a_point_south_of_a_720_row_grid():
    lat, lon = grid(721, 1440, rows=720)                                       # FourCastNet's rows: no south pole
    with pytest.raises(ValueError, match="'mcmurdo'.*outside the source latitudes"):
        P.records({"ankara": (39.9, 32.9), "mcmurdo": (-89.9, 166.7)}, lat, lon)
    n = P.records({"ankara": (39.9, 32.9), "mcmurdo": (-89.9, 166.7)}, lat, lon, "nearest")
    assert (n["row"][1], n["nr"][1]) == (719, 1)
    assert P.records({"edge": (-89.75, 0.0)}, lat, lon)["row"][0] == 719       # the last row itself is inside


@pytest.mark.parametrize("method", ["bilinear", "nearest"])
def test_records_of_the_nodes_of_a_regrid_target_are_its_tables(method):
    lat, lon = grid(721, 1440)
    dlat, dlon = G.target_grid("1.5deg", lat, lon)
    t = G.tables(lat, lon, dlat, dlon, method)
    assert (dlat.size, dlon.size) == (121, 240)
    pts = [(f"{j}_{i}", dlat[j], dlon[i]) for j in range(dlat.size) for i in range(dlon.size)]          # all 29 040 nodes
    rec = P.records(pts, lat, lon, method)
    jj, ii = (a.reshape(-1) for a in np.meshgrid(np.arange(dlat.size), np.arange(dlon.size), indexing="ij"))
    assert rec.size == 121 * 240
    assert np.array_equal(rec["row"], t.rows.start[jj]) and np.array_equal(rec["nr"], t.rows.count[jj])
    assert np.array_equal(rec["col"], t.cols.start[ii]) and np.array_equal(rec["ncol"], t.cols.count[ii])
    for name, w in (("wr0", t.rows.weight[jj, 0]), ("wr1", t.rows.weight[jj, 1]), ("wc0", t.cols.weight[ii, 0]), ("wc1", t.cols.weight[ii, 1])):
        assert np.array_equal(rec[name].view(np.uint32), np.ascontiguousarray(w).view(np.uint32)), name        # bit for bit
    assert t.rows.count.max() <= 2 and t.cols.count.max() <= 2


# ---- Points ----------------------------------------------------------------------------------------------------------------------------- #
def test_points_parsing_and_refusals(tmp_path):
    a = P.Points({"Istanbul": (41.01, 28.98), "Lisbon": (38.72, -9.14)})
    b = P.Points([("Istanbul", 41.01, 28.98), ("Lisbon", 38.72, 350.86)])
    assert a.names == b.names == ["Istanbul", "Lisbon"] and len(a) == 2
    assert np.array_equal(a.lat, b.lat) and np.allclose(a.lon, [28.98, 350.86]) and np.all((a.lon >= 0) & (a.lon < 360))
    path = tmp_path / "stations.csv"
    path.write_text("name,lat,lon\nIstanbul, 41.01, 28.98\n\nLisbon,38.72,-9.14\n")
    c = P.Points(str(path))
    assert c.names == a.names and np.array_equal(c.lat, a.lat) and np.array_equal(c.lon, a.lon) and c.key() == a.key()
    assert P.Points(c).key() == a.key() and P.Points(path).names == a.names
    assert P.Points({"w": (0, -180.0)}).lon[0] == 180.0
    for bad, msg in (({"a": (0, 0), "b": (91, 0)}, "lat"), ([("a", 0, 0), ("a", 1, 1)], "twice"), ({"a": (np.nan, 0)}, "non-finite"),
                     ({"a": (0, np.inf)}, "non-finite"), ({"a": (0, 360.0)}, "longitude"), ({"a": (0, -180.5)}, "longitude"), ({}, "at least one"),
                     ([("a", 0)], "name, lat, lon"), ({"a": ("x", 0)}, "numbers"), (7, "CSV")):
        with pytest.raises(ValueError, match=msg):
            P.Points(bad)
    (tmp_path / "bad.csv").write_text("station,latitude,longitude\nA,1,2\n")
    with pytest.raises(ValueError, match="header name,lat,lon"):
        P.Points(str(tmp_path / "bad.csv"))
    (tmp_path / "short.csv").write_text("name,lat,lon\nA,1\n")
    with pytest.raises(ValueError, match="lacks a column"):
        P.Points(str(tmp_path / "short.csv"))


# ---- the arithmetic --------------------------------------------------------------------------------------------------------------------- #
def test_the_restatement_stays_within_the_bound_of_its_float64_twin():
    rng = np.random.default_rng(0)
    H, W, M, C = 33, 64, 3, 6
    scale = np.array([250.0, 54000.0, 25.0, 1e-3, 1e-30, 1e8])
    x = (rng.normal(0, 1, (M, C, H, W)) * scale[None, :, None, None] + scale[None, :, None, None] * np.array([1, 1, 0, 0, 0, -1])[None, :, None, None])
    x = x.astype(np.float32)
    n = 5000
    rec = np.zeros(n, R.REC)
    rec["nr"], rec["ncol"] = rng.integers(1, 3, n), rng.integers(1, 3, n)
    rec["row"] = np.where(rec["nr"] == 2, rng.integers(0, H - 1, n), rng.integers(0, H, n))
    rec["col"] = rng.integers(0, W, n)
    for k in ("wr0", "wr1", "wc0", "wc1"):
        rec[k] = (rng.normal(0, 1, n) * 10.0 ** rng.integers(-3, 3, n)).astype(np.float32)
        rec[k][rec[k] == 0] = 1.0
    P.validate_records(rec, H, W)
    got = R.gather(x, list(range(C)), rec)
    exact, S = R.gather64(x, list(range(C)), rec)
    share = np.abs(got.astype(np.float64) - exact) / R.bound(rec, S)
    print(f"restatement against float64: worst share of the bound {share.max():.3f}")
    assert share.max() <= 1.0 and share.max() > 0.05                           # (a bound nothing comes near would check nothing)
    one = np.zeros(3, R.REC)
    one[:] = [(r, c, 1, 1, 1.0, 0.0, 1.0, 0.0) for r, c in ((0, 0), (H - 1, W - 1), (7, 9))]
    y = x.copy()
    y.view(np.uint32)[0, 0, 7, 9] = 0x7FC00123
    y[1, 0, 0, 0] = -0.0
    assert np.array_equal(R.gather(y, [0], one).view(np.uint32), y[:, [0]][:, :, [0, H - 1, 7], [0, W - 1, 9]].view(np.uint32))      # a bit copy


# ---- PointForecast ---------------------------------------------------------------------------------------------------------------------- #
T0 = datetime.datetime(2024, 5, 13, 18)


def forecast(M=5, T=3, C=2, n=40, seed=0):
    rng = np.random.default_rng(seed)
    x = (rng.normal(0, 2, (M, T, C, n)) + np.array([280.0, 5.0])[None, None, :C, None]).astype(np.float32)
    pts = P.Points([(f"s{i}", la, lo) for i, (la, lo) in enumerate(zip(rng.uniform(-80, 80, n), rng.uniform(0, 359, n)))])
    times = [T0 + k * datetime.timedelta(hours=6) for k in range(T)]
    return P.PointForecast.build(x, times, ["t2m", "ws10m"][:C], pts, "bilinear", "toy"), x, rng


def test_verify_with_missing_observations_equals_the_restatement():
    pf, x, rng = forecast()
    M, T, C, n = x.shape
    obs = x[0].astype(np.float64) + rng.normal(0, 1.5, (T, C, n))
    obs[rng.random((T, C, n)) < 0.1] = np.nan
    obs[1, 1] = np.nan                                                         # one (time, channel) without any observation
    want = R.station_scores(x, obs)
    from skyrim_amd.labeled import DataArray
    for form in ({"t2m": obs[:, 0], "ws10m": obs[:, 1]},
                 DataArray(obs[:, ::-1][:, :, ::-1], ["time", "channel", "point"],
                           dict(time=pf.times, channel=["ws10m", "t2m"], point=pf.names[::-1]))):       # picked by name, whatever the order
        got = pf.verify(form)
        assert got["channels"] == ["t2m", "ws10m"] and got["times"] == pf.times
        assert np.array_equal(got["n"], np.isfinite(obs).sum(axis=2)) and np.array_equal(got["n"], want["n"])
        assert got["n"][1, 1] == 0 and 0 < got["n"].max() <= n and got["n"][0, 0] < n
        for k in ("bias", "mae", "rmse", "crps", "spread", "ssr"):
            assert np.isnan(got[k][1, 1]) and np.isfinite(np.delete(got[k].reshape(-1), 1 * C + 1)).all(), k
            np.testing.assert_allclose(got[k], want[k], rtol=1e-12, atol=0, equal_nan=True, err_msg=k)
        assert np.array_equal(got["rank_histogram"], want["rank_histogram"])
        assert np.array_equal(got["rank_histogram"].sum(axis=2), got["n"]) and not got["rank_histogram"][1, 1].any()
    with pytest.raises(ValueError, match="not sampled channels"):
        pf.verify({"msl": obs[:, 0]})
    with pytest.raises(ValueError, match="shape"):
        pf.verify({"t2m": obs[:, 0, :-1]})


def test_verify_without_missing_values_equals_the_score_reference_on_one_row():
    pf, x, rng = forecast(seed=3)
    M, T, C, n = x.shape
    obs = (x[1] + rng.normal(0, 1.0, (T, C, n))).astype(np.float32)
    got = pf.verify({"t2m": obs[:, 0], "ws10m": obs[:, 1]})
    for t in range(T):
        val, _, counts = SR.scores(x[:, t][:, :, None, :], obs[t][:, None, :], np.ones(1))      # the points as one row of unit weight
        table = SR.table(val, M)
        # the other restatement forms the mean error as sum(x_m - y) / M and the variance from x_m - x_0: each term of a score differs by a
        # few roundings of values up to 300 (ulp 5.7e-14), (M + 2) of them at the most: 4e-13 absolute, against scores above 0.05
        np.testing.assert_allclose(got["bias"][t], table["bias"], rtol=0, atol=4e-13)
        for k in ("mae", "rmse", "crps", "spread", "ssr"):
            assert np.all(np.abs(table[k]) > 0.05)
            np.testing.assert_allclose(got[k][t], table[k], rtol=4e-13 / 0.05, err_msg=k)
        assert np.array_equal(got["rank_histogram"][t], counts[:, 0, :])
    assert np.all(got["n"] == n)
    one = P.PointForecast.build(x[:1], pf.times, pf.channels, P.Points(list(zip(pf.names, pf.values.lat.values, pf.values.lon.values))), "nearest")
    s = one.verify({"t2m": x[0, :, 0].astype(np.float64)})
    assert s["channels"] == ["t2m"] and np.all(s["rmse"] == 0) and np.all(s["crps"] == 0) and np.isnan(s["spread"]).all()


def test_statistics_follow_the_ensemble_header(tmp_path):
    import _ens_reference as ER
    pf, x, _ = forecast(M=7, seed=5)
    M, T, C, n = x.shape
    levels = [0.0, 0.1, 0.5, 0.9, 1.0]
    r = ER.stats(x.reshape(M, -1), thresholds=[280.5], levels=levels)
    assert np.array_equal(pf.mean().values.reshape(-1), r["mean"]) and pf.mean().dims == ("time", "channel", "point")
    np.testing.assert_allclose(pf.spread().values.reshape(-1), r["spread"], rtol=1e-13)
    q = pf.quantile(levels)
    assert q.dims == ("quantile", "time", "channel", "point") and q.quantile.values.tolist() == levels
    for i in range(len(levels)):
        np.testing.assert_allclose(q.values[i].reshape(-1), r["quant"][i][0], rtol=1e-14)
    ex = pf.exceedance("t2m", [280.5, 1e9])
    assert ex.dims == ("threshold", "time", "point") and not ex.values[1].any()
    assert np.array_equal(ex.values[0].astype(np.float32), r["exceed"][0].reshape(T, C, n)[:, 0])
    pl = pf.plume("ws10m", "s3")
    assert pl["members"].shape == (M, T) and np.array_equal(pl["members"], x[:, :, 1, 3].astype(np.float64)) and pl["times"] == pf.times
    assert np.array_equal(pl["mean"], pf.mean().values[:, 1, 3]) and np.array_equal(pl["quantiles"][0.5], pf.quantile([0.5]).values[0, :, 1, 3])
    with pytest.raises(ValueError):
        pf.plume("ws10m", "nowhere")
    with pytest.raises(ValueError):
        pf.exceedance("msl", [1.0])
    # the coordinates and the files
    v = pf.values
    assert v.dims == ("member", "time", "channel", "point") and v.point.values.tolist() == pf.names and str(v.method.values) == "bilinear"
    assert v.lat.values.shape == (n,) and v.lon.values.shape == (n,)
    import csv
    import json
    path = pf.to_csv(tmp_path / "p.csv")
    rows = list(csv.reader(open(path)))
    assert rows[0] == ["time", "member", "channel", "point", "value"] and len(rows) == 1 + x.size
    back = np.array([np.float32(r[4]) for r in rows[1:]]).reshape(T, M, C, n).transpose(1, 0, 2, 3)
    assert np.array_equal(back, x) and rows[1][:4] == [T0.isoformat(), "0", "t2m", "s0"]
    doc = json.loads(pf.to_json())
    assert doc["points"] == pf.names and doc["channels"] == pf.channels and doc["method"] == "bilinear" and doc["n_members"] == M
    assert np.array_equal(np.asarray(doc["values"], np.float32), x) and doc["times"][0] == T0.isoformat()
    pf.forecast_id = "abc"
    assert pf.save(tmp_path) == str(tmp_path / "abc" / "toy-points.json") and json.loads(Path(pf.path).read_text()) == doc | {"forecast_id": "abc"}


# ---- refusals before the device ---------------------------------------------------------------------------------------------------------- #
def test_the_host_limit_and_the_request_checks():
    from skyrim_amd.core.models.utils import _PINNED_LIMIT
    lat, lon = grid(721, 1440)
    names = [f"c{k}" for k in range(69)]
    P.host_limit(50, 41, 8, 100000)
    with pytest.raises(ValueError, match="GiB on the host"):
        P.host_limit(64, 41, 69, _PINNED_LIMIT // (64 * 41 * 69 * 4) + 1)
    pts = {"a": (10.0, 20.0), "b": (-33.3, 151.2)}
    p, ch, rec = P.check_request(names, lat, lon, 50, pts, ["c3", "c0"])
    assert p.names == ["a", "b"] and ch == ["c3", "c0"] and rec.size == 2
    for kw, msg in ((dict(channels=["t2m"]), "not channels"), (dict(n_members=65), "n_members"), (dict(method="cubic"), "unknown method"),
                    (dict(channels=[]), "channels")):
        args = dict(names=names, lat=lat, lon=lon, n_members=50, points=pts, channels=None)
        args.update(kw)
        with pytest.raises(ValueError, match=msg):
            P.check_request(**args)
    with pytest.raises(ValueError, match="'pole'"):
        P.check_request(names, lat[:720], lon, 1, {"pole": (-90.0, 0.0)})
    assert P._sources(["a", "b"], ["d"], None) == (["a", "b", "d"], ["a", "b"], ["d"])
    assert P._sources(["a", "b"], ["d"], ["d", "b"]) == (["d", "b"], ["b"], ["d"])
    with pytest.raises(ValueError, match="neither"):
        P._sources(["a", "b"], [], ["d"])


def test_the_public_entry_points_refuse_before_the_device():
    """Through ``ensemble_forecast`` and ``point_forecast`` of a model whose grid lacks the southern rows and whose loop must not start."""
    import types
    from test_ens_cpu import GEOM, _Loop, _Model
    from skyrim_amd import ensemble as E

    class Loop(_Loop):
        geom = grid = types.SimpleNamespace(lat=np.asarray(GEOM.lat)[:-2], lon=np.asarray(GEOM.lon))

    class Model(_Model):
        def build_model(self):
            return Loop()
    m, full = Model(), _Model()
    south = {"ankara": (39.9, 32.9), "mcmurdo": (-77.8, 166.7)}
    assert np.asarray(m.model.grid.lat).min() > -77.8 > np.asarray(full.model.grid.lat).min()
    for call in (lambda: m.ensemble_forecast(T0, n_steps=2, n_members=3, points=south),
                 lambda: m.ensemble_forecast(T0, n_steps=2, n_members=3, points=south, aggregates=["t2m:max:12h"], point_channels=["t2m"]),
                 lambda: m.point_forecast(T0, 2, points=south), lambda: E.validate(m.model, 2, 3, 0, (), None, None, None, 1, False, points=south)):
        with pytest.raises(ValueError, match="'mcmurdo'.*outside the source latitudes"):
            call()
    assert E.validate(m.model, 2, 3, 0, (), None, None, None, 1, False, points=south, point_method="nearest")[3] == [0, 1, 2]
    for kw, msg in ((dict(point_channels=["msl"]), "msl"), (dict(point_method="cubic"), "unknown method"),
                    (dict(points=[("a", 1, 2), ("a", 3, 4)]), "twice"), (dict(points={"a": (95, 0)}), "lat")):
        with pytest.raises(ValueError, match=msg):
            full.ensemble_forecast(T0, n_steps=2, n_members=3, **{"points": {"ankara": (39.9, 32.9)}, **kw})
    with pytest.raises(ValueError, match="msl"):
        full.point_forecast(T0, 2, points=south, channels=["msl"])
    with pytest.raises(ValueError, match="GiB on the host"):
        full.ensemble_forecast(T0, n_steps=40, n_members=64, points=[(f"s{i}", 0.0, i * 1e-4) for i in range(1 << 20)], point_method="nearest")
    with pytest.raises(RuntimeError, match="GPU"):                             # everything valid: the work itself needs the device
        full.point_forecast(T0, 2, points=south)


# ---- the command line -------------------------------------------------------------------------------------------------------------------- #
def test_command_line_options_and_refusals(tmp_path):
    from click.testing import CliRunner
    from skyrim_amd import point_cli as cli
    assert cli.parse_point("Istanbul:41.01,28.98") == ("Istanbul", 41.01, 28.98)
    assert cli.parse_point("a:b:-3,-9.5") == ("a:b", -3.0, -9.5)
    for bad in ("Istanbul", "Istanbul:41.01", ":1,2", "x:1,2,3", "x:a,b"):
        with pytest.raises(ValueError):
            cli.parse_point(bad)
    csv_path = tmp_path / "st.csv"
    csv_path.write_text("name,lat,lon\nA,1,2\nB,3,-4\n")
    assert cli.request(("A:1,2", "B:3,-4"), "", "out.csv").key() == cli.request((), str(csv_path), "out.JSON").key()
    for args, msg in ((((), "", ""), "not both and not neither"), ((("A:1,2",), str(csv_path), ""), "not both"),
                      ((("A:1,2",), "", "out.txt"), ".json or a .csv"), ((("A:1,2", "A:3,4"), "", ""), "twice"), ((("A:95,2",), "", ""), "lat")):
        with pytest.raises(ValueError, match=msg):
            cli.request(*args)
    with pytest.raises(ValueError, match="n_steps"):
        cli.request(("A:1,2",), "", "", n_steps=-1)
    run = CliRunner().invoke
    for argv in (["--point", "A:1,2", "--stations", str(csv_path)], [], ["--point", "A"], ["--point", "A:1,2", "--output", "x.txt"],
                 ["--point", "A:1,2", "--method", "cubic"], ["--stations", str(tmp_path / "missing.csv")], ["--point", "A:1,2", "--modal"]):
        res = run(cli.point, argv)
        assert res.exit_code == 2, (argv, res.output)
    names = {o.name for o in cli.point.params}
    assert {"point", "stations", "channels", "method", "n_steps", "members", "output", "observations", "model_name", "date", "time",
            "lead_time", "initial_conditions"} <= names
    obs = tmp_path / "obs.csv"
    times = [T0, T0 + datetime.timedelta(hours=6)]
    obs.write_text("time,channel,point,value\n2024-05-13T18:00:00,t2m,A,280.5\n2024-05-14T00:00:00,t2m,B,281\n2024-05-14T00:00:00,msl,B,1\n"
                   "2024-05-14T00:00:00,t2m,C,3\n")
    o = P.read_observations(obs, ["t2m", "ws10m"], times, ["A", "B"])
    assert o["t2m"][0, 0] == 280.5 and o["t2m"][1, 1] == 281 and np.isnan(o["t2m"][0, 1]) and np.isnan(o["ws10m"]).all() and set(o) == {"t2m", "ws10m"}
