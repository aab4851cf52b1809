"""Weather objects without a GPU (include/skyrim_object.h, skyrim_amd/objects.py): the binding policy of libskyrim_object.so, the
argument errors the library finds before anything touches a device, the request parser, the geometry tables, the numpy reference
against scipy's labelling, and the host's float64 formulas on an analytic cap and band."""
import ctypes
import math
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import _object_reference as R
from skyrim_amd import native, objects

INCLUDE = Path(__file__).resolve().parent.parent / "include"
E_ARG = -1


# ---- the binding (the checks of test_native.py for this library) --------------------------------------------------------------------- #
@pytest.fixture
def fresh(monkeypatch):
    monkeypatch.setattr(objects, "_lib", None)


def header() -> str:
    return re.sub(r"/\*.*?\*/", "", (INCLUDE / f"{objects.SPEC.stem}.h").read_text(), flags=re.S)


def test_header_symbols_equal_exports():
    spec = objects.SPEC
    assert spec.env == "SKYRIM_OBJECT_LIB"
    declared = set(re.findall(rf"\b({spec.prefix}_[a-z0-9_]+)\s*\(", header()))
    assert declared == set(objects.EXPORTS) and len(declared) == 5
    lib = objects.load_library()
    for s in sorted(declared):
        assert hasattr(lib, s), f"{s} declared in {spec.stem}.h but not exported"


def test_abi_version_is_the_headers():
    define = int(re.search(r"#define SKOBJ_ABI_VERSION (\d+)", header()).group(1))
    assert objects.load_library().skobj_abi_version() == define == objects.ABI_VERSION == 1


def test_missing_library_is_not_found(fresh, monkeypatch, tmp_path):
    monkeypatch.setenv(objects.SPEC.env, str(tmp_path / "missing.so"))
    with pytest.raises(RuntimeError, match="not found"):
        objects.load_library()


def test_abi_mismatch_is_refused(fresh, monkeypatch):
    monkeypatch.setattr(objects.SPEC, "abi", objects.SPEC.abi + 1)
    with pytest.raises(RuntimeError, match=r"ABI 1, this package binds ABI 2.*rebuild"):
        objects.load_library()


def test_record_and_descriptor_layouts_are_the_headers():
    assert objects.RECORD.itemsize == 128 and R.RECORD == objects.RECORD
    assert objects.RECORD.fields["area"][1] == 32 and objects.RECORD.fields["ext_value"][1] == 120
    assert ctypes.sizeof(objects.PlaneC) == 24
    from skyrim_amd import ops
    assert {"object_label", "object_attributes", "object_probability"} <= set(ops.OP_NAMES)


# ---- argument errors, all found before the device is touched ---------------------------------------------------------------------------- #
def desc(**changes):
    """A descriptor every call accepts as far as the host can tell (the pointers are never followed on this path), then ``changes``."""
    M, P, C, H, W = 2, 2, 3, 19, 70
    d = objects.ObjDesc()
    d.M, d.C, d.H, d.W, d.P, d.periodic, d.min_pixels, d.capacity = M, C, H, W, P, 1, 1, 16
    for p in range(P):
        d.planes[p] = objects.PlaneC(p, 1.0, 1 if p == 0 else -1, 8 if p == 0 else 4, 1.0, 0)
    for k, name in enumerate(("members", "labels", "ids", "n_found", "workspace", "row_tables", "col_tables", "records", "keep", "counts")):
        setattr(d, name, 0x10000 * (k + 1))
    d.workspace_bytes = objects.workspace_bytes(M, P, H, W)
    for k, v in changes.items():
        if k.startswith("plane_"):
            setattr(d.planes[1], k[6:], v)
        else:
            setattr(d, k, v)
    return d


LABEL_ERRORS = [dict(members=0), dict(labels=0), dict(ids=0), dict(n_found=0), dict(workspace=0), dict(members=0x10004), dict(labels=0x20002),
                dict(ids=0x30001), dict(n_found=0x40002), dict(workspace=0x50004), dict(P=0), dict(P=9), dict(M=0), dict(M=65),
                dict(plane_connectivity=5), dict(plane_direction=0), dict(plane_channel=3), dict(plane_channel=-1), dict(plane_value_scale=3.0),
                dict(plane_value_scale=0.0), dict(plane_threshold=math.nan), dict(capacity=0), dict(capacity=(1 << 20) + 1), dict(min_pixels=0),
                dict(workspace_bytes=objects.workspace_bytes(2, 2, 19, 70) - 1), dict(H=0), dict(W=0), dict(C=0), dict(C=1 << 20, H=1 << 10, W=2)]


@pytest.mark.parametrize("change", LABEL_ERRORS, ids=lambda c: ",".join(f"{k}={v}" for k, v in c.items()))
def test_label_argument_errors(change):
    assert objects.load_library().skobj_label(ctypes.byref(desc(**change)), None) == E_ARG


@pytest.mark.parametrize("change", [dict(members=0), dict(labels=0), dict(ids=0x30002), dict(n_found=0), dict(row_tables=0), dict(row_tables=0x60004),
                                    dict(col_tables=0), dict(col_tables=0x70004), dict(records=0), dict(records=0x80004), dict(P=9), dict(M=65),
                                    dict(plane_connectivity=5), dict(capacity=0)], ids=lambda c: ",".join(f"{k}={v}" for k, v in c.items()))
def test_attributes_argument_errors(change):
    assert objects.load_library().skobj_attributes(ctypes.byref(desc(**change)), None) == E_ARG


@pytest.mark.parametrize("change", [dict(ids=0), dict(ids=0x30002), dict(keep=0), dict(counts=0), dict(counts=0xa0002), dict(P=0), dict(P=9), dict(M=0),
                                    dict(M=65), dict(capacity=0)], ids=lambda c: ",".join(f"{k}={v}" for k, v in c.items()))
def test_probability_argument_errors(change):
    assert objects.load_library().skobj_probability(ctypes.byref(desc(**change)), None) == E_ARG


def test_null_descriptor_and_workspace_query():
    lib = objects.load_library()
    for call in (lib.skobj_label, lib.skobj_attributes, lib.skobj_probability):
        assert call(None, None) == E_ARG
    assert objects.workspace_bytes(2, 2, 19, 70) == 4 * 2 * 2 * (19 * 70 + 2)
    assert objects.workspace_bytes(1, 1, 721, 1440) % 8 == 0 and objects.workspace_bytes(1, 1, 3, 3) == 40
    for bad in ((0, 1, 4, 4), (65, 1, 4, 4), (1, 0, 4, 4), (1, 9, 4, 4), (1, 1, 0, 4), (1, 1, 4, 0), (1, 1, 1 << 16, 1 << 16)):
        assert objects.workspace_bytes(*bad) == 0


# ---- the request ------------------------------------------------------------------------------------------------------------------------ #
def test_request_is_normalised():
    req = objects.parse_request({"ivt": {"above": [250.0, 500.0], "min_area_km2": 2e5, "min_length_km": 2000.0, "min_elongation": 2.0},
                                 "t2m": {"below": [253.15]}, "connectivity": 8, "min_pixels": 4, "capacity": 1024}, ["t2m", "msl", "ivt"], 50)
    assert [p.label for p in req.planes] == ["ivt>=250", "ivt>=500", "t2m<=253.15"]
    assert [(p.direction, p.value_scale) for p in req.planes] == [(1, 256.0), (1, 512.0), (-1, 256.0)]
    assert req.planes[2].threshold == float(np.float32(253.15)) and req.planes[0].min_length_km == 2000.0 and req.planes[2].min_area_km2 == 0.0
    assert (req.connectivity, req.min_pixels, req.capacity) == (8, 4, 1024)
    assert objects.parse_request(req, ["ivt", "t2m"]) is req
    assert objects.parse_request({"msl": {"below": 100000.0}}, ["msl"]).planes[0].value_scale == 131072.0


def test_value_scale_is_the_power_of_two_at_or_above():
    assert [objects.value_scale(t) for t in (0.0, 1.0, -1.0, 250.0, 256.0, 257.0, 0.3, 17.0, -253.15)] == [1, 1, 1, 256, 256, 512, 0.5, 32, 256]


@pytest.mark.parametrize("request_,n,match", [
    ({"ivt": {"above": [250.0]}}, 1, "neither output channels"),
    ({"msl": {"above": list(range(9))}}, 1, "9 planes"),
    ({}, 1, "0 planes"),
    ({"msl": {"above": [1.0]}}, 65, "1 to 64 members"),
    ({"msl": {"above": [1.0]}}, 0, "1 to 64 members"),
    ({"msl": {"over": [1.0]}}, 1, "unknown keys"),
    ({"msl": {"min_area_km2": 5.0}}, 1, "no threshold"),
    ({"msl": {"above": [math.inf]}}, 1, "not finite"),
    ({"msl": {"above": [1.0, 1.0]}}, 1, "named twice"),
    ({"msl": {"above": [1.0], "min_area_km2": -1.0}}, 1, "filters are >= 0"),
    ({"msl": {"above": [1.0]}, "connectivity": 5}, 1, "connectivity is 4 or 8"),
    ({"msl": {"above": [1.0]}, "capacity": 0}, 1, "capacity"),
    ({"msl": {"above": [1.0]}, "min_pixels": 0}, 1, "min_pixels"),
    ({"msl": [1.0]}, 1, "a dict with"),
    ([("msl", 1.0)], 1, "objects: a dict"),
])
def test_request_refusals(request_, n, match):
    with pytest.raises(ValueError, match=match):
        objects.parse_request(request_, ["msl", "t2m"], n)


# ---- the tables ------------------------------------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize("H,W,poles", [(721, 1440, True), (720, 1440, False), (33, 64, True), (19, 70, True)])
def test_tables_sum_to_the_sphere(H, W, poles):
    lat = np.linspace(90.0, -90.0, H) if poles else 90.0 - (np.arange(H) + 0.5) * 180.0 / H
    g = objects.tables(lat, np.arange(W) * 360.0 / W)
    assert g.periodic and g.row.shape == (6, H) and g.col.shape == (5, W) and g.row.dtype == g.col.dtype == np.float64
    total = int(np.rint(g.row[0]).astype(np.int64).sum()) * W     # what `area` sums to over the whole grid
    assert abs(total - 2 ** 52) <= H * W                        # one rounding of at most 0.5 per point, and float64 noise in sin
    assert np.all(np.abs(g.row[1:]) <= g.row[0] * (1 + 1e-15)) and np.all(np.abs(g.col) <= 1)
    np.testing.assert_allclose(g.row[3] + g.row[5], g.row[0], rtol=1e-14)
    rr, cc = R.tables(lat, np.arange(W) * 360.0 / W)
    np.testing.assert_allclose(g.row, rr, rtol=1e-12, atol=1e-3)
    np.testing.assert_array_equal(g.col, cc)


def test_regional_box_is_not_periodic():
    g = objects.tables(np.linspace(60.0, 30.0, 31), np.arange(-20.0, 41.0))
    assert not g.periodic
    band = (math.sin(math.radians(60.5)) - math.sin(math.radians(29.5))) / 2 * 61 / 360
    assert abs(np.rint(g.row[0]).sum() * 61 / 2 ** 52 - band) < 1e-12
    with pytest.raises(ValueError, match="uniform longitudes"):
        objects.tables(np.linspace(60.0, 30.0, 31), np.array([0.0, 1.0, 3.0]))
    with pytest.raises(ValueError, match="monotonic latitude"):
        objects.tables(np.array([0.0, 1.0, 0.5]), np.arange(4.0))


# ---- the reference against scipy -------------------------------------------------------------------------------------------------------- #
def relabel(lab):
    """Any labelling -> 1 + the smallest index of each label's points."""
    out = np.zeros(lab.shape, np.int32)
    flat = lab.ravel()
    idx = np.flatnonzero(flat)
    first = {}
    for q in idx.tolist():
        first.setdefault(int(flat[q]), q + 1)
    out.ravel()[idx] = [first[int(flat[q])] for q in idx.tolist()]
    return out


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("periodic", [False, True])
def test_reference_labels_equal_scipy(connectivity, periodic):
    ndimage = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(5)
    H, W = 23, 37
    mask = rng.random((H, W)) < 0.45
    mask[:, 0] |= rng.random(H) < 0.5
    mask[:, -1] |= rng.random(H) < 0.5
    structure = np.ones((3, 3), int) if connectivity == 8 else ndimage.generate_binary_structure(2, 1)
    got = R.flood_labels(mask, connectivity, periodic)
    if not periodic:
        np.testing.assert_array_equal(got, relabel(ndimage.label(mask, structure)[0]))
        return
    # the image padded by wrapping: one copy of the last column in front, one of the first behind.  A padded point and the point it
    # copies are the same point of the circle, so their labels are joined
    lab = ndimage.label(np.concatenate([mask[:, -1:], mask, mask[:, :1]], axis=1), structure)[0]
    parent = list(range(int(lab.max()) + 1))

    def find(v):
        while parent[v] != v:
            v = parent[v]
        return v
    for j in range(H):
        for a, b in ((lab[j, 0], lab[j, W]), (lab[j, W + 1], lab[j, 1])):
            if a:
                parent[find(int(a))] = find(int(b))
    merged = np.array([find(v) for v in range(len(parent))])[lab[:, 1:W + 1]]
    np.testing.assert_array_equal(got, relabel(merged))


def test_reference_numbering_and_counts():
    lab = np.array([[1, 0, 3, 3], [1, 0, 0, 3], [0, 10, 0, 0], [13, 0, 0, 16]], np.int32)
    ids, n, roots = R.number(lab, 2, 8)
    np.testing.assert_array_equal(ids, [[1, 0, 2, 2], [1, 0, 0, 2], [0, 0, 0, 0], [0, 0, 0, 0]])
    assert n == 2 and roots.tolist() == [0, 2]
    ids, n, roots = R.number(lab, 1, 3)
    assert n == 5 and ids[3, 0] == 0 and ids[2, 1] == 3 and roots.tolist() == [0, 2, 9]
    keep = np.zeros((2, 1, 4), np.uint8)
    keep[0, 0, 2] = keep[1, 0, 1] = keep[1, 0, 2] = 1
    both = np.stack([ids, ids])[:, None]
    np.testing.assert_array_equal(R.probability_counts(both, keep)[0], (ids == 2) * 2 + (ids == 1) * 1)


def test_extreme_key_orders_values_then_lower_index():
    v = np.array([1.0, -0.0, 0.0, 3.5, 3.5, -np.inf, np.inf, -2.0], np.float32)
    idx = np.arange(v.size)
    hi, lo = R.ordered_key(v, 1, idx), R.ordered_key(v, -1, idx)
    assert R.key_value(hi[:6].max(), 1) == (np.float32(3.5), 3) and R.key_value(hi.max(), 1) == (np.float32(np.inf), 6)
    assert R.key_value(lo.max(), -1) == (np.float32(-np.inf), 5) and R.key_value(lo[[0, 1, 2, 3]].max(), -1)[1] == 1


# ---- the host's formulas on analytic shapes ------------------------------------------------------------------------------------------- #
LAT, LON = np.linspace(90.0, -90.0, 181), np.arange(360.0)


def shape_properties(mask, periodic=True):
    g = objects.tables(LAT, LON)
    ids, n, _ = R.number(R.flood_labels(mask, 8, periodic), 1, 16)
    v = np.where(mask, 7.0, 0.0).astype(np.float32)
    rec = R.records(v, ids, g.row, g.col, 1, 8.0)
    return rec, objects.properties(rec, LAT, LON, 8.0)


@pytest.mark.parametrize("lat0,lon0", [(35.0, 40.0), (-50.0, 359.0), (10.0, 180.0)])
def test_cap_centroid_area_and_axes(lat0, lon0):
    radius = 20.0
    p0, l0 = math.radians(lat0), math.radians(lon0)
    phi, lam = np.radians(LAT)[:, None], np.radians(LON)[None, :]
    cosd = np.sin(phi) * math.sin(p0) + np.cos(phi) * math.cos(p0) * np.cos(lam - l0)
    rec, pr = shape_properties(cosd >= math.cos(math.radians(radius)))
    assert len(pr) == 1 and pr["n_pixels"][0] == rec["n_pixels"][0] > 1000          # one object, also across the date line
    assert objects.great_circle_km(pr["lat"][0], pr["lon"][0], lat0, lon0) < 30.0     # the axis, within a fraction of a 111-km cell
    exact = 2 * math.pi * R.R_KM ** 2 * (1 - math.cos(math.radians(radius)))
    # discretisation: the boundary cells, a strip of at most one cell diagonal along the cap's perimeter
    strip = 2 * math.pi * R.R_KM * math.sin(math.radians(radius)) * math.hypot(111.2, 111.2)
    assert abs(pr["area_km2"][0] - exact) <= strip and abs(pr["area_km2"][0] - exact) / exact < 0.02
    # a disc of angular radius r: both variances are about (R sin r)^2 / 4, so both axes about the chord 2 R sin r
    chord = 2 * R.R_KM * math.sin(math.radians(radius))
    assert 0.9 * chord < pr["width_km"][0] <= pr["length_km"][0] < 1.1 * chord
    bound = 0.5 * rec["n_pixels"][0] * 2.0 ** -40 * 8.0 / (rec["area"][0] / 2.0 ** 52)          # the header's bound on the mean
    assert abs(pr["mean"][0] - 7.0) <= bound < 1e-6 and pr["extreme"][0] == 7.0 and pr["saturated"][0] == 0
    ref = R.host_properties(rec, LAT, LON, 8.0)
    for k in ("area_km2", "lat", "lon", "mean"):
        np.testing.assert_allclose(pr[k], ref[k], rtol=1e-12, atol=1e-9)


def test_zonal_band_is_long_thin_and_east_west():
    mask = np.zeros((181, 360), bool)
    rows = np.nonzero((LAT >= 10.0) & (LAT <= 15.0))[0]
    mask[rows[0]:rows[-1] + 1, 20:101] = True                    # 6 rows x 81 columns at 12.5 N
    rec, pr = shape_properties(mask)
    o = pr[0]
    length = math.radians(81.0) * R.R_KM * math.cos(math.radians(12.5))
    assert o["length_km"] > 8 * o["width_km"]
    assert 0.9 * length * 4 / math.sqrt(12) < o["length_km"] < 1.1 * length * 4 / math.sqrt(12)      # a uniform strip: variance L^2 / 12
    assert 0.8 * 6 * 111.2 * 4 / math.sqrt(12) < o["width_km"] < 1.2 * 6 * 111.2 * 4 / math.sqrt(12)
    assert min(o["orientation_deg"], 180.0 - o["orientation_deg"]) < 2.0
    # the mean unit vector of an arc of a parallel: its equatorial part shrinks by sin(h) / h (h = half the arc), so it points poleward
    h = math.radians(40.5)
    assert abs(o["lat"] - math.degrees(math.atan(math.tan(math.radians(12.5)) * h / math.sin(h)))) < 0.1 and abs(o["lon"] - 60.0) < 1e-6
    exact = R.R_KM ** 2 * math.radians(81.0) * (math.sin(math.radians(15.5)) - math.sin(math.radians(9.5)))
    assert abs(o["area_km2"] - exact) / exact < 1e-9             # whole cells: only float64 rounding
    plane = objects.Plane("x", 1, 1.0, 1.0, min_area_km2=1e5, min_length_km=2000.0, min_elongation=2.0)
    assert objects.keep_mask(pr, plane).tolist() == [True]
    assert objects.keep_mask(pr, objects.Plane("x", 1, 1.0, 1.0, min_elongation=50.0)).tolist() == [False]


def test_objects_json_round_trip_and_probability(tmp_path):
    mask = np.zeros((181, 360), bool)
    mask[80:90, 350:] = mask[80:90, :12] = True
    mask[20:24, 100:130] = True
    rec, pr = shape_properties(mask)
    req = objects.parse_request({"x": {"above": [1.0], "min_area_km2": 1e6}, "capacity": 1}, ["x"])
    pr["keep"] = objects.keep_mask(pr, req.planes[0])
    counts = [[(mask & (np.arange(181)[:, None] >= 50)).astype(np.int32)]]
    when = __import__("datetime").datetime(2024, 1, 1, 6)
    with pytest.warns(UserWarning, match="more than capacity"):
        obj = objects.Objects("toy", 1, [when], LAT, LON, req, [[[pr]]], counts, [[[2]]], [[pr]], [[np.array([0.0, 1.0])]], "abc")
    assert obj.truncated.tolist() == [[[True]]] and obj.count(0).tolist() == [[1]] and obj.planes == ["x>=1"]
    prob = obj.probability("x>=1")
    assert tuple(prob.dims) == ("time", "lat", "lon") and float(np.asarray(prob.values).max()) == 1.0
    path = obj.save(tmp_path)
    assert path.endswith("abc/toy-objects.json")
    back = objects.Objects.load(path)
    assert back.to_json() == obj.to_json()
    np.testing.assert_array_equal(np.asarray(back.probability(0).values), np.asarray(prob.values))
    rows = back.verify()
    assert rows[0]["hit_rate"] == 1.0 and rows[0]["centroid_error_km"] == 0.0 and rows[0]["false_alarm_ratio"] == 0.0
    assert rows[0]["area_ratio"] == 1.0 and rows[0]["probability"] == 1.0 and rows[0]["n_truth"] == 1
    with pytest.raises(ValueError, match="no plane"):
        obj.probability("y>=1")


def test_command_line_parses_its_planes():
    import click
    from click.testing import CliRunner
    from skyrim_amd import object_cli
    res = CliRunner().invoke(object_cli.objects, ["--help"])
    assert res.exit_code == 0 and object_cli.objects.name == "objects" and "--min_area_km2" in res.output
    req = object_cli.parse_objects(["ivt:above:250,500", "t2m:below:253.15", "ivt:below:10"], 4, 3, None, min_area_km2=2e5, min_length_km=None)
    assert req == {"ivt": {"min_area_km2": 2e5, "above": [250.0, 500.0], "below": [10.0]}, "t2m": {"min_area_km2": 2e5, "below": [253.15]},
                   "connectivity": 4, "min_pixels": 3}
    assert [p.label for p in objects.parse_request(req, ["ivt", "t2m"]).planes] == ["ivt>=250", "ivt>=500", "ivt<=10", "t2m<=253.15"]
    for bad in (["ivt:over:250"], ["ivt:above"], ["ivt:above:a"], []):
        with pytest.raises(click.UsageError):
            object_cli.parse_objects(bad)


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not installed")
def test_kernels_use_no_scratch():
    r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "--cuda-device-only", "-c",
                        "object_ops.hip", "-o", "/dev/null", "-Rpass-analysis=kernel-resource-usage"], cwd=INCLUDE.parent / "skyrim_amd" / "csrc",
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    out, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"\sScratchSize \[bytes/lane\]: (\d+)", line)
        if m and name:
            out[name] = int(m.group(1))
    kernels = ("tile", "border", "flatten", "chunk", "scan", "number", "id", "init", "sum", "finish", "probability")
    assert len(out) == len(kernels) and all(any(f"obj_{k}_kernel" in n for n in out) for k in kernels)
    assert set(out.values()) == {0}, out
