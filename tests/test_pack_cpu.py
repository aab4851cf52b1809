"""Packed member archives without a GPU: the binding of libskyrim_pack.so against its header, every SKPACK_E_ARG path through the host-only
``*_check`` entry points, the numpy restatement's own properties against float64 (the header's bound, the endpoints, the special planes),
the packed netCDF-3 format, ``open_saved`` on packed files, the manifest, and every refusal of ``archive=`` and of ``replay``."""
import ctypes
import datetime
import inspect
import json
import re
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

import _pack_reference as R
from skyrim_amd import archive as A
from skyrim_amd import native, ncio
from skyrim_amd.labeled import DataArray, open_dataarray

ROOT = Path(__file__).resolve().parents[1]
E_ARG = -1
PTR = 0x7F0000001000                          # a 16-byte aligned address that is never read: every refusal comes before the GPU
T0 = datetime.datetime(2024, 5, 13, 18, 0)
LAT, LON = np.linspace(90, -90, 5), np.arange(7) * 51.0


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- the binding ------------------------------------------------------------------------------------------------------------------------- #
def test_header_binding_and_build_line():
    text = (ROOT / "include/skyrim_pack.h").read_text()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(skpack_[a-z0-9_]+)\s*\(", code))
    lib = A.load_library()
    assert declared == set(A.EXPORTS) and all(hasattr(lib, s) for s in declared)
    assert lib.skpack_abi_version() == A.ABI_VERSION == int(re.search(r"#define SKPACK_ABI_VERSION (\d+)", text).group(1))
    assert A.SPEC.env == "SKYRIM_PACK_LIB"
    for name, value in (("MAX_MEMBERS", A.MAX_MEMBERS), ("MAX_CHANNELS", A.MAX_CHANNELS), ("RANGE_TILE", A.RANGE_TILE)):
        assert re.search(rf"#define SKPACK_{name} {value}\b", text), name
    assert "#define SKPACK_FILL (-32768)" in text and A.FILL == R.FILL == ncio.PACK_FILL == -32768
    assert "#define SKPACK_E_ARG (-1)" in text and "#define SKPACK_E_HIP (-2)" in text
    assert ctypes.sizeof(A.Entry) == 40 == A.ENTRY.itemsize == R.ENTRY.itemsize and A.ENTRY == R.ENTRY
    assert [(n, A.ENTRY.fields[n][1]) for n in A.ENTRY.names] == [(n, getattr(A.Entry, n).offset) for n, _ in A.Entry._fields_]
    # members, five ints, channels, (padding), table, workspace and its size, out and its stride
    assert ctypes.sizeof(A.Desc) == 8 + 5 * 4 + 4 * 256 + 4 + 5 * 8
    assert ctypes.sizeof(A.UnpackDesc) == 8 + 8 + 3 * 4 + 4 + 8
    assert "subnormals are KEPT" in text and "0.5 t.scale (1 + 2^-20) + 2^-24 max(|t.lo|, |t.hi|) + 2^-149" in text
    make = (ROOT / "skyrim_amd/csrc/Makefile").read_text()
    assert "-ffp-contract=off -shared -o $@ pack_ops.hip" in make and "$(LIB_PACK)" in make.split("all:")[1].splitlines()[0]
    assert "$(LIB_PACK)" in make.split("clean:")[1]
    for doc in (native.__doc__, make.splitlines()[0]):
        assert ",pack," in doc
    from skyrim_amd import ops
    assert {"pack_range", "pack_quantize", "pack_unpack"} <= set(ops.OP_NAMES)
    assert all(f"    {n}" in ops.__doc__ or f"/ {n}" in ops.__doc__ for n in ("pack_range", "pack_quantize", "pack_unpack"))
    assert "skpack_abi_version() == 1" in (ROOT / "__graft_entry__.py").read_text()
    tiles = -(-721 * 1440 // A.RANGE_TILE)
    assert A.workspace_bytes(50, 69, 721, 1440) == 12 * 50 * 69 * tiles and A.workspace_bytes(1, 1, 1, 2) == 12
    assert [A.workspace_bytes(*a) for a in ((0, 1, 2, 2), (1025, 1, 2, 2), (1, 0, 2, 2), (1, 257, 2, 2), (1, 1, 0, 2), (1, 5, 1 << 14, 1 << 14))] == [0] * 6


def good(out=True):
    d = A.describe(3, 5, 9, 12, [4, 0, 4])
    d.members, d.table, d.workspace, d.workspace_bytes = PTR, PTR, PTR, A.workspace_bytes(3, 3, 9, 12)
    d.out, d.member_stride_bytes = PTR + 2, 2 * 3 * 9 * 12 + 6
    return d


def test_range_and_quantize_refuse_bad_arguments_without_a_gpu():
    lib = A.load_library()
    for fn in (lib.skpack_range, lib.skpack_quantize):
        assert fn(None, None) == E_ARG
    assert lib.skpack_range_check(None) == lib.skpack_quantize_check(None) == lib.skpack_unpack_check(None) == E_ARG
    assert lib.skpack_range_check(ctypes.byref(good())) == 0 and lib.skpack_quantize_check(ctypes.byref(good())) == 0

    def refused(check, edit=None, **kw):
        d = good()
        for k, v in kw.items():
            setattr(d, k, v)
        if edit is not None:
            edit(d)
        return check(ctypes.byref(d)) == E_ARG
    for check in (lib.skpack_range_check, lib.skpack_quantize_check):
        assert refused(check, members=None) and refused(check, members=PTR + 4) and refused(check, table=None) and refused(check, table=PTR + 4)
        assert refused(check, M=0) and refused(check, M=1025) and refused(check, nc=0) and refused(check, nc=257)
        assert refused(check, C=0) and refused(check, H=0) and refused(check, W=0)
        assert refused(check, C=1 << 15, H=1 << 8, W=1 << 8) and refused(check, C=5, nc=5, H=1 << 14, W=1 << 14)      # C H W, nc H W > 2^30
        assert refused(check, lambda d: d.channels.__setitem__(1, 5)) and refused(check, lambda d: d.channels.__setitem__(2, -1))
    rc, qc = lib.skpack_range_check, lib.skpack_quantize_check
    assert refused(rc, workspace=None) and refused(rc, workspace=PTR + 2) and refused(rc, workspace_bytes=A.workspace_bytes(3, 3, 9, 12) - 1)
    assert not refused(rc, out=None, member_stride_bytes=1)                                    # what the other call reads is ignored
    assert refused(qc, out=None) and refused(qc, out=PTR + 1) and refused(qc, member_stride_bytes=2 * 3 * 9 * 12 + 1)
    assert refused(qc, member_stride_bytes=2 * 3 * 9 * 12 - 2) and not refused(qc, member_stride_bytes=2 * 3 * 9 * 12)
    assert not refused(qc, workspace=None, workspace_bytes=0)
    # the calls themselves refuse the same descriptors before they touch a GPU
    d = good()
    d.M = 0
    assert lib.skpack_range(ctypes.byref(d), None) == E_ARG and lib.skpack_quantize(ctypes.byref(d), None) == E_ARG
    with pytest.raises(NotImplementedError):
        import torch
        torch.ops.skyrim_hip.pack_unpack(torch.zeros(8, dtype=torch.uint8), torch.zeros(1, 5, dtype=torch.float64), torch.zeros(1, 2, 2))


def test_unpack_refuses_bad_arguments_without_a_gpu():
    lib = A.load_library()

    def refused(**kw):
        d = A.UnpackDesc()
        d.codes, d.table, d.nc, d.H, d.W, d.out = PTR + 2, PTR, 3, 5, 7, PTR + 4
        for k, v in kw.items():
            setattr(d, k, v)
        return lib.skpack_unpack_check(ctypes.byref(d)) == E_ARG and lib.skpack_unpack(ctypes.byref(d), None) == E_ARG
    d = A.UnpackDesc()
    d.codes, d.table, d.nc, d.H, d.W, d.out = PTR + 2, PTR, 3, 5, 7, PTR + 4
    assert lib.skpack_unpack_check(ctypes.byref(d)) == 0
    assert refused(codes=None) and refused(codes=PTR + 1) and refused(table=None) and refused(table=PTR + 4)
    assert refused(out=None) and refused(out=PTR + 2) and refused(nc=0) and refused(nc=257) and refused(H=0) and refused(W=0)
    assert refused(nc=5, H=1 << 14, W=1 << 14)


# ---- the restatement's own properties, against float64 --------------------------------------------------------------------------------------- #
def field(M, H, W, seed, c=6):
    """field() of tests/test_point_kernels_gpu.py: mixed magnitude."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((M, c, H, W), dtype=np.float32)
    scale = np.array([250.0, 54000.0, 25.0, 8.0, 1e-3, 1e-30, 1e5, 3.0, 0.02] * 8)[:c]
    shift = np.array([250.0, 5e4, 0.0, 0.0, 5e-3, 0.0, 1e5, -3.0, 0.0] * 8)[:c]
    x *= scale.astype(np.float32)[None, :, None, None]
    x += shift.astype(np.float32)[None, :, None, None]
    return x


def round_trip(plane):
    """(record, codes, decoded) of one plane (H, W)."""
    tab = R.table([plane[None]], [0])
    c = R.codes(plane[None], tab[0])
    return tab[0, 0], c[0], R.decode(c, tab[0])[0]


def test_the_bound_holds_and_the_endpoints_get_the_end_codes():
    rng = np.random.default_rng(3)
    planes = [p for st in field(2, 40, 50, 1) for p in st]
    planes.append((rng.standard_normal((40, 50)) * 1e-41).astype(np.float32))                        # subnormal
    planes.append((rng.standard_normal((40, 50)) * 4e37).astype(np.float32) + np.float32(2e38))      # near FLT_MAX
    planes.append(np.float32(3.3e38) * (rng.random((40, 50), dtype=np.float32) * 2 - 1))             # the whole range
    planes.append((rng.standard_normal((40, 50)) * 1e-3 + 1000.0).astype(np.float32))                 # a spread of a few ulps
    planes.append(np.float32(1e-42) * rng.integers(-5, 6, (40, 50)).astype(np.float32))
    worst = 0.0
    for p in planes:
        rec, c, dec = round_trip(p)
        assert np.isfinite(dec).all() and c.min() == -32767 and c.max() == 32767
        assert np.all(c[p == rec["lo"]] == -32767) and np.all(c[p == rec["hi"]] == 32767)
        err = np.abs(dec.astype(np.float64) - p.astype(np.float64))
        ratio = float((err / R.bound(err, rec)).max())
        assert ratio <= 1.0, (ratio, rec)
        worst = max(worst, ratio)
        assert rec["scale"] * rec["inv"] == pytest.approx(1.0, rel=1e-15) and rec["lo"] == p.min() and rec["hi"] == p.max() and rec["n_bad"] == 0
    assert worst > 0.5                                     # the bound is not slack by more than a factor of two


def test_special_planes():
    rec, c, dec = round_trip(np.full((5, 7), -273.15, np.float32))                  # constant: codes 0, decoded exactly
    assert (rec["scale"], rec["inv"]) == (1.0, 1.0) and not c.any() and np.array_equal(bits(dec), bits(np.full((5, 7), -273.15, np.float32)))
    rec, c, dec = round_trip(np.full((5, 7), np.nan, np.float32))                   # no finite value
    assert tuple(rec)[:5] == (0.0, 1.0, 1.0, 0.0, 0.0) and rec["n_bad"] == 35 and np.all(c == R.FILL)
    assert np.all(bits(dec) == 0x7FC00000)
    rec, c, dec = round_trip(np.full((5, 7), -0.0, np.float32))                     # -0 is +0
    assert bits(rec["lo"]) == 0 and bits(rec["hi"]) == 0 and np.all(bits(dec) == 0) and not c.any()
    p = np.linspace(-1, 1, 35, dtype=np.float32).reshape(5, 7)
    p[0, 0], p[2, 3], p[4, 6] = np.inf, np.nan, -np.inf                             # the infinities do not widen the range
    rec, c, dec = round_trip(p)
    assert rec["n_bad"] == 3 and rec["hi"] == p[np.isfinite(p)].max() and rec["lo"] == p[np.isfinite(p)].min()
    assert c[0, 0] == c[2, 3] == c[4, 6] == R.FILL and np.all(bits(dec)[~np.isfinite(p)] == 0x7FC00000) and np.isfinite(dec[np.isfinite(p)]).all()
    assert (c[np.isfinite(p)] != R.FILL).all()
    rec, c, dec = round_trip(np.array([[-0.0, 1.5]], np.float32))                   # 1 x 2
    assert c.tolist() == [[-32767, 32767]] and dec.tolist() == [[0.0, 1.5]]
    half = np.array([[0.0, 65534.0, 0.5, 1.5, 2.5]], np.float32)                    # scale 1, offset 32767: halves go to the even code
    rec, c, dec = round_trip(half)
    assert rec["scale"] == 1.0 and c[0, 2:].tolist() == [-32766, -32766, -32764]
    img = R.quantize([half[None]], [0])[0]
    assert img[:4] == b"\x80\x01\x7f\xff"                                           # big-endian -32767, 32767


# ---- the file format ----------------------------------------------------------------------------------------------------------------------- #
def packed(nc, seed=0, t=T0):
    """(DataArray, state, table row, image bytes) of one state (nc, 5, 7)."""
    st = field(1, 5, 7, seed, nc)[0]
    st[0, 1, 1] = np.nan
    tab = R.table([st], range(nc))
    img = R.quantize([st], range(nc), tab)[0]
    names = [f"c{k}" for k in range(nc)]
    return A.packed_dataarray(np.frombuffer(img, np.uint8), tab[0], t, names, LAT, LON), st, tab[0], img


@pytest.mark.parametrize("nc", [2, 3])                     # 70 codes, and 105: an odd count, two bytes of padding
def test_packed_file_is_byte_identical_to_the_plain_writer_and_reads_back(tmp_path, nc):
    from scipy.io import netcdf_file
    da, st, tab, img = packed(nc)
    ncio.write_dataarray_netcdf3(da, tmp_path / "image.nc")                         # header by scipy, the image by pwrite
    plain = DataArray(np.frombuffer(img, ">i2").reshape(1, nc, 5, 7).astype(np.int16), da.dims, dict(da._coords))
    plain._packed = ncio.PackedImage(np.frombuffer(img, np.uint8), (1, nc, 5, 7), tab["scale"], tab["offset"])
    ncio._write_netcdf3(plain, tmp_path / "plain.nc", False, None, plain._packed)    # scipy writes the same int16 array itself
    a, b = (tmp_path / "image.nc").read_bytes(), (tmp_path / "plain.nc").read_bytes()
    assert a == b and img in a and not list(tmp_path.glob("*.part"))
    with netcdf_file(str(tmp_path / "image.nc"), "r", mmap=False) as f:
        v = f.variables[ncio.UNNAMED]
        assert v.typecode() == "h" and v.dimensions == ("time", "channel", "lat", "lon") and v._FillValue == -32768
        assert f.skyrim_packing == b"linear16"
        for name, key in (("scale_factor", "scale"), ("add_offset", "offset")):
            t = f.variables[name]
            assert t.typecode() == "d" and t.dimensions == ("time", "channel") and np.array_equal(t[...].reshape(-1), tab[key])
    want = R.unpack(img, tab, (nc, 5, 7))
    got = open_dataarray(tmp_path / "image.nc")
    assert got.dtype == np.float32 and got.dims == ("time", "channel", "lat", "lon") and sorted(got._coords) == ["channel", "lat", "lon", "time"]
    assert np.array_equal(bits(got.values[0]), bits(want)) and bits(got.values[0, 0, 1, 1]) == 0x7FC00000
    assert got.channel.values.tolist() == [f"c{k}" for k in range(nc)] and np.array_equal(got._coords["lat"], LAT)
    raw = open_dataarray(tmp_path / "image.nc", raw=True)
    assert raw.dtype.kind == "i" and raw.dtype.itemsize == 2 and np.array_equal(raw.values[0], R.codes(st, tab))
    assert bytes(raw.packed.image) == img and np.array_equal(raw.packed.scale[0], tab["scale"]) and np.array_equal(raw.packed.offset[0], tab["offset"])
    assert np.array_equal(bits(raw.packed.decode()[0]), bits(want))
    ncio.write_dataarray_netcdf3(raw, tmp_path / "again.nc")                         # a raw read writes the same file again
    assert (tmp_path / "again.nc").read_bytes() == a
    raw.values = raw.values.astype(np.float32)                                      # assigning values drops the packing
    assert raw.packed is None


def test_unmarked_files_read_as_before(tmp_path):
    x = field(1, 5, 7, 4, 2)
    da = DataArray(x, ["time", "channel", "lat", "lon"], dict(time=np.asarray([np.datetime64(T0, "ns")]), channel=["a", "b"], lat=LAT, lon=LON))
    for thr in (None, 0):
        ncio.write_dataarray_netcdf3(da, tmp_path / "f.nc", fast_threshold=thr)
        back = open_dataarray(tmp_path / "f.nc")
        assert back.dtype == np.float32 and np.array_equal(bits(back.values), bits(x)) and back.packed is None
        assert np.array_equal(ncio.read_payload_netcdf3(tmp_path / "f.nc"), x) and ncio.read_payload_netcdf3(tmp_path / "f.nc").dtype == np.dtype(">f4")
    with pytest.raises(ValueError, match="not a packed file"):
        open_dataarray(tmp_path / "f.nc", raw=True)
    codes = DataArray(np.arange(70, dtype=np.int16).reshape(1, 2, 5, 7), da.dims, dict(da._coords))      # plain int16: no marker, no decoding
    ncio.write_dataarray_netcdf3(codes, tmp_path / "i.nc")
    assert np.array_equal(open_dataarray(tmp_path / "i.nc").values, codes.values)
    with pytest.raises(ValueError, match="packed image of"):
        ncio.PackedImage(np.zeros(10, np.uint8), (1, 2, 5, 7), np.ones(2), np.zeros(2))


def test_open_saved_takes_packed_files(tmp_path):
    from skyrim_amd.leads import open_saved
    files, want = [], []
    for k in range(2):
        da, st, tab, img = packed(3, seed=k, t=T0 + k * datetime.timedelta(hours=6))
        files.append(str(tmp_path / A.member_file("pangu", 3, 1, "gfs", T0, T0 + k * datetime.timedelta(hours=6))))
        da.to_netcdf(files[-1])
        want.append(R.unpack(img, tab, (3, 5, 7)))
    assert Path(files[1]).name == "pangu-ens3-m001__gfs__20240513_18:00__20240514_00:00.nc"
    saved = open_saved(files, "test")
    assert saved.names == ["c0", "c1", "c2"] and saved.model_name == "pangu-ens3-m001" and len(saved.entries) == 2
    for k, (t, da, at) in enumerate(saved.entries):
        assert t == T0 + k * datetime.timedelta(hours=6) and np.array_equal(bits(da.values[at]), bits(want[k]))


# ---- the archive: manifest, request, replay ---------------------------------------------------------------------------------------------------- #
NAMES = ["t2m", "u10m", "v10m", "msl"]


def written(tmp_path, leads=(0, 1, 2), channels=("t2m", "msl"), M=2):
    """An int16 archive of M members made on the host with the reference: what ``LeadArchive`` writes, without a device."""
    files, bad = [], []
    for i, k in enumerate(leads):
        t = T0 + k * datetime.timedelta(hours=6)
        files.append([A.member_file("toy", M, m, "gfs", T0, t) for m in range(M)])
        bad.append([])
        for m in range(M):
            st = field(1, 5, 7, 10 * i + m, len(channels))[0]
            tab = R.table([st], range(len(channels)))
            A.packed_dataarray(np.frombuffer(R.quantize([st], range(len(channels)), tab)[0], np.uint8), tab[0], t, channels, LAT,
                               LON).to_netcdf(tmp_path / files[-1][m])
            bad[-1].append([int(v) for v in tab[0]["n_bad"]])
    manifest = dict(model="toy", n_members=M, seed=5, perturbation="white", perturb_scale=0.05, packing="int16", channels=list(channels),
                    lat=LAT.tolist(), lon=LON.tolist(), time_step_s=21600.0, start_time=T0.isoformat(), source="gfs", leads=list(leads),
                    valid_times=[(T0 + k * datetime.timedelta(hours=6)).isoformat() for k in leads], files=files, n_bad=bad)
    (tmp_path / A.MANIFEST).write_text(json.dumps(manifest))
    return manifest


def test_manifest_round_trip(tmp_path):
    from skyrim_amd.core import Skyrim
    m = written(tmp_path)
    arch = Skyrim.open_archive(tmp_path)
    assert isinstance(arch, A.MemberArchive) and arch.manifest == m and arch.complete
    assert (arch.model_name, arch.M, arch.packing, arch.channels, arch.leads) == ("toy", 2, "int16", ["t2m", "msl"], [0, 1, 2])
    assert arch.start_time == T0 and arch.valid_times[2] == T0 + datetime.timedelta(hours=12) and arch.time_step == datetime.timedelta(hours=6)
    assert len(arch.paths) == 6 and all(Path(p).exists() for p in arch.paths)
    info = arch.info()
    assert info["grid"] == (5, 7) and info["n_files"] == 6 and info["payload_bytes"] == 2 * 2 * 35 * 2 * 3 and info["n_bad"] == 0
    assert info["seed"] == 5 and info["time_step_h"] == 6.0 and info["complete"]
    da = arch.member(1, 2)
    assert da.shape == (1, 2, 5, 7) and da.channel.values.tolist() == ["t2m", "msl"]
    assert np.abs(da.values[0] - field(1, 5, 7, 21, 2)[0]).max() < 54000 * 8 / 65534
    with pytest.raises(IndexError):
        arch.member(2, 0)
    with pytest.raises(ValueError, match="no manifest.json"):
        A.open(tmp_path / "nowhere")
    (tmp_path / "bad").mkdir()
    (tmp_path / "bad" / A.MANIFEST).write_text(json.dumps({k: v for k, v in m.items() if k != "files"}))
    with pytest.raises(ValueError, match="lacks"):
        A.open(tmp_path / "bad")
    from click.testing import CliRunner
    from skyrim_amd import archive_cli
    res = CliRunner().invoke(archive_cli.archive, ["info", str(tmp_path)])
    assert res.exit_code == 0 and json.loads(res.output)["channels"] == ["t2m", "msl"]
    assert {"--product", "--exceed", "--quantile", "--derived", "--output_dir"} <= {o for p in archive_cli.replay.params for o in p.opts}


def test_archive_request_refusals_and_signatures():
    from skyrim_amd import ensemble as E
    from skyrim_amd.core.models.base import GlobalModel
    assert A.check_request(NAMES, {}, True) == dict(packing="int16", channels=NAMES, indices=[0, 1, 2, 3], dir=None)
    assert A.check_request(NAMES, dict(packing="float32", channels=["msl", "t2m"], dir="/x"), False)["indices"] == [3, 0]
    for req, save, match in ((["int16"], True, "is a dict"), (dict(pack="int16"), True, "unknown keys"), (dict(packing="int8"), True, "packing = 'int8'"),
                             (dict(channels=["z500"]), True, r"channels \['z500'\]"), (dict(channels=[]), True, "at least one"),
                             (dict(channels=["t2m", "t2m"]), True, "distinct"), (dict(), False, "needs save=True"),
                             (dict(dir=None), False, "needs save=True")):
        with pytest.raises(ValueError, match=match):
            A.check_request(NAMES, req, save)
    model = SimpleNamespace(out_channel_names=NAMES, in_channel_names=NAMES, grid=SimpleNamespace(lat=LAT, lon=LON),
                            time_step=datetime.timedelta(hours=6))
    args = (model, 2, 3, 0, ("mean",), None, None, None, 1, False)
    assert E.plan_request(*args).archive is None and E.validate(*args) == E.validate(*args, archive=dict(dir="/x"))
    assert E.plan_request(*args, archive=dict(channels=["msl"]), save=True).archive["indices"] == [3]
    with pytest.raises(ValueError, match="needs save=True"):
        E.validate(*args, archive={})
    with pytest.raises(ValueError, match="packing"):
        E.validate(*args, archive=dict(packing="zip"), save=True)
    for fn in (E.run, GlobalModel.ensemble_forecast, E.validate, E.plan_request):
        assert inspect.signature(fn).parameters["archive"].default is None
    assert E.EnsembleForecast("pangu", 3, 0, 1e-3).archive is None and E.Stage().close is None
    big = SimpleNamespace(out_channel_names=NAMES, in_channel_names=NAMES, grid=SimpleNamespace(lat=np.linspace(90, -90, 721), lon=np.arange(1440) * 0.25))
    with pytest.raises(ValueError, match=r"keep_members=True would hold .* archive="):
        E.validate(big, 40, 50, 0, ("mean",), None, None, None, 1, True)


def test_replay_refusals_come_before_any_file_is_read(tmp_path, monkeypatch):
    written(tmp_path)
    arch = A.open(tmp_path)
    monkeypatch.setattr(A.MemberArchive, "states", lambda *a, **k: pytest.fail("a file was opened for data"))
    for request, match in ((dict(perturbation="spherical"), "not arguments of a replay"), (dict(breeding={}), "not arguments of a replay"),
                           (dict(stochastic={}), "not arguments of a replay"), (dict(n_members=3), "not arguments of a replay"),
                           (dict(scores=True), "needs truth="), (dict(scenarios=dict(channels=["t2m"], normalise="std")), "channel_std"),
                           (dict(exceed={"u10m": [5.0]}), r"'u10m' is not an output channel.*holds the channels \['t2m', 'msl'\]"),
                           (dict(channels=["v10m"]), "not output channels"), (dict(derived=["ws10m"]), "u10m"),
                           (dict(products=("median",)), "unknown products")):
        with pytest.raises(ValueError, match=match):
            arch.replay(**request)
    (tmp_path / "gap").mkdir()
    written(tmp_path / "gap", leads=(0, 2, 4))
    gap = A.open(tmp_path / "gap")
    assert not gap.complete
    for request in (dict(tracks=True), dict(aggregates=["t2m:max:12h"])):
        with pytest.raises(ValueError, match=r"needs every lead from 0; the archive holds the leads \[0, 2, 4\]"):
            gap.replay(**request)
    import torch
    if not torch.cuda.is_available():                      # a valid request gets as far as the device, and is refused for the lack of one
        with pytest.raises(RuntimeError, match="needs a GPU"):
            arch.replay(products=("mean",))
