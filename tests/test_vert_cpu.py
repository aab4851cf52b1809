"""Vertical interpolation without a GPU: the binding policy of libskyrim_vert.so, every refusal of skvert_run, the names
``<field>@<surface>`` and their refusals in ``derived.plan``, op merging and slot numbering beside the derive and thermo ops, the host
constants, and the fp32 restatement against exact arithmetic within the bounds of include/skyrim_vert.h."""
from __future__ import annotations

import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

import _vert_reference as R
from skyrim_amd import derived as D
from skyrim_amd import native, ops
from skyrim_amd import thermo as TH
from skyrim_amd import vertical as V

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "skyrim_vert.h"
LAT, LON = np.linspace(90.0, -90.0, 33), np.arange(64) * (360.0 / 64)
U = 2.0 ** -24
# include/skyrim_vert.h "Bounds": the largest relative difference of p@ from float64 over 100 000 columns per coordinate kind, and what is
# asserted (four times that)
MEASURED_P = 1.67e-5
ASSERTED_P = 4 * MEASURED_P


def _header() -> str:
    return re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)


def _pangu():
    from skyrim_amd.pangu.spec import CHANNELS
    return list(CHANNELS)


# ---- 1. the binding ------------------------------------------------------------------------------------------------------------------- #
def test_header_symbols_constants_and_housekeeping():
    assert V.SPEC.stem == "skyrim_vert" and V.SPEC.env == "SKYRIM_VERT_LIB" and V.SPEC.prefix == "skvert"
    declared = set(re.findall(r"\b(skvert_[a-z0-9_]+)\s*\(", _header()))
    assert declared == set(V.EXPORTS) == {"skvert_abi_version", "skvert_run"}
    lib = V.load_library()
    assert all(hasattr(lib, s) for s in declared)
    define = int(re.search(r"#define SKVERT_ABI_VERSION (\d+)", _header()).group(1))
    assert lib.skvert_abi_version() == define == V.ABI_VERSION == 1
    assert "vert_fields" in ops.OP_NAMES
    text = _header()
    for name, val in (("MAX_MEMBERS", V.MAX_MEMBERS), ("MAX_OPS", V.MAX_OPS), ("MAX_LEVELS", V.MAX_LEVELS), ("MAX_TARGETS", V.MAX_TARGETS),
                      ("MAX_FIELDS", V.MAX_FIELDS), ("P", V.P), ("Z", V.Z), ("Z_AGL", V.Z_AGL), ("THETA", V.THETA), ("T", V.T), ("PLAIN", V.PLAIN),
                      ("SPEED", V.SPEED), ("THETA_F", V.THETA_F), ("PRESSURE", V.PRESSURE), ("NAN", V.NAN), ("NEAREST", V.NEAREST),
                      ("NODE_NONE", V.NODE_NONE), ("NODE_ZS", V.NODE_ZS), ("E_ARG", -1), ("E_HIP", -2)):
        assert int(re.search(rf"SKVERT_{name} \(?(-?\d+)\)?", text).group(1)) == val, name
    assert (R.P, R.Z, R.Z_AGL, R.THETA, R.T, R.PLAIN, R.SPEED, R.THETA_F, R.PRESSURE) == (V.P, V.Z, V.Z_AGL, V.THETA, V.T, V.PLAIN, V.SPEED, V.THETA_F, V.PRESSURE)
    make = (ROOT / "skyrim_amd/csrc/Makefile").read_text()
    assert "vert" in native.__doc__.split("}")[0] and "vert" in make.splitlines()[0] and "LIB_VERT" in make
    assert "-ffp-contract=off -shared -o $@ vert_ops.hip" in make
    assert "skvert_abi_version() == 1" in (ROOT / "__graft_entry__.py").read_text()


def test_descriptor_layout_matches_the_header(tmp_path):
    import shutil
    import subprocess
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not installed")
    structs = (("skvert_desc", V.VertDesc), ("skvert_op", V.OpDesc), ("skvert_field", V.FieldDesc))
    body = "".join(f'  printf(" %zu", sizeof({c}));\n' + "".join(f'  printf(" %zu", offsetof({c}, {f}));\n' for f, _ in s._fields_) for c, s in structs)
    src = tmp_path / "layout.cpp"
    src.write_text('#include <cstdio>\n#include <cstddef>\n#include "skyrim_vert.h"\nint main() {\n' + body + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    r = subprocess.run(["hipcc", "-x", "c++", "-std=c++17", f"-I{ROOT / 'include'}", str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    want = []
    for _, s in structs:
        want += [ctypes.sizeof(s)] + [getattr(s, f).offset for f, _ in s._fields_]
    assert got == want


# ---- 2. every refusal of skvert_run, without a device ---------------------------------------------------------------------------------- #
LV = tuple(float(p) for p in R.LEVELS[13])
LAY = R.layout(13)


def speed(out=(0,), node=(V.NODE_NONE, V.NODE_NONE), gh=0.0, a=LAY["u"], b=LAY["v"]):
    return V.Field(V.SPEED, a, b, out, node, gh)


def zop(fields=None, targets=(14709.975,), coord=V.Z, c=LAY["z"], z=(), p=LV, **kw):
    return V.Op(coord, p, c, z, targets, (speed(),) if fields is None else tuple(fields), **kw)


def code(ops_=None, zs=0, **kw):
    """the return code of skvert_run on a descriptor whose pointers are never dereferenced: the argument checks come first"""
    geo = dict(M=4, C=LAY["C"], H=5, W=8, D=6, member_stride=6 * 5 * 8)
    geo.update({k: kw.pop(k) for k in list(kw) if k in geo})
    d = V.describe([zop()] if ops_ is None else ops_, geo["M"], geo["C"], geo["H"], geo["W"], geo["D"], geo["member_stride"], kw.pop("member_align", 16))
    d.members, d.out, d.zs = 4096, 4096, zs
    for k, v in kw.items():
        setattr(d, k, v)
    return V.load_library().skvert_run(ctypes.byref(d), None)


def test_every_argument_error_is_found_before_the_device():
    lib = V.load_library()
    E = -1                                                                                           # SKVERT_E_ARG
    assert lib.skvert_run(None, None) == E
    assert code(members=None) == E and code(out=None) == E and code(out=4098) == E and code(zs=4098) == E
    assert code(M=0) == E and code(M=65) == E and code(member_align=8) == E
    assert code(C=0) == E and code(H=0) == E and code(D=0) == E and code(member_stride=6 * 5 * 8 - 1) == E
    assert code(H=1 << 15, W=1 << 15, member_stride=6 << 30) == E                                    # C H W beyond 32-bit byte offsets
    assert code([]) == E and code([zop([speed((k % 6,))]) for k in range(17)]) == E                   # no op; too many ops
    assert code([zop(), zop([speed((0,))])]) == E                                                     # a slot written twice, by two ops
    assert code([zop([speed((1, 1))], targets=(1.0, 2.0))]) == E                                      # ... by two targets of a field
    assert code([zop([speed((2,)), V.Field(V.PLAIN, LAY["t"], (), (2,))])]) == E                      # ... by two fields
    assert code([zop([speed((-1,))])]) == E                                                           # no slot at all
    assert code([zop([speed((6,))])]) == E and code([zop([speed((-2,))])]) == E                       # slot outside [0, D)
    assert code([zop(p=LV[:1], c=LAY["z"][:1], fields=[speed(a=LAY["u"][:1], b=LAY["v"][:1])])]) == E      # L = 1
    d = V.describe([zop()], 4, LAY["C"], 5, 8, 6, 240)
    d.members, d.out = 4096, 4096
    d.ops[0].n_levels = 17                                                                            # L = 17 cannot be described: set it
    assert lib.skvert_run(ctypes.byref(d), None) == E
    assert code([zop(p=LV[:5] + (600.0,) + LV[6:])]) == E                                             # pressures not decreasing (600, 600)
    assert code([zop(p=LV[:5] + (650.0,) + LV[6:])]) == E and code([zop(p=LV[:12] + (0.0,))]) == E
    assert code([zop(coord=V.Z_AGL)]) == E                                                            # AGL without zs
    assert code([zop(coord=V.P, c=(), mask=1)]) == E                                                  # a P op that masks needs zs
    d = V.describe([zop()], 4, LAY["C"], 5, 8, 6, 240)
    d.members, d.out = 4096, 4096
    d.ops[0].n_targets = 5                                                                            # too many targets
    assert lib.skvert_run(ctypes.byref(d), None) == E
    d.ops[0].n_targets, d.ops[0].n_fields = 1, 9                                                      # too many fields
    assert lib.skvert_run(ctypes.byref(d), None) == E
    assert code([zop(targets=(float("nan"),))]) == E and code([zop(targets=(float("inf"),))]) == E
    assert code([zop(coord=0)]) == E and code([zop(coord=6)]) == E and code([zop(outside=2)]) == E
    assert code([zop(c=LAY["z"][:12] + (LAY["C"],))]) == E and code([zop([speed(b=LAY["v"][:12] + (-1,))])]) == E      # channel outside [0, C)
    assert code([zop([V.Field(5, LAY["t"], (), (0,))])]) == E                                         # field kind
    assert code([zop([speed(node=(LAY["u10m"], LAY["v10m"]), gh=98.0)])]) == E                        # a node on another coordinate than Z_AGL
    with pytest.raises(ValueError, match="0 members"):
        V.run([], None, [zop()], None)
    assert V._shape_error(zop(coord=V.Z_AGL), False) == "a Z_AGL op needs the surface geopotential" and V._shape_error(zop(coord=V.Z_AGL), True) is None
    assert V._shape_error(zop(coord=V.T, c=LAY["t"]), True) is not None and V._shape_error(zop(coord=V.T, c=LAY["t"], z=LAY["z"]), True) is None
    assert V._shape_error(zop(targets=(1.0,) * 5), False) is not None and V._shape_error(zop([speed((0,))] * 9), False) is not None


def test_encode_decode_round_trip():
    import torch
    prog = [zop([speed((0, -1), (LAY["u10m"], LAY["v10m"]), 98.0625), V.Field(V.PLAIN, LAY["z"], (), (-1, 3), (V.NODE_ZS, V.NODE_NONE))],
                 targets=(980.665, 49.0), coord=V.Z_AGL, outside=V.NEAREST),
            V.Op(V.P, LV, (), (), (6.5,), (V.Field(V.PRESSURE, (), (), (-1,)), V.Field(V.THETA_F, LAY["t"], (), (4,)))),
            V.Op(V.THETA, LV[:2], LAY["t"][:2], LAY["z"][:2], (320.0, 300.0, 280.0, 340.0), (V.Field(V.PRESSURE, (), (), (5, -1, 1, 2)),))]
    i, f = V.encode(prog)
    assert V.decode(i, f) == prog
    with pytest.raises(ValueError, match="ends inside an op"):
        V.decode(i[:-3], f)
    with pytest.raises(ValueError, match="ends inside an op"):
        V.decode(i, f[:-1])
    with pytest.raises(ValueError, match="unknown coordinate kind 7"):
        V.decode([7] + i[1:], f)
    with pytest.raises(NotImplementedError):                     # CPU tensors: no fallback, the dispatcher has no CPU kernel
        x = torch.zeros(LAY["C"], 5, 8)
        torch.ops.skyrim_hip.vert_fields([x], torch.zeros(1, dtype=torch.int64), i, f, torch.zeros(1, 6, 5, 8), None)


# ---- 3. the names ---------------------------------------------------------------------------------------------------------------------- #
def test_names_parse():
    assert D._parse_vert("ws@100magl") == ("ws", "Z_AGL", 100.0) and D._parse_vert("t@1500m") == ("t", "Z", 1500.0)
    assert D._parse_vert("z@-10C") == ("z", "T", -10.0) and D._parse_vert("u@320K") == ("u", "THETA", 320.0)
    assert D._parse_vert("ws@875hPa") == ("ws", "P", 875.0) and D._parse_vert("theta@87.5hPa") == ("theta", "P", 87.5)
    assert D._parse_vert("p@2.5m") == ("p", "Z", 2.5) and D._parse_vert("q@0C") == ("q", "T", 0.0)
    for bad in ("ws@100", "ws@magl", "w@100m", "ws@1e3m", "ws@100 m", "ws@.5m", "ws@100m ", "ws10m", "ws@100ft"):
        assert D._parse_vert(bad) is None, bad
    from skyrim_amd import aggregate, events
    r = aggregate.parse_request("ws@100magl:max:24h")
    assert (r.channel, r.stat, r.window, r.name) == ("ws@100magl", "max", "24h", "ws@100magl_max_24h")
    assert aggregate.parse_request("ws@100magl:hours_above@12:all").stat == "hours_above@12"
    assert events.parse_event("ws@100magl:12") == ("ws@100magl", [12.0])                              # --event 'ws@100magl:12'
    known = _pangu() + ["ws@100magl"]
    assert events.check_request(known, {"ws@100magl": [12.0]}, (), 3)[0] == {"ws@100magl": [12.0]}


def test_every_refusal_is_a_value_error_by_name():
    names = _pangu()
    plan = lambda f, **kw: D.plan(names, f, LAT, LON, **kw)     # noqa: E731
    with pytest.raises(ValueError, match="'ws@100magl' is a height above the ground: it needs the surface geopotential, derived_surface="):
        plan(["ws@100magl"])
    with pytest.raises(ValueError, match=r"'ws@1100hPa': 1100 hPa lies outside the column 1000 \.\. 50 hPa"):
        plan(["ws@1100hPa"])
    with pytest.raises(ValueError, match="'t@30hPa': 30 hPa lies outside"):
        plan(["t@30hPa"])
    with pytest.raises(ValueError, match="'p@500hPa' is the pressure on a pressure surface: the constant 500 hPa"):
        plan(["p@500hPa"])
    with pytest.raises(ValueError, match="'theta@320K' is theta on an isentrope: a constant"):
        plan(["theta@320K"])
    with pytest.raises(ValueError, match="'t@-10C' is t on an isotherm: a constant"):
        plan(["t@-10C"])
    with pytest.raises(ValueError, match="'t@0m': a height must be positive"):
        plan(["t@0m"])
    with pytest.raises(ValueError, match="'ws@0magl': a height must be positive"):
        plan(["ws@0magl"], surface=True)
    with pytest.raises(ValueError, match="'u@0K': a potential temperature must be positive"):
        plan(["u@0K"])
    with pytest.raises(ValueError, match="'ws@-5m': a height must be positive"):                      # only <T>C may be negative
        plan(["ws@-5m"])
    with pytest.raises(ValueError, match=r"'r@1500m' needs the level variable 'r' \(r<level>\), which this model lacks"):
        plan(["r@1500m"])
    with pytest.raises(ValueError, match="'ws@1500m' runs over 2 to 16 levels with the channels z<level>, u<level>, v<level>; this model has 1"):
        D.plan([n for n in names if not (n[0] == "z" and n != "z500")], ["ws@1500m"], LAT, LON)
    with pytest.raises(ValueError, match=r"^derived: unknown field 'gust@'; known are ws10m, .*iwv, <field>@<surface> \(field: z, q, r, t, u, v, ws, theta or p; "
                                         r"surface: <P>hPa, <Z>m above sea level, <Z>magl above the ground, <theta>K or <T>C\), td<level>.*mucape_src$"):
        plan(["gust@"])
    many = [f"t@{1000 + 100 * k}m" for k in range(4 * 16 + 1)]                                          # four targets an op: a seventeenth op
    with pytest.raises(ValueError, match="17 vertical-interpolation ops .* one call holds 16"):
        plan(many)
    assert len(plan(many[:-1]).vert_ops) == 16
    with pytest.raises(ValueError, match='vertical: outside is "nan" or "nearest", not \'clamp\''):
        plan(["t@1500m"], vertical={"outside": "clamp"})
    with pytest.raises(ValueError, match="vertical: unknown keys"):
        plan(["t@1500m"], vertical={"below": "nan"})
    with pytest.raises(ValueError, match="vertical: outside"):                                        # refused with or without an @ name
        D.check_request(names, ["ws10m"], LAT, LON, vertical={"outside": 3})


def test_ops_merge_and_share_the_slot_numbering():
    names = _pangu()
    ch = names.index
    levels = [1000, 925, 850, 700, 600, 500, 400, 300, 250, 200, 150, 100, 50]
    col = lambda x: tuple(ch(f"{x}{l}") for l in levels)       # noqa: E731
    fields = ["ws@100magl", "mucape", "t@1500m", "ws10m", "u@320K", "t@100magl", "p@320K", "ws@150magl", "z@-10C", "z@100magl", "theta@500hPa", "ws@1500m"]
    p = D.plan(names, fields, LAT, LON, surface=True, vertical={"outside": "nearest"})
    assert [op.kind for op in p.ops] == [D.SPEED] and p.ops[0].outputs == (3,) and p.thermo_ops[0].outputs == (1, -1, -1)
    g10, g2 = float(np.float32(9.80665 * 10)), float(np.float32(9.80665 * 2))
    agl, z, th, t, pr = p.vert_ops
    assert (agl.coord, agl.c, agl.z, agl.outside) == (V.Z_AGL, col("z"), (), V.NEAREST)
    assert agl.targets == (float(np.float32(980.665)), float(np.float32(9.80665 * 150)))
    assert agl.fields == (V.Field(V.SPEED, col("u"), col("v"), (0, 7), (ch("u10m"), ch("v10m")), g10),
                          V.Field(V.PLAIN, col("t"), (), (5, -1), (ch("t2m"), V.NODE_NONE), g2),
                          V.Field(V.PLAIN, col("z"), (), (9, -1), (V.NODE_ZS, V.NODE_NONE), 0.0))
    assert (z.coord, z.targets) == (V.Z, (float(np.float32(9.80665 * 1500)),))
    assert z.fields == (V.Field(V.PLAIN, col("t"), (), (2,)), V.Field(V.SPEED, col("u"), col("v"), (11,)))
    assert (th.coord, th.c, th.z, th.targets) == (V.THETA, col("t"), col("z"), (320.0,))
    assert th.fields == (V.Field(V.PLAIN, col("u"), (), (4,)), V.Field(V.PRESSURE, (), (), (6,)))
    assert (t.coord, t.targets, t.fields) == (V.T, (float(np.float32(263.15)),), (V.Field(V.PLAIN, col("z"), (), (8,)),))
    assert (pr.coord, pr.c, pr.z, pr.mask) == (V.P, (), (), 0) and pr.fields == (V.Field(V.THETA_F, col("t"), (), (10,)),)
    assert pr.targets == (float(TH.sk_log(np.float32(500))),) and all(op.pressures == tuple(float(l) for l in levels) for op in p.vert_ops)
    assert p.column == {"parcel": levels, "vert": levels}
    assert p.inputs["ws@100magl"] == [f"z{l}" for l in levels] + [f"u{l}" for l in levels] + [f"v{l}" for l in levels] + ["u10m", "v10m"]
    assert p.inputs["u@320K"][:13] == [f"t{l}" for l in levels] and p.inputs["u@320K"][13] == "z1000" and p.inputs["p@320K"][-1] == "z50"
    # without a surface the isentrope does not name z; a fifth target and a ninth field go to further ops
    free = D.plan(names, ["u@320K"], LAT, LON)
    assert free.vert_ops[0].z == () and free.vert_ops[0].outside == V.NAN and free.inputs["u@320K"] == [f"{x}{l}" for x in "tu" for l in levels]
    five = D.plan(names, [f"t@{h}m" for h in (500, 1000, 1500, 2000, 2500)] + ["u@500m"], LAT, LON)
    assert [len(op.targets) for op in five.vert_ops] == [4, 1] and five.vert_ops[0].fields[1].outputs == (5, -1, -1, -1)
    nine = D.plan(names, [f"{x}@1500m" for x in ("z", "q", "t", "u", "v", "ws", "theta", "p")] + ["u@850hPa", "ws@850hPa"], LAT, LON)
    assert [len(op.fields) for op in nine.vert_ops] == [8, 2] and nine.vert_ops[0].fields[7] == V.Field(V.PRESSURE, (), (), (7,))
    # the truth: the forecast's column, and what it lacks by name
    from types import SimpleNamespace
    truth = D.TruthDeriver(["t@1500m", "ws@1500m"], LAT, LON, column=dict(vert=[1000, 850, 500]))
    have = ["z1000", "z850", "z500", "t1000", "t850", "t500", "u1000", "u850", "v1000", "v850", "v500"]
    assert truth.names(SimpleNamespace(names=have)) == ["t@1500m"] and truth.dropped == {"ws@1500m": ["u500"]}
    assert D.plan(have, ["t@1500m"], LAT, LON, column=dict(vert=[1000, 500])).vert_ops[0].pressures == (1000.0, 500.0)


def test_a_request_without_at_names_never_loads_the_library(monkeypatch):
    def boom():
        raise AssertionError("vertical.load_library called")
    monkeypatch.setattr(V, "load_library", boom)
    p = D.LeadDeriver(_pangu(), LAT, LON, 2, ["ws10m", "mucape"]).plan
    assert p.vert_ops == [] and "vert" not in p.column
    assert len(D.LeadDeriver(_pangu(), LAT, LON, 2, ["ws@1500m"]).plan.vert_ops) == 1                   # (planning needs no library either)


def test_host_constants_are_thermos():
    import _thermo_reference as TR
    p = np.asarray(R.LEVELS[16] + (875, 87.5, 1, 1013.25), np.float32)
    assert np.array_equal(TH.sk_log(p).view(np.uint32), TR.fp32.log(p).view(np.uint32))
    x = np.linspace(-90, 90, 4001).astype(np.float32)
    assert np.array_equal(TH.sk_exp(x).view(np.uint32), TR.fp32.exp(x).view(np.uint32))
    lnp, ex = V.level_constants(R.LEVELS[13])
    rl, rx = R.fp32.constants(R.LEVELS[13])
    assert lnp.dtype == ex.dtype == np.float32 and np.array_equal(lnp.view(np.uint32), rl.view(np.uint32)) and np.array_equal(ex.view(np.uint32), rx.view(np.uint32))
    # ex_k is the factor of SKTHERMO_MOIST's theta = t * sk_exp(kappa * (LN1000 - sk_log(p)))
    t = np.float32(281.37)
    assert all(TR.fp32.moist(t, t, lv, TR.Q, theta_only=True)[3] == t * ex[k] for k, lv in enumerate(R.LEVELS[13]))
    assert V.target_value(V.T, -10) == float(np.float32(263.15)) and V.target_value(V.Z, 1500) == float(np.float32(9.80665 * 1500))
    assert V.target_value(V.P, 700) == float(lnp[3]) and V.target_value(V.THETA, 320) == 320.0 and V.target_value(V.Z_AGL, 100) == float(np.float32(980.665))


# ---- 4. fp32 against exact arithmetic ---------------------------------------------------------------------------------------------------- #
N = 100000
KINDS = {"P": (V.P, (700.0, 875.0, 333.0, 61.0)), "Z": (V.Z, (1500.0, 5000.0, 300.0, 11000.0)), "Z_AGL": (V.Z_AGL, (100.0, 5.0, 1500.0, 40.0)),
         "THETA": (V.THETA, (320.0, 300.0, 350.0, 285.0)), "T": (V.T, (-10.0, 0.0, -40.0, 15.0))}


@pytest.fixture(scope="module")
def sample():
    L = 13
    t, u, v, q, z, zs = R.columns(11, N, R.LEVELS[L])
    state = np.concatenate([t, u, v, q, z, 0.7 * u[:1], 0.7 * v[:1], t[:1] + 1.0]).astype(np.float32)
    return state, zs.astype(np.float32)


def program(kind, L=13):
    """One op of the coordinate ``kind`` with its four targets: t (PLAIN), ws (SPEED), theta (THETA_F), p (PRESSURE) -- slots 4 f + t"""
    lay = R.layout(L)
    coord, values = KINDS[kind]
    agl = coord == V.Z_AGL
    g10, g2 = float(np.float32(9.80665 * 10)), float(np.float32(9.80665 * 2))
    fields = (V.Field(V.PLAIN, lay["t"], (), (0, 1, 2, 3), (lay["t2m"], V.NODE_NONE) if agl else (V.NODE_NONE,) * 2, g2 if agl else 0.0),
              V.Field(V.SPEED, lay["u"], lay["v"], (4, 5, 6, 7), (lay["u10m"], lay["v10m"]) if agl else (V.NODE_NONE,) * 2, g10 if agl else 0.0),
              V.Field(V.THETA_F, lay["t"], (), (8, 9, 10, 11)), V.Field(V.PRESSURE, (), (), (12, 13, 14, 15)))
    c = {V.P: (), V.Z: lay["z"], V.Z_AGL: lay["z"], V.THETA: lay["t"], V.T: lay["t"]}[coord]
    z = lay["z"] if coord in (V.THETA, V.T) else ()
    return V.Op(coord, tuple(float(p) for p in R.LEVELS[L]), c, z, tuple(V.target_value(coord, x) for x in values), fields)


@pytest.mark.parametrize("kind", list(KINDS))
def test_fp32_restatement_within_the_headers_bounds(sample, kind):
    """Against exact arithmetic on the same fp32 inputs (float64 with the fp32 host constants), wherever both choose the same layer:
    PLAIN within 7 u (|f_k| + |f_u|), THETA_F within 8 u, each plus |f_u - f_k| 2 rho for the kinds that round c or tau; and those columns
    are all but 0.1 % of the sample at the most."""
    state, zs = sample
    op = program(kind)
    consts = R.fp32.constants(op.pressures)
    ia, ib = {}, {}
    a = R.fp32.apply(op, state, zs, info=ia)
    b = R.f64.apply(op, state.astype(np.float64), zs.astype(np.float64), consts=consts, info=ib)
    lnp, ex = (np.asarray(x, np.float64) for x in consts)
    s64 = state.astype(np.float64)
    differ, worst = 0, {}
    np.seterr(divide="ignore", invalid="ignore")                # (rho of columns without a layer: not selected below)
    for f, fd in enumerate(op.fields[:3]):
        for t in range(4):
            (ma, la, ua), (mb, lb, ub) = ia[(f, t)], ib[(f, t)]
            same = (ma == mb) & (la == lb) & (ua == ub)
            differ = max(differ, int((~same).sum()))
            layer = same & (ma == R.LAYER)                       # (the node's layer obeys the same bound; it is measured with the levels' alone)
            assert layer.sum() > N // 20 or kind == "Z_AGL", (kind, f, t, int(layer.sum()))
            got, ref = a[fd.outputs[t]].astype(np.float64), b[fd.outputs[t]]
            assert np.array_equal(np.isnan(got[same]), np.isnan(ref[same]))
            pick = lambda ch, k: np.take_along_axis(s64[list(ch)], k[None], 0)[0]      # noqa: E731
            if op.coord == V.P:
                ck, cu_, tau = lnp[la], lnp[ua], np.full(N, op.targets[t])
            else:
                scale = ex if op.coord == V.THETA else np.ones(13)
                ck, cu_ = pick(op.c, la) * scale[la], pick(op.c, ua) * scale[ua]
                tau = zs.astype(np.float64) + op.targets[t] if op.coord == V.Z_AGL else np.full(N, op.targets[t])
            rho = U * np.maximum(np.maximum(np.abs(ck), np.abs(cu_)), np.abs(tau)) / np.abs(cu_ - ck) if op.coord in (V.THETA, V.Z_AGL) else np.zeros(N)
            comps = (fd.a, fd.b) if fd.kind == V.SPEED else (fd.a,)
            scale = ex if fd.kind == V.THETA_F else np.ones(13)
            fk, fu = [pick(c, la) * scale[la] for c in comps], [pick(c, ua) * scale[ua] for c in comps]
            n_u = 8 if fd.kind == V.THETA_F else 7
            bounds = [(n_u * U * (np.abs(k) + np.abs(w)) + np.abs(w - k) * 2 * rho) * (1 + 1e-6) + 2.0 ** -100 for k, w in zip(fk, fu)]
            if fd.kind == V.SPEED:
                # s = sqrt(u^2 + v^2) of components within du, dv of the exact ones: |ds| <= hypot(du, dv), and the SPEED of
                # skyrim_derive.h adds its own roundings, 2 u s at the most (two squares, a sum, a root: 1/2 + 1/2 + 1/2 + 1 halves)
                bound = np.hypot(*bounds) + 2 * U * np.abs(ref) * (1 + 1e-6)
            else:
                bound = bounds[0]
            sel = layer & (rho <= 0.25)
            err = np.abs(got - ref)[sel] / bound[sel]
            worst[(f, t)] = float(err.max()) if err.size else 0.0
    np.seterr(divide="warn", invalid="warn")
    print(f"{kind}: columns where fp32 and float64 choose another layer: {differ} of {N}; worst share of the bound {max(worst.values()):.3f}")
    assert differ <= N // 1000                                   # a condition on the sample: coordinates continuous and well separated
    assert max(worst.values()) <= 1.0, worst


def test_pressure_on_a_surface_against_float64_and_the_headers_figures(sample):
    """p@ against float64 with np.exp / np.log (the yardstick makes its own constants): the measured figure of the header, the asserted
    one four times it."""
    state, zs = sample
    worst = 0.0
    for kind in ("Z", "Z_AGL", "THETA", "T"):
        op = program(kind)
        ia, ib = {}, {}
        a = R.fp32.apply(op, state, zs, info=ia)
        b = R.f64.apply(op, state.astype(np.float64), zs.astype(np.float64), info=ib)
        for t in range(4):
            same = (ia[(3, t)][0] == ib[(3, t)][0]) & (ia[(3, t)][1] == ib[(3, t)][1]) & (ia[(3, t)][2] == ib[(3, t)][2]) & (ia[(3, t)][0] == R.LAYER)
            rel = np.abs(a[12 + t].astype(np.float64)[same] / b[12 + t][same] - 1)
            worst = max(worst, float(rel.max()))
    print(f"p@: largest relative difference from float64 {worst:.2e} (header: measured {MEASURED_P:.1e}, asserted {ASSERTED_P:.1e})")
    assert worst <= ASSERTED_P
    line = next(l for l in HEADER.read_text().splitlines() if l.startswith(" *   p@ "))
    nums = [float(x) for x in re.findall(r"(?<![\w.\[-])(\d+\.\d+(?:e-?\d+)?)", line)]
    assert nums[0] == pytest.approx(MEASURED_P, rel=0.06) and nums[-1] == pytest.approx(4 * nums[0], rel=0.1)
    assert worst == pytest.approx(nums[0], rel=0.25)             # the header's measured figure is this sample's


def test_planted_corners_do_what_they_were_planted_for():
    L, (H, W) = 13, (5, 12)
    lay = R.layout(L)
    state, zs = R.planted(3, H, W, R.LEVELS[L])
    flat = lambda x: x.reshape(-1)                               # noqa: E731
    lv = tuple(float(p) for p in R.LEVELS[L])
    fz = (V.Field(V.PLAIN, lay["q"], (), (0,)),)
    info = {}
    got = flat(R.fp32.apply(V.Op(V.Z, lv, lay["z"], (), (float(R.GZ),), fz), state, None, info=info)[0])
    q = state[list(lay["q"])].reshape(L, -1)
    assert got[0].view(np.uint32) == q[L // 2, 0].view(np.uint32) and flat(info[(0, 0)][1])[0] == L // 2      # on an interior level: its value, bit for bit
    assert abs(got[1] - q[L - 1, 1]) <= 4 * U * (abs(q[L - 1, 1]) + abs(q[L - 2, 1]))                 # on the top level: to rounding only (frac = 1)
    assert np.isnan(got[2]) and flat(info[(0, 0)][1])[5] == 2 and got[5].view(np.uint32) == q[2, 5].view(np.uint32)      # the a = b layer (1, 2) is skipped
    assert np.isnan(got[12]) and np.isfinite(got[13])
    near = flat(R.fp32.apply(V.Op(V.Z, lv, lay["z"], (), (float(R.GZ),), fz, V.NEAREST), state, None)[0])
    assert near[2] == q[L - 1, 2] and np.array_equal(near[[0, 1, 5]].view(np.uint32), got[[0, 1, 5]].view(np.uint32))
    th = V.Op(V.THETA, lv, lay["t"], lay["z"], (320.0,), (V.Field(V.PRESSURE, (), (), (0,)),))
    info = {}
    R.fp32.apply(th, state, None, info=info)
    assert flat(info[(0, 0)][1])[4] == 2 and flat(info[(0, 0)][2])[4] == 3                            # three crossings of 320 K: the upper one
    agl = V.Op(V.Z_AGL, lv, lay["z"], (), tuple(V.target_value(V.Z_AGL, x) for x in R.AGL_M),
               (V.Field(V.SPEED, lay["u"], lay["v"], (0, 1, 2), (lay["u10m"], lay["v10m"]), float(np.float32(98.0665))), V.Field(V.PLAIN, lay["q"], (), (3, 4, 5))))
    info = {}
    out = R.fp32.apply(agl, state, zs, info=info)
    mode = flat(info[(0, 0)][0])
    assert mode[9] == R.NODE_LAYER and mode[10] == R.NODE_LAYER and flat(info[(0, 0)][2])[10] == 1    # 100 m: between the node and the lowest unmasked level
    assert flat(info[(0, 1)][0])[9] == R.NONE and np.isnan(flat(out[1])[9])                           # 5 m: below the node
    assert np.isnan(flat(out[3])[9]) and np.isfinite(flat(out[0])[9])                                 # a field without a node does not see it
    assert np.isnan(flat(out[0])[8]) and np.isnan(flat(out[0])[14]) and flat(info[(0, 2)][1])[6] >= 1 and flat(info[(0, 2)][1])[7] >= 3
    assert flat(out[0])[11] >= 0 and np.isfinite(flat(out[0])[11])                                    # -0.0 in u: a speed all the same
