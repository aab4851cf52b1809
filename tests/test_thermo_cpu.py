"""Column thermodynamics without a GPU: the binding policy of libskyrim_thermo.so, every refusal of skthermo_run, the catalogue
(``derived.plan``) on the channel lists of the models, the accuracy of sk_exp and sk_log, the physics of the float64 restatement (the
yardstick is itself checked), the fp32 restatement against it within the bounds of include/skyrim_thermo.h, and the compiler's resource
report of the kernel (no scratch memory)."""
from __future__ import annotations

import ctypes
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import _thermo_reference as R
from skyrim_amd import derived as D
from skyrim_amd import native, ops
from skyrim_amd import thermo as T

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "skyrim_thermo.h"
LAT, LON = np.linspace(90.0, -90.0, 33), np.arange(64) * (360.0 / 64)

# Measured (100 000 columns per configuration, 200 000 arguments: include/skyrim_thermo.h "Bounds") and asserted (four times that)
MEASURED = dict(exp=8.2e-8, log=9.8e-8, cape=0.030, li=9.6e-5, td=2.7e-5, rh=1.8e-4, q=1.5e-6, thetae=1.2e-4, theta=2.8e-5, kx=3.9e-5, tt=3.9e-5,
                zdeg0=0.059)
BOUND = {k: 4 * v for k, v in MEASURED.items()}
Q_FLOOR = 1e-5                                                  # q is compared relative to max(q, Q_FLOOR)


# ---- 1. the binding ------------------------------------------------------------------------------------------------------------------- #
def _header() -> str:
    return re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)


def test_header_symbols_equal_exports_and_are_exported():
    assert T.SPEC.stem == "skyrim_thermo" and T.SPEC.env == "SKYRIM_THERMO_LIB" and T.SPEC.prefix == "skthermo"
    declared = set(re.findall(r"\b(skthermo_[a-z0-9_]+)\s*\(", _header()))
    assert declared == set(T.EXPORTS) == {"skthermo_abi_version", "skthermo_run"}
    lib = T.load_library()
    for s in declared:
        assert hasattr(lib, s)
    assert "thermo_fields" in ops.OP_NAMES
    text = _header()
    for name, val in (("MAX_MEMBERS", T.MAX_MEMBERS), ("MAX_OPS", T.MAX_OPS), ("MAX_LEVELS", T.MAX_LEVELS), ("MOIST", T.MOIST), ("INDEX", T.INDEX),
                      ("FREEZE", T.FREEZE), ("PARCEL", T.PARCEL), ("Q", T.Q), ("R", T.R), ("SRC_LOWEST", T.SRC_LOWEST),
                      ("SRC_MAX_THETAE", T.SRC_MAX_THETAE), ("NSUB", R.NSUB), ("NITER", R.NITER), ("E_ARG", -1), ("E_HIP", -2)):
        assert int(re.search(rf"SKTHERMO_{name} \(?(-?\d+)\)?", text).group(1)) == val, name
    assert (R.Q, R.R, R.SRC_LOWEST, R.SRC_MAX_THETAE) == (T.Q, T.R, T.SRC_LOWEST, T.SRC_MAX_THETAE)
    make = (ROOT / "skyrim_amd/csrc/Makefile").read_text()
    assert "thermo" in native.__doc__.split("}")[0] and "thermo" in make.splitlines()[0]
    assert "-ffp-contract=off -shared -o $@ thermo_ops.hip" in make


def test_abi_version_is_the_headers():
    define = int(re.search(r"#define SKTHERMO_ABI_VERSION (\d+)", _header()).group(1))
    assert T.load_library().skthermo_abi_version() == define == T.ABI_VERSION


def test_missing_library_is_not_found(monkeypatch, tmp_path):
    monkeypatch.setattr(T, "_lib", None)
    monkeypatch.setenv(T.SPEC.env, str(tmp_path / "missing.so"))
    with pytest.raises(RuntimeError, match="not found"):
        T.load_library()


def test_abi_mismatch_is_refused(monkeypatch):
    monkeypatch.setattr(T, "_lib", None)
    monkeypatch.setattr(T.SPEC, "abi", T.SPEC.abi + 1)
    with pytest.raises(RuntimeError, match=rf"ABI {T.ABI_VERSION}, this package binds ABI {T.ABI_VERSION + 1}.*rebuild"):
        T.load_library()


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not installed")
def test_descriptor_layout_matches_the_header(tmp_path):
    fields, op_fields = [n for n, _ in T.ThermoDesc._fields_], [n for n, _ in T.OpDesc._fields_]
    src = tmp_path / "layout.cpp"
    src.write_text('#include <cstdio>\n#include <cstddef>\n#include "skyrim_thermo.h"\nint main() {\n  printf("%zu", sizeof(skthermo_desc));\n'
                   + "".join(f'  printf(" %zu", offsetof(skthermo_desc, {f}));\n' for f in fields)
                   + '  printf(" %zu", sizeof(skthermo_op));\n'
                   + "".join(f'  printf(" %zu", offsetof(skthermo_op, {f}));\n' for f in op_fields) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    r = subprocess.run(["hipcc", "-x", "c++", "-std=c++17", f"-I{ROOT / 'include'}", str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    n = len(fields)
    assert got[0] == ctypes.sizeof(T.ThermoDesc) and got[1:n + 1] == [getattr(T.ThermoDesc, f).offset for f in fields]
    assert got[n + 1] == ctypes.sizeof(T.OpDesc) and got[n + 2:] == [getattr(T.OpDesc, f).offset for f in op_fields]


# ---- 2. every refusal of skthermo_run, without a device -------------------------------------------------------------------------------- #
LV = tuple(float(p) for p in R.PANGU_LEVELS)
TCH, MCH, ZCH = tuple(range(13)), tuple(range(13, 26)), tuple(range(26, 39))


def parcel(out=(0, 1, 2), t=TCH, m=MCH, z=(), p=LV, **kw):
    return T.Op(T.PARCEL, t, m, z, out, T.Q, p, kw.pop("source", T.SRC_MAX_THETAE), **kw)


def code(ops_=None, zs=0, **kw):
    """the return code of skthermo_run on a descriptor whose pointers are never dereferenced: the argument checks come first"""
    geo = dict(M=4, C=39, H=5, W=8, D=6, member_stride=6 * 5 * 8)
    geo.update({k: kw.pop(k) for k in list(kw) if k in geo})
    d = T.describe([parcel()] if ops_ is None else ops_, geo["M"], geo["C"], geo["H"], geo["W"], geo["D"], geo["member_stride"], kw.pop("member_align", 16))
    d.members, d.out, d.zs = 4096, 4096, zs
    for k, v in kw.items():
        setattr(d, k, v)
    return T.load_library().skthermo_run(ctypes.byref(d), None)


def test_every_argument_error_is_found_before_the_device():
    lib = T.load_library()
    assert lib.skthermo_run(None, None) == -1
    assert code(members=None) == -1 and code(out=None) == -1 and code(out=4098) == -1 and code(zs=4098) == -1
    assert code(M=0) == -1 and code(M=65) == -1
    assert code(member_align=8) == -1 and code(member_align=0) == -1
    assert code(C=0) == -1 and code(H=0) == -1 and code(D=0) == -1 and code(member_stride=6 * 5 * 8 - 1) == -1
    assert code(H=1 << 15, W=1 << 15, member_stride=6 << 30) == -1                                 # C H W beyond 32-bit byte offsets
    assert code([]) == -1 and code([T.Op(T.MOIST, (0,), (13,), (), (k % 6, -1, -1, -1), T.Q, (850.0,)) for k in range(17)]) == -1
    assert code([parcel(t=TCH[:1], m=MCH[:1], p=LV[:1])]) == -1                                      # L = 1
    assert code([T.Op(T.FREEZE, (0,), (), (26,), (0,))]) == -1
    d = T.describe([parcel()], 4, 39, 5, 8, 6, 240)
    d.members, d.out = 4096, 4096
    d.ops[0].n_levels = 17                                                                           # L = 17 cannot be described: set it
    assert lib.skthermo_run(ctypes.byref(d), None) == -1
    assert code([parcel(p=LV[:5] + (600.0,) + LV[6:])]) == -1                                        # p not decreasing (600, 600)
    assert code([parcel(p=LV[:5] + (650.0,) + LV[6:])]) == -1                                        # p increasing
    assert code([parcel(p=LV[:12] + (float("nan"),))]) == -1 and code([parcel(p=LV[:12] + (0.0,))]) == -1
    assert code([parcel(), parcel(out=(3, 4, 2))]) == -1                                             # a slot written twice
    assert code([parcel(out=(1, 1, -1))]) == -1
    assert code([parcel(out=(-1, -1, -1))]) == -1                                                    # all slots -1
    assert code([parcel(out=(0, 6, -1))]) == -1 and code([parcel(out=(0, -2, -1))]) == -1            # slot outside [0, D)
    assert code([parcel(t=TCH[:12] + (39,))]) == -1 and code([parcel(m=MCH[:12] + (-1,))]) == -1     # channel outside [0, C)
    no500 = tuple(p for p in LV if p != 500.0)
    assert code([parcel(t=TCH[:12], m=MCH[:12], p=no500)]) == -1                                     # li without a 500-hPa level
    assert code([parcel(p_top=600.0)]) == -1                                                         # li above the top of the ascent
    assert code([parcel(p_top=2000.0)]) == -1 and code([parcel(p_top=0.0)]) == -1 and code([parcel(p_src_min=-1.0)]) == -1
    assert code([parcel(source=2)]) == -1
    assert code([T.Op(9, (0,), (13,), (), (0,), T.Q, (850.0,))]) == -1
    assert code([T.Op(T.MOIST, (0,), (13,), (), (0, 1, 2, 3), 2, (850.0,))]) == -1                   # moisture neither Q nor R
    assert code([T.Op(T.MOIST, (0,), (13,), (), (0, 1, 2, 3), T.Q, (-850.0,))]) == -1
    d = T.describe([T.Op(T.MOIST, (0,), (), (), (0, -1, -1, 1), T.Q, (850.0,))], 4, 39, 5, 8, 6, 240)
    d.members, d.out = 4096, 4096
    d.ops[0].in_m[0] = 39
    assert lib.skthermo_run(ctypes.byref(d), None) == -1                                             # td reads the moisture channel
    assert code([T.Op(T.INDEX, (0, 3, 39), (13, 16), (), (0, 1), T.R)]) == -1


def test_the_binding_refuses_what_it_can_name():
    import torch
    with pytest.raises(ValueError, match="0 members"):
        T.run([], None, [parcel()], None)
    assert T._shape_ok(parcel(), False) and not T._shape_ok(parcel(), True) and T._shape_ok(parcel(z=ZCH), True)      # a surface needs the z channels
    assert not T._shape_ok(parcel(p=LV[:12]), False) and not T._shape_ok(T.Op(T.FREEZE, TCH, (), ZCH[:12], (0,)), False)
    i, f = T.encode([parcel(), T.Op(T.MOIST, (0,), (13,), (), (0, -1, 2, -1), T.R, (850.0,)), T.Op(T.FREEZE, TCH, (), ZCH, (5,))])
    assert T.decode(i, f) == [parcel(), T.Op(T.MOIST, (0,), (13,), (), (0, -1, 2, -1), T.R, (850.0,)), T.Op(T.FREEZE, TCH, (), ZCH, (5,))]
    with pytest.raises(ValueError, match="ends inside an op"):
        T.decode(i[:-3], f)
    with pytest.raises(ValueError, match="unknown op kind 7"):
        T.decode([7] + i[1:], f)
    with pytest.raises(NotImplementedError):                     # CPU tensors: no fallback, the dispatcher has no CPU kernel
        x = torch.zeros(39, 5, 8)
        torch.ops.skyrim_hip.thermo_fields([x], torch.zeros(1, dtype=torch.int64), i, f, torch.zeros(1, 6, 5, 8), None)


# ---- 3. the catalogue ------------------------------------------------------------------------------------------------------------------ #
def _channels(which):
    from skyrim_amd.dlwp.spec import CHANNELS as dlwp
    from skyrim_amd.fcn.spec import CHANNELS as fcn
    from skyrim_amd.fuxi.spec import CHANNELS as fuxi
    from skyrim_amd.pangu.spec import CHANNELS as pangu
    from skyrim_amd.sfno.spec import CHANNELS as sfno
    return list(dict(pangu=pangu, fourcastnet_v2=sfno, fuxi=fuxi, fourcastnet=fcn, dlwp=dlwp)[which])


def test_plan_merges_ops_and_shares_the_slot_numbering():
    names = _channels("pangu")
    fields = ["mucape", "thetae850", "ws10m", "muli", "mucape_src", "sbcape", "sbli", "td850", "rh850", "theta850", "kx", "tt", "zdeg0", "ivt"]
    p = D.plan(names, fields, LAT, LON)
    assert [op.kind for op in p.ops] == [D.SPEED, D.COLUMN] and p.ops[0].outputs == (2,) and p.ops[1].outputs == (-1, -1, 13, -1)
    kinds = [(op.kind, op.outputs, op.source) for op in p.thermo_ops]
    assert kinds == [(T.PARCEL, (0, 3, 4), T.SRC_MAX_THETAE), (T.MOIST, (7, 8, 1, 9), 0), (T.PARCEL, (5, 6, -1), T.SRC_LOWEST),
                     (T.INDEX, (10, 11), 0), (T.FREEZE, (12,), 0)]
    assert p.moisture == "q" and all(op.moisture == T.Q for op in p.thermo_ops)
    levels = [1000, 925, 850, 700, 600, 500, 400, 300, 250, 200, 150, 100, 50]
    assert p.column == {"parcel": levels, "freeze": levels}
    mu = p.thermo_ops[0]
    assert mu.t == tuple(names.index(f"t{l}") for l in levels) and mu.m == tuple(names.index(f"q{l}") for l in levels) and mu.z == ()
    assert mu.pressures == tuple(float(l) for l in levels) and (mu.p_src_min, mu.p_top) == (700.0, 100.0)
    assert p.inputs["thetae850"] == ["t850", "q850"] and p.inputs["theta850"] == ["t850"] and p.inputs["kx"] == ["t850", "t700", "t500", "q850", "q700"]
    with_z = D.plan(names, ["mucape"], LAT, LON, surface=True).thermo_ops[0]
    assert with_z.z == tuple(names.index(f"z{l}") for l in levels)
    sub = D.plan(names, ["sbcape", "zdeg0"], LAT, LON, column=dict(parcel=[1000, 850, 500], freeze=[500, 1000]))
    assert sub.thermo_ops[0].pressures == (1000.0, 850.0, 500.0) and sub.thermo_ops[1].t == (names.index("t1000"), names.index("t500"))


@pytest.mark.parametrize("model", ["fourcastnet_v2", "fuxi"])
def test_plan_takes_relative_humidity_where_there_is_no_q(model):
    names = _channels(model)
    p = D.plan(names, ["mucape", "q850", "thetae850", "td850", "kx", "muli"], LAT, LON)
    assert p.moisture == "r" and all(op.moisture == T.R for op in p.thermo_ops) and not p.ops
    assert [(op.kind, op.outputs) for op in p.thermo_ops] == [(T.PARCEL, (0, 5, -1)), (T.MOIST, (3, 1, 2, -1)), (T.INDEX, (4, -1))]
    assert p.thermo_ops[0].m == tuple(names.index(f"r{l}") for l in p.column["parcel"]) and len(p.column["parcel"]) == 13
    with pytest.raises(ValueError, match="carries relative humidity itself"):
        D.plan(names, ["rh850"], LAT, LON)
    with pytest.raises(ValueError, match="need specific humidity"):                                  # ivt keeps refusing models without q
        D.plan(names, ["ivt"], LAT, LON)


def test_plan_refusals_name_what_is_missing():
    dlwp, fcn, pangu = _channels("dlwp"), _channels("fourcastnet"), _channels("pangu")
    for f in ("mucape", "sbcape", "td850", "thetae850", "kx"):
        with pytest.raises(ValueError, match="neither specific humidity .* nor relative humidity"):
            D.plan(dlwp, [f], LAT, LON)
    assert D.plan(dlwp, ["theta850"], LAT, LON).thermo_ops[0].m == ()                                # theta needs t alone
    with pytest.raises(ValueError, match="'zdeg0' runs over 2 to 16 levels .* this model has 0"):
        D.plan(dlwp, ["zdeg0"], LAT, LON)
    # FourCastNet v1 carries r at 850 and 500 hPa only: its level fields work, a parcel is lifted through the one layer it has (L = 2, the
    # least the library takes), kx lacks 700 hPa
    assert D.plan(fcn, ["td850", "thetae850", "q850"], LAT, LON).moisture == "r"
    two = D.plan(fcn, ["mucape", "muli", "sbcape"], LAT, LON)
    assert two.column == {"parcel": [850, 500]} and [op.pressures for op in two.thermo_ops] == [(850.0, 500.0)] * 2
    with pytest.raises(ValueError, match="runs over 2 to 16 levels with the channels t<level>, r<level>, z<level>; this model has 1"):
        D.plan([c for c in fcn if c != "z500"], ["mucape"], LAT, LON, surface=True)
    with pytest.raises(ValueError, match="'kx' needs the channels 't700', 'r700', which this model lacks"):
        D.plan(fcn, ["kx"], LAT, LON)
    with pytest.raises(ValueError, match="'td333' needs the channels 't333', 'q333'"):
        D.plan(pangu, ["td333"], LAT, LON)
    with pytest.raises(ValueError, match="no such level"):
        D.plan(pangu, ["muli"], LAT, LON, column=dict(parcel=[1000, 850, 700]))
    with pytest.raises(ValueError, match=r"^derived: unknown field 'cin'; known are ws10m, ws100m, ws<level>, thk<a>_<b>.*mucape_src$"):
        D.plan(pangu, ["cin"], LAT, LON)
    with pytest.raises(ValueError, match="'q850' is a channel of this model"):
        D.plan(pangu, ["q850"], LAT, LON)
    with pytest.raises(ValueError, match=r"surface geopotential must be \(33, 64\)"):
        D.LeadDeriver(pangu, LAT, LON, 1, ["mucape"], surface=np.zeros((3, 4)))


def test_a_request_without_thermo_names_never_loads_the_library(monkeypatch):
    def boom():
        raise AssertionError("thermo.load_library called")
    monkeypatch.setattr(T, "load_library", boom)
    p = D.LeadDeriver(_channels("pangu"), LAT, LON, 2, ["ws10m", "ivt", "vo850"]).plan
    assert p.thermo_ops == [] and p.moisture is None and p.column == {} and len(p.ops) == 3
    assert D.LeadDeriver(_channels("pangu"), LAT, LON, 2, ["mucape"]).plan.ops == []                # (planning needs no library either)
    truth = D.TruthDeriver(["mucape", "thetae850", "ws10m"], LAT, LON, column=dict(parcel=[1000, 850, 500]), moisture="q")
    from types import SimpleNamespace
    assert truth.names(SimpleNamespace(names=["t1000", "t850", "t500", "q1000", "q850", "q500", "u10m"])) == ["mucape", "thetae850"]
    assert truth.dropped == {"ws10m": ["v10m"]}
    # what a truth lacks is named channel by channel, also where it holds no whole column
    lacking = D.TruthDeriver(["mucape", "zdeg0", "kx"], LAT, LON)
    assert lacking.names(SimpleNamespace(names=["t1000", "t850", "t500", "q1000", "z500", "u10m"])) == []
    assert lacking.dropped == {"mucape": ["q850", "q500"], "zdeg0": ["z1000", "z850"], "kx": ["t700", "q850", "q700"]}


# ---- 4. sk_exp and sk_log ---------------------------------------------------------------------------------------------------------------- #
def test_sk_exp_and_sk_log_against_float64():
    rng = np.random.default_rng(5)
    x = np.concatenate([rng.uniform(-87, 88, 100000), [-87.0, 88.0, 0.0, -0.0, 1e-8, -1e-8], np.arange(-125, 127) * np.log(2.0)]).astype(np.float32)
    rel = np.abs(R.fp32.exp(x).astype(np.float64) / np.exp(x.astype(np.float64)) - 1).max()
    y = np.concatenate([np.exp(rng.uniform(np.log(1e-30), np.log(1e30), 100000)), [1.0, 2.0, 0.5, 0.70710678, 0.70710683, 1e-30, 1e30]]).astype(np.float32)
    ref = np.log(y.astype(np.float64))
    err = (np.abs(R.fp32.log(y).astype(np.float64) - ref) / np.maximum(np.abs(ref), 1)).max()
    print(f"sk_exp: {rel:.2e} relative (bound {BOUND['exp']:.1e}); sk_log: {err:.2e} relative to max(|log|, 1) (bound {BOUND['log']:.1e})")
    assert rel <= BOUND["exp"] and err <= BOUND["log"]
    assert R.fp32.exp(np.float32(0)) == 1 and R.fp32.log(np.float32(1)) == 0
    assert np.all(np.diff(R.fp32.exp(np.linspace(-87, 88, 20001).astype(np.float32)).astype(np.float64)) > 0)     # monotonic on a coarse grid
    assert R.fp32.exp(np.float32(-1000)) == R.fp32.exp(np.float32(-87)) and R.fp32.exp(np.float32(1000)) == R.fp32.exp(np.float32(88))


# ---- 5. the physics of the float64 restatement ------------------------------------------------------------------------------------------ #
P13 = np.asarray(R.PANGU_LEVELS, np.float64)


def test_saturation_pressure_and_the_humidity_round_trips():
    F = R.f64
    assert F.es(273.15) == 6.112
    rng = np.random.default_rng(0)
    t, rh, p = rng.uniform(220, 310, 2000), rng.uniform(1, 100, 2000), rng.uniform(300, 1000, 2000)
    td, q, _, _ = (np.array(v) for v in zip(*(F.moist(a, b, c, R.R) for a, b, c in zip(t[:50], rh[:50], p[:50]))))
    assert np.allclose(F.es(td), rh[:50] / 100 * F.es(t[:50]), rtol=1e-12)                           # es(td) = e
    back = np.array([F.moist(a, b, c, R.Q)[1] for a, b, c in zip(t[:50], q, p[:50])])
    assert np.allclose(back, rh[:50], rtol=1e-10)                                                    # r -> q -> r
    sat = np.array([F.moist(a, 100.0, c, R.R)[0] for a, c in zip(t[:50], p[:50])])
    assert np.allclose(sat, t[:50], rtol=1e-12)                                                      # saturated: td = t
    th = np.array([F.moist(a, 0.0, 1000.0, R.R)[3] for a in t[:5]])
    assert np.allclose(th, t[:5], rtol=1e-12)                                                        # theta at 1000 hPa is t
    assert all(np.isfinite(v).all() for v in F.moist(t, np.zeros_like(t), 850.0, R.Q)) and all(np.isfinite(v).all() for v in F.moist(t, 0 * t, 850.0, R.R))


def _adiabat(F, T0, r0, p):
    """The parcel lifted from p[0] with temperature T0 and relative humidity r0 %: (its temperature at the levels, its mixing ratio there,
    whether it is saturated there, and its virtual temperature at the NSUB nodes of every layer), from the trace of ``F.parcel``"""
    L = p.size
    t = np.full((L, 1), 250.0)
    t[0] = T0
    m = np.full((L, 1), 50.0)
    m[0] = r0
    trace = {}
    F.parcel(t, m, p, R.R, R.SRC_LOWEST, p_top=p[-1], trace=trace)
    w0 = F.mixr(F.vapour(R.R, np.float64(r0), np.float64(T0), p[0]), p[0])
    lnp = np.log(p)
    tv_nodes = np.zeros((L - 1, R.NSUB))
    for (k, s), (T, _, wet) in trace.items():
        pp = np.exp(lnp[k] + (s + 1) / R.NSUB * (lnp[k + 1] - lnp[k]))
        tv_nodes[k, s] = F.tv(T[0], F.mixr(F.es(T[0]), pp) if wet[0] else w0)
    Tp = np.array([T0] + [trace[(k, R.NSUB - 1)][0][0] for k in range(L - 1)])
    sat = np.array([False] + [bool(trace[(k, R.NSUB - 1)][2][0]) for k in range(L - 1)])
    w = np.where(sat, F.mixr(F.es(Tp), p), w0)
    return Tp, w, sat, tv_nodes, trace


def test_thetae_is_constant_along_the_moist_adiabat_and_theta_below_the_lcl():
    F = R.f64
    p = P13[:12]
    Tp, _, sat, _, trace = _adiabat(F, 300.0, 60.0, p)
    assert not sat[1] and sat[3:].all()                                                              # the LCL lies between the levels
    e0 = F.vapour(R.R, 60.0, 300.0, p[0])
    the = F.thetae(300.0, F.tlcl(300.0, F.dewpoint(e0)), np.log(1000 / p[0]), F.mixr(e0, p[0]))
    for (k, s), (T, _, wet) in trace.items():
        lp = np.log(p[k]) + (s + 1) / R.NSUB * (np.log(p[k + 1]) - np.log(p[k]))
        if wet[0]:
            assert abs(F.thetae_sat(T[0], np.exp(lp), np.log(1000) - lp) - the) <= 1e-9 * the
        else:
            assert abs(T[0] * np.exp(F.KAPPA * (np.log(1000) - lp)) - 300.0 * (1000 / p[0]) ** F.KAPPA) <= 1e-9


def test_cape_of_constructed_environments():
    F = R.f64
    p = P13[:12]                                                                                     # 1000 .. 100 hPa
    lnp = np.log(p)
    Tp, w, sat, tv_nodes, _ = _adiabat(F, 300.0, 70.0, p)
    q = w / (1 + w)                                                                                  # specific humidity: w of a level does not depend on t
    g = (1 + w / F.EPS) / (1 + w)
    tvp = Tp * g
    # 1. the environment is the parcel's own adiabat at the levels: LI is 0, and CAPE is what the curvature of the parcel's tv between the
    #    levels leaves above the environment's straight line in ln p -- the stated error of the trapezoid on these layers
    cape, li, psrc = F.parcel(Tp[:, None], q[:, None], p, R.Q, R.SRC_LOWEST)
    a = (np.arange(R.NSUB) + 1) / R.NSUB
    line = tvp[:-1, None] + a[None] * (tvp[1:] - tvp[:-1])[:, None]
    curv = np.abs(tv_nodes[:11] - line[:11]).max()
    assert psrc[0] == 1000 and abs(li[0]) <= 1e-9 and curv < 0.5
    own, prev = 0.0, 0.0                                                                             # that remainder, restated from the nodes
    for k in range(11):
        for s in range(R.NSUB):
            B = max(tv_nodes[k, s] - line[k, s], 0.0)
            own += 0.5 * (B + prev) * (lnp[k] - lnp[k + 1]) / R.NSUB
            prev = B
    own *= F.RD
    assert abs(cape[0] - own) <= 1e-9 * max(own, 1.0) and 0 <= cape[0] <= F.RD * curv * (lnp[0] - lnp[-1])
    # 2. the environment's tv is the parcel's minus delta at every level above the source: the trapezoid over the nodes, restated here
    #    from the parcel's node values, and R_d delta (ln(p_src / p_top) - ln(p_src / p_1) / 2) to within the curvature term
    delta = 3.0
    tenv = (tvp - delta) / g
    tenv[0] = Tp[0]
    cape_d, li_d, _ = F.parcel(tenv[:, None], q[:, None], p, R.Q, R.SRC_LOWEST)
    tve = tenv * g
    want, prev = 0.0, 0.0
    for k in range(11):
        for s in range(R.NSUB):
            B = max(tv_nodes[k, s] - (tve[k] + a[s] * (tve[k + 1] - tve[k])), 0.0)
            want += 0.5 * (B + prev) * (lnp[k] - lnp[k + 1]) / R.NSUB
            prev = B
    want *= F.RD
    exact = F.RD * delta * ((lnp[0] - lnp[-1]) - 0.5 * (lnp[0] - lnp[1]))
    print(f"own adiabat: cape {cape[0]:.3f} J/kg, curvature {curv:.3f} K; delta = 3 K: {cape_d[0]:.3f}, restated {want:.3f}, analytic {exact:.3f}")
    assert abs(cape_d[0] - want) <= 1e-9 * want
    assert abs(cape_d[0] - exact) <= F.RD * curv * (lnp[0] - lnp[-1])
    assert abs(li_d[0] + delta / g[5]) <= 1e-9
    # 3. a stable isothermal column: exactly zero, in both precisions
    iso = np.full((12, 4), 250.0)
    cape_i, li_i, _ = F.parcel(iso, np.full((12, 4), 40.0), p, R.R, R.SRC_MAX_THETAE)
    assert np.all(cape_i == 0) and np.all(li_i > 0)
    assert np.all(R.fp32.parcel(iso, np.full((12, 4), 40.0), p, R.R, R.SRC_MAX_THETAE)[0] == 0)


def test_masking_the_source_moves_it_up_one_level_and_all_masked_is_nan():
    t, q, r, z, _ = R.columns(3, 64)
    for F, cast in ((R.f64, np.float64), (R.fp32, np.float32)):
        a = F.parcel(t.astype(cast), q.astype(cast), P13, R.Q, R.SRC_LOWEST, z=z.astype(cast), zs=np.full(64, -1e6, cast))
        assert np.all(a[2] == 1000)
        zs = (0.5 * (z[0].astype(np.float64) + z[1])).astype(cast)
        b = F.parcel(t.astype(cast), q.astype(cast), P13, R.Q, R.SRC_LOWEST, z=z.astype(cast), zs=zs)
        assert np.all(b[2] == 925)
        c = F.parcel(t[1:].astype(cast), q[1:].astype(cast), P13[1:], R.Q, R.SRC_LOWEST)                # the same column without its lowest level
        assert np.array_equal(b[0], c[0]) and np.array_equal(b[1], c[1])
        none = F.parcel(t.astype(cast), q.astype(cast), P13, R.Q, R.SRC_LOWEST, z=z.astype(cast), zs=np.full(64, 1e9, cast))
        assert all(np.isnan(v).all() for v in none)
        assert np.isnan(F.freeze(t.astype(cast), z.astype(cast), np.full(64, 1e9, cast))).all()
        top = F.freeze(t.astype(cast), z.astype(cast), (0.5 * (z[-2].astype(np.float64) + z[-1])).astype(cast))
        assert np.array_equal(top, z[-1].astype(cast))                                               # one unmasked level: its z


def test_freezing_level_interpolates_and_falls_back():
    F = R.f64
    t = np.array([[280.0, 270.0, 273.15, 290.0], [276.0, 265.0, 270.0, 285.0], [270.0, 260.0, 265.0, 280.0]])
    z = np.array([[100.0] * 4, [1100.0] * 4, [2100.0] * 4])
    got = F.freeze(t, z)
    assert np.allclose(got, [1100 + 1000 * (276 - 273.15) / 6, 100.0, 100.0, 100.0])                 # crossing; all cold; exactly 0 C at the lowest; all warm
    wave = np.array([[270.0], [276.0], [270.0]])                                                     # two crossings: the upper one counts
    assert np.allclose(F.freeze(wave, z[:, :1]), 1100 + 1000 * (276 - 273.15) / 6)


# ---- 6. fp32 against float64, source forced to the same level -------------------------------------------------------------------------- #
@pytest.fixture(scope="module")
def sample():
    return R.columns(2, 12000)


@pytest.mark.parametrize("kind", ["q", "r"])
def test_fp32_restatement_against_float64_within_the_headers_bounds(sample, kind):
    t, q, r, z, zs = sample
    m, k = (q, R.Q) if kind == "q" else (r, R.R)
    d = lambda a: a.astype(np.float64)                            # noqa: E731
    worst = {}

    def add(name, got, ref, floor=None):
        assert np.array_equal(np.isnan(got), np.isnan(ref)), name
        err = np.abs(got.astype(np.float64) - ref)
        if floor is not None:
            err = err / np.maximum(np.abs(ref), floor)
        worst[name] = max(worst.get(name, 0.0), float(np.nanmax(err)))
    for src in (0, 1, 3):
        a, b = R.fp32.parcel(t, m, P13, k, force_src=src), R.f64.parcel(d(t), d(m), P13, k, force_src=src)
        add("cape", a[0], b[0])
        add("li", a[1], b[1])
    for lev in (0, 2, 5, 8):
        a, b = R.fp32.moist(t[lev], m[lev], P13[lev], k), R.f64.moist(d(t[lev]), d(m[lev]), P13[lev], k)
        add("td", a[0], b[0])
        add("thetae", a[2], b[2])
        add("theta", a[3], b[3])
        if k == R.Q:
            add("rh", a[1], b[1])
        else:
            add("q", a[1], b[1], Q_FLOOR)
    a, b = R.fp32.index(t[2], t[3], t[5], m[2], m[3], k), R.f64.index(d(t[2]), d(t[3]), d(t[5]), d(m[2]), d(m[3]), k)
    add("kx", a[0], b[0])
    add("tt", a[1], b[1])
    for s in (None, zs):                                          # t decreases strictly with height: one crossing at the most, in both
        add("zdeg0", R.fp32.freeze(t, z, s), R.f64.freeze(d(t), d(z), None if s is None else d(s)))
    print(f"fp32 against float64 ({kind}): " + " ".join(f"{n} {v:.2e} (bound {BOUND[n]:.1e})" for n, v in worst.items()))
    assert all(v <= BOUND[n] for n, v in worst.items()), {n: (v, BOUND[n]) for n, v in worst.items() if v > BOUND[n]}


def test_the_header_states_the_bounds_the_tests_assert():
    text = HEADER.read_text()
    for name, key in (("sk_exp", "exp"), ("sk_log", "log"), ("cape", "cape"), ("li", "li"), ("td", "td"), ("rh", "rh"), ("q", "q"),
                      ("thetae", "thetae"), ("theta", "theta"), ("kx, tt", "kx"), ("zdeg0", "zdeg0")):
        line = next(l for l in text.splitlines() if l.startswith(f" *   {name} "))
        nums = [float(x) for x in re.findall(r"(?<![\w.\[-])(\d+\.\d+(?:e-?\d+)?)", line)]
        assert nums[0] == pytest.approx(MEASURED[key], rel=0.06) and nums[-1] == pytest.approx(BOUND[key], rel=0.06), (name, nums)


# ---- 7. the compiler's resource report --------------------------------------------------------------------------------------------------- #
@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not installed")
def test_the_kernels_use_no_scratch_memory():
    r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "--cuda-device-only", "-c", "thermo_ops.hip",
                        "-o", "/dev/null", "-Rpass-analysis=kernel-resource-usage"], cwd=ROOT / "skyrim_amd" / "csrc", capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    found, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            found[name] = {}
        for key in ("VGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "LDS Size [bytes/block]"):
            m = re.search(re.escape(key) + r": (\d+)", line)
            if m and name:
                found[name][key] = int(m.group(1))
    kernels = [k for k in found if "thermo_kernel" in k]
    assert len(kernels) == 2 and len(found) == 2, list(found)                                         # the vector and the scalar path
    for k in kernels:
        print(k, found[k])
        assert found[k]["ScratchSize [bytes/lane]"] == 0 and found[k]["LDS Size [bytes/block]"] == 0, (k, found[k])
        assert found[k]["VGPRs"] <= 128 and found[k]["Occupancy [waves/SIMD]"] >= 4, (k, found[k])
