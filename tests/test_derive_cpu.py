"""Derived fields without a GPU: the C ABI of include/skyrim_derive.h (exports, argument errors), the catalogue on the channel lists of
all seven models, the row table against the restatement's, the definitions of vorticity and divergence against analytic flows, and the
derived names in ``ensemble.validate``."""
from __future__ import annotations

import ctypes
import re
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

import _derive_reference as R
from skyrim_amd import derived as D

HEADER = Path(__file__).resolve().parent.parent / "include" / "skyrim_derive.h"


def grid(n_lat, n_lon, rows=None, ascending=False):
    lat = np.linspace(90.0, -90.0, n_lat)[:rows]
    return (lat[::-1].copy() if ascending else lat), np.arange(n_lon) * (360.0 / n_lon)


# ---- 1. ABI ------------------------------------------------------------------------------------------------------------------------------ #
def test_library_exports_every_declared_symbol():
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    syms = sorted(set(re.findall(r"\b(skderive_[a-z0-9_]+)\s*\(", text)))
    lib = D.load_library()
    assert syms == sorted(D.EXPORTS) and len(syms) == 2
    for s in syms:
        assert hasattr(lib, s)
    const = lambda name: int(re.search(rf"SKDERIVE_{name} \(?(-?\d+)", text).group(1))      # noqa: E731
    assert lib.skderive_abi_version() == D.ABI_VERSION == const("ABI_VERSION")
    assert D.SPEC.env == "SKYRIM_DERIVE_LIB"
    assert (const("MAX_MEMBERS"), const("MAX_OPS"), const("MAX_LEVELS")) == (D.MAX_MEMBERS, D.MAX_OPS, D.MAX_LEVELS) == (64, 16, 16)
    assert (const("SPEED"), const("DIFF"), const("COLUMN"), const("VORTDIV")) == (D.SPEED, D.DIFF, D.COLUMN, D.VORTDIV)
    assert (const("EDGE_ONESIDED"), const("EDGE_POLE")) == (D.EDGE_ONESIDED, D.EDGE_POLE)
    assert ctypes.sizeof(D.OpDesc) == 4 * (2 + 4 * 16 + 4)
    from skyrim_amd import ops
    assert "derive_fields" in ops.OP_NAMES


def _ops():
    L = 8
    return [D.Op(D.SPEED, (0, 1), (0,)), D.Op(D.DIFF, (2, 3), (1,)),
            D.Op(D.COLUMN, (tuple(range(4, 4 + L)), tuple(range(12, 12 + L)), tuple(range(20, 20 + L))), (2, 3, 4, 5), (1.0,) * L),
            D.Op(D.VORTDIV, (0, 1), (6, 7))]


def _desc(ops=None, C=30, H=33, W=64, Dn=8, M=4):
    fake = 4096                                                # never dereferenced: the argument checks come first
    d = D.describe(_ops() if ops is None else ops, M, C, H, W, Dn, Dn * H * W)
    d.members = d.out = d.rowc = fake
    return d


def test_argument_errors_need_no_gpu():
    lib = D.load_library()
    assert lib.skderive_run(None, None) == -1
    changes = [("members", None), ("out", None), ("out", 4098), ("rowc", None), ("rowc", 4100), ("M", 0), ("M", 65), ("n_ops", 0), ("n_ops", 17),
               ("H", 2), ("W", 3), ("C", 1 << 20), ("C", 4), ("D", 7), ("D", 0), ("D", 1 << 20), ("member_stride", 8 * 33 * 64 - 1),
               ("member_align", 8), ("edge_first", 0), ("edge_last", 3)]
    for name, value in changes:
        d = _desc()
        setattr(d, name, value)
        assert lib.skderive_run(ctypes.byref(d), None) == -1, (name, value)

    def with_op(k, **kw):
        ops = _ops()
        ops[k] = D.Op(**{**dict(kind=ops[k].kind, inputs=ops[k].inputs, outputs=ops[k].outputs, weights=ops[k].weights), **kw})
        return _desc(ops)
    col = _ops()[2]
    one = tuple(x[:1] for x in col.inputs)
    bad = [with_op(0, kind=0), with_op(0, kind=5), with_op(0, inputs=(30, 1)), with_op(1, inputs=(2, -1)), with_op(0, outputs=(8,)),
           with_op(0, outputs=(-2,)), with_op(0, outputs=(-1,)), with_op(1, outputs=(0,)), with_op(3, outputs=(6, 6)), with_op(3, outputs=(-1, 5)),
           with_op(2, inputs=one, weights=(1.0,)), with_op(2, inputs=(col.inputs[0], col.inputs[1], (30,) + col.inputs[2][1:])),
           with_op(2, outputs=(-1, -1, -1, -1))]
    for k, d in enumerate(bad):
        assert lib.skderive_run(ctypes.byref(d), None) == -1, k
    d = _desc()
    d.ops[2].n_levels = 17                                     # (the arrays hold 16: only the count can say more)
    assert lib.skderive_run(ctypes.byref(d), None) == -1
    d = _desc(C=1 << 10, H=1 << 10, W=(1 << 10) + 4)           # C H W > 2^30
    assert lib.skderive_run(ctypes.byref(d), None) == -1
    with pytest.raises(ValueError, match="ends inside an op"):
        D.decode([D.SPEED, 0, 0, -1, -1, -1, 3], [])
    ints, floats = D.encode(_ops())
    assert D.decode(ints, floats) == _ops()


# ---- 2. the catalogue -------------------------------------------------------------------------------------------------------------------- #
def _channels():
    from skyrim_amd.dlwp.spec import CHANNELS as DLWP
    from skyrim_amd.fcn.spec import CHANNELS as FCN
    from skyrim_amd.fengwu.spec import CHANNELS as FENGWU
    from skyrim_amd.fuxi.spec import CHANNELS as FUXI
    from skyrim_amd.graphcast.spec import CHANNELS as GRAPHCAST
    from skyrim_amd.pangu.spec import CHANNELS as PANGU
    from skyrim_amd.sfno.spec import CHANNELS as SFNO
    return dict(pangu=PANGU, fengwu=FENGWU, graphcast=GRAPHCAST, fcn=FCN, sfno=SFNO, fuxi=FUXI, dlwp=DLWP)


def test_plan_on_the_channels_of_all_seven_models():
    lat, lon = grid(33, 64)
    ch = _channels()
    levels = [300, 400, 500, 600, 700, 850, 925, 1000]
    for model in ("pangu", "fengwu", "graphcast"):
        names = list(ch[model])
        p = D.plan(names, ["ivt", "ws10m", "iwv", "vo850", "div850", "thk500_1000"], lat, lon)
        assert p.levels == levels and len(p.ops) == 4, model
        col = next(op for op in p.ops if op.kind == D.COLUMN)
        assert [names[i] for i in col.inputs[0]] == [f"q{l}" for l in levels] and [names[i] for i in col.inputs[1]] == [f"u{l}" for l in levels]
        assert [names[i] for i in col.inputs[2]] == [f"v{l}" for l in levels] and col.outputs == (-1, -1, 0, 2)
        assert abs(p.weights.sum() - 100.0 * (1000 - 300) / 9.80665) <= 1e-12 * p.weights.sum()
        assert np.array_equal(p.weights, R.column_weights(levels)) and col.weights == tuple(float(np.float32(w)) for w in p.weights)
        vd = next(op for op in p.ops if op.kind == D.VORTDIV)
        assert vd.inputs == (names.index("u850"), names.index("v850")) and vd.outputs == (3, 4)            # both: one op
        assert next(op for op in p.ops if op.kind == D.DIFF).inputs == (names.index("z500"), names.index("z1000"))
        assert p.inputs["iwv"] == [f"q{l}" for l in levels] and p.inputs["ws10m"] == ["u10m", "v10m"] and p.edges == (D.EDGE_POLE, D.EDGE_POLE)
    sfno = list(ch["sfno"])
    p = D.plan(sfno, ["ws100m", "ws10m", "ws850", "vo10m"], lat, lon)
    assert p.ops[0] == D.Op(D.SPEED, (sfno.index("u100m"), sfno.index("v100m")), (0,)) and len(p.ops) == 4
    for model in ("sfno", "fcn", "fuxi", "dlwp"):
        with pytest.raises(ValueError, match=r"specific humidity.*no channel q<level>"):
            D.plan(ch[model], ["ivt"], lat, lon)
    with pytest.raises(ValueError, match=r"'ws10m' needs the channels 'u10m', 'v10m'"):
        D.plan(ch["dlwp"], ["ws10m"], lat, lon)
    with pytest.raises(ValueError, match=r"'ws100m' needs.*'u100m'"):
        D.plan(ch["pangu"], ["ws100m"], lat, lon)
    with pytest.raises(ValueError, match=r"'thk500_975' needs the channel 'z975'"):
        D.plan(ch["pangu"], ["thk500_975"], lat, lon)
    with pytest.raises(ValueError, match="is a channel of this model"):
        D.plan(list(ch["pangu"]) + ["ws10m"], ["ws10m"], lat, lon)
    with pytest.raises(ValueError, match="unknown field 'gust'"):
        D.plan(ch["pangu"], ["gust"], lat, lon)
    with pytest.raises(ValueError, match="named twice"):
        D.plan(ch["pangu"], ["ivt", "ivt"], lat, lon)
    with pytest.raises(ValueError, match="uniform longitudes"):
        D.plan(ch["pangu"], ["vo850"], lat, lon[:40])
    with pytest.raises(ValueError, match="1 to 64 members"):
        D.check_request(ch["pangu"], ["ws10m"], lat, lon, 65)
    many = [f"ws{l}" for l in (50, 100, 150, 200, 250, 300, 400, 500, 600, 700, 850, 925, 1000)] + ["ws10m", "thk500_1000", "thk300_500", "ivt"]
    with pytest.raises(ValueError, match="17 ops"):
        D.plan(ch["pangu"], many, lat, lon)


@pytest.mark.parametrize("case", ["descending", "ascending", "32of33"])
def test_row_table_equals_the_restatement(case):
    lat, lon = dict(descending=grid(33, 64), ascending=grid(33, 64, ascending=True), **{"32of33": grid(33, 64, rows=32)})[case]
    rowc, e0, e1 = D.row_table(lat, lon)
    want, w0, w1 = R.row_table(lat, lon)
    assert rowc.dtype == np.float32 and rowc.shape == (lat.size, 4) and D.row_table(lat, lon)[0] is rowc                  # cached
    assert (e0, e1) == (w0, w1) == ((D.EDGE_POLE, D.EDGE_ONESIDED) if case == "32of33" else (D.EDGE_POLE, D.EDGE_POLE))
    assert np.array_equal(rowc, want)
    from skyrim_amd.tracks import row_coefficients
    assert np.array_equal(rowc[1:-1], row_coefficients(lat, lon)[1:-1])                # interior rows: the tracker's coefficients
    north = 0 if lat[0] > 0 else -1
    assert rowc[north, 0] > 0 and rowc[north, 1] == -rowc[north, 0]
    if case != "32of33":
        assert rowc[-1 - north if north else -1, 0] < 0


# ---- 3. the definitions themselves -------------------------------------------------------------------------------------------------------- #
def _exact_table(lat, lon):
    """The row table in float64 (the restatement's formulas before the rounding to fp32)."""
    H = lat.size
    phi, dlam, a = np.deg2rad(lat), 2 * np.pi / len(lon), R.A_M
    rc = np.zeros((H, 4))
    for j in range(H):
        n, s = min(j + 1, H - 1), max(j - 1, 0)
        if abs(lat[j]) == 90.0:
            r = 1 if j == 0 else H - 2
            f = np.sign(lat[j]) * np.cos(phi[r]) / (a * (1 - abs(np.sin(phi[r]))))
            rc[j] = [f, -f, 0, 0]
        else:
            den = a * np.cos(phi[j]) * (phi[n] - phi[s])
            rc[j] = [1 / (2 * a * np.cos(phi[j]) * dlam), np.cos(phi[n]) / den, np.cos(phi[s]) / den, 0]
    return rc


@pytest.mark.parametrize("ascending", [False, True])
def test_solid_body_rotation_and_a_divergent_wave(ascending):
    lat, lon = grid(91, 180, ascending=ascending)
    _, e0, e1 = D.row_table(lat, lon)
    rc = _exact_table(lat, lon)
    phi, lam = np.deg2rad(lat)[:, None], np.deg2rad(lon)[None, :]
    a, U0 = R.A_M, 40.0
    h = np.deg2rad(2.0)
    # solid-body rotation: vo = 2 U sin(phi) / a, div = 0; centred differences over 2 h are exact to O(h^2)
    u, v = U0 * np.cos(phi) + 0 * lam, 0 * phi + 0 * lam
    out = R.vortdiv(u, v, None, e0, e1, exact_rowc=rc)
    want = 2 * U0 * np.sin(phi) / a + 0 * lam
    scale = 2 * U0 / a
    assert np.abs(out["vo"][0] - want).max() <= 2 * h ** 2 * scale                  # pole rows included: U (1 + sin(phi_1)) / a there
    assert np.abs(out["vo"][0][[0, -1]] - want[[0, -1]]).max() <= h ** 2 * scale and np.abs(out["div"][0]).max() <= 1e-12 * scale
    # a divergent zonal-wavenumber-2 flow from the potential chi = X cos^2(phi) cos(2 lam): u = d chi / (a cos(phi) d lam), v = d chi / (a d phi)
    X = 1.0e7
    u = -2 * X * np.cos(phi) * np.sin(2 * lam) / a
    v = -2 * X * np.cos(phi) * np.sin(phi) * np.cos(2 * lam) / a
    out = R.vortdiv(u, v, None, e0, e1, exact_rowc=rc)
    # div = laplacian(chi) = (1 / cos) d/dphi(cos d chi/dphi) / a^2 + d2 chi/dlam2 / (a cos)^2 = X cos(2 lam) (4 sin^2(phi) - 2 cos^2(phi) - 4) / a^2
    want = X * np.cos(2 * lam) * (4 * np.sin(phi) ** 2 - 2 * np.cos(phi) ** 2 - 4.0) / a ** 2
    scale = 6 * X / a ** 2
    assert np.abs(out["div"][0] - want)[1:-1].max() <= 4 * h ** 2 * scale
    assert np.abs(out["div"][0][[0, -1]]).max() <= 1e-9 * scale                     # wavenumber 2 has no mean on a latitude circle
    assert np.abs(out["vo"][0])[1:-1].max() <= 4 * h ** 2 * scale                   # and the flow is irrotational


# ---- 4. ensemble.validate ------------------------------------------------------------------------------------------------------------------ #
def test_validate_learns_the_derived_names():
    from skyrim_amd import ensemble as E
    from skyrim_amd.pangu.spec import CHANNELS
    lat, lon = grid(49, 192)
    model = SimpleNamespace(out_channel_names=list(CHANNELS), in_channel_names=list(CHANNELS), grid=SimpleNamespace(lat=lat, lon=lon))
    args = (model, 2, 3, 0, ("mean",))
    tail = (None, 1, False)
    _, ex, qu, saved = E.validate(*args, {"ws10m": [10.0], "t2m": [280.0]}, {"ivt": [0.5]}, *tail, derived=["ws10m", "ivt"])
    assert ex == {"ws10m": [10.0], "t2m": [280.0]} and qu == {"ivt": [0.5]} and saved == [0, 1, 2]
    with pytest.raises(ValueError, match="'ws10m' is not an output channel"):
        E.validate(*args, {"ws10m": [10.0]}, None, *tail)
    with pytest.raises(ValueError, match="'ws10m' is not an output channel"):
        E.validate(*args, {"ws10m": [10.0]}, None, *tail, derived=["ivt"])
    with pytest.raises(ValueError, match="'ivt' is not an output channel"):
        E.validate(*args, None, {"ivt": [0.5]}, *tail, derived=["ws10m"])
    with pytest.raises(ValueError, match="unknown field 'gust'"):
        E.validate(*args, None, None, *tail, derived=["gust"])
    from skyrim_amd.fcn.spec import CHANNELS as FCN
    fcn = SimpleNamespace(out_channel_names=list(FCN), in_channel_names=list(FCN), grid=SimpleNamespace(lat=lat, lon=lon))
    with pytest.raises(ValueError, match="specific humidity"):
        E.validate(fcn, 2, 3, 0, ("mean",), None, None, *tail, derived=["ivt"])
