"""Time-window aggregates without a GPU: the C ABI of include/skyrim_agg.h (exports, argument errors, the descriptor's layout), the
request grammar, the window plan, the slots of ``when_*``, the flat program, the refusals, the command line's options and the compiler's
resource report of csrc/agg_ops.hip."""
from __future__ import annotations

import ctypes
import datetime
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

import _agg_reference as R
from skyrim_amd import aggregate as A
from skyrim_amd import native

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "skyrim_agg.h"
T0 = datetime.datetime(2024, 5, 13, 18, 0)
H6 = datetime.timedelta(hours=6)


# ---- 1. ABI --------------------------------------------------------------------------------------------------------------------------- #
def test_library_exports_every_declared_symbol():
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    syms = sorted(set(re.findall(r"\b(skagg_[a-z0-9_]+)\s*\(", text)))
    assert len(syms) == 2                                        # (that they are EXPORTS, exported, and the ABI version: tests/test_native.py)
    assert A.SPEC.stem == "skyrim_agg" and A.SPEC.prefix == "skagg"
    for name, val in (("MAX_MEMBERS", A.MAX_MEMBERS), ("MAX_OPS", A.MAX_OPS), ("MAX", A.MAX), ("MIN", A.MIN), ("SUM", A.SUM),
                      ("COUNT_ABOVE", A.COUNT_ABOVE), ("FIRST", A.FIRST), ("LAST", A.LAST), ("E_ARG", -1), ("E_HIP", -2)):
        assert int(re.search(rf"SKAGG_{name} \(?(-?\d+)\)?", text).group(1)) == val, name
    assert (R.MAX, R.MIN, R.SUM, R.COUNT_ABOVE, R.FIRST, R.LAST) == (A.MAX, A.MIN, A.SUM, A.COUNT_ABOVE, A.FIRST, A.LAST)
    for doc in (native.__doc__, (ROOT / "skyrim_amd/csrc/Makefile").read_text().splitlines()[0]):
        assert "regrid,agg,event}" in doc
    assert "-ffp-contract=off -shared -o $@ agg_ops.hip" in (ROOT / "skyrim_amd/csrc/Makefile").read_text()


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not installed")
def test_descriptor_layout_matches_the_header(tmp_path):
    fields = [n for n, _ in A.AggDesc._fields_]
    op_fields = [n for n, _ in A.OpDesc._fields_]
    src = tmp_path / "layout.cpp"
    src.write_text('#include <cstdio>\n#include <cstddef>\n#include "skyrim_agg.h"\nint main() {\n  printf("%zu", sizeof(skagg_desc));\n'
                   + "".join(f'  printf(" %zu", offsetof(skagg_desc, {f}));\n' for f in fields)
                   + '  printf(" %zu", sizeof(skagg_op));\n'
                   + "".join(f'  printf(" %zu", offsetof(skagg_op, {f.rstrip("_")}));\n' for f in op_fields) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    r = subprocess.run(["hipcc", "-x", "c++", "-std=c++17", f"-I{ROOT / 'include'}", str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    n = len(fields)
    assert got[0] == ctypes.sizeof(A.AggDesc) and got[1:n + 1] == [getattr(A.AggDesc, f).offset for f in fields]
    assert got[n + 1] == ctypes.sizeof(A.OpDesc) and got[n + 2:] == [getattr(A.OpDesc, f).offset for f in op_fields]


def _desc(ops=None, **kw):
    fake = 4096                                                # never dereferenced: the argument checks come first
    ops = [A.Op(A.MAX, 0, 0, when=1, phase=A.FIRST), A.Op(A.SUM, 2, 2, phase=A.FIRST | A.LAST)] if ops is None else ops
    geo = dict(M=4, C=3, H=5, W=8, D=4, member_stride=4 * 5 * 8)
    geo.update({k: kw.pop(k) for k in list(kw) if k in geo})
    d = A.describe(ops, geo["M"], geo["C"], geo["H"], geo["W"], geo["D"], geo["member_stride"], 6.0, kw.pop("member_align", 16))
    d.members, d.acc = fake, fake
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_argument_errors_need_no_gpu():
    lib = A.load_library()
    run = lambda d: lib.skagg_update(ctypes.byref(d), None)      # noqa: E731
    assert lib.skagg_update(None, None) == -1
    # NULL or misaligned pointers
    assert run(_desc(members=None)) == -1 and run(_desc(acc=None)) == -1
    assert run(_desc(acc=4098)) == -1 and run(_desc(acc=4097)) == -1 and run(_desc(members=4100)) == -1
    assert run(_desc(member_align=8)) == -1 and run(_desc(member_align=0)) == -1
    # counts
    for M in (0, 65, -1):
        assert run(_desc(M=M)) == -1, M
    for name in ("C", "H", "W", "D"):
        assert run(_desc(**{name: 0})) == -1 and run(_desc(**{name: -3})) == -1, name
    assert run(_desc(ops=[])) == -1 and run(_desc(n_ops=17)) == -1 and run(_desc(n_ops=-1)) == -1
    # channels and slots
    op = lambda **k: A.Op(**dict(dict(kind=A.MAX, channel=0, out=0, when=-1, phase=A.FIRST), **k))      # noqa: E731
    for bad in (op(channel=-1), op(channel=3), op(out=-1), op(out=4), op(when=4), op(when=-2)):
        assert run(_desc(ops=[bad])) == -1, bad
    # a slot named twice, out and when together
    assert run(_desc(ops=[op(out=1), op(kind=A.SUM, out=1)])) == -1
    assert run(_desc(ops=[op(out=1, when=1)])) == -1
    assert run(_desc(ops=[op(out=0, when=1), op(kind=A.MIN, out=2, when=1)])) == -1
    assert run(_desc(ops=[op(out=0, when=1), op(kind=A.SUM, channel=1, out=1)])) == -1
    # when on SUM or COUNT_ABOVE
    assert run(_desc(ops=[op(kind=A.SUM, when=1)])) == -1 and run(_desc(ops=[op(kind=A.COUNT_ABOVE, when=1)])) == -1
    # kinds and phases outside the defined ones
    for kind in (0, 5, -1):
        assert run(_desc(ops=[op(kind=kind)])) == -1, kind
    for phase in (-1, 4, 8):
        assert run(_desc(ops=[op(phase=phase)])) == -1, phase
    # beyond the 32-bit byte offsets, and a stride shorter than the slots
    assert run(_desc(C=1 << 10, H=1 << 11, W=1 << 10, D=1, member_stride=1 << 21)) == -1
    assert run(_desc(C=1, H=1 << 11, W=1 << 10, D=1 << 10, member_stride=1 << 31)) == -1
    assert run(_desc(H=1 << 16, W=1 << 16, member_stride=1 << 40)) == -1
    assert run(_desc(member_stride=4 * 5 * 8 - 1)) == -1
    # the Python binding refuses what it can see, before the library is asked
    with pytest.raises(ValueError, match="1 to 16"):
        A.run([torch.zeros(1, 2, 4)], torch.zeros(1, dtype=torch.int64), [], torch.zeros(1, 1, 2, 4), 0.0)
    with pytest.raises(ValueError, match="expected a contiguous float32 tensor"):
        A.run([torch.zeros(1, 2, 4)], torch.zeros(1, dtype=torch.int64), [A.Op(A.MAX, 0, 0)], torch.zeros(1, 1, 2, 4), 0.0)


def test_op_is_registered_and_has_no_cpu_kernel():
    from skyrim_amd import ops
    assert "agg_update" in ops.OP_NAMES
    with pytest.raises(NotImplementedError):
        torch.ops.skyrim_hip.agg_update([torch.zeros(1, 2, 4)], torch.zeros(1, dtype=torch.int64), [A.MAX, 0, 0, -1, A.FIRST], [0.0, 1.0], 6.0,
                                        torch.zeros(1, 1, 2, 4))


# ---- 2. requests ---------------------------------------------------------------------------------------------------------------------- #
def test_request_grammar_and_names():
    r = A.parse_request("ws10m:max:24h")
    assert r == A.Request("ws10m", "max", "24h") and r.name == "ws10m_max_24h"
    assert A.parse_request("ws10m:hours_above@15:24h").name == "ws10m_hours_above@15_24h"
    assert A.parse_request("t2m:hours_above@273.15:all").name == "t2m_hours_above@273.15_all"
    assert A.parse_request("t2m:hours_above@-inf:all").stat == "hours_above@-inf"
    assert A.parse_request(A.Request("msl", "when_min", "all")).name == "msl_when_min_all"

    class Mine:                                                  # any object with the three fields
        channel, stat, window = "t2m", "mean", "12h"
    assert A.parse_request(Mine()) == A.Request("t2m", "mean", "12h")
    for stat in ("max", "min", "mean", "sum", "when_max", "when_min"):
        assert A.parse_request(f"t2m:{stat}:6h").stat == stat
    for bad in ("t2m", "t2m:max", "t2m:max:24h:x", ":max:24h", "t2m:median:24h", "t2m:hours_above:24h", "t2m:hours_above@:24h",
                "t2m:hours_above@warm:24h", "t2m:hours_above@nan:24h", "t2m:max:24", "t2m:max:0h", "t2m:max:-6h", "t2m:max:1.5h",
                "t2m:max:daily", "t2m:max:", 7, ("t2m", "max", "24h")):
        with pytest.raises(ValueError, match="aggregates"):
            A.parse_request(bad)


def test_window_plan():
    names = ["u10m", "t2m", "ws10m"]
    p = A.plan(names, ["ws10m:max:24h", "t2m:mean:24h"], H6, 10)
    assert [g.label for g in p.groups] == ["24h"] and p.D == 2 and p.dt == 6.0
    g = p.groups[0]
    assert (g.length, g.n_windows, g.fields, g.slots) == (4, 2, ["ws10m_max_24h", "t2m_mean_24h"], [0, 1])
    assert list(g.steps(0)) == [1, 2, 3, 4] and list(g.steps(1)) == [5, 6, 7, 8]
    assert p.incomplete == {"24h": (9, 10)}                      # steps 9 and 10 open a window the rollout does not complete
    assert p.ops_at(0) == [] and p.ops_at(9) == [] and p.ops_at(10) == [] and p.ops_at(11) == []
    for k, phase in ((1, A.FIRST), (2, 0), (3, 0), (4, A.LAST), (5, A.FIRST), (6, 0), (7, 0), (8, A.LAST)):
        assert [o.phase for o in p.ops_at(k)] == [phase, phase], k
    assert [[(g.label, w) for g, w in p.closing(k)] for k in range(11)] == [[], [], [], [], [("24h", 0)], [], [], [], [("24h", 1)], [], []]
    mx, mean = p.ops_at(1)
    assert (mx.kind, mx.channel, mx.out, mx.when) == (A.MAX, 2, 0, -1)
    assert (mean.kind, mean.channel, mean.out, mean.scale) == (A.SUM, 1, 1, 0.25)
    # all: one window over every step; a one-step window sets both bits; groups are ordered as first requested and contiguous
    p = A.plan(names, ["t2m:sum:all", "ws10m:hours_above@15:6h", "u10m:min:all"], H6, 5)
    assert [(g.label, g.length, g.n_windows, g.slots) for g in p.groups] == [("all", 5, 1, [0, 1]), ("6h", 1, 5, [2])]
    assert p.incomplete == {} and p.group("all").fields == ["t2m_sum_all", "u10m_min_all"]
    assert [o.phase for o in p.ops_at(1)] == [A.FIRST, A.FIRST, A.FIRST | A.LAST]
    assert [o.phase for o in p.ops_at(5)] == [A.LAST, A.LAST, A.FIRST | A.LAST]
    assert [(g.label, w) for g, w in p.closing(5)] == [("all", 0), ("6h", 4)] and [(g.label, w) for g, w in p.closing(3)] == [("6h", 2)]
    hrs = p.group("6h").ops[0]
    assert (hrs.kind, hrs.thr, hrs.scale) == (A.COUNT_ABOVE, 15.0, 6.0) and p.group("all").ops[0].scale == 1.0
    assert A.plan(names, ["t2m:mean:all"], H6, 3).groups[0].ops[0].scale == float(np.float32(1 / 3))
    assert A.plan(names, ["t2m:mean:12h"], 6, 2).groups[0].length == 2              # the step in hours is accepted too
    # refusals
    with pytest.raises(ValueError, match="not a positive multiple"):
        A.plan(names, ["t2m:max:9h"], H6, 10)
    with pytest.raises(ValueError, match="not a positive multiple"):
        A.plan(names, ["t2m:max:3h"], H6, 10)
    with pytest.raises(ValueError, match="does not fit"):
        A.plan(names, ["t2m:max:24h"], H6, 3)
    with pytest.raises(ValueError, match="does not fit"):
        A.plan(names, ["t2m:max:all"], H6, 0)
    with pytest.raises(ValueError, match="requested twice"):
        A.plan(names, ["t2m:max:24h", "t2m:max:24h"], H6, 4)
    with pytest.raises(ValueError, match="not an output channel"):
        A.plan(names, ["q700:max:24h"], H6, 4)
    with pytest.raises(ValueError, match="at least one"):
        A.plan(names, [], H6, 4)
    with pytest.raises(ValueError, match="one call holds 16"):
        A.plan(names, [f"t2m:hours_above@{k}:6h" for k in range(17)], H6, 4)
    assert len(A.plan(names, [f"t2m:hours_above@{k}:6h" for k in range(16)], H6, 4).ops_at(1)) == 16


def test_when_shares_the_slot_of_its_extreme():
    names = ["msl", "ws10m"]
    p = A.plan(names, ["ws10m:when_max:24h", "ws10m:max:24h", "msl:when_min:24h", "ws10m:when_min:all"], H6, 4)
    g = p.group("24h")
    assert g.fields == ["ws10m_when_max_24h", "ws10m_max_24h", "msl_when_min_24h"] and g.slots == [0, 1, 2]
    assert g.ops == [A.Op(A.MAX, 1, 1, when=0), A.Op(A.MIN, 0, 4, when=2)]     # max's slot is shared; msl's minimum goes to a hidden slot
    assert p.group("all").slots == [3] and p.group("all").ops == [A.Op(A.MIN, 1, 5, when=3)]
    assert p.D == 6                                              # four fields, then two hidden value slots
    slots = [s for o in p.ops_at(4) for s in (o.out, o.when) if s >= 0]
    assert len(slots) == len(set(slots)) == 6


def test_encode_decode_round_trip():
    ops = [A.Op(A.MAX, 3, 0, when=5, phase=A.FIRST), A.Op(A.SUM, 1, 1, phase=A.LAST, scale=float(np.float32(1 / 7))),
           A.Op(A.COUNT_ABOVE, 0, 2, phase=3, thr=float("-inf"), scale=6.0), A.Op(A.MIN, 2, 3)]
    ints, floats = A.encode(ops)
    assert len(ints) == 20 and len(floats) == 8 and all(isinstance(i, int) for i in ints)
    assert A.decode(ints, floats) == ops
    d = A.describe(A.decode(ints, floats), 2, 4, 5, 8, 6, 240, 12.0, 4)
    assert (d.n_ops, d.stamp, d.member_align, d.ops[0].when, d.ops[1].scale, d.ops[2].thr) == (4, 12.0, 4, 5, np.float32(1 / 7), -np.inf)
    assert d.ops[2].in_ == 0 and d.ops[0].in_ == 3
    for bad in ((ints[:-1], floats), (ints, floats[:-1]), ([9] + ints[1:], floats)):
        with pytest.raises(ValueError, match="agg_update"):
            A.decode(*bad)


def test_reference_restates_the_header():
    """The restatement on a hand-made case: max / when with a tie and a NaN, mean, hours above."""
    x = [np.array(v, np.float32).reshape(1, 1, 1, 4) for v in ([1, 5, 2, 3], [4, 5, np.nan, 1], [2, 7, 9, 3])]
    ops = [A.Op(A.MAX, 0, 0, when=1), A.Op(A.SUM, 0, 2, scale=float(np.float32(1 / 3))), A.Op(A.COUNT_ABOVE, 0, 3, thr=2.0, scale=6.0)]
    per = [[A.Op(o.kind, o.channel, o.out, o.when, ph, o.thr, o.scale) for o in ops] for ph in (A.FIRST, 0, A.LAST)]
    acc = R.fold(x, per, [6.0, 12.0, 18.0], 4)[0, :, 0]
    assert np.array_equal(acc[0], [4, 7, np.nan, 3], equal_nan=True) and np.array_equal(acc[1], [12, 18, np.nan, 6], equal_nan=True)
    assert np.array_equal(acc[2, [0, 1, 3]], (np.array([7, 17, 7], np.float32) * np.float32(1 / 3)))
    assert np.array_equal(acc[3], [6, 18, np.nan, 12], equal_nan=True)


# ---- 3. the refusals of the public surface -------------------------------------------------------------------------------------------- #
def _model():
    from test_ens_cpu import _Model
    return _Model()


def test_refusals():
    from skyrim_amd import ensemble
    m = _model()
    ens = dict(n_steps=4, n_members=3)
    with pytest.raises(ValueError, match="not an output channel"):
        m.ensemble_forecast(T0, aggregates=["ws10m:max:24h"], **ens)              # a derived field that derived= does not list
    with pytest.raises(ValueError, match="needs the channel"):
        m.ensemble_forecast(T0, aggregates=["ws10m:max:24h"], derived=["ws10m"], **ens)      # ... and one the model cannot form
    with pytest.raises(ValueError, match="unknown statistic"):
        m.ensemble_forecast(T0, aggregates=["t2m:median:24h"], **ens)
    with pytest.raises(ValueError, match="not a positive multiple"):
        m.ensemble_forecast(T0, aggregates=["t2m:max:9h"], **ens)
    with pytest.raises(ValueError, match="does not fit"):
        m.ensemble_forecast(T0, aggregates=["t2m:max:48h"], **ens)
    with pytest.raises(ValueError, match="a list of requests"):
        m.ensemble_forecast(T0, aggregates="t2m:max:24h", **ens)
    with pytest.raises(ValueError, match="at least one"):
        m.ensemble_forecast(T0, aggregates=[], **ens)
    with pytest.raises(ValueError, match="or one of the aggregates"):
        m.ensemble_forecast(T0, aggregates=["t2m:max:24h"], exceed={"t2m_max_12h": [280.0]}, **ens)
    with pytest.raises(ValueError, match="1 to 4 values"):
        m.ensemble_forecast(T0, aggregates=["t2m:max:24h"], exceed={"t2m_max_24h": [1.0, 2.0, 3.0, 4.0, 5.0]}, **ens)
    with pytest.raises(ValueError, match="needs scores=True"):
        m.ensemble_forecast(T0, aggregates=["t2m:max:24h"], events={"t2m_max_24h": [280.0]}, **ens)
    with pytest.raises(ValueError, match="does not fit"):
        m.aggregate_forecast(T0, 2, ["t2m:max:24h"])
    with pytest.raises(ValueError, match="not an output channel"):
        m.aggregate_forecast(T0, 4, ["msl:when_min:all"])
    # everything valid: the names of aggregates are known to exceed=, and the work itself needs the device
    lat, lon = m.model.grid.lat, m.model.grid.lon
    out = ensemble.validate(m.model, 4, 3, 0, ("mean",), {"t2m_max_24h": [280.0]}, {"u1000_mean_12h": [0.5]}, None, 1, False,
                            aggregates=["t2m:max:24h", "u1000:mean:12h"])
    assert out[1] == {"t2m_max_24h": [280.0]} and out[2] == {"u1000_mean_12h": [0.5]}
    with pytest.raises(RuntimeError, match="GPU"):
        m.aggregate_forecast(T0, 4, ["t2m:max:24h"])
    with pytest.raises(ValueError, match="65"):
        A.check_request(["t2m"], ["t2m:max:all"], H6, 4, lat, lon, 65)
    with pytest.raises(ValueError, match="2\\^30"):
        A.check_request(["t2m"], ["t2m:max:all", "t2m:min:all"], H6, 4, np.zeros(1 << 15), np.zeros(1 << 15))
    with pytest.raises(ValueError, match="needs n_steps"):
        A.LeadAggregator(["t2m"], lat, lon, 3, ["t2m:max:all"], T0, H6)
    agg = A.LeadAggregator(["t2m"], lat, lon, 3, ["t2m:max:12h"], T0, H6, n_steps=5)
    assert agg.incomplete == {"12h": (5, 5)} and agg.plan.D == 1
    with pytest.raises(ValueError, match="one window group"):
        A.TruthAggregator(["t2m:max:12h", "t2m:max:all"], lat, lon, T0, H6)


def test_wrappers_that_cannot_aggregate_say_what_to_do():
    from skyrim_amd.core.models.ensemble import GlobalEnsemble
    from skyrim_amd.core.models.graphcast import GraphcastModel
    with pytest.raises(NotImplementedError, match="aggregate_prediction"):
        GraphcastModel.aggregate_forecast(object.__new__(GraphcastModel), T0, 4, ["t2m:max:all"])
    with pytest.raises(ValueError, match="aggregate_prediction"):
        ge = object.__new__(GlobalEnsemble)
        ge.model_names = ["pangu", "fuxi"]
        ge.aggregate_forecast(T0, 4, ["t2m:max:all"])


def test_aggregate_prediction_checks_before_the_device():
    from skyrim_amd.labeled import DataArray
    lat, lon = np.linspace(60, -60, 5), np.arange(8) * 45.0
    times = [T0 + k * H6 for k in range(5)]
    da = DataArray(np.zeros((5, 2, 5, 8), np.float32), ["time", "channel", "lat", "lon"], dict(time=times, channel=["t2m", "msl"], lat=lat, lon=lon))
    with pytest.raises(ValueError, match="not an output channel"):
        A.aggregate_prediction(da, ["ws10m:max:all"])
    with pytest.raises(ValueError, match="does not fit"):
        A.aggregate_prediction(da, ["t2m:max:48h"])
    uneven = DataArray(da.values[:3], da.dims, dict(time=[times[0], times[1], times[3]], channel=["t2m", "msl"], lat=lat, lon=lon))
    with pytest.raises(ValueError, match="equally spaced"):
        A.aggregate_prediction(uneven, ["t2m:max:all"])
    with pytest.raises(ValueError, match="two time entries"):
        A.aggregate_prediction(da.isel(time=slice(0, 1)), ["t2m:max:all"])
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="GPU"):
            A.aggregate_prediction(da, ["t2m:max:all"])


# ---- 4. the command line ---------------------------------------------------------------------------------------------------------------- #
def test_command_line_options():
    from click.testing import CliRunner
    from skyrim_amd import aggregate_cli
    res = CliRunner().invoke(aggregate_cli.aggregate, ["--help"])
    assert res.exit_code == 0 and "--aggregate" in res.output and "--derived" in res.output
    v = {p.name: p for p in aggregate_cli.aggregate.params}
    assert v["aggregates"].multiple and v["members"].default == 1 and v["derived"].default == ""
    res = CliRunner().invoke(aggregate_cli.aggregate, ["-m", "pangu"])
    assert res.exit_code != 0 and "--aggregate" in res.output
    res = CliRunner().invoke(aggregate_cli.aggregate, ["-m", "pangu", "--aggregate", "t2m:median:24h"])
    assert res.exit_code != 0 and "unknown statistic" in repr(res.exception)
    from skyrim_amd.labeled import DataArray
    da = DataArray(np.arange(2 * 1 * 2 * 2, dtype=np.float32).reshape(2, 1, 2, 2), ["time", "channel", "lat", "lon"],
                   dict(time=[T0 + 2 * H6, T0 + 4 * H6], channel=["t2m_max_12h"], lat=[1.0, 0.0], lon=[0.0, 1.0], window_start=[T0, T0 + 2 * H6]))
    assert aggregate_cli.lines({"12h": da}) == ["(0h, 12h] t2m_max_12h: min=0 mean=1.5 max=3", "(12h, 24h] t2m_max_12h: min=4 mean=5.5 max=7"]


# ---- 5. the compiler's resource report -------------------------------------------------------------------------------------------------- #
@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not installed")
def test_kernels_use_no_scratch_and_no_lds():
    r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "--cuda-device-only", "-c", "agg_ops.hip",
                        "-o", "/dev/null", "-Rpass-analysis=kernel-resource-usage"], cwd=ROOT / "skyrim_amd" / "csrc", capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    scratch, lds, name = {}, {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and name:
            scratch[name] = int(m.group(1))
        m = re.search(r"LDS Size \[bytes/block\]: (\d+)", line)
        if m and name:
            lds[name] = int(m.group(1))
    assert sum("agg_kernel" in k for k in scratch) == 2                                        # vector, scalar
    assert all(v == 0 for v in scratch.values()) and all(v == 0 for v in lds.values()), (scratch, lds)
