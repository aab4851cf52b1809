"""Column thermodynamics on the device (include/skyrim_thermo.h): dew point, humidity conversion, theta and theta-e of a
level, the K and total-totals indices, the 0 C level, CAPE and lifted index -- the binding of libskyrim_thermo.so (``SPEC``,
``load_library``, ``run``); the same call is ``torch.ops.skyrim_hip.thermo_fields``.  The catalogue that resolves user-facing names
(``mucape``, ``thetae850`` ...) into these ops is ``derived.plan``; ``derived.LeadDeriver`` launches them after the derive ops into
the same buffer.  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass

import numpy as np

from . import native, program

MAX_MEMBERS, MAX_OPS, MAX_LEVELS = 64, 16, 16                   # include/skyrim_thermo.h SKTHERMO_MAX_*
MOIST, INDEX, FREEZE, PARCEL = 1, 2, 3, 4                       # SKTHERMO_MOIST ...
Q, R = 0, 1                                                     # SKTHERMO_Q, SKTHERMO_R
SRC_LOWEST, SRC_MAX_THETAE = 0, 1                               # SKTHERMO_SRC_*
RESULTS = {MOIST: 4, INDEX: 2, FREEZE: 1, PARCEL: 3}            # output slots of an op
P_SRC_MIN, P_TOP = 700.0, 100.0                                 # the customary most-unstable layer and top of the integral, hPa
_P = ctypes.c_void_p


class OpDesc(ctypes.Structure):
    """skthermo_op."""
    _fields_ = [("kind", ctypes.c_int32), ("n_levels", ctypes.c_int32), ("moisture", ctypes.c_int32), ("source", ctypes.c_int32),
                ("in_t", ctypes.c_int32 * MAX_LEVELS), ("in_m", ctypes.c_int32 * MAX_LEVELS), ("in_z", ctypes.c_int32 * MAX_LEVELS),
                ("p", ctypes.c_float * MAX_LEVELS), ("p_src_min", ctypes.c_float), ("p_top", ctypes.c_float), ("out", ctypes.c_int32 * 4)]


class ThermoDesc(ctypes.Structure):
    """skthermo_desc."""
    _fields_ = [("members", _P), ("M", ctypes.c_int), ("member_align", ctypes.c_int), ("C", ctypes.c_int), ("H", ctypes.c_int),
                ("W", ctypes.c_int), ("D", ctypes.c_int), ("out", _P), ("member_stride", ctypes.c_size_t), ("zs", _P),
                ("n_ops", ctypes.c_int), ("ops", OpDesc * MAX_OPS)]


SPEC = native.Spec("skyrim_thermo", "SKYRIM_THERMO_LIB", "skthermo", 1, {       # include/skyrim_thermo.h SKTHERMO_ABI_VERSION
    "skthermo_abi_version": (ctypes.c_int, []),
    "skthermo_run": (ctypes.c_int, [ctypes.POINTER(ThermoDesc), _P]),
}, " -- column thermodynamics has no torch fallback")
EXPORTS, ABI_VERSION = SPEC.exports, SPEC.abi

_lib = None


def load_library() -> ctypes.CDLL:
    """libskyrim_thermo.so (built in-tree by ``__graft_entry__.build()`` / ``make -C skyrim_amd/csrc``)."""
    global _lib
    if _lib is None:
        _lib = native.load(SPEC)
    return _lib


def sk_log(x) -> np.ndarray:
    """fp32 sk_log of include/skyrim_thermo.h (x positive, normal, finite) in numpy: the bits csrc/thermo_math.h makes on the host and the device"""
    f = np.float32
    m, e = np.frexp(np.asarray(x, f))
    lo = m < f("0.70710678")
    m = np.where(lo, m + m, m).astype(f)
    e = (e - lo).astype(f)
    s = (m - f(1)) / (m + f(1))
    z = s * s
    p = f("0.181818182")
    for c in ("0.222222222", "0.285714286", "0.4", "0.666666667", "2"):
        p = p * z + f(c)
    return ((e * f("-2.12194440e-4") + s * p) + e * f("0.693359375")).astype(f)


def sk_exp(x) -> np.ndarray:
    """fp32 sk_exp of include/skyrim_thermo.h in numpy"""
    f = np.float32
    x = np.clip(np.asarray(x, f), f(-87), f(88)).astype(f)
    n = np.rint(x * f("1.44269504")).astype(f)
    r = (x - n * f("0.693359375")) - n * f("-2.12194440e-4")
    p = f("1.98412698e-4")
    for c in ("1.38888889e-3", "8.33333333e-3", "4.16666667e-2", "1.66666667e-1", "0.5"):
        p = p * r + f(c)
    p = ((p * r) * r + r) + f(1)
    return np.ldexp(p, n.astype(np.int32)).astype(f)


@dataclass(frozen=True)
class Op:
    """One op of a program.  Channel indices: ``t``, ``m`` (the moisture planes, of kind ``moisture``) and ``z`` -- one each for MOIST
    (no z), (t850, t700, t500) and (m850, m700) for INDEX, L each for FREEZE (no m) and PARCEL (z only when a surface is given);
    ``pressures``: hPa, one for MOIST, L strictly decreasing for PARCEL; ``outputs``: one slot per result (``RESULTS``), -1 = not computed."""
    kind: int
    t: tuple
    m: tuple
    z: tuple
    outputs: tuple
    moisture: int = Q
    pressures: tuple = ()
    source: int = SRC_LOWEST
    p_src_min: float = P_SRC_MIN
    p_top: float = P_TOP


def encode(ops) -> tuple:
    """(ints, floats): the flat form ``torch.ops.skyrim_hip.thermo_fields`` takes.  Per op: kind, moisture, source, the counts of t, m, z
    and pressures, four slots, then the t, m and z channels; the floats are the pressures, p_src_min and p_top, op after op."""
    ints, floats = [], []
    for op in ops:
        slots = list(op.outputs) + [-1] * (4 - len(op.outputs))
        ints += [int(op.kind), int(op.moisture), int(op.source), len(op.t), len(op.m), len(op.z), len(op.pressures)] + [int(s) for s in slots]
        ints += [int(c) for c in tuple(op.t) + tuple(op.m) + tuple(op.z)]
        floats += [float(p) for p in op.pressures] + [float(op.p_src_min), float(op.p_top)]
    return ints, floats


def decode(ints, floats) -> list:
    ops, i, f = [], 0, 0
    ints, floats = list(ints), list(floats)
    while i < len(ints):
        if i + 11 > len(ints):
            raise ValueError("thermo_fields: the program ends inside an op")
        kind, moisture, source, nt, nm, nz, npr = ints[i:i + 7]
        slots = ints[i + 7:i + 11]
        i += 11
        if kind not in RESULTS:
            raise ValueError(f"thermo_fields: unknown op kind {kind}")
        if min(nt, nm, nz, npr) < 0 or i + nt + nm + nz > len(ints) or f + npr + 2 > len(floats):
            raise ValueError("thermo_fields: the program ends inside an op")
        t, m, z = tuple(ints[i:i + nt]), tuple(ints[i + nt:i + nt + nm]), tuple(ints[i + nt + nm:i + nt + nm + nz])
        i += nt + nm + nz
        ops.append(Op(kind, t, m, z, tuple(slots[:RESULTS[kind]]), moisture, tuple(floats[f:f + npr]), source, floats[f + npr], floats[f + npr + 1]))
        f += npr + 2
    return ops


def describe(ops, M, C, H, W, D, member_stride, member_align=16) -> ThermoDesc:
    """The descriptor of a program, its pointers still NULL."""
    d = ThermoDesc()
    program.fill_head(d, M, C, H, W, D, member_stride, member_align)
    ops = list(ops)
    d.n_ops = len(ops)
    for k, op in enumerate(ops[:MAX_OPS]):
        o = d.ops[k]
        o.kind, o.moisture, o.source, o.p_src_min, o.p_top = op.kind, op.moisture, op.source, op.p_src_min, op.p_top
        o.n_levels = len(op.t) if op.kind in (FREEZE, PARCEL) else 0
        for r in range(4):
            o.out[r] = int(op.outputs[r]) if r < len(op.outputs) else -1
        for dst, src in ((o.in_t, op.t), (o.in_m, op.m), (o.in_z, op.z), (o.p, op.pressures)):
            for l, v in enumerate(tuple(src)[:MAX_LEVELS]):
                dst[l] = v
    return d


_SHAPES = {MOIST: "a MOIST op has one t, at most one moisture channel and one pressure",
           INDEX: "an INDEX op has t850, t700, t500 and the moisture at 850 and 700",
           FREEZE: f"a FREEZE op has 2 to {MAX_LEVELS} levels, each with t and z",
           PARCEL: f"a PARCEL op has 2 to {MAX_LEVELS} levels, each with t, moisture and a pressure (and z with a surface)"}


def _shape_ok(op, surface: bool) -> bool:
    nt, nm, nz, npr = len(op.t), len(op.m), len(op.z), len(op.pressures)
    if op.kind == MOIST:
        return nt == 1 and nm <= 1 and npr == 1
    if op.kind == INDEX:
        return nt == 3 and nm == 2
    if op.kind == FREEZE:
        return 2 <= nt <= MAX_LEVELS and nz == nt
    return 2 <= nt <= MAX_LEVELS and nm == nt and npr == nt and (nz == nt or (nz == 0 and not surface))


def run(members, table, ops, out, surface=None) -> None:
    """One ``skthermo_run``: the program ``ops`` on the M ``members`` (equal-shaped contiguous float32 (C, H, W) device tensors;
    ``table`` = ``members.member_table(members)``) into ``out``, float32 (M, D, H, W).  ``surface``: float32 (H, W) on the device, the
    surface geopotential that masks the levels below the ground, or None.  Queued on torch's current stream.  As in ``derived.run``,
    the contents of ``table`` are trusted to be the addresses of ``members``."""
    import torch
    ops = list(ops)
    M, dev, align, C, H, W, D, po = program.bind("thermo_fields", members, table, ops, out, "thermo_fields: out", MAX_MEMBERS, MAX_OPS)
    for op in ops:
        if op.kind not in RESULTS:
            raise ValueError(f"thermo_fields: unknown op kind {op.kind}")
        if not _shape_ok(op, surface is not None):
            raise ValueError(f"thermo_fields: {_SHAPES[op.kind]}")
        if len(op.outputs) != RESULTS[op.kind]:
            raise ValueError("thermo_fields: an op has one slot per result (MOIST: 4; INDEX: 2; FREEZE: 1; PARCEL: 3)")
    d = describe(ops, M, C, H, W, D, D * H * W, align)
    d.members, d.out = table.data_ptr(), po
    if surface is not None:
        d.zs = program.plane("thermo_fields", surface, "surface", (H, W), torch.float32, dev)
    lib = load_library()
    program.launch(lib, lib.skthermo_run, d, dev)
