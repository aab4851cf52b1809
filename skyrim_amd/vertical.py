"""Vertical interpolation on the device (include/skyrim_vert.h): fields on a pressure, a height above sea level or above
the ground, an isentrope or an isotherm -- the binding of libskyrim_vert.so (``SPEC``, ``load_library``, ``run``); the same call is
``torch.ops.skyrim_hip.vert_fields``.  The catalogue that resolves user-facing names (``ws@100magl``, ``t@1500m``, ``z@-10C``,
``u@320K``, ``ws@875hPa``) into these ops is ``derived.plan``; ``derived.LeadDeriver`` launches them after the derive and thermo ops into
the same buffer.  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass

import numpy as np

from . import native, program
from .thermo import sk_exp, sk_log

MAX_MEMBERS, MAX_OPS, MAX_LEVELS, MAX_TARGETS, MAX_FIELDS = 64, 16, 16, 4, 8      # include/skyrim_vert.h SKVERT_MAX_*
P, Z, Z_AGL, THETA, T = 1, 2, 3, 4, 5                           # SKVERT_P ...: the coordinate
PLAIN, SPEED, THETA_F, PRESSURE = 1, 2, 3, 4                    # SKVERT_PLAIN ...: the field
NAN, NEAREST = 0, 1                                             # SKVERT_NAN, SKVERT_NEAREST
NODE_NONE, NODE_ZS = -1, -2                                     # SKVERT_NODE_*
GRAVITY = 9.80665
KAPPA = "0.2854"
_P = ctypes.c_void_p


class FieldDesc(ctypes.Structure):
    """skvert_field."""
    _fields_ = [("kind", ctypes.c_int32), ("in_a", ctypes.c_int32 * MAX_LEVELS), ("in_b", ctypes.c_int32 * MAX_LEVELS),
                ("node_a", ctypes.c_int32), ("node_b", ctypes.c_int32), ("gh", ctypes.c_float), ("out", ctypes.c_int32 * MAX_TARGETS)]


class OpDesc(ctypes.Structure):
    """skvert_op."""
    _fields_ = [("coord", ctypes.c_int32), ("n_levels", ctypes.c_int32), ("n_targets", ctypes.c_int32), ("n_fields", ctypes.c_int32),
                ("outside", ctypes.c_int32), ("mask", ctypes.c_int32), ("in_c", ctypes.c_int32 * MAX_LEVELS),
                ("in_z", ctypes.c_int32 * MAX_LEVELS), ("p", ctypes.c_float * MAX_LEVELS), ("target", ctypes.c_float * MAX_TARGETS),
                ("fields", FieldDesc * MAX_FIELDS)]


class VertDesc(ctypes.Structure):
    """skvert_desc."""
    _fields_ = [("members", _P), ("M", ctypes.c_int), ("member_align", ctypes.c_int), ("C", ctypes.c_int), ("H", ctypes.c_int),
                ("W", ctypes.c_int), ("D", ctypes.c_int), ("out", _P), ("member_stride", ctypes.c_size_t), ("zs", _P),
                ("n_ops", ctypes.c_int), ("ops", OpDesc * MAX_OPS)]


SPEC = native.Spec("skyrim_vert", "SKYRIM_VERT_LIB", "skvert", 1, {             # include/skyrim_vert.h SKVERT_ABI_VERSION
    "skvert_abi_version": (ctypes.c_int, []),
    "skvert_run": (ctypes.c_int, [ctypes.POINTER(VertDesc), _P]),
}, " -- vertical interpolation has no torch fallback")
EXPORTS, ABI_VERSION = SPEC.exports, SPEC.abi

_lib = None


def load_library() -> ctypes.CDLL:
    """libskyrim_vert.so (built in-tree by ``__graft_entry__.build()`` / ``make -C skyrim_amd/csrc``)."""
    global _lib
    if _lib is None:
        _lib = native.load(SPEC)
    return _lib


# ---- the host constants, made with thermo.py's fp32 sk_exp / sk_log ---------------------------------------------------------------------- #
def level_constants(pressures) -> tuple:
    """(lnp_k, ex_k) of the header for pressure levels in hPa: fp32 arrays"""
    lnp = sk_log(np.asarray(pressures, np.float32))
    return lnp, sk_exp(np.float32(KAPPA) * (sk_log(np.float32(1000)) - lnp))


def target_value(coord: int, value: float) -> float:
    """The fp32 target of the header for a user's value: hPa -> sk_log(P); metres -> g Z; K as it is; for T the value is degrees Celsius
    and the target fp32(273.15 + C), the sum made in float64."""
    if coord == P:
        return float(sk_log(np.float32(value)))
    if coord in (Z, Z_AGL):
        return float(np.float32(GRAVITY * float(value)))
    if coord == T:
        return float(np.float32(273.15 + float(value)))
    return float(np.float32(value))


# ---- the program ------------------------------------------------------------------------------------------------------------------------- #
@dataclass(frozen=True)
class Field:
    """One field of an op.  ``a``: the channels of f_k (PLAIN), u_k (SPEED) or t_k (THETA_F), () for PRESSURE; ``b``: v_k of SPEED;
    ``outputs``: one slot per target of the op, -1 = not computed; ``node``: (node_a, node_b) of the surface node -- channel indices,
    ``NODE_ZS`` or ``NODE_NONE`` -- and ``gh`` its height as geopotential."""
    kind: int
    a: tuple
    b: tuple
    outputs: tuple
    node: tuple = (NODE_NONE, NODE_NONE)
    gh: float = 0.0


@dataclass(frozen=True)
class Op:
    """One op of a program: the coordinate ``coord`` over the levels ``pressures`` (hPa, bottom-up), read from the channels ``c`` (none
    for P), masked with the channels ``z`` (THETA, T, and P with ``mask``) when a surface is given; ``targets``: the header's fp32 targets
    (``target_value``); ``fields``: ``Field``s; ``outside``: NAN or NEAREST."""
    coord: int
    pressures: tuple
    c: tuple
    z: tuple
    targets: tuple
    fields: tuple
    outside: int = NAN
    mask: int = 0


def encode(ops) -> tuple:
    """(ints, floats): the flat form ``torch.ops.skyrim_hip.vert_fields`` takes.  Per op: coord, L, T, F, outside, mask, the counts of c
    and z, then the c and z channels, then per field: kind, the counts of a and b, node_a, node_b, T slots, the a and b channels; the floats
    are the pressures, the targets and every field's gh, op after op."""
    ints, floats = [], []
    for op in ops:
        ints += [int(op.coord), len(op.pressures), len(op.targets), len(op.fields), int(op.outside), int(op.mask), len(op.c), len(op.z)]
        ints += [int(x) for x in tuple(op.c) + tuple(op.z)]
        floats += [float(p) for p in op.pressures] + [float(t) for t in op.targets]
        for fd in op.fields:
            slots = list(fd.outputs) + [-1] * (len(op.targets) - len(fd.outputs))
            ints += [int(fd.kind), len(fd.a), len(fd.b), int(fd.node[0]), int(fd.node[1])] + [int(s) for s in slots[:len(op.targets)]]
            ints += [int(x) for x in tuple(fd.a) + tuple(fd.b)]
            floats.append(float(fd.gh))
    return ints, floats


def decode(ints, floats) -> list:
    ops, i, f = [], 0, 0
    ints, floats = list(ints), list(floats)
    end = ValueError("vert_fields: the program ends inside an op")
    while i < len(ints):
        if i + 8 > len(ints):
            raise end
        coord, L, nt, nf, outside, mask, nc, nz = ints[i:i + 8]
        i += 8
        if coord not in (P, Z, Z_AGL, THETA, T):
            raise ValueError(f"vert_fields: unknown coordinate kind {coord}")
        if min(L, nt, nf, nc, nz) < 0 or i + nc + nz > len(ints) or f + L + nt > len(floats):
            raise end
        c, z = tuple(ints[i:i + nc]), tuple(ints[i + nc:i + nc + nz])
        i += nc + nz
        pressures, targets = tuple(floats[f:f + L]), tuple(floats[f + L:f + L + nt])
        f += L + nt
        fields = []
        for _ in range(nf):
            if i + 5 + nt > len(ints) or f + 1 > len(floats):
                raise end
            kind, na, nb, node_a, node_b = ints[i:i + 5]
            slots = tuple(ints[i + 5:i + 5 + nt])
            i += 5 + nt
            if kind not in (PLAIN, SPEED, THETA_F, PRESSURE):
                raise ValueError(f"vert_fields: unknown field kind {kind}")
            if min(na, nb) < 0 or i + na + nb > len(ints):
                raise end
            fields.append(Field(kind, tuple(ints[i:i + na]), tuple(ints[i + na:i + na + nb]), slots, (node_a, node_b), floats[f]))
            i += na + nb
            f += 1
        ops.append(Op(coord, pressures, c, z, targets, tuple(fields), outside, mask))
    return ops


def describe(ops, M, C, H, W, D, member_stride, member_align=16) -> VertDesc:
    """The descriptor of a program, its pointers still NULL.  What does not fit the descriptor's arrays is cut; the counts say what was
    asked for, so the library refuses it."""
    d = VertDesc()
    program.fill_head(d, M, C, H, W, D, member_stride, member_align)
    ops = list(ops)
    d.n_ops = len(ops)
    for k, op in enumerate(ops[:MAX_OPS]):
        o = d.ops[k]
        o.coord, o.n_levels, o.n_targets, o.n_fields, o.outside, o.mask = op.coord, len(op.pressures), len(op.targets), len(op.fields), op.outside, op.mask
        for dst, src, cap in ((o.in_c, op.c, MAX_LEVELS), (o.in_z, op.z, MAX_LEVELS), (o.p, op.pressures, MAX_LEVELS), (o.target, op.targets, MAX_TARGETS)):
            for l, v in enumerate(tuple(src)[:cap]):
                dst[l] = v
        for j in range(MAX_FIELDS):
            o.fields[j].node_a = o.fields[j].node_b = NODE_NONE
            for t in range(MAX_TARGETS):
                o.fields[j].out[t] = -1
        for j, fd in enumerate(tuple(op.fields)[:MAX_FIELDS]):
            g = o.fields[j]
            g.kind, g.node_a, g.node_b, g.gh = fd.kind, fd.node[0], fd.node[1], fd.gh
            for dst, src in ((g.in_a, fd.a), (g.in_b, fd.b)):
                for l, v in enumerate(tuple(src)[:MAX_LEVELS]):
                    dst[l] = v
            for t, s in enumerate(tuple(fd.outputs)[:MAX_TARGETS]):
                g.out[t] = int(s)
    return d


def _shape_error(op, surface: bool):
    """What is wrong with the lengths of an op's tuples, or None"""
    L = len(op.pressures)
    if not 2 <= L <= MAX_LEVELS:
        return f"an op has 2 to {MAX_LEVELS} levels"
    if not 1 <= len(op.targets) <= MAX_TARGETS or not 1 <= len(op.fields) <= MAX_FIELDS:
        return f"an op has 1 to {MAX_TARGETS} targets and 1 to {MAX_FIELDS} fields"
    if len(op.c) != (0 if op.coord == P else L):
        return "an op names one coordinate channel per level (none for P)"
    needs_z = (op.coord in (THETA, T) and surface) or (op.coord == P and op.mask)
    if needs_z and len(op.z) != L:
        return "with a surface, a THETA or T op (and a P op that masks) names one z channel per level"
    if op.coord == Z_AGL and not surface:
        return "a Z_AGL op needs the surface geopotential"
    for fd in op.fields:
        if len(fd.a) != (0 if fd.kind == PRESSURE else L) or len(fd.b) != (L if fd.kind == SPEED else 0):
            return "a field names one channel per level (SPEED: u and v; PRESSURE: none)"
        if len(fd.outputs) != len(op.targets):
            return "a field has one slot per target"
    return None


def run(members, table, ops, out, surface=None) -> None:
    """One ``skvert_run``: the program ``ops`` on the M ``members`` (equal-shaped contiguous float32 (C, H, W) device tensors;
    ``table`` = ``members.member_table(members)``) into ``out``, float32 (M, D, H, W).  ``surface``: float32 (H, W) on the device, the
    surface geopotential of Z_AGL and of the mask, or None.  Queued on torch's current stream.  As in ``thermo.run``, the contents of
    ``table`` are trusted to be the addresses of ``members``."""
    import torch
    ops = list(ops)
    M, dev, align, C, H, W, D, po = program.bind("vert_fields", members, table, ops, out, "vert_fields: out", MAX_MEMBERS, MAX_OPS)
    for op in ops:
        err = _shape_error(op, surface is not None)
        if err:
            raise ValueError(f"vert_fields: {err}")
    d = describe(ops, M, C, H, W, D, D * H * W, align)
    d.members, d.out = table.data_ptr(), po
    if surface is not None:
        d.zs = program.plane("vert_fields", surface, "surface", (H, W), torch.float32, dev)
    lib = load_library()
    program.launch(lib, lib.skvert_run, d, dev)
