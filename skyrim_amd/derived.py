"""Derived fields on the device (include/skyrim_derive.h): wind speed, thickness, integrated vapour transport, vorticity
and divergence of forecast states, made where the states lie in HBM as D compact channels per member, so that the ensemble statistics
and the scorer read them like raw channels.

Layers:

* the binding of libskyrim_derive.so (``SPEC``, ``load_library``, ``run``); the same call is ``torch.ops.skyrim_hip.derive_fields``.
  Derivation has no CPU fallback;
* the catalogue: ``plan`` resolves user-facing names (``ws10m``, ``thk500_1000``, ``vo850``, ``div850``, ``ivt`` ...) against a model's
  channels into a program of ops, ``row_table`` makes the row coefficients of vorticity and divergence in float64.  The names of column
  thermodynamics (``td850``, ``thetae850``, ``kx``, ``zdeg0``, ``mucape`` ...: DESIGN.md 30) resolve into ops of libskyrim_thermo.so
  (skyrim_amd/thermo.py), which write into the same buffer; a request that names none of them never loads that library.  The names
  ``<field>@<surface>`` (``ws@100magl``, ``t@1500m``, ``z@-10C``, ``u@320K``, ``ws@875hPa``: DESIGN.md 34) resolve into ops of
  libskyrim_vert.so (skyrim_amd/vertical.py) in the same way;
* the drivers: ``LeadDeriver`` (what ``ensemble.run`` calls at every lead time with ``derived=[...]``), ``TruthDeriver`` (the hook that
  lets ``verify.LeadScorer`` score derived fields against a truth of raw channels), ``derive_model`` (``GlobalModel.derive_fields``)
  and ``derive_prediction`` for forecasts that are already on disk.
"""
from __future__ import annotations

import ctypes
import datetime
import re
from dataclasses import dataclass, field

import numpy as np

from . import native, program
from .common import world_size as _world_size
from .leads import open_saved, require_gpu, run_model

MAX_MEMBERS, MAX_OPS, MAX_LEVELS = 64, 16, 16                   # include/skyrim_derive.h SKDERIVE_MAX_*
SPEED, DIFF, COLUMN, VORTDIV = 1, 2, 3, 4                       # SKDERIVE_SPEED ...
EDGE_ONESIDED, EDGE_POLE = 1, 2                                 # SKDERIVE_EDGE_*
RESULTS = {SPEED: 1, DIFF: 1, COLUMN: 4, VORTDIV: 2}            # output slots of an op
EARTH_RADIUS_M = 6371000.0
GRAVITY = 9.80665
COLUMN_FIELDS = ("ivtu", "ivtv", "ivt", "iwv")                  # in the order of a COLUMN op's slots
_P = ctypes.c_void_p


class OpDesc(ctypes.Structure):
    """skderive_op."""
    _fields_ = [("kind", ctypes.c_int32), ("n_levels", ctypes.c_int32), ("in_a", ctypes.c_int32 * MAX_LEVELS),
                ("in_b", ctypes.c_int32 * MAX_LEVELS), ("in_c", ctypes.c_int32 * MAX_LEVELS), ("weight", ctypes.c_float * MAX_LEVELS),
                ("out", ctypes.c_int32 * 4)]


class DeriveDesc(ctypes.Structure):
    """skderive_desc."""
    _fields_ = [("members", _P), ("M", ctypes.c_int), ("member_align", ctypes.c_int), ("C", ctypes.c_int), ("H", ctypes.c_int),
                ("W", ctypes.c_int), ("D", ctypes.c_int), ("out", _P), ("member_stride", ctypes.c_size_t), ("rowc", _P),
                ("edge_first", ctypes.c_int), ("edge_last", ctypes.c_int), ("n_ops", ctypes.c_int), ("ops", OpDesc * MAX_OPS)]


SPEC = native.Spec("skyrim_derive", "SKYRIM_DERIVE_LIB", "skderive", 1, {       # include/skyrim_derive.h SKDERIVE_ABI_VERSION
    "skderive_abi_version": (ctypes.c_int, []),
    "skderive_run": (ctypes.c_int, [ctypes.POINTER(DeriveDesc), _P]),
}, " -- derived fields have no torch fallback")
EXPORTS, ABI_VERSION = SPEC.exports, SPEC.abi

_lib = None


def load_library() -> ctypes.CDLL:
    """libskyrim_derive.so (built in-tree by ``__graft_entry__.build()`` / ``make -C skyrim_amd/csrc``)."""
    global _lib
    if _lib is None:
        _lib = native.load(SPEC)
    return _lib


# ---- the program ------------------------------------------------------------------------------------------------------------------------- #
@dataclass(frozen=True)
class Op:
    """One op of a program.  ``inputs``: (u, v) for SPEED and VORTDIV, (a, b) for DIFF, (q levels, u levels, v levels) for COLUMN --
    channel indices; ``outputs``: one slot per result (``RESULTS``), -1 = not computed; ``weights``: the fp32 level weights of COLUMN."""
    kind: int
    inputs: tuple
    outputs: tuple
    weights: tuple = ()


def encode(ops) -> tuple:
    """(ints, floats): the flat form ``torch.ops.skyrim_hip.derive_fields`` takes.  Per op: kind, L, four slots, then the inputs (two
    channels, or 3 L for COLUMN: q, u, v); the floats are the COLUMN weights, op after op."""
    ints, floats = [], []
    for op in ops:
        column = op.kind == COLUMN
        L = len(op.inputs[0]) if column else 0
        slots = list(op.outputs) + [-1] * (4 - len(op.outputs))
        ints += [int(op.kind), L] + [int(s) for s in slots]
        ints += [int(c) for level in op.inputs for c in level] if column else [int(op.inputs[0]), int(op.inputs[1])]
        floats += [float(w) for w in op.weights]
    return ints, floats


def decode(ints, floats) -> list:
    ops, i, f = [], 0, 0
    ints, floats = list(ints), list(floats)
    while i < len(ints):
        if i + 6 > len(ints):
            raise ValueError("derive_fields: the program ends inside an op")
        kind, L, slots = ints[i], ints[i + 1], ints[i + 2:i + 6]
        i += 6
        if kind not in RESULTS:
            raise ValueError(f"derive_fields: unknown op kind {kind}")
        n = 3 * L if kind == COLUMN else 2
        if i + n > len(ints) or (kind == COLUMN and f + L > len(floats)):
            raise ValueError("derive_fields: the program ends inside an op")
        if kind == COLUMN:
            ops.append(Op(kind, (tuple(ints[i:i + L]), tuple(ints[i + L:i + 2 * L]), tuple(ints[i + 2 * L:i + 3 * L])), tuple(slots),
                          tuple(floats[f:f + L])))
            f += L
        else:
            ops.append(Op(kind, (ints[i], ints[i + 1]), tuple(slots[:RESULTS[kind]])))
        i += n
    return ops


def describe(ops, M, C, H, W, D, member_stride, member_align=16, edges=(EDGE_POLE, EDGE_POLE)) -> DeriveDesc:
    """The descriptor of a program, its pointers still NULL."""
    d = DeriveDesc()
    program.fill_head(d, M, C, H, W, D, member_stride, member_align)
    d.edge_first, d.edge_last = int(edges[0]), int(edges[1])
    ops = list(ops)
    d.n_ops = len(ops)
    for k, op in enumerate(ops[:MAX_OPS]):
        o = d.ops[k]
        o.kind = op.kind
        for r in range(4):
            o.out[r] = int(op.outputs[r]) if r < len(op.outputs) else -1
        if op.kind == COLUMN:
            q, u, v = op.inputs
            o.n_levels = len(q)
            for l in range(min(len(q), MAX_LEVELS)):
                o.in_a[l], o.in_b[l], o.in_c[l], o.weight[l] = q[l], u[l], v[l], op.weights[l]
        else:
            o.in_a[0], o.in_b[0] = op.inputs
    return d


def run(members, table, ops, out, rowc=None, edges=(EDGE_POLE, EDGE_POLE)) -> None:
    """One ``skderive_run``: the program ``ops`` on the M ``members`` (equal-shaped contiguous float32 (C, H, W) device tensors;
    ``table`` = ``ensemble.member_table(members)``) into ``out``, float32 (M, D, H, W).  ``rowc``: float32 (H, 4) on the device and
    ``edges`` = (edge_first, edge_last), needed with a VORTDIV op (``row_table``).  Queued on torch's current stream.  As in
    ``verify.score``, the contents of ``table`` are trusted to be the addresses of ``members``."""
    import torch
    ops = list(ops)
    M, dev, align, C, H, W, D, po = program.bind("derive_fields", members, table, ops, out, "derive_fields: out", MAX_MEMBERS, MAX_OPS)
    for op in ops:
        if op.kind == COLUMN and (len(set(len(x) for x in op.inputs)) != 1 or len(op.weights) != len(op.inputs[0])
                                  or not 2 <= len(op.weights) <= MAX_LEVELS):
            raise ValueError(f"derive_fields: a COLUMN op has 2 to {MAX_LEVELS} levels, each with q, u, v and a weight")
        if len(op.outputs) != RESULTS.get(op.kind, 0):
            raise ValueError("derive_fields: an op has one slot per result (SPEED, DIFF: 1; VORTDIV: 2; COLUMN: 4)")
    d = describe(ops, M, C, H, W, D, D * H * W, align, edges)
    d.members, d.out = table.data_ptr(), po
    if any(op.kind == VORTDIV for op in ops):
        if rowc is None or tuple(rowc.shape) != (H, 4):
            raise ValueError(f"derive_fields: vorticity and divergence need rowc ({H}, 4)")
        d.rowc = native.tensor_ptr(rowc, "derive_fields: rowc", torch.float32, dev)
    lib = load_library()
    program.launch(lib, lib.skderive_run, d, dev)


# ---- the row coefficients of vorticity and divergence ------------------------------------------------------------------------------------- #
def _uniform_lon(lon) -> float:
    from .tracks import _uniform_lon as check
    if len(lon) < 4:
        raise ValueError("vorticity and divergence need a periodic longitude axis of at least 4 points")
    return check(lon)


_row_cache: dict = {}


def row_table(lat, lon) -> tuple:
    """(rowc float32 (H, 4), edge_first, edge_last) of include/skyrim_derive.h, made in float64 and rounded once; cached per grid.
    Interior rows: A, B+, B-, sgn(lat) as ``tracks.row_coefficients``.  A first or last row at +-90 degrees is a pole row: its entry is
    (f, -f, 0, 0) with f = +-cos(lat_r) / (a (1 - |sin(lat_r)|)) of the neighbouring row r, + at the north pole; any other first or last
    row is one-sided: the same A, and B+- over the latitude step between the row and its one neighbour."""
    lat, lon = np.asarray(lat, np.float64), np.asarray(lon, np.float64)
    key = (lat.tobytes(), lon.tobytes())
    hit = _row_cache.get(key)
    if hit is not None:
        return hit
    H = lat.size
    step = np.diff(lat)
    if H < 3 or not (np.all(step > 0) or np.all(step < 0)) or np.any(np.abs(lat) > 90):
        raise ValueError("vorticity and divergence need a strictly monotonic latitude axis in degrees of at least 3 rows")
    dlam = _uniform_lon(lon)
    phi = np.radians(lat)
    a = EARTH_RADIUS_M
    rowc = np.zeros((H, 4), np.float64)
    edges = []
    for j in range(H):
        jn, js = min(j + 1, H - 1), max(j - 1, 0)
        if j in (0, H - 1) and abs(abs(lat[j]) - 90.0) < 1e-9:
            r = 1 if j == 0 else H - 2
            f = np.sign(lat[j]) * np.cos(phi[r]) / (a * (1.0 - abs(np.sin(phi[r]))))
            rowc[j] = (f, -f, 0.0, 0.0)
            edges.append(EDGE_POLE)
            continue
        if j in (0, H - 1):
            edges.append(EDGE_ONESIDED)
        c, dphi = np.cos(phi[j]), phi[jn] - phi[js]
        rowc[j] = (1.0 / (2 * a * c * dlam), np.cos(phi[jn]) / (a * c * dphi), np.cos(phi[js]) / (a * c * dphi), np.sign(phi[j]))
    hit = (rowc.astype(np.float32), edges[0], edges[1])
    _row_cache[key] = hit
    return hit


# ---- the catalogue ----------------------------------------------------------------------------------------------------------------------- #
@dataclass
class Plan:
    """A resolved request.  ``fields``: the derived names, slot d = fields[d]; ``ops``: the program; ``inputs[name]``: the raw channels a
    derived field reads; ``rowc / edges``: the row table when vorticity or divergence is asked for; ``levels / weights``: the pressure
    levels (hPa) and float64 trapezoid weights of the column integrals, when asked for.  ``thermo_ops``: the program of
    libskyrim_thermo.so (``thermo.Op``), whose slots are numbered with those of ``ops``; ``moisture``: "q" or "r", what they read;
    ``column``: {"parcel" / "freeze" / "vert": the pressure levels (hPa, bottom-up) of their columns}.  ``vert_ops``: the program of
    libskyrim_vert.so (``vertical.Op``) for the names ``<field>@<surface>``, its slots numbered with the others."""
    fields: list
    ops: list
    inputs: dict
    rowc: object = None
    edges: tuple = (EDGE_POLE, EDGE_POLE)
    levels: list = field(default_factory=list)
    weights: object = None
    thermo_ops: list = field(default_factory=list)
    moisture: str | None = None
    column: dict = field(default_factory=dict)
    vert_ops: list = field(default_factory=list)


def column_weights(levels) -> np.ndarray:
    """Float64 trapezoid weights w_k = 100 dp_k / g of pressure levels in hPa (ascending): half the distance to both neighbours, half an
    interval at the ends."""
    p = np.asarray(levels, np.float64)
    dp = np.empty_like(p)
    dp[0], dp[-1] = (p[1] - p[0]) / 2, (p[-1] - p[-2]) / 2
    dp[1:-1] = (p[2:] - p[:-2]) / 2
    return 100.0 * dp / GRAVITY


def _height(tag: str) -> bool:
    return tag in ("10m", "100m") or tag.isdigit()


def _parse(name: str):
    """(kind, raw channel names it reads or None for COLUMN, slot within the op) of a derived name; None when it is not one."""
    if name in COLUMN_FIELDS:
        return COLUMN, None, COLUMN_FIELDS.index(name)
    m = re.fullmatch(r"ws(\d+m?)", name)
    if m and _height(m.group(1)):
        return SPEED, (f"u{m.group(1)}", f"v{m.group(1)}"), 0
    m = re.fullmatch(r"thk(\d+)_(\d+)", name)
    if m:
        return DIFF, (f"z{m.group(1)}", f"z{m.group(2)}"), 0
    m = re.fullmatch(r"(vo|div)(\d+m?)", name)
    if m and _height(m.group(2)):
        return VORTDIV, (f"u{m.group(2)}", f"v{m.group(2)}"), 0 if m.group(1) == "vo" else 1
    return None


MOIST_FIELDS = ("td", "rh", "thetae", "theta")                 # in the order of a MOIST op's slots; slot 1 is ``q<level>`` for a model with r
INDEX_FIELDS = ("kx", "tt")
PARCEL_FIELDS = {"sbcape": (0, 0), "sbli": (0, 1), "mucape": (1, 0), "muli": (1, 1), "mucape_src": (1, 2)}      # (thermo.SRC_*, slot)
THERMO_KNOWN = "td<level>, rh<level> (q<level> for a model with r), thetae<level>, theta<level>, kx, tt, zdeg0, sbcape, sbli, mucape, muli, mucape_src"


def _parse_thermo(name: str):
    """(op, key, slot) of a name of column thermodynamics -- op one of "moist", "index", "freeze", "parcel"; key the level (moist) or
    the source (parcel) -- or None."""
    if name in INDEX_FIELDS:
        return "index", None, INDEX_FIELDS.index(name)
    if name == "zdeg0":
        return "freeze", None, 0
    if name in PARCEL_FIELDS:
        return ("parcel",) + PARCEL_FIELDS[name]
    m = re.fullmatch(r"(td|rh|q|thetae|theta)(\d+)", name)
    if m:
        return "moist", int(m.group(2)), 1 if m.group(1) == "q" else MOIST_FIELDS.index(m.group(1))
    return None


def moisture_of(names):
    """"q" when the channels hold specific humidity on a level, else "r" (relative humidity), else None"""
    for letter in "qr":
        if any(re.fullmatch(letter + r"\d+", n) for n in names):
            return letter
    return None


def thermo_levels(names, letters, what: str, given=None, lo: int = 2) -> list:
    """The pressure levels (hPa, descending: bottom-up) at which ``names`` holds every channel ``<letter><level>`` of ``letters``, or
    ``given`` (then every channel must be there)."""
    names = set(names)
    if given is not None:
        use = sorted((int(l) for l in given), reverse=True)
        missing = [f"{x}{l}" for l in use for x in letters if f"{x}{l}" not in names]
        if missing:
            raise ValueError(f"derived: {what} needs the channels {missing}, which this model lacks")
    else:
        have = sorted((int(n[1:]) for n in names if re.fullmatch(letters[0] + r"\d+", n)), reverse=True)
        use = [l for l in have if all(f"{x}{l}" in names for x in letters)]
    if not lo <= len(use) <= MAX_LEVELS:
        raise ValueError(f"derived: {what} runs over {lo} to {MAX_LEVELS} levels with the channels "
                         f"{', '.join(x + '<level>' for x in letters)}; this model has {len(use)}")
    return use


def _thermo_raw(op: str, key, slot: int, moisture, surface: bool, levels) -> list:
    """The raw channel names a thermo field reads, given the levels of its column (None for the fields of fixed levels)"""
    if op == "moist":
        return [f"t{key}"] + ([] if slot == 3 else [f"{moisture}{key}"])
    if op == "index":
        return ["t850", "t700", "t500", f"{moisture}850", f"{moisture}700"]
    letters = "tz" if op == "freeze" else "t" + moisture + ("z" if surface else "")
    return [f"{x}{l}" for x in letters for l in levels]


def thermo_inputs(name: str, names, moisture, surface: bool, column=None):
    """(raw channel names a thermo field reads, the levels of its column or None); every refusal of such a name is a ValueError here."""
    op, key, slot = _parse_thermo(name)
    names = list(names)
    wet = not (op == "moist" and slot == 3) and op != "freeze"
    if wet and moisture is None:
        raise ValueError(f"derived: {name!r} needs humidity: this model has neither specific humidity (q<level>) nor relative humidity "
                         "(r<level>) among its channels")
    levels = None
    if op == "moist" and name.startswith("rh") and moisture == "r":
        raise ValueError(f"derived: {name!r}: this model carries relative humidity itself (r{key}); q{key} is what can be derived")
    if op == "freeze":
        levels = thermo_levels(names, "tz", repr(name), (column or {}).get("freeze"))
    elif op == "parcel":
        levels = thermo_levels(names, "t" + moisture + ("z" if surface else ""), repr(name), (column or {}).get("parcel"))
        if slot == 1 and 500 not in levels:
            raise ValueError(f"derived: {name!r} is the parcel's temperature against the environment's at 500 hPa: the column {levels} has no such level")
    raw = _thermo_raw(op, key, slot, moisture, surface, levels)
    missing = [c for c in raw if c not in names]
    if missing:
        raise ValueError(f"derived: {name!r} needs the channel{'s' if len(missing) > 1 else ''} "
                         f"{', '.join(repr(c) for c in missing)}, which this model lacks")
    return raw, levels


def _thermo_plan(out: Plan, names, requests, surface: bool, column) -> None:
    """The thermo ops of ``requests`` = [(slot, name)]: the four fields of a level share a MOIST op, kx and tt the INDEX op, the fields of
    one source a PARCEL op."""
    from . import thermo
    names = list(names)
    ch = names.index
    out.moisture = moisture_of(names)
    kind = thermo.R if out.moisture == "r" else thermo.Q
    merged = {}
    for slot, name in requests:
        op, key, result = _parse_thermo(name)
        raw, levels = thermo_inputs(name, names, out.moisture, surface, column)
        out.inputs[name] = raw
        if levels is not None:
            out.column.setdefault(op, levels)
        if (op, key) not in merged:
            merged[(op, key)] = len(out.thermo_ops)
            if op == "moist":
                m = f"{out.moisture}{key}"
                new = thermo.Op(thermo.MOIST, (ch(f"t{key}"),), (ch(m),) if m in names else (), (), (-1,) * 4, kind, (float(key),))
            elif op == "index":
                new = thermo.Op(thermo.INDEX, tuple(ch(c) for c in raw[:3]), tuple(ch(c) for c in raw[3:]), (), (-1,) * 2, kind)
            elif op == "freeze":
                new = thermo.Op(thermo.FREEZE, tuple(ch(f"t{l}") for l in levels), (), tuple(ch(f"z{l}") for l in levels), (-1,))
            else:
                new = thermo.Op(thermo.PARCEL, tuple(ch(f"t{l}") for l in levels), tuple(ch(f"{out.moisture}{l}") for l in levels),
                                tuple(ch(f"z{l}") for l in levels) if surface else (), (-1,) * 3, kind, tuple(float(l) for l in levels), key)
            out.thermo_ops.append(new)
        k = merged[(op, key)]
        old = out.thermo_ops[k]
        slots = list(old.outputs)
        slots[result] = slot
        out.thermo_ops[k] = thermo.Op(old.kind, old.t, old.m, old.z, tuple(slots), old.moisture, old.pressures, old.source, old.p_src_min, old.p_top)
    if len(out.thermo_ops) > thermo.MAX_OPS:
        raise ValueError(f"derived: {len(out.thermo_ops)} thermodynamic ops for {[n for _, n in requests]}; one call holds {thermo.MAX_OPS}")


# ---- fields on chosen surfaces --------------------------------------------------------------------------------------------- #
VERT_LEVEL_FIELDS = ("z", "q", "r", "t", "u", "v")             # a level variable the model carries
VERT_KNOWN = ("<field>@<surface> (field: z, q, r, t, u, v, ws, theta or p; surface: <P>hPa, <Z>m above sea level, <Z>magl above the ground, "
              "<theta>K or <T>C)")
_VERT_NAME = re.compile(r"(z|q|r|t|u|v|ws|theta|p)@(-?\d+(?:\.\d+)?)(hPa|magl|m|K|C)")
_VERT_UNITS = {"hPa": "P", "m": "Z", "magl": "Z_AGL", "K": "THETA", "C": "T"}
NODE_HEIGHT_M = {"u10m": 10.0, "v10m": 10.0, "t2m": 2.0}       # the surface channels that serve as the node of a column above the ground


def _parse_vert(name: str):
    """(field, coordinate kind as the name of ``vertical``'s constant, value in the surface's own unit) of ``<field>@<surface>``, or None"""
    m = _VERT_NAME.fullmatch(name)
    if not m:
        return None
    return m.group(1), _VERT_UNITS[m.group(3)], float(m.group(2))


def vertical_options(vertical) -> int:
    """``vertical={"outside": "nan" | "nearest"}`` -> ``vertical.NAN`` / ``vertical.NEAREST``"""
    from . import vertical as V
    opts = dict(vertical or {})
    unknown = [k for k in opts if k != "outside"]
    if unknown:
        raise ValueError(f"vertical: unknown keys {unknown}; it takes \"outside\"")
    outside = opts.get("outside", "nan")
    if outside not in ("nan", "nearest"):
        raise ValueError(f"vertical: outside is \"nan\" or \"nearest\", not {outside!r}")
    return V.NEAREST if outside == "nearest" else V.NAN


def vert_inputs(name: str, names, surface: bool, column=None) -> dict:
    """What ``<field>@<surface>`` reads, every refusal of such a name a ValueError: dict(field, coord, value, levels, c, z, a, b, node,
    raw) -- the channel NAMES of the coordinate, the mask, the field's components and its surface node, and all of them in ``raw``."""
    fld, coord, value = _parse_vert(name)
    names = list(names)
    if fld == "p" and coord == "P":
        raise ValueError(f"derived: {name!r} is the pressure on a pressure surface: the constant {value:g} hPa")
    if (fld, coord) in (("theta", "THETA"), ("t", "T")):
        raise ValueError(f"derived: {name!r} is {'theta on an isentrope' if fld == 'theta' else 't on an isotherm'}: a constant")
    if coord in ("Z", "Z_AGL", "THETA") and not value > 0:
        raise ValueError(f"derived: {name!r}: a {'potential temperature' if coord == 'THETA' else 'height'} must be positive")
    if coord == "Z_AGL" and not surface:
        raise ValueError(f"derived: {name!r} is a height above the ground: it needs the surface geopotential, derived_surface=")
    letters = {"ws": "uv", "theta": "t", "p": ""}.get(fld, fld)
    coord_letters = {"P": "", "Z": "z", "Z_AGL": "z", "THETA": "t", "T": "t"}[coord]
    mask_letters = "z" if surface and coord in ("THETA", "T") else ""
    for x in letters:
        if not any(re.fullmatch(x + r"\d+", n) for n in names):
            raise ValueError(f"derived: {name!r} needs the level variable {x!r} ({x}<level>), which this model lacks")
    need = "".join(dict.fromkeys(coord_letters + mask_letters + letters))
    levels = thermo_levels(names, need, repr(name), (column or {}).get("vert"))
    if coord == "P" and not levels[-1] <= value <= levels[0]:
        raise ValueError(f"derived: {name!r}: {value:g} hPa lies outside the column {levels[0]} .. {levels[-1]} hPa of this model")
    on = lambda x: [f"{x}{l}" for l in levels]                  # noqa: E731
    node = []
    if coord == "Z_AGL":
        if fld in ("u", "v") and f"{fld}10m" in names:
            node = [f"{fld}10m"]
        elif fld == "ws" and "u10m" in names and "v10m" in names:
            node = ["u10m", "v10m"]
        elif fld == "t" and "t2m" in names:
            node = ["t2m"]
        elif fld == "z":
            node = ["zs"]
    out = dict(field=fld, coord=coord, value=value, levels=levels, c=on(coord_letters) if coord_letters else [],
               z=on("z") if mask_letters else [], a=on(letters[0]) if letters else [], b=on("v") if fld == "ws" else [], node=node)
    out["raw"] = list(dict.fromkeys(out["c"] + out["z"] + out["a"] + out["b"] + [c for c in node if c != "zs"]))
    return out


def _vert_plan(out: Plan, names, requests, surface: bool, column, outside: int) -> None:
    """The vert ops of ``requests`` = [(slot, name)]: fields on the same coordinate kind and column share an op, up to the targets and
    fields one op holds; beyond them they go to further ops."""
    from . import vertical as V
    names = list(names)
    ch = names.index
    groups = []                                                 # dict(key, coord, levels, c, z, targets: [fp32], fields: {field key: [Field parts, {target: slot}]})
    for slot, name in requests:
        r = vert_inputs(name, names, surface, column)
        out.inputs[name] = r["raw"]
        out.column.setdefault("vert", r["levels"])
        coord = getattr(V, r["coord"])
        target = V.target_value(coord, r["value"])
        key = (coord, tuple(r["levels"]))
        kind = {"ws": V.SPEED, "theta": V.THETA_F, "p": V.PRESSURE}.get(r["field"], V.PLAIN)
        g = None
        for cand in groups:
            if cand["key"] != key:
                continue
            if (target in cand["targets"] or len(cand["targets"]) < V.MAX_TARGETS) and (r["field"] in cand["fields"] or len(cand["fields"]) < V.MAX_FIELDS):
                g = cand
                break
        if g is None:
            g = dict(key=key, coord=coord, levels=r["levels"], c=tuple(ch(c) for c in r["c"]), z=(), targets=[], fields={})
            groups.append(g)
        if r["z"]:
            g["z"] = tuple(ch(c) for c in r["z"])
        if target not in g["targets"]:
            g["targets"].append(target)
        if r["field"] not in g["fields"]:
            node, gh = (V.NODE_NONE, V.NODE_NONE), 0.0
            if r["node"] == ["zs"]:
                node = (V.NODE_ZS, V.NODE_NONE)
            elif r["node"]:
                node = (ch(r["node"][0]), ch(r["node"][1]) if len(r["node"]) > 1 else V.NODE_NONE)
                gh = float(np.float32(V.GRAVITY * NODE_HEIGHT_M[r["node"][0]]))
            g["fields"][r["field"]] = (kind, tuple(ch(c) for c in r["a"]), tuple(ch(c) for c in r["b"]), node, gh, {})
        g["fields"][r["field"]][5][target] = slot
    for g in groups:
        fields = tuple(V.Field(kind, a, b, tuple(slots.get(t, -1) for t in g["targets"]), node, gh)
                       for kind, a, b, node, gh, slots in g["fields"].values())
        out.vert_ops.append(V.Op(g["coord"], tuple(float(l) for l in g["levels"]), g["c"], g["z"], tuple(g["targets"]), fields, outside))
    if len(out.vert_ops) > V.MAX_OPS:
        raise ValueError(f"derived: {len(out.vert_ops)} vertical-interpolation ops for {[n for _, n in requests]}; one call holds {V.MAX_OPS}")


def column_levels(names, levels=None) -> list:
    """The pressure levels (hPa, ascending) with q, u and v among ``names`` and 300 <= level <= 1000 (or those of ``levels``)."""
    names = set(names)
    have = sorted(int(n[1:]) for n in names if re.fullmatch(r"q\d+", n))
    if not have:
        raise ValueError("the column integrals (ivt, ivtu, ivtv, iwv) need specific humidity: this model has no channel q<level> "
                         "(q from relative humidity is out of scope)")
    if levels is not None:
        use = sorted(int(l) for l in levels)
    else:
        use = [l for l in have if 300 <= l <= 1000]
    missing = [f"{x}{l}" for l in use for x in "quv" if f"{x}{l}" not in names]
    if missing:
        raise ValueError(f"the column integrals need the channels {missing}, which this model lacks")
    if not 2 <= len(use) <= MAX_LEVELS:
        raise ValueError(f"the column integrals run over 2 to {MAX_LEVELS} levels, not {len(use)}")
    return use


def plan(names, fields, lat, lon, levels=None, surface: bool = False, column=None, vertical=None) -> Plan:
    """Resolve the derived ``fields`` against the channels ``names`` of a (C, H, W) state on the grid (lat, lon).  Every refusal is a
    ValueError before the device is touched: an unknown name, a name that is one of the model's channels, missing input channels (named),
    more than ``MAX_OPS`` ops, a grid vorticity cannot be formed on.  ``vo<X>`` and ``div<X>`` of one level share an op, and so do the
    four column integrals.  ``surface``: a surface geopotential will be given, so the parcel columns need z; ``column``: the levels of the
    thermodynamic columns when they are not to be taken from the channels (``Plan.column`` of the forecast, for its truth);
    ``vertical``: ``{"outside": "nan" | "nearest"}``, what a field on a surface is where the surface does not cross the column."""
    names, fields = list(names), list(fields)
    outside = vertical_options(vertical)
    if not fields:
        raise ValueError("derived: at least one field")
    if len(set(fields)) != len(fields):
        raise ValueError(f"derived: a field is named twice in {fields}")
    ops, inputs, merged, thermal, surfaces = [], {}, {}, [], []
    out = Plan(fields, ops, inputs)
    for slot, name in enumerate(fields):
        if name in names:
            raise ValueError(f"derived: {name!r} is a channel of this model, not a derived field")
        parsed = _parse(name)
        if parsed is None and _parse_thermo(name) is not None:
            thermal.append((slot, name))
            continue
        if parsed is None and _parse_vert(name) is not None:
            surfaces.append((slot, name))
            continue
        if parsed is None:
            raise ValueError(f"derived: unknown field {name!r}; known are ws10m, ws100m, ws<level>, thk<a>_<b>, vo<X>, div<X> "
                             f"(X a level, 10m or 100m), {', '.join(COLUMN_FIELDS)}, {VERT_KNOWN}, {THERMO_KNOWN}")
        kind, raw, result = parsed
        if kind == COLUMN:
            if not out.levels:
                out.levels = column_levels(names, levels)
                out.weights = column_weights(out.levels)
            raw = tuple(f"{x}{l}" for x in ("q" if name == "iwv" else "quv") for l in out.levels)
            key = (COLUMN,)
        else:
            missing = [c for c in raw if c not in names]
            if missing:
                raise ValueError(f"derived: {name!r} needs the channel{'s' if len(missing) > 1 else ''} "
                                 f"{', '.join(repr(c) for c in missing)}, which this model lacks")
            key = (kind,) + raw if kind == VORTDIV else (kind, name)
        inputs[name] = list(raw)
        if key not in merged:
            merged[key] = len(ops)
            if kind == COLUMN:
                idx = tuple(tuple(names.index(f"{x}{l}") for l in out.levels) for x in "quv")
                ops.append(Op(COLUMN, idx, (-1, -1, -1, -1), tuple(float(np.float32(w)) for w in out.weights)))
            else:
                ops.append(Op(kind, (names.index(raw[0]), names.index(raw[1])), (-1,) * RESULTS[kind]))
        k = merged[key]
        slots = list(ops[k].outputs)
        slots[result] = slot
        ops[k] = Op(ops[k].kind, ops[k].inputs, tuple(slots), ops[k].weights)
    if len(ops) > MAX_OPS:
        raise ValueError(f"derived: {len(ops)} ops for {fields}; one call holds {MAX_OPS}")
    if thermal:
        _thermo_plan(out, names, thermal, surface, column)
    if surfaces:
        _vert_plan(out, names, surfaces, surface, column, outside)
    if any(op.kind == VORTDIV for op in ops):
        out.rowc, e0, e1 = row_table(lat, lon)
        out.edges = (e0, e1)
    elif len(lat) < 3 or len(lon) < 4:
        raise ValueError("derived fields need a grid of at least 3 rows and 4 columns")
    return out


def check_request(names, fields, lat, lon, n_members: int = 1, levels=None, surface: bool = False, column=None, vertical=None) -> Plan:
    """Every refusal that needs no device; returns the plan."""
    if _world_size() > 1:
        raise NotImplementedError("derived fields are made on one GPU from members that all lie there; members sharded over the ranks of "
                                  "a process group are out of scope (DESIGN.md 21)")
    if not 1 <= int(n_members) <= MAX_MEMBERS:
        raise ValueError(f"n_members = {n_members}: derived fields are made for 1 to {MAX_MEMBERS} members (SKDERIVE_MAX_MEMBERS)")
    return plan(names, fields, lat, lon, levels, surface, column, vertical)


# ---- the drivers ------------------------------------------------------------------------------------------------------------------------- #
class LeadDeriver:
    """Derives one lead time after the other into its own (M, D, H, W) buffer.  ``names``: the forecast's channels in the order of its
    (C, H, W) states; ``fields``: the derived names, channel d of the buffer is fields[d].  ``surface``: the (H, W) surface geopotential
    in the units of z, which masks the levels below the ground for zdeg0 and the parcel fields (None: they are treated as air);
    ``column``: ``Plan.column`` of another plan, whose thermodynamic columns this one is to use.  For the fields ``<field>@<surface>`` the
    surface is also the ground of ``@<Z>magl``, and ``vertical`` (``{"outside": "nan" | "nearest"}``) says what they are where the surface does
    not cross the column."""

    def __init__(self, names, lat, lon, n_members, fields, device="cuda:0", levels=None, surface=None, column=None, vertical=None):
        self.plan = check_request(names, fields, lat, lon, n_members, levels, surface is not None, column, vertical)
        self.names, self.fields, self.M = list(names), list(fields), int(n_members)
        self.lat, self.lon, self.device = np.asarray(lat, np.float64), np.asarray(lon, np.float64), device
        self.surface = None
        if surface is not None:
            self.surface = np.ascontiguousarray(np.asarray(surface, np.float32))
            if self.surface.shape != (self.lat.size, self.lon.size):
                raise ValueError(f"derived: the surface geopotential must be ({self.lat.size}, {self.lon.size}), not {self.surface.shape}")
        self._dev = None

    def _buffers(self):
        if self._dev is None:
            import torch
            from .ensemble import member_table
            dev = torch.device(self.device)
            out = torch.empty((self.M, len(self.fields), self.lat.size, self.lon.size), dtype=torch.float32, device=dev)
            states = [out[m] for m in range(self.M)]
            self._dev = dict(out=out, states=states, table=member_table(states),
                             rowc=None if self.plan.rowc is None else torch.from_numpy(self.plan.rowc).to(dev),
                             surface=None if self.surface is None or not (self.plan.thermo_ops or self.plan.vert_ops) else torch.from_numpy(self.surface).to(dev))
        return self._dev

    def add(self, states, table=None) -> tuple:
        """ONE derive launch over the M device states (C, H, W), then one of the thermodynamic ops and one of the vertical interpolation
        when the request names any; returns
        (derived_states, derived_table): M (D, H, W) views of the buffer and their ``ensemble.member_table``, ready for
        ``ensemble.stats`` and ``LeadScorer.add``.  The next ``add`` overwrites them."""
        from .ensemble import member_table
        if len(states) != self.M:
            raise ValueError(f"{len(states)} states for a deriver of {self.M} members")
        b = self._buffers()
        table = member_table(states) if table is None else table
        if self.plan.ops:
            run(states, table, self.plan.ops, b["out"], b["rowc"], self.plan.edges)
        if self.plan.thermo_ops:
            from . import thermo
            thermo.run(states, table, self.plan.thermo_ops, b["out"], b["surface"])
        if self.plan.vert_ops:
            from . import vertical
            vertical.run(states, table, self.plan.vert_ops, b["out"], b["surface"])
        return b["states"], b["table"]


class TruthDeriver:
    """The hook ``verify.LeadScorer(adapt=...)`` calls so that a truth (or climatology) of RAW channels scores derived fields: the raw
    inputs of a valid time are uploaded into a (C, H, W) state and derived by the same kernel with M = 1.  A derived field whose inputs
    the truth lacks is not offered to the scorer; ``dropped`` names it and the channels that are missing (for a thermodynamic column the
    truth holds no part of, the plan's own refusal).  ``levels``: the pressure levels of the forecast's column integrals, so that the
    truth's are the same integral (None: those the truth holds between 300 and 1000 hPa).
    ``surface``, ``column``, ``moisture``: the surface geopotential, ``Plan.column`` and ``Plan.moisture`` of the forecast's deriver, so
    that the truth's thermodynamic fields are made from the same levels and the same kind of humidity; ``vertical``: the forecast's, so
    that the truth's fields on surfaces go through the same ops."""

    def __init__(self, fields, lat, lon, device="cuda:0", levels=None, surface=None, column=None, moisture=None, vertical=None):
        self.fields, self.lat, self.lon, self.device, self.levels = list(fields), lat, lon, device, levels
        self.surface, self.column, self.moisture, self.vertical = surface, column, moisture, vertical
        self.dropped: dict = {}
        self._derivers: dict = {}

    def _needs(self, name, have) -> list:
        if _parse(name) is None and _parse_vert(name) is not None:      # a field on a surface, over the forecast's levels when they are given
            return vert_inputs(name, have, self.surface is not None, self.column)["raw"]
        if _parse(name) is None:                               # column thermodynamics, over the forecast's levels when they are given
            op, key, slot = _parse_thermo(name)
            moisture = self.moisture or moisture_of(have) or "q"
            levels = (self.column or {}).get(op)
            if levels is None and op in ("freeze", "parcel"):          # (no column to be had from these channels: the plan's ValueError)
                levels = thermo_inputs(name, have, moisture, self.surface is not None)[1]
            return _thermo_raw(op, key, slot, moisture, self.surface is not None, levels)
        kind, raw, _ = _parse(name)
        if kind == COLUMN:
            lv = self.levels
            if lv is None:
                lv = [l for l in sorted(int(n[1:]) for n in have if re.fullmatch(r"q\d+", n)) if 300 <= l <= 1000]
            raw = [f"{x}{l}" for x in ("q" if name == "iwv" else "quv") for l in lv] or ["q<level>"]
        return list(raw)

    def _partners(self, name, have) -> list:
        """The channels that would complete the levels ``have`` holds in part for the column of ``name``: t850 without z850 names z850"""
        if _parse_vert(name) is not None:
            levels = (self.column or {}).get("vert") or []
            fld, coord, _ = _parse_vert(name)
            letters = {"P": "", "Z": "z", "Z_AGL": "z", "THETA": "t", "T": "t"}[coord] + {"ws": "uv", "theta": "t", "p": ""}.get(fld, fld)
            return [f"{x}{l}" for l in levels for x in dict.fromkeys(letters) if f"{x}{l}" not in have]
        op = _parse_thermo(name)[0]
        letters = "tz" if op == "freeze" else "t" + (self.moisture or moisture_of(have) or "q") + ("z" if self.surface is not None else "")
        levels = sorted({int(n[1:]) for n in have if n[0] in letters and n[1:].isdigit()}, reverse=True)
        return [f"{x}{l}" for l in levels for x in letters if f"{x}{l}" not in have]

    def names(self, fields) -> list:
        """The derived names that can be formed from the channels ``fields`` (a ``verify._Fields``) holds."""
        have, ok = set(fields.names), []
        for name in self.fields:
            try:
                missing = [c for c in self._needs(name, have) if c not in have]
            except ValueError as e:                            # no thermodynamic column in these channels
                missing = self._partners(name, have) or [str(e)]
            if missing:
                self.dropped.setdefault(name, missing)
            else:
                ok.append(name)
        return ok

    def upload(self, fields, time, scored, dst, idx_dev) -> None:
        """Fill the rows ``idx_dev`` of ``dst`` (the scorer's (D, H, W) truth buffer) with the fields ``scored`` at ``time``."""
        import torch
        key = (id(fields), tuple(scored))
        hit = self._derivers.get(key)
        if hit is None:
            raw = []
            for name in scored:
                raw += [c for c in self._needs(name, set(fields.names)) if c not in raw]
            hit = (raw, LeadDeriver(raw, self.lat, self.lon, 1, list(scored), self.device, self.levels, self.surface, self.column, self.vertical), fields)
            self._derivers[key] = hit                          # (holds ``fields``: its id stays taken while the entry lives)
        raw, deriver, _ = hit
        state = torch.from_numpy(fields.at(time, raw)).to(deriver.device)
        states, _ = deriver.add([state])
        dst[idx_dev] = states[0]


@dataclass
class DerivedProducts:
    """``EnsembleForecast.derived``: the attributes of the raw products, labelled with the derived names.  ``dropped``: the derived
    fields that could not be scored, with the truth channels that are missing."""
    fields: list
    mean: object = None
    spread: object = None
    min: object = None
    max: object = None
    exceedance: dict = field(default_factory=dict)
    quantile: dict = field(default_factory=dict)
    members: object = None
    scores: object = None
    dropped: dict = field(default_factory=dict)


def derive_model(gm, start_time: datetime.datetime, n_steps: int, fields, save: bool = False, save_config: dict | None = None, surface=None,
                 vertical=None):
    """``GlobalModel.derive_fields`` (core/models/base.py has the user-facing description)."""
    from .labeled import DataArray
    model = gm.model
    if n_steps < 0:
        raise ValueError("n_steps >= 0")
    check_request(model.out_channel_names, fields, model.grid.lat, model.grid.lon, 1, surface=surface is not None, vertical=vertical)      # before anything of the device
    deriver = LeadDeriver(model.out_channel_names, model.grid.lat, model.grid.lon, 1, fields, device=model.device, surface=surface, vertical=vertical)
    require_gpu(model.device, "derive_fields derives with HIP kernels where the forecast lies: the model must be on a GPU")
    times, host = [], []

    def each(k, time, state):
        states, _ = deriver.add([state])
        times.append(time)
        host.append(states[0].cpu().numpy())
    run_model(gm, start_time, n_steps, each)
    da = DataArray(np.stack(host), ["time", "channel", "lat", "lon"],
                   dict(time=times, channel=list(fields), lat=np.asarray(model.grid.lat), lon=np.asarray(model.grid.lon)))
    if save:
        from .common import save_config_with_id, save_forecast
        cfg = save_config_with_id(save_config)
        da.path = save_forecast(da, f"{gm.model_name}-derived", times[0], times[-1], gm.source_label, config=cfg)
    return da


def derive_prediction(pred, fields, device="cuda:0", surface=None, vertical=None):
    """Derived fields of a forecast that already exists: a ``GlobalPrediction``, a (time, channel, lat, lon) DataArray, a saved netCDF
    file or zarr store, or a list of such files (their time entries in order, duplicates of a valid time derived once).  Each time
    entry is uploaded on its own and goes through the same kernel as ``derive_fields``.  ``surface``: the (lat, lon) surface
    geopotential of ``LeadDeriver``, ``vertical`` its options for the fields ``<field>@<surface>``.  Returns DataArray(time, channel=fields, lat, lon)."""
    from .labeled import DataArray
    saved = open_saved(pred, "derive_prediction")
    lat, lon = saved.lat, saved.lon
    deriver = LeadDeriver(saved.names, lat, lon, 1, fields, device=device, surface=surface, vertical=vertical)
    require_gpu(device, "derive_prediction derives with HIP kernels: it needs a GPU", present=True)
    times, host = [], []
    for _, time, state in saved.states(deriver.device):
        states, _ = deriver.add([state])
        times.append(time)
        host.append(states[0].cpu().numpy())
    return DataArray(np.stack(host), ["time", "channel", "lat", "lon"], dict(time=times, channel=list(fields), lat=lat, lon=lon))
