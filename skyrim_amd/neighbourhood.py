"""Neighbourhood fields on the device (include/skyrim_nbr.h): the maximum, minimum, area-weighted mean and the fraction above
a threshold of a channel over the great-circle disc of R km around every grid point, folded per member into an (M, D, H, W) buffer that
the ensemble statistics, the scorer, the event counter and the point sampler read like raw channels -- ``exceed={"ws10m_max_100km": [25]}``
is the chance of 25 m/s SOMEWHERE within 100 km.

Layers:

* the binding of libskyrim_nbr.so (``SPEC``, ``load_library``, ``run``); the same call is ``torch.ops.skyrim_hip.nbr_fields``.
  Neighbourhood fields have no CPU fallback;
* the requests: ``parse_request`` reads ``channel:stat:radius``, ``check_request`` resolves a list of them against a model's channels and
  grid into slots, ops and the disc tables (``discs``: THE definition of the disc, made once on the host);
* the drivers: ``LeadNeighbourhood`` (what ``ensemble.run`` calls with ``neighbourhood=[...]``), ``TruthNeighbourhood`` (the hook that lets
  ``verify.LeadScorer`` score a neighbourhood field against the same field of the truth), ``neighbourhood_model``
  (``GlobalModel.neighbourhood_forecast``) and ``neighbourhood_prediction`` for forecasts that are already on disk.
"""
from __future__ import annotations

import ctypes
import datetime
import math
import re
from dataclasses import dataclass, field, replace

import numpy as np

from . import native, program
from .common import world_size as _world_size
from .leads import open_saved, require_gpu, run_model

MAX_MEMBERS, MAX_OPS, MAX_RADII = 64, 16, 4                     # include/skyrim_nbr.h SKNBR_MAX_*
MAX_W, MAX_REACH = 2048, 128                                    # SKNBR_MAX_W, SKNBR_MAX_REACH
MAX, MIN, MEAN, FRAC_ABOVE = 1, 2, 3, 4                         # SKNBR_MAX ...
KINDS = (MAX, MIN, MEAN, FRAC_ABOVE)
STATS = ("max", "min", "mean", "frac_above@<threshold>")
_P = ctypes.c_void_p


class OpDesc(ctypes.Structure):
    """sknbr_op (``in_`` is the header's ``in``)."""
    _fields_ = [("kind", ctypes.c_int32), ("in_", ctypes.c_int32), ("out", ctypes.c_int32), ("radius", ctypes.c_int32), ("thr", ctypes.c_float)]


class RadiusDesc(ctypes.Structure):
    """sknbr_radius."""
    _fields_ = [("reach", ctypes.c_int32), ("half", _P)]


class NbrDesc(ctypes.Structure):
    """sknbr_desc."""
    _fields_ = [("members", _P), ("M", ctypes.c_int), ("member_align", ctypes.c_int), ("C", ctypes.c_int), ("H", ctypes.c_int),
                ("W", ctypes.c_int), ("D", ctypes.c_int), ("out", _P), ("member_stride", ctypes.c_size_t), ("weights", _P),
                ("n_radii", ctypes.c_int), ("radii", RadiusDesc * MAX_RADII), ("n_ops", ctypes.c_int), ("ops", OpDesc * MAX_OPS)]


SPEC = native.Spec("skyrim_nbr", "SKYRIM_NBR_LIB", "sknbr", 1, {                # include/skyrim_nbr.h SKNBR_ABI_VERSION
    "sknbr_abi_version": (ctypes.c_int, []),
    "sknbr_check": (ctypes.c_int, [ctypes.POINTER(NbrDesc)]),
    "sknbr_run": (ctypes.c_int, [ctypes.POINTER(NbrDesc), _P]),
}, " -- neighbourhood fields have no torch fallback")
EXPORTS, ABI_VERSION = SPEC.exports, SPEC.abi

_lib = None


def load_library() -> ctypes.CDLL:
    """libskyrim_nbr.so (built in-tree by ``__graft_entry__.build()`` / ``make -C skyrim_amd/csrc``)."""
    global _lib
    if _lib is None:
        _lib = native.load(SPEC)
    return _lib


# ---- the program ------------------------------------------------------------------------------------------------------------------------- #
@dataclass(frozen=True)
class Op:
    """One op of a call: ``channel`` is the input channel (the header's ``in``), ``out`` the slot of the result, ``radius`` the index of
    the disc table, ``thr`` the threshold of FRAC_ABOVE."""
    kind: int
    channel: int
    out: int
    radius: int = 0
    thr: float = 0.0


def encode(ops) -> tuple:
    """(ints, floats): the flat form ``torch.ops.skyrim_hip.nbr_fields`` takes.  Per op four ints (kind, channel, out, radius) and one
    float (thr)."""
    ints, floats = [], []
    for op in ops:
        ints += [int(op.kind), int(op.channel), int(op.out), int(op.radius)]
        floats.append(float(op.thr))
    return ints, floats


def decode(ints, floats) -> list:
    ints, floats = list(ints), list(floats)
    if len(ints) % 4 or len(floats) * 4 != len(ints):
        raise ValueError("nbr_fields: a program holds four ints and one float per op")
    ops = []
    for k in range(len(ints) // 4):
        if ints[4 * k] not in KINDS:
            raise ValueError(f"nbr_fields: unknown op kind {ints[4 * k]}")
        ops.append(Op(*ints[4 * k:4 * k + 4], float(floats[k])))
    return ops


def describe(ops, M, C, H, W, D, member_stride, reaches, member_align=16) -> NbrDesc:
    """The descriptor of a call, its pointers still NULL.  ``reaches``: the reach of each radius."""
    d = NbrDesc()
    program.fill_head(d, M, C, H, W, D, member_stride, member_align)
    reaches = list(reaches)
    d.n_radii = len(reaches)
    for k, r in enumerate(reaches[:MAX_RADII]):
        d.radii[k].reach = int(r)
    ops = list(ops)
    d.n_ops = len(ops)
    for k, op in enumerate(ops[:MAX_OPS]):
        o = d.ops[k]
        o.kind, o.in_, o.out, o.radius, o.thr = op.kind, op.channel, op.out, op.radius, op.thr
    return d


def run(members, table, ops, half, weights, out) -> None:
    """One ``sknbr_run``: the ops ``ops`` over the M ``members`` (equal-shaped contiguous float32 (C, H, W) device tensors; ``table`` =
    ``ensemble.member_table(members)``) into ``out``, float32 (M, D, H, W).  ``half``: one int32 (H, 2 reach + 1) device tensor per radius
    (``discs``); ``weights``: float64 (H) on the device.  Queued on torch's current stream.  As in ``derived.run``, the contents of
    ``table`` are trusted to be the addresses of ``members``."""
    import torch
    ops, half = list(ops), list(half)
    program.counts("nbr_fields", members, ops, MAX_MEMBERS, MAX_OPS)
    if not 1 <= len(half) <= MAX_RADII:
        raise ValueError(f"nbr_fields: {len(half)} radii; 1 to {MAX_RADII} are supported")
    M, dev, align, C, H, W, D, po = program.bind("nbr_fields", members, table, ops, out, "nbr_fields: out", MAX_MEMBERS, MAX_OPS, counted=True)
    pw = native.tensor_ptr(weights, "nbr_fields: weights", torch.float64, dev)
    if tuple(weights.shape) != (H,):
        raise ValueError(f"nbr_fields: weights must be ({H},)")
    reaches, ph = [], []
    for k, t in enumerate(half):
        ph.append(native.tensor_ptr(t, f"nbr_fields: half[{k}]", torch.int32, dev))
        if t.dim() != 2 or t.shape[0] != H or t.shape[1] % 2 != 1:
            raise ValueError(f"nbr_fields: half[{k}] must be ({H}, 2 reach + 1)")
        reaches.append((t.shape[1] - 1) // 2)
    d = describe(ops, M, C, H, W, D, D * H * W, reaches, align)
    d.members, d.out, d.weights = table.data_ptr(), po, pw
    for k, p in enumerate(ph):
        d.radii[k].half = p
    lib = load_library()
    program.launch(lib, lib.sknbr_run, d, dev)


# ---- the disc ---------------------------------------------------------------------------------------------------------------------------- #
def _axes(lat, lon) -> tuple:
    """(lat, lon) as float64 after the refusals of the grid: a strictly monotonic latitude axis within +-90, a uniformly spaced longitude
    axis that closes the circle."""
    lat, lon = np.asarray(lat, np.float64), np.asarray(lon, np.float64)
    if lat.ndim != 1 or lon.ndim != 1 or lat.size < 1 or lon.size < 1 or not np.all(np.isfinite(lat)) or np.any(np.abs(lat) > 90):
        raise ValueError("neighbourhood: one-dimensional axes, latitudes in degrees within +-90")
    step = np.diff(lat)
    if lat.size > 1 and not (np.all(step > 0) or np.all(step < 0)):
        raise ValueError("neighbourhood: the latitude axis must be strictly monotonic")
    W = lon.size
    dlon = np.diff(lon)
    if W < 2 or not np.all(np.isfinite(lon)) or dlon[0] == 0 or not np.allclose(dlon, dlon[0], rtol=0, atol=1e-6 * abs(dlon[0])) \
            or abs(abs(dlon[0]) * W - 360.0) > 1e-6 * 360.0:
        raise ValueError("neighbourhood: discs need a uniformly spaced longitude axis that closes the circle (W * dlon = 360); on a regional "
                         "grid (a regional regrid target, for one) discs periodic in longitude are not defined (DESIGN.md 35, out of scope)")
    return lat, lon


def _cos_lat(lat) -> np.ndarray:
    """cos of the latitudes, exactly 0 at exactly +-90: all nodes of a pole row are one place."""
    c = np.cos(np.deg2rad(lat))
    c[np.abs(lat) == 90.0] = 0.0
    return c


def haversine_km(phi1, phi2, dlam, cos1=None, cos2=None):
    """The great-circle distance in km (float64, a = ``tracks.EARTH_RADIUS_KM``) between points at the latitudes ``phi1`` and ``phi2``
    (radians) whose longitudes differ by ``dlam`` (radians); ``cos1`` / ``cos2``: their cosines when the caller has pinned them."""
    from .tracks import EARTH_RADIUS_KM
    cos1 = np.cos(phi1) if cos1 is None else cos1
    cos2 = np.cos(phi2) if cos2 is None else cos2
    h = np.sin((phi2 - phi1) / 2) ** 2 + cos1 * cos2 * np.sin(dlam / 2) ** 2
    return 2.0 * EARTH_RADIUS_KM * np.arcsin(np.sqrt(np.minimum(h, 1.0)))


def _row_reach(lat, R) -> int:
    """The largest |d| for which some row j + d has a point within R of row j: the nearest point of a row lies on the same meridian."""
    phi, c = np.deg2rad(lat), _cos_lat(lat)
    near = haversine_km(phi[:, None], phi[None, :], 0.0, c[:, None], c[None, :]) <= R
    j, r = np.nonzero(near)
    return int(np.abs(r - j).max())


def discs(lat, lon, radius_km) -> tuple:
    """(reach, half): THE disc of ``radius_km`` around every point of a global grid.  ``half``: int32 (H, 2 reach + 1);
    ``half[j, reach + d]`` is -1 when row j + d is off the grid or has no point within R of a point of row j, else the largest n in
    [0, W // 2] for which the great-circle distance between (lat_j, 0) and (lat_{j+d}, n dlon) is <= R: the disc around (j, i) holds the
    columns i - n ... i + n of that row (periodic), or the whole row, each of its W points once, when 2 n + 1 >= W.  The distance is the
    haversine in float64 with a = ``tracks.EARTH_RADIUS_KM``; cos(lat) of a row at exactly +-90 is exactly 0, so a disc that reaches the
    pole takes the whole pole row.  ``reach``: the largest |d| used."""
    lat, lon = _axes(lat, lon)
    R = float(radius_km)
    if not (R > 0 and math.isfinite(R)):
        raise ValueError(f"neighbourhood: a radius in km is finite and positive, got {radius_km}")
    H, W = lat.size, lon.size
    reach = _row_reach(lat, R)
    phi, c = np.deg2rad(lat), _cos_lat(lat)
    lam = np.arange(W // 2 + 1, dtype=np.float64) * (2.0 * math.pi / W)
    half = np.full((H, 2 * reach + 1), -1, np.int32)
    for d in range(-reach, reach + 1):
        j = np.arange(max(0, -d), min(H, H - d))
        if j.size == 0:
            continue
        inside = haversine_km(phi[j, None], phi[j + d, None], lam[None, :], c[j, None], c[j + d, None]) <= R      # (rows, W // 2 + 1)
        # the distance grows with n on [0, W // 2]: the columns inside are n = 0 ... count - 1
        half[j, reach + d] = inside.sum(axis=1).astype(np.int32) - 1
    return reach, half


def disc_points(half, W: int) -> np.ndarray:
    """N_j: the points of the disc around a point of row j (int64 [H])."""
    h = np.asarray(half, np.int64)
    return np.where(h < 0, 0, np.minimum(2 * h + 1, W)).sum(axis=1)


# ---- requests ---------------------------------------------------------------------------------------------------------------------------- #
@dataclass(frozen=True)
class Request:
    """``channel:stat:radius``.  ``stat``: max, min, mean, frac_above@<threshold>; ``radius``: ``<N>km``."""
    channel: str
    stat: str
    radius: str

    @property
    def name(self) -> str:
        """The field's channel name: the request with ``:`` replaced by ``_``."""
        return f"{self.channel}_{self.stat}_{self.radius}"

    @property
    def km(self) -> int:
        return int(self.radius[:-2])


def _threshold(stat: str) -> float:
    """The threshold of ``frac_above@<threshold>``, rounded to float32 as the kernel compares it."""
    try:
        v = float(stat.split("@", 1)[1])
    except ValueError:
        v = math.nan
    if math.isnan(v):
        raise ValueError(f"neighbourhood: {stat!r}: frac_above@<threshold> needs a number (inf and -inf are allowed)")
    return float(np.float32(v))


def parse_request(req) -> Request:
    """A ``Request`` from ``"channel:stat:radius"`` or from an object with these three fields; ValueError when it is not one."""
    if isinstance(req, str):
        parts = req.split(":")
        if len(parts) != 3:
            raise ValueError(f"neighbourhood: {req!r} is not channel:stat:radius (for example ws10m:max:100km)")
        req = Request(*(p.strip() for p in parts))
    elif all(hasattr(req, a) for a in ("channel", "stat", "radius")):
        req = Request(str(req.channel), str(req.stat), str(req.radius))
    else:
        raise ValueError("neighbourhood: a request is a string channel:stat:radius or has the fields channel, stat, radius, not "
                         f"{type(req).__name__}")
    if not req.channel:
        raise ValueError(f"neighbourhood: {req}: the channel is empty")
    if req.stat.startswith("frac_above@"):
        _threshold(req.stat)
    elif req.stat not in ("max", "min", "mean"):
        raise ValueError(f"neighbourhood: unknown statistic {req.stat!r}; known are {', '.join(STATS)} -- other kernels than the flat disc "
                         "(Gaussian weights, percentiles within the disc) are out of scope (DESIGN.md 35)")
    if not re.fullmatch(r"[1-9]\d*km", req.radius):
        raise ValueError(f"neighbourhood: radius {req.radius!r} is not <N>km (N a positive whole number of kilometres; one radius for every "
                         "point: radii that vary from point to point are out of scope)")
    return req


def op_of(r: Request, channel: int, slot: int, radius: int) -> Op:
    if r.stat.startswith("frac_above@"):
        return Op(FRAC_ABOVE, channel, slot, radius, _threshold(r.stat))
    return Op({"max": MAX, "min": MIN, "mean": MEAN}[r.stat], channel, slot, radius)


@dataclass
class Plan:
    """A resolved list of requests.  ``names``: the channels the ops' inputs index (the model's, then the derived fields); ``fields``: the
    neighbourhood fields' names, slot k is fields[k]; ``ops``: one per request; ``radii``: the distinct radii in km, in the order they first
    appear; ``reach`` / ``half``: their disc tables; ``weights``: the row weights of the mean."""
    names: list
    requests: list
    fields: list
    ops: list
    radii: list
    reach: list
    half: list
    weights: np.ndarray

    @property
    def D(self) -> int:
        return len(self.fields)


def check_request(names, requests, lat, lon, n_members: int = 1, derived=(), other=()) -> Plan:
    """Every refusal that needs no device; returns the plan.  ``names``: the model's output channels; ``derived``: the fields of
    ``derived=``, which requests may name as well; ``other``: names of other products of the same forecast (aggregates), which a request
    may neither name as its input nor clash with."""
    from .verify import area_weights
    if _world_size() > 1:
        raise NotImplementedError("neighbourhood fields are made on one GPU from members that all lie there; members sharded over the ranks "
                                  "of a process group are out of scope (DESIGN.md 35)")
    if not 1 <= int(n_members) <= MAX_MEMBERS:
        raise ValueError(f"n_members = {n_members}: neighbourhood fields are made for 1 to {MAX_MEMBERS} members (SKNBR_MAX_MEMBERS)")
    if isinstance(requests, (str, Request)) or not hasattr(requests, "__iter__"):
        raise ValueError("neighbourhood: a list of requests channel:stat:radius")
    reqs = [parse_request(r) for r in requests]
    if not reqs:
        raise ValueError("neighbourhood: at least one request")
    names, derived, other = list(names), list(derived), list(other)
    known = names + derived
    seen = set()
    for r in reqs:
        if r.name in seen:
            raise ValueError(f"neighbourhood: {r.name!r} is requested twice")
        seen.add(r.name)
        if r.channel in other:
            raise ValueError(f"neighbourhood: {r.channel!r} is an aggregate; aggregates as input to neighbourhoods are out of scope "
                             "(DESIGN.md 35)")
        if r.channel not in known:
            raise ValueError(f"neighbourhood: channel {r.channel!r} is not an output channel of this model or one of the derived fields "
                             "named in derived=")
    clash = [r.name for r in reqs if r.name in known or r.name in other]
    if clash:
        raise ValueError(f"neighbourhood: {clash} are already channels, derived fields or aggregates of this forecast")
    if len(reqs) > MAX_OPS:
        raise ValueError(f"neighbourhood: {len(reqs)} ops for {[r.name for r in reqs]}; one call holds {MAX_OPS} (SKNBR_MAX_OPS)")
    radii = list(dict.fromkeys(r.km for r in reqs))
    if len(radii) > MAX_RADII:
        raise ValueError(f"neighbourhood: {len(radii)} distinct radii {radii}; one call holds {MAX_RADII} (SKNBR_MAX_RADII)")
    lat, lon = _axes(lat, lon)
    if lon.size > MAX_W:
        raise ValueError(f"neighbourhood: a grid of {lon.size} columns; the kernel holds rows of at most {MAX_W} (SKNBR_MAX_W)")
    if len(reqs) * lat.size * lon.size > 2 ** 30 or len(known) * lat.size * lon.size > 2 ** 30:
        raise ValueError(f"neighbourhood: {len(reqs)} slots of {lat.size} x {lon.size} points exceed 2^30 elements per member")
    for km in radii:
        reach = _row_reach(lat, float(km))
        if reach > MAX_REACH:
            raise ValueError(f"neighbourhood: a radius of {km} km reaches {reach} rows either side on this grid; the kernel streams at most "
                             f"{MAX_REACH} (SKNBR_MAX_REACH)")
    tables = [discs(lat, lon, km) for km in radii]
    ops = [op_of(r, known.index(r.channel), k, radii.index(r.km)) for k, r in enumerate(reqs)]
    return Plan(known, reqs, [r.name for r in reqs], ops, radii, [t[0] for t in tables], [t[1] for t in tables], area_weights(lat))


# ---- the drivers ------------------------------------------------------------------------------------------------------------------------- #
class LeadNeighbourhood:
    """Makes the neighbourhood fields of one lead time after the other in its own (M, D, H, W) buffer.  ``names``: the forecast's channels
    in the order of its (C, H, W) states; ``derived``: the names of the planes of a ``LeadDeriver``'s buffer, which requests may name as
    well.  ``fields``: the names of the D planes."""

    def __init__(self, names, lat, lon, n_members, requests, device="cuda:0", derived=(), other=()):
        self.names, self.derived, self.M = list(names), list(derived), int(n_members)
        self.plan = check_request(self.names, requests, lat, lon, n_members, self.derived, other)
        self.fields = list(self.plan.fields)
        self.lat, self.lon, self.device = np.asarray(lat, np.float64), np.asarray(lon, np.float64), device
        self._dev = None

    def _buffers(self):
        if self._dev is None:
            import torch
            from .ensemble import member_table
            dev = torch.device(self.device)
            out = torch.empty((self.M, self.plan.D, self.lat.size, self.lon.size), dtype=torch.float32, device=dev)
            states = [out[m] for m in range(self.M)]
            self._dev = dict(out=out, states=states, table=member_table(states), half=[torch.from_numpy(h).to(dev) for h in self.plan.half],
                             weights=torch.from_numpy(np.ascontiguousarray(self.plan.weights, np.float64)).to(dev))
        return self._dev

    def add(self, states, table=None, derived=None) -> tuple:
        """ONE ``nbr_fields`` for the ops that read the M device states (C, H, W), and one more for those that read ``derived`` =
        (derived_states, derived_table) of ``LeadDeriver.add``, when requests name derived fields.  Returns (states, table): M (D, H, W)
        views of the buffer and their ``ensemble.member_table``, ready for ``ensemble.stats`` and ``LeadScorer.add``.  The next ``add``
        overwrites them."""
        from .ensemble import member_table
        if len(states) != self.M:
            raise ValueError(f"{len(states)} states for a neighbourhood of {self.M} members")
        b = self._buffers()
        C = len(self.names)
        own = [op for op in self.plan.ops if op.channel < C]
        other = [replace(op, channel=op.channel - C) for op in self.plan.ops if op.channel >= C]
        if own:
            run(states, member_table(states) if table is None else table, own, b["half"], b["weights"], b["out"])
        if other:
            if derived is None:
                raise ValueError("requests name derived fields: add() needs derived=(states, table) of the deriver")
            run(derived[0], derived[1], other, b["half"], b["weights"], b["out"])
        return b["states"], b["table"]


class TruthNeighbourhood:
    """The hook ``verify.LeadScorer(adapt=...)`` calls so that a truth (or climatology) of point values scores neighbourhood fields: the
    truth's inputs at a valid time are uploaded into a (C, H, W) state and go through the same kernel with M = 1.  ``inner``: a
    ``derived.TruthDeriver`` for the requests that name derived fields.  A field whose channel the truth lacks is not offered to the
    scorer; ``dropped`` names it."""

    def __init__(self, requests, lat, lon, device="cuda:0", inner=None):
        self.requests = [parse_request(r) for r in requests]
        self.lat, self.lon, self.device, self.inner = lat, lon, device, inner
        self.dropped: dict = {}
        self._cache: dict = {}

    def names(self, fields) -> list:
        have = set(fields.names)
        derivable = set(self.inner.names(fields)) if self.inner is not None else set()
        ok = []
        for r in self.requests:
            if r.channel in have or r.channel in derivable:
                ok.append(r.name)
            else:
                self.dropped.setdefault(r.name, [r.channel])
        return ok

    def upload(self, fields, time, scored, dst, idx_dev) -> None:
        """Fill the rows ``idx_dev`` of ``dst`` with the neighbourhood fields ``scored`` of the truth at ``time``."""
        import torch
        key = (id(fields), tuple(scored))
        hit = self._cache.get(key)
        if hit is None:
            reqs = [r for r in self.requests if r.name in scored]
            reqs.sort(key=lambda r: list(scored).index(r.name))
            have = set(fields.names)
            raw = [c for c in dict.fromkeys(r.channel for r in reqs) if c in have]
            der = [c for c in dict.fromkeys(r.channel for r in reqs) if c not in have]
            nb = LeadNeighbourhood(raw + der, self.lat, self.lon, 1, reqs, self.device)
            dev = torch.device(self.device)
            state = torch.zeros((len(raw) + len(der), len(self.lat), len(self.lon)), dtype=torch.float32, device=dev)
            hit = (raw, der, nb, state, torch.arange(len(raw), len(raw) + len(der), device=dev), fields)      # (holds ``fields``: its id stays taken)
            self._cache[key] = hit
        raw, der, nb, state, der_idx, _ = hit
        if raw:
            state[:len(raw)] = torch.from_numpy(fields.at(time, raw)).to(state.device)
        if der:
            self.inner.upload(fields, time, der, state, der_idx)
        out, _ = nb.add([state])
        dst[idx_dev] = out[0]


@dataclass
class NeighbourhoodProducts:
    """``EnsembleForecast.neighbourhood``: the attributes of the raw products, labelled with the neighbourhood fields' names.  ``dropped``:
    the fields that could not be scored, with the truth channels that are missing."""
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
    points: object = None        # points.PointForecast of the fields with ``points=...``


def _sequence(names, lat, lon, requests, device, drive, derived=None):
    """The neighbourhood fields of ONE forecast (M = 1): ``drive(each)`` calls ``each(k, time, state)`` with the (C, H, W) device state
    of every time entry.  Returns DataArray(time, channel = fields, lat, lon)."""
    from .labeled import DataArray
    dnames = list(derived or [])
    nb = LeadNeighbourhood(names, lat, lon, 1, requests, device, dnames)
    deriver = None
    if dnames:
        from .derived import LeadDeriver
        deriver = LeadDeriver(names, lat, lon, 1, dnames, device=device)
    times, host = [], []

    def each(k, time, state):
        states, _ = nb.add([state], None, deriver.add([state]) if deriver is not None else None)
        times.append(time)
        host.append(states[0].cpu().numpy())
    drive(each)
    return DataArray(np.stack(host), ["time", "channel", "lat", "lon"], dict(time=times, channel=list(nb.fields), lat=np.asarray(lat), lon=np.asarray(lon)))


def _checked(names, lat, lon, requests, derived):
    if derived is not None:
        from . import derived as deriving
        deriving.check_request(names, list(derived), lat, lon, 1)
    check_request(names, requests, lat, lon, 1, list(derived or []))


def neighbourhood_model(gm, start_time: datetime.datetime, n_steps: int, neighbourhood, derived=None, save: bool = False,
                        save_config: dict | None = None):
    """``GlobalModel.neighbourhood_forecast`` (core/models/base.py has the user-facing description)."""
    model = gm.model
    names = list(model.out_channel_names)
    if n_steps < 0:
        raise ValueError("n_steps >= 0")
    _checked(names, model.grid.lat, model.grid.lon, neighbourhood, derived)      # before the device
    require_gpu(model.device, "neighbourhood_forecast makes its fields with HIP kernels where the forecast lies: the model must be on a GPU")
    da = _sequence(names, model.grid.lat, model.grid.lon, neighbourhood, model.device, lambda each: run_model(gm, start_time, n_steps, each), derived)
    if save:
        from .common import save_config_with_id, save_forecast
        cfg = save_config_with_id(save_config)
        times = list(da.time.values.astype("datetime64[s]").astype(datetime.datetime))
        da.path = save_forecast(da, f"{gm.model_name}-nbr", times[0], times[-1], gm.source_label, config=cfg)
    return da


def neighbourhood_prediction(pred, neighbourhood, derived=None, device="cuda:0"):
    """Neighbourhood fields of a forecast that already exists: a ``GlobalPrediction``, a (time, channel, lat, lon) DataArray, a saved netCDF
    file or zarr store, or a list of such files (their time entries in order, duplicates of a valid time used once).  Each entry is
    uploaded on its own and goes through the same kernel as ``neighbourhood_forecast``.  Returns DataArray(time, channel = fields, lat, lon)."""
    saved = open_saved(pred, "neighbourhood_prediction")
    _checked(list(saved.names), saved.lat, saved.lon, neighbourhood, derived)
    require_gpu(device, "neighbourhood_prediction makes its fields with HIP kernels: it needs a GPU", present=True)

    def drive(each):
        for k, time, state in saved.states(device):
            each(k, time, state)
    return _sequence(list(saved.names), saved.lat, saved.lon, neighbourhood, device, drive, derived)
