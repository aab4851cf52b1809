"""Time-window aggregates on the device (include/skyrim_agg.h): the maximum, minimum, mean, sum, hours above a threshold and
the time of the extreme of a channel over windows of lead times, folded per member into an (M, D, H, W) accumulator that stays in HBM
across the lead times, so that the ensemble statistics, the scorer and the event counter read a closed window like raw channels.

Layers:

* the binding of libskyrim_agg.so (``SPEC``, ``load_library``, ``run``); the same call is ``torch.ops.skyrim_hip.agg_update``.
  Aggregation has no CPU fallback;
* the requests: ``parse_request`` reads ``channel:stat:window``, ``plan`` / ``check_request`` resolve a list of them against a model's
  channels and step into slots, ops and the window plan (which lead times open and close which window);
* the drivers: ``LeadAggregator`` (what ``ensemble.run`` calls at every lead time with ``aggregates=[...]``), ``TruthAggregator`` (the
  hook that lets ``verify.LeadScorer`` score an aggregate against the same aggregate of the truth), ``aggregate_model``
  (``GlobalModel.aggregate_forecast``) and ``aggregate_prediction`` for forecasts that are already on disk.
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

MAX_MEMBERS, MAX_OPS = 64, 16                                   # include/skyrim_agg.h SKAGG_MAX_*
MAX, MIN, SUM, COUNT_ABOVE = 1, 2, 3, 4                         # SKAGG_MAX ...
FIRST, LAST = 1, 2                                              # SKAGG_FIRST, SKAGG_LAST
KINDS = (MAX, MIN, SUM, COUNT_ABOVE)
STATS = ("max", "min", "mean", "sum", "hours_above@<threshold>", "when_max", "when_min")
_P = ctypes.c_void_p


class OpDesc(ctypes.Structure):
    """skagg_op (``in_`` is the header's ``in``)."""
    _fields_ = [("kind", ctypes.c_int32), ("in_", ctypes.c_int32), ("out", ctypes.c_int32), ("when", ctypes.c_int32),
                ("phase", ctypes.c_int32), ("thr", ctypes.c_float), ("scale", ctypes.c_float)]


class AggDesc(ctypes.Structure):
    """skagg_desc."""
    _fields_ = [("members", _P), ("M", ctypes.c_int), ("member_align", ctypes.c_int), ("C", ctypes.c_int), ("H", ctypes.c_int),
                ("W", ctypes.c_int), ("D", ctypes.c_int), ("acc", _P), ("member_stride", ctypes.c_size_t), ("stamp", ctypes.c_float),
                ("n_ops", ctypes.c_int), ("ops", OpDesc * MAX_OPS)]


SPEC = native.Spec("skyrim_agg", "SKYRIM_AGG_LIB", "skagg", 1, {                # include/skyrim_agg.h SKAGG_ABI_VERSION
    "skagg_abi_version": (ctypes.c_int, []),
    "skagg_update": (ctypes.c_int, [ctypes.POINTER(AggDesc), _P]),
}, " -- time-window aggregates have no torch fallback")
EXPORTS, ABI_VERSION = SPEC.exports, SPEC.abi

_lib = None


def load_library() -> ctypes.CDLL:
    """libskyrim_agg.so (built in-tree by ``__graft_entry__.build()`` / ``make -C skyrim_amd/csrc``)."""
    global _lib
    if _lib is None:
        _lib = native.load(SPEC)
    return _lib


# ---- the program ------------------------------------------------------------------------------------------------------------------------- #
@dataclass(frozen=True)
class Op:
    """One op of a call: ``channel`` is the input channel (the header's ``in``), ``out`` the slot of the value, ``when`` the slot of the
    stamp of a MAX / MIN (-1: none), ``phase`` the FIRST / LAST bits, ``thr`` the threshold of COUNT_ABOVE, ``scale`` the factor SUM and
    COUNT_ABOVE apply with LAST."""
    kind: int
    channel: int
    out: int
    when: int = -1
    phase: int = 0
    thr: float = 0.0
    scale: float = 1.0


def encode(ops) -> tuple:
    """(ints, floats): the flat form ``torch.ops.skyrim_hip.agg_update`` takes.  Per op five ints (kind, channel, out, when, phase) and two
    floats (thr, scale)."""
    ints, floats = [], []
    for op in ops:
        ints += [int(op.kind), int(op.channel), int(op.out), int(op.when), int(op.phase)]
        floats += [float(op.thr), float(op.scale)]
    return ints, floats


def decode(ints, floats) -> list:
    ints, floats = list(ints), list(floats)
    if len(ints) % 5 or len(floats) * 5 != len(ints) * 2:
        raise ValueError("agg_update: a program holds five ints and two floats per op")
    ops = []
    for k in range(len(ints) // 5):
        kind = ints[5 * k]
        if kind not in KINDS:
            raise ValueError(f"agg_update: unknown op kind {kind}")
        ops.append(Op(kind, *ints[5 * k + 1:5 * k + 5], float(floats[2 * k]), float(floats[2 * k + 1])))
    return ops


def describe(ops, M, C, H, W, D, member_stride, stamp=0.0, member_align=16) -> AggDesc:
    """The descriptor of a call, its pointers still NULL."""
    d = AggDesc()
    program.fill_head(d, M, C, H, W, D, member_stride, member_align)
    d.stamp = stamp
    ops = list(ops)
    d.n_ops = len(ops)
    for k, op in enumerate(ops[:MAX_OPS]):
        o = d.ops[k]
        o.kind, o.in_, o.out, o.when, o.phase, o.thr, o.scale = op.kind, op.channel, op.out, op.when, op.phase, op.thr, op.scale
    return d


def run(members, table, ops, acc, stamp) -> None:
    """One ``skagg_update``: fold the M ``members`` (equal-shaped contiguous float32 (C, H, W) device tensors of one lead time; ``table`` =
    ``ensemble.member_table(members)``) into ``acc``, float32 (M, D, H, W), by the ops ``ops``; ``stamp``: the lead time in hours.
    Queued on torch's current stream.  As in ``derived.run``, the contents of ``table`` are trusted to be the addresses of ``members``."""
    ops = list(ops)
    M, dev, align, C, H, W, D, pa = program.bind("agg_update", members, table, ops, acc, "agg_update: acc", MAX_MEMBERS, MAX_OPS)
    d = describe(ops, M, C, H, W, D, D * H * W, float(stamp), align)
    d.members, d.acc = table.data_ptr(), pa
    lib = load_library()
    program.launch(lib, lib.skagg_update, d, dev)


# ---- requests ---------------------------------------------------------------------------------------------------------------------------- #
@dataclass(frozen=True)
class Request:
    """``channel:stat:window``.  ``stat``: max, min, mean, sum, hours_above@<threshold>, when_max, when_min; ``window``: ``<N>h`` or ``all``."""
    channel: str
    stat: str
    window: str

    @property
    def name(self) -> str:
        """The aggregate's channel name: the request with ``:`` replaced by ``_``."""
        return f"{self.channel}_{self.stat}_{self.window}"


def _threshold(stat: str) -> float:
    """The threshold of ``hours_above@<threshold>``, rounded to float32 as the kernel compares it."""
    try:
        v = float(stat.split("@", 1)[1])
    except ValueError:
        v = math.nan
    if math.isnan(v):
        raise ValueError(f"aggregates: {stat!r}: hours_above@<threshold> needs a number (inf and -inf are allowed)")
    return float(np.float32(v))


def parse_request(req) -> Request:
    """A ``Request`` from ``"channel:stat:window"`` or from an object with these three fields; ValueError when it is not one."""
    if isinstance(req, str):
        parts = req.split(":")
        if len(parts) != 3:
            raise ValueError(f"aggregates: {req!r} is not channel:stat:window (for example ws10m:max:24h)")
        req = Request(*(p.strip() for p in parts))
    elif all(hasattr(req, a) for a in ("channel", "stat", "window")):
        req = Request(str(req.channel), str(req.stat), str(req.window))
    else:
        raise ValueError(f"aggregates: a request is a string channel:stat:window or has the fields channel, stat, window, not {type(req).__name__}")
    if not req.channel:
        raise ValueError(f"aggregates: {req}: the channel is empty")
    if req.stat.startswith("hours_above@"):
        _threshold(req.stat)
    elif req.stat not in ("max", "min", "mean", "sum", "when_max", "when_min"):
        raise ValueError(f"aggregates: unknown statistic {req.stat!r}; known are {', '.join(STATS)}")
    if req.window != "all" and not re.fullmatch(r"[1-9]\d*h", req.window):
        raise ValueError(f"aggregates: window {req.window!r} is neither <N>h (N a positive whole number of hours) nor all")
    return req


def step_hours(time_step) -> float:
    h = time_step.total_seconds() / 3600 if isinstance(time_step, datetime.timedelta) else float(time_step)
    if not h > 0:
        raise ValueError("aggregates: the model's time step must be positive")
    return h


def group_ops(requests, channel_of, length: int, dt: float, slot0: int = 0, hidden0: int | None = None) -> tuple:
    """(fields, ops, hidden): the requests of ONE window length (``length`` steps of ``dt`` hours) as slots ``slot0 ..`` in the order of
    the requests and ops with phase 0.  ``when_*`` runs a MAX / MIN op whose value slot is that of the ``max`` / ``min`` request of the same
    channel when there is one; otherwise the value goes to a hidden slot, counted from ``hidden0`` (default: right after the fields)."""
    requests = list(requests)
    fields = [r.name for r in requests]
    slot = {r.name: slot0 + k for k, r in enumerate(requests)}
    hidden_at = slot0 + len(requests) if hidden0 is None else hidden0
    hidden = 0
    ops, extreme = [], {}                                          # extreme[(kind, channel)] = index of its op
    for r in requests:
        c = channel_of(r.channel)
        if r.stat in ("max", "min"):
            extreme[(MAX if r.stat == "max" else MIN, r.channel)] = len(ops)
            ops.append(Op(MAX if r.stat == "max" else MIN, c, slot[r.name]))
        elif r.stat in ("mean", "sum"):
            ops.append(Op(SUM, c, slot[r.name], scale=float(np.float32(1.0 / length)) if r.stat == "mean" else 1.0))
        elif r.stat.startswith("hours_above@"):
            ops.append(Op(COUNT_ABOVE, c, slot[r.name], thr=_threshold(r.stat), scale=float(np.float32(dt))))
    for r in requests:
        if r.stat in ("when_max", "when_min"):
            key = (MAX if r.stat == "when_max" else MIN, r.channel)
            if key not in extreme:
                extreme[key] = len(ops)
                ops.append(Op(key[0], channel_of(r.channel), hidden_at + hidden))
                hidden += 1
            ops[extreme[key]] = replace(ops[extreme[key]], when=slot[r.name])
    return fields, ops, hidden


@dataclass
class Group:
    """The requests of one window length.  ``label``: ``"24h"`` or ``"all"``; ``length``: steps of a window; ``n_windows``: the complete
    windows of the rollout; ``fields``: the aggregates' names, slot ``slot0 + k`` is fields[k]; ``ops``: the group's ops, phase 0."""
    label: str
    length: int
    n_windows: int
    requests: list
    fields: list
    slot0: int
    ops: list

    @property
    def slots(self) -> list:
        return list(range(self.slot0, self.slot0 + len(self.fields)))

    def steps(self, w: int) -> range:
        """The step numbers of window w: the valid times t0 + (w N, (w + 1) N]."""
        return range(w * self.length + 1, (w + 1) * self.length + 1)


@dataclass
class Plan:
    """A resolved list of requests.  ``names``: the channels the ops' inputs index; ``D``: slots per member (the groups' fields, then the
    hidden value slots of ``when_*``); ``incomplete[label]`` = (first, last) step of a trailing window the rollout does not complete."""
    names: list
    requests: list
    groups: list
    D: int
    dt: float
    n_steps: int
    incomplete: dict = field(default_factory=dict)

    def ops_at(self, k: int) -> list:
        """The ops of step k (1 .. n_steps) with their phases; none at step 0 and in a window that stays incomplete."""
        out = []
        for g in self.groups:
            if 1 <= k <= g.n_windows * g.length:
                pos = (k - 1) % g.length
                phase = (FIRST if pos == 0 else 0) | (LAST if pos == g.length - 1 else 0)
                out += [replace(op, phase=phase) for op in g.ops]
        return out

    def closing(self, k: int) -> list:
        """(group, window number) of every window that step k closes."""
        return [(g, k // g.length - 1) for g in self.groups if 1 <= k <= g.n_windows * g.length and k % g.length == 0]

    def group(self, label: str) -> Group:
        return next(g for g in self.groups if g.label == label)


def plan(names, requests, time_step, n_steps: int) -> Plan:
    """Resolve ``requests`` against the channels ``names`` for a rollout of ``n_steps`` steps of ``time_step`` (a timedelta, or hours).
    Every refusal is a ValueError before the device is touched."""
    names = list(names)
    dt = step_hours(time_step)
    reqs = [parse_request(r) for r in (requests or [])]
    if not reqs:
        raise ValueError("aggregates: at least one request")
    seen = set()
    for r in reqs:
        if r.name in seen:
            raise ValueError(f"aggregates: {r.name!r} is requested twice")
        seen.add(r.name)
        if r.channel not in names:
            raise ValueError(f"aggregates: channel {r.channel!r} is not an output channel of this model or one of the derived fields "
                             "named in derived=")
    by_label: dict = {}
    for r in reqs:
        by_label.setdefault(r.window, []).append(r)
    lengths = {}
    for label in by_label:
        if label == "all":
            length = int(n_steps)
        else:
            steps = int(label[:-1]) / dt
            if abs(steps - round(steps)) > 1e-9 or round(steps) < 1:
                raise ValueError(f"aggregates: a window of {label} is not a positive multiple of the model's time step of {dt:g} h")
            length = int(round(steps))
        if length < 1 or length > n_steps:
            raise ValueError(f"aggregates: the first window of {label!r} ({length} steps of {dt:g} h) does not fit in n_steps = {n_steps}")
        lengths[label] = length
    groups, incomplete, slot0 = [], {}, 0
    visible = len(reqs)
    hidden0 = visible
    for label, rs in by_label.items():
        length = lengths[label]
        fields, ops, hidden = group_ops(rs, names.index, length, dt, slot0, hidden0)
        groups.append(Group(label, length, n_steps // length, rs, fields, slot0, ops))
        slot0 += len(rs)
        hidden0 += hidden
        if n_steps % length:
            incomplete[label] = (n_steps // length * length + 1, int(n_steps))
    if sum(len(g.ops) for g in groups) > MAX_OPS:
        raise ValueError(f"aggregates: {sum(len(g.ops) for g in groups)} ops for {[r.name for r in reqs]}; one call holds {MAX_OPS}")
    return Plan(names, reqs, groups, hidden0, dt, int(n_steps), incomplete)


def check_request(names, requests, time_step, n_steps, lat, lon, n_members: int = 1) -> Plan:
    """Every refusal that needs no device; returns the plan."""
    if _world_size() > 1:
        raise NotImplementedError("aggregates are made on one GPU from members that all lie there; members sharded over the ranks of a "
                                  "process group are out of scope (DESIGN.md 24)")
    if not 1 <= int(n_members) <= MAX_MEMBERS:
        raise ValueError(f"n_members = {n_members}: aggregates are made for 1 to {MAX_MEMBERS} members (SKAGG_MAX_MEMBERS)")
    if isinstance(requests, (str, Request)) or not hasattr(requests, "__iter__"):
        raise ValueError("aggregates: a list of requests channel:stat:window")
    out = plan(names, list(requests), time_step, n_steps)
    if out.D * len(lat) * len(lon) > 2 ** 30:
        raise ValueError(f"aggregates: {out.D} slots of {len(lat)} x {len(lon)} points exceed 2^30 elements per member")
    return out


# ---- the drivers ------------------------------------------------------------------------------------------------------------------------- #
@dataclass
class Closed:
    """A window group that closed: ``label``; ``fields`` and ``slots``: its aggregates and their slots in the accumulator; ``states`` /
    ``table``: M (len(fields), H, W) views of the accumulator and their ``ensemble.member_table``, ready for ``ensemble.stats`` and
    ``LeadScorer.add`` until the group's next window opens; ``start`` / ``end``: the window is (start, end]; ``times``: its valid times."""
    label: str
    fields: list
    slots: list
    states: list
    table: object
    window: int
    start: datetime.datetime
    end: datetime.datetime
    times: list


class LeadAggregator:
    """Folds one lead time after the other into its own (M, D, H, W) accumulator.  ``names``: the forecast's channels in the order of its
    (C, H, W) states; ``derived``: the names of the planes of a ``LeadDeriver``'s buffer, which requests may name as well; ``n_steps``: the
    length of the rollout, which fixes the window ``all`` and the windows that stay incomplete."""

    def __init__(self, names, lat, lon, n_members, requests, t0, time_step, device="cuda:0", n_steps=None, derived=()):
        if n_steps is None:
            raise ValueError("LeadAggregator needs n_steps: the window plan depends on the length of the rollout")
        self.names, self.derived, self.M = list(names), list(derived), int(n_members)
        self.plan = check_request(self.names + self.derived, requests, time_step, n_steps, lat, lon, n_members)
        self.lat, self.lon, self.device = np.asarray(lat, np.float64), np.asarray(lon, np.float64), device
        self.t0, self.step = t0, datetime.timedelta(hours=self.plan.dt)
        self._dev = None

    @property
    def incomplete(self) -> dict:
        return self.plan.incomplete

    def _buffers(self):
        if self._dev is None:
            import torch
            from .ensemble import member_table
            dev = torch.device(self.device)
            acc = torch.empty((self.M, self.plan.D, self.lat.size, self.lon.size), dtype=torch.float32, device=dev)
            views = {}
            for g in self.plan.groups:
                states = [acc[m, g.slot0:g.slot0 + len(g.fields)] for m in range(self.M)]
                views[g.label] = (states, member_table(states))
            self._dev = dict(acc=acc, views=views)
        return self._dev

    def add(self, k, time, states, table=None, derived=None) -> list:
        """Fold step k (valid time ``time``) of the M device states (C, H, W): ONE ``agg_update`` for the ops that read the states, and one
        more for those that read ``derived`` = (derived_states, derived_table) of ``LeadDeriver.add``, when requests name derived fields.
        Returns the ``Closed`` groups whose window this step closes."""
        from .ensemble import member_table
        if len(states) != self.M:
            raise ValueError(f"{len(states)} states for an aggregator of {self.M} members")
        ops = self.plan.ops_at(k)
        if not ops:
            return []
        b = self._buffers()
        stamp = (time - self.t0).total_seconds() / 3600
        C = len(self.names)
        own = [op for op in ops if op.channel < C]
        other = [replace(op, channel=op.channel - C) for op in ops if op.channel >= C]
        if own:
            run(states, member_table(states) if table is None else table, own, b["acc"], stamp)
        if other:
            if derived is None:
                raise ValueError("requests name derived fields: add() needs derived=(states, table) of the deriver")
            run(derived[0], derived[1], other, b["acc"], stamp)
        out = []
        for g, w in self.plan.closing(k):
            st, tb = b["views"][g.label]
            steps = g.steps(w)
            out.append(Closed(g.label, list(g.fields), g.slots, st, tb, w, self.t0 + (steps[0] - 1) * self.step, self.t0 + steps[-1] * self.step,
                              [self.t0 + s * self.step for s in steps]))
        return out


class TruthAggregator:
    """The hook ``verify.LeadScorer(adapt=...)`` calls so that a truth (or climatology) of instantaneous fields scores the aggregates of
    ONE window group: before the scorer's ``add`` the caller names the valid times of the closing window (``window``); the truth at each
    of them is uploaded and folded by the same kernel with M = 1.  ``requests``: the group's requests; ``inner``: a
    ``derived.TruthDeriver`` for the requests that name derived fields.  An aggregate whose channel the truth lacks is not offered to
    the scorer; ``dropped`` names it.  A truth that lacks one of the window's times raises what ``_Fields.at`` raises."""

    def __init__(self, requests, lat, lon, t0, time_step, device="cuda:0", inner=None):
        self.requests = [parse_request(r) for r in requests]
        if len({r.window for r in self.requests}) != 1:
            raise ValueError("TruthAggregator: the requests of one window group")
        self.lat, self.lon, self.t0, self.dt, self.device, self.inner = lat, lon, t0, step_hours(time_step), device, inner
        self.dropped: dict = {}
        self.times: list = []
        self._cache: dict = {}

    def window(self, times) -> None:
        """The valid times of the window the next ``upload`` aggregates."""
        self.times = list(times)

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
        """Fill the rows ``idx_dev`` of ``dst`` with the aggregates ``scored`` of the truth over the window set by ``window``."""
        import torch
        from .ensemble import member_table
        if not self.times:
            raise ValueError("TruthAggregator: window(times) names the valid times before the scorer's add")
        length = len(self.times)
        key = (id(fields), tuple(scored), length)
        hit = self._cache.get(key)
        if hit is None:
            reqs = [r for r in self.requests if r.name in scored]
            reqs.sort(key=lambda r: list(scored).index(r.name))
            have = set(fields.names)
            raw = [c for c in dict.fromkeys(r.channel for r in reqs) if c in have]
            der = [c for c in dict.fromkeys(r.channel for r in reqs) if c not in have]
            inputs = raw + der
            _, ops, hidden = group_ops(reqs, inputs.index, length, self.dt)
            dev = torch.device(self.device)
            H, W = len(self.lat), len(self.lon)
            state = torch.zeros((len(inputs), H, W), dtype=torch.float32, device=dev)
            acc = torch.empty((1, len(reqs) + hidden, H, W), dtype=torch.float32, device=dev)
            der_idx = torch.arange(len(raw), len(inputs), device=dev)
            hit = (raw, der, ops, state, member_table([state]), acc, der_idx, len(reqs), fields)      # (holds ``fields``: its id stays taken)
            self._cache[key] = hit
        raw, der, ops, state, table, acc, der_idx, n, _ = hit
        for k, t in enumerate(self.times):
            if raw:
                state[:len(raw)] = torch.from_numpy(fields.at(t, raw)).to(state.device)
            if der:
                self.inner.upload(fields, t, der, state, der_idx)
            phase = (FIRST if k == 0 else 0) | (LAST if k == length - 1 else 0)
            run([state], table, [replace(op, phase=phase) for op in ops], acc, (t - self.t0).total_seconds() / 3600)
        dst[idx_dev] = acc[0, :n]


@dataclass
class AggregatedProducts:
    """``EnsembleForecast.aggregated[label]``: the attributes of the raw products for the aggregates of one window group.  The arrays'
    ``time`` is the end of each window, their coordinate ``window_start`` its start (the window is (start, end]).  ``incomplete``: the
    (first, last) steps of a trailing window the rollout did not complete, or None; ``dropped``: aggregates that could not be scored."""
    label: str
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
    incomplete: object = None
    points: object = None        # points.PointForecast of the group's fields with ``points=...``
    extremes: object = None      # extremes.Extremes of the group's fields with ``extremes={...}``, the slice chosen by each window's end


def _labelled(arr, fields, ends, starts, lat, lon):
    from .labeled import DataArray
    return DataArray(arr, ["time", "channel", "lat", "lon"], dict(time=ends, channel=list(fields), lat=lat, lon=lon, window_start=starts))


def _fold_sequence(names, lat, lon, requests, t0, time_step, n_steps, device, drive, derived=None):
    """The aggregates of ONE forecast (M = 1): ``drive(each)`` calls ``each(k, time, state)`` with the (C, H, W) device state of step
    k = 0 .. n_steps.  Returns {label: DataArray(time = window ends, channel, lat, lon)}, each with the dict of incomplete windows."""
    dnames = list(derived or [])
    agg = LeadAggregator(names, lat, lon, 1, requests, t0, time_step, device=device, n_steps=n_steps, derived=dnames)
    deriver = None
    if dnames:
        from .derived import LeadDeriver
        deriver = LeadDeriver(names, lat, lon, 1, dnames, device=device)
    host = {g.label: ([], [], []) for g in agg.plan.groups}

    def each(k, time, state):
        if k == 0:
            return                                             # the initial state belongs to no window
        for c in agg.add(k, t0 + k * agg.step, [state], None, deriver.add([state]) if deriver is not None else None):
            arrs, ends, starts = host[c.label]
            arrs.append(c.states[0].cpu().numpy())
            ends.append(c.end)
            starts.append(c.start)
    drive(each)
    lat, lon = np.asarray(lat), np.asarray(lon)
    out = {g.label: _labelled(np.stack(host[g.label][0]), g.fields, host[g.label][1], host[g.label][2], lat, lon) for g in agg.plan.groups}
    incomplete = dict(agg.incomplete)
    for da in out.values():
        da.incomplete = incomplete
    return out


def _save(out: dict, model_name: str, source: str, save_config):
    from .common import save_config_with_id, save_forecast
    from .labeled import DataArray
    cfg = save_config_with_id(save_config)
    zarr = (cfg.get("file_type") or "netcdf") == "zarr"
    for label, da in out.items():
        times = list(da.time.values.astype("datetime64[s]").astype(datetime.datetime))
        plain = DataArray(da.values, da.dims, {k: v for k, v in da._coords.items() if k != "window_start"})
        name = f"{model_name}-agg{label}"
        pcfg = dict(cfg, forecast_id=f"{cfg['forecast_id']}/{name}") if zarr else cfg
        start = np.asarray(da._coords["window_start"]).astype("datetime64[s]").astype(datetime.datetime)[0]
        da.path = save_forecast(plain, name, start, times[-1], source, config=pcfg)


def aggregate_model(gm, start_time: datetime.datetime, n_steps: int, aggregates, derived=None, save: bool = False, save_config: dict | None = None):
    """``GlobalModel.aggregate_forecast`` (core/models/base.py has the user-facing description)."""
    model = gm.model
    names = list(model.out_channel_names)
    if n_steps < 0:
        raise ValueError("n_steps >= 0")
    if derived is not None:
        from . import derived as deriving
        deriving.check_request(names, list(derived), model.grid.lat, model.grid.lon, 1)
    check_request(names + list(derived or []), aggregates, model.time_step, n_steps, model.grid.lat, model.grid.lon, 1)      # before the device
    require_gpu(model.device, "aggregate_forecast aggregates with HIP kernels where the forecast lies: the model must be on a GPU")
    out = _fold_sequence(names, model.grid.lat, model.grid.lon, aggregates, start_time, model.time_step, n_steps, model.device,
                         lambda each: run_model(gm, start_time, n_steps, each), derived)
    if save:
        _save(out, gm.model_name, gm.source_label, save_config)
    return out


def aggregate_prediction(pred, aggregates, derived=None, device="cuda:0"):
    """Aggregates of a forecast that already exists: a ``GlobalPrediction``, a (time, channel, lat, lon) DataArray, a saved netCDF file or
    zarr store, or a list of such files (their time entries in order, duplicates of a valid time used once).  The first time entry is the
    initial state; the entries must be equally spaced.  Each entry is uploaded on its own and goes through the same kernel as
    ``aggregate_forecast``.  Returns {window label: DataArray(time = window ends, channel = aggregates, lat, lon)}."""
    saved = open_saved(pred, "aggregate_prediction")
    names, lat, lon, entries = saved.names, saved.lat, saved.lon, saved.entries
    if len(entries) < 2:
        raise ValueError("aggregate_prediction: a forecast of at least one step (two time entries)")
    step = entries[1][0] - entries[0][0]
    if any(b[0] - a[0] != step for a, b in zip(entries, entries[1:])) or step <= datetime.timedelta(0):
        raise ValueError("aggregate_prediction: the time entries must be equally spaced and ascending")
    n_steps = len(entries) - 1
    if derived is not None:
        from . import derived as deriving
        deriving.check_request(names, list(derived), lat, lon, 1)
    check_request(names + list(derived or []), aggregates, step, n_steps, lat, lon, 1)
    require_gpu(device, "aggregate_prediction aggregates with HIP kernels: it needs a GPU", present=True)

    def drive(each):
        for k, time, state in saved.states(device):
            each(k, time, state)
    return _fold_sequence(names, lat, lon, aggregates, entries[0][0], step, n_steps, device, drive, derived)
