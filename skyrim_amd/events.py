"""Event verification on the device (include/skyrim_event.h): for threshold events "x > thr" of a forecast or an
ensemble against a truth state, the Brier score and its decomposition, the reliability curve, the ROC and its area, the 2 x 2
contingency scores of a deterministic forecast and the fractions skill score over neighbourhoods.

Three layers:

* the binding of libskyrim_event.so (``SPEC``, ``load_library``, ``run``); the same call is ``torch.ops.skyrim_hip.event_counts``.  The
  kernels deliver exact integers only: the per-row joint counts of (observed, members above) and the neighbourhood row sums;
* ``windows`` -- the neighbourhood of a radius in km as rows and columns of a global grid -- and ``EventScores``, the labelled scores
  the host forms in float64 from those integers, area-weighted with ``verify.area_weights`` as the rank histogram is;
* ``LeadEvents`` -- what ``verify.LeadScorer`` calls at every lead time, after the scores and on the same states and truth.
"""
from __future__ import annotations

import ctypes
import math

import numpy as np
import torch

from . import native
from .members import member_count, member_set

MAX_MEMBERS, MAX_CHANNELS, MAX_THRESHOLDS, MAX_SCALES, MAX_WIDTH = 64, 16, 4, 4, 8192       # include/skyrim_event.h SKEVENT_MAX_*
_P = ctypes.c_void_p


class EventDesc(ctypes.Structure):
    """skevent_desc."""
    _fields_ = [("members", _P), ("M", ctypes.c_int), ("member_align", ctypes.c_int), ("truth", _P),
                ("C", ctypes.c_int), ("H", ctypes.c_int), ("W", ctypes.c_int), ("n_events", ctypes.c_int),
                ("channel", ctypes.c_int * MAX_CHANNELS), ("n_thr", ctypes.c_int * MAX_CHANNELS),
                ("thr", (ctypes.c_float * MAX_THRESHOLDS) * MAX_CHANNELS), ("counts", _P), ("n_scales", ctypes.c_int),
                ("hy", ctypes.c_int * MAX_SCALES), ("hx", _P), ("sums", _P), ("workspace", _P), ("workspace_bytes", ctypes.c_size_t)]


SPEC = native.Spec("skyrim_event", "SKYRIM_EVENT_LIB", "skevent", 1, {          # include/skyrim_event.h SKEVENT_ABI_VERSION
    "skevent_abi_version": (ctypes.c_int, []),
    "skevent_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "skevent_run": (ctypes.c_int, [ctypes.POINTER(EventDesc), _P]),
}, " -- event counts have no torch fallback")
EXPORTS, ABI_VERSION = SPEC.exports, SPEC.abi

_lib = None


def load_library() -> ctypes.CDLL:
    """libskyrim_event.so (built in-tree by ``__graft_entry__.build()`` / ``make -C skyrim_amd/csrc``)."""
    global _lib
    if _lib is None:
        _lib = native.load(SPEC)
    return _lib


def run(members, table: torch.Tensor, truth: torch.Tensor, channels, thresholds, counts: torch.Tensor, hy=(), hx=None, sums=None,
        workspace=None) -> None:
    """One ``skevent_run``: the M ``members`` (equal-shaped contiguous float32 (C, H, W) device tensors; ``table`` =
    ``ensemble.member_table(members)``) against ``truth`` for the event channels ``channels`` (indices, any order) with
    ``thresholds[e]`` (1 to 4 values each).  ``counts``: int32 (E, 4, H, 2, M + 1); entries of thresholds a channel does not have are not
    written.  Scales: ``hy`` (rows, one int per scale), ``hx`` int32 (S, H) on the device, ``sums`` int64 (E, 4, S, H, 3) and ``workspace``
    uint8 of E * 4 * 2 * H * W bytes, which holds the k and o planes afterwards.  Queued on torch's current stream.

    As in ``verify.score`` the CONTENTS of ``table`` are trusted to be the addresses of ``members`` in order."""
    E, S = len(channels), len(hy)
    member_count(members, "event_counts", MAX_MEMBERS)
    if truth.dim() != 3:
        raise ValueError("event_counts: states are (C, H, W)")
    C, H, W = truth.shape
    if E > MAX_CHANNELS or len(thresholds) != E or S > MAX_SCALES:
        raise ValueError(f"event_counts: at most {MAX_CHANNELS} event channels, one list of thresholds each, and {MAX_SCALES} scales")
    d = EventDesc()
    M, dev, align = member_set(members, table, "event_counts", MAX_MEMBERS, ndim=None, same="numel", dev=truth.device)
    if members[0].numel() != truth.numel():
        raise ValueError(f"event_counts: a member holds {members[0].numel()} elements, the truth {truth.numel()}")
    d.members, d.M, d.member_align, d.truth = table.data_ptr(), M, align, native.tensor_ptr(truth, "event_counts: truth", torch.float32, dev)
    d.C, d.H, d.W, d.n_events, d.n_scales = C, H, W, E, S
    for e, (ch, thr) in enumerate(zip(channels, thresholds)):
        if not 0 <= int(ch) < C or not 1 <= len(thr) <= MAX_THRESHOLDS or any(math.isnan(float(v)) for v in thr):
            raise ValueError(f"event_counts: channel {ch} with thresholds {list(thr)}: a channel of the states and 1 to {MAX_THRESHOLDS} numbers")
        d.channel[e], d.n_thr[e] = int(ch), len(thr)
        for k, v in enumerate(thr):
            d.thr[e][k] = float(v)
    d.counts = native.tensor_ptr(counts, "event_counts: counts", torch.int32, dev)
    if counts.numel() != E * MAX_THRESHOLDS * H * 2 * (M + 1):
        raise ValueError(f"event_counts: counts must hold E * {MAX_THRESHOLDS} * H * 2 * (M + 1) = {E * MAX_THRESHOLDS * H * 2 * (M + 1)} int32")
    lib = load_library()
    if S:
        for s, v in enumerate(hy):
            if int(v) < 0:
                raise ValueError("event_counts: a half-height is a number of rows >= 0")
            d.hy[s] = min(int(v), 2 ** 31 - 1)
        d.hx = native.tensor_ptr(hx, "event_counts: hx", torch.int32, dev)
        d.sums = native.tensor_ptr(sums, "event_counts: sums", torch.int64, dev)
        if hx.numel() != S * H or sums.numel() != E * MAX_THRESHOLDS * S * H * 3:
            raise ValueError(f"event_counts: hx must hold S * H int32 and sums E * {MAX_THRESHOLDS} * S * H * 3 int64")
        need = lib.skevent_workspace_bytes(E, H, W, S)
        d.workspace, d.workspace_bytes = native.tensor_ptr(workspace, "event_counts: workspace", torch.uint8, dev), workspace.numel()
        if E and (need == 0 or d.workspace_bytes < need):
            raise ValueError(f"event_counts: the workspace holds {workspace.numel()} bytes, {need} are needed"
                             if need else f"event_counts: neighbourhoods need W <= {MAX_WIDTH}")
    with torch.cuda.device(dev):
        native.check(lib.skevent_run(ctypes.byref(d), native.stream(dev)), "skevent_run", lib)


# ---- the request ---------------------------------------------------------------------------------------------------------------------- #
def check_request(names, events, neighbourhoods_km=(), n_members: int = 1, what: str = "an output channel of this model") -> tuple[dict, list]:
    """The refusals that need no device; returns ({channel: [float32 thresholds]}, [radii in km]) normalised."""
    if not isinstance(events, dict) or not events:
        raise ValueError("events: a dict {channel: [thresholds]} with at least one channel")
    if not 1 <= int(n_members) <= MAX_MEMBERS:
        raise ValueError(f"n_members = {n_members}: events of 1 to {MAX_MEMBERS} members can be counted (SKEVENT_MAX_MEMBERS)")
    if len(events) > MAX_CHANNELS:
        raise ValueError(f"events: {len(events)} event channels; at most {MAX_CHANNELS} in one request (SKEVENT_MAX_CHANNELS)")
    names, out = list(names), {}
    for ch, vals in events.items():
        if ch not in names:
            raise ValueError(f"events: channel {ch!r} is not {what}")
        vals = [vals] if np.isscalar(vals) else list(vals)
        if not 1 <= len(vals) <= MAX_THRESHOLDS:
            raise ValueError(f"events[{ch!r}]: 1 to {MAX_THRESHOLDS} thresholds per channel, got {len(vals)}")
        out[ch] = [float(np.float32(v)) for v in vals]
        if any(math.isnan(v) for v in out[ch]):
            raise ValueError(f"events[{ch!r}]: a threshold is a number, not NaN")
    radii = [float(r) for r in (neighbourhoods_km if neighbourhoods_km is not None else ())]
    if len(radii) > MAX_SCALES:
        raise ValueError(f"neighbourhoods_km: {len(radii)} scales; at most {MAX_SCALES} (SKEVENT_MAX_SCALES)")
    if any(not (r >= 0 and math.isfinite(r)) for r in radii):
        raise ValueError(f"neighbourhoods_km: radii are finite and not negative, got {radii}")
    return out, radii


def parse_event(text: str) -> tuple[str, list]:
    """``ws10m:15,25`` of the command line -> ("ws10m", [15.0, 25.0])."""
    name, sep, vals = text.partition(":")
    try:
        thr = [float(v) for v in vals.split(",")] if sep else []
    except ValueError:
        thr = []
    if not name or not thr:
        raise ValueError(f"--event {text!r}: expected NAME:THRESHOLD[,THRESHOLD...], such as ws10m:15,25")
    return name, thr


# ---- neighbourhoods ------------------------------------------------------------------------------------------------------------------- #
def windows(lat, lon, radius_km: float) -> tuple[int, np.ndarray]:
    """The neighbourhood of ``radius_km`` on a global grid as (hy, hx[H] int32): hy = floor(R / (a dphi)) rows either side and, in row
    j, hx_j = floor(R / (a cos(phi_j) dlambda)) columns either side, clamped to H - 1 and (W - 1) // 2 (towards the poles a window
    becomes the whole latitude circle, never more).  a = ``tracks.EARTH_RADIUS_KM``; radius 0 is the point itself.  Needs a uniformly
    spaced latitude axis and a uniformly spaced longitude axis that closes the circle."""
    from .tracks import EARTH_RADIUS_KM
    lat, lon, R = np.asarray(lat, np.float64), np.asarray(lon, np.float64), float(radius_km)
    if not (R >= 0 and math.isfinite(R)):
        raise ValueError(f"windows: a radius in km is finite and not negative, got {radius_km}")
    H, W = lat.size, lon.size
    why = None
    if lat.ndim != 1 or lon.ndim != 1 or H < 2 or W < 2 or np.any(np.abs(lat) > 90):
        why = "one-dimensional axes of at least two points"
    else:
        dlat, dlon = np.diff(lat), np.diff(lon)
        if not np.allclose(dlat, dlat[0], rtol=0, atol=1e-6 * abs(dlat[0])) or dlat[0] == 0:
            why = "a uniformly spaced latitude axis"
        elif not np.allclose(dlon, dlon[0], rtol=0, atol=1e-6 * abs(dlon[0])) or abs(abs(dlon[0]) * W - 360.0) > 1e-6 * 360.0:
            why = "a uniformly spaced longitude axis that closes the circle (W * dlon = 360)"
    if why:
        raise ValueError(f"neighbourhoods need {why}: on this grid (a regional regrid target, for one) windows periodic in longitude are "
                         "not defined.  Point-wise event scores (Brier, reliability, ROC, contingency) are still available: leave "
                         "neighbourhoods_km empty")
    dphi, dlam = np.deg2rad(abs(dlat[0])), np.deg2rad(abs(dlon[0]))
    hy = min(int(math.floor(R / (EARTH_RADIUS_KM * dphi))), H - 1)
    cap = (W - 1) // 2
    arc = EARTH_RADIUS_KM * np.cos(np.deg2rad(lat)) * dlam               # km per column in row j
    hx = np.full(H, 0 if R == 0 else cap, np.int64)
    ok = (arc * (cap + 1) > R) & (R > 0)                                            # elsewhere (the poles among them) the clamp holds
    hx[ok] = np.minimum(np.floor(R / arc[ok]), cap).astype(np.int64)
    return hy, hx.astype(np.int32)


def window_points(hy: int, hx, H: int, W: int) -> np.ndarray:
    """n_j: the points in the window of a point of row j (int64 [H]), with the kernel's clamps."""
    j = np.arange(H)
    hy = min(int(hy), H)
    rows = np.minimum(j + hy, H - 1) - np.maximum(j - hy, 0) + 1
    return rows.astype(np.int64) * (2 * np.clip(np.asarray(hx, np.int64), 0, (W - 1) // 2) + 1)


# ---- the scores ----------------------------------------------------------------------------------------------------------------------- #
def _clean(a):                                                  # JSON has no NaN: undefined ratios are written as null
    return [_clean(v) for v in a] if isinstance(a, list) else (a if isinstance(a, int) or math.isfinite(a) else None)


class EventScores:
    """The event scores of ``verify.Scores.events``.  Every score is a DataArray over (time, channel, threshold) -- ``threshold`` counts
    0 .. 3, ``thresholds[channel]`` holds the values, and entries of thresholds a channel does not have are NaN -- made in float64 from

    * ``frequency`` (time, channel, threshold, observed, members): the area-weighted joint frequency of (o, k), which sums to 1, and
    * ``fss_terms`` (time, channel, threshold, scale, term): the area means <(Pf - Po)^2>, <Pf^2>, <Po^2> per neighbourhood,

    next to ``counts``, the exact integers summed over the latitude rows.  For every M: ``base_rate``, ``brier`` and its decomposition
    ``reliability``, ``resolution``, ``uncertainty`` over the M + 1 forecast values k / M (BS = REL - RES + UNC holds exactly with these
    bins), ``reliability_curve`` (dict: ``forecast_probability`` [M + 1], ``observed_frequency`` and ``weight`` with a ``members``
    axis), ``roc`` (..., point, (pofd, pod)) for "at least i members", i = 0 .. M + 1, and ``auc`` by the trapezoid rule.  M > 1:
    ``brier_fair`` = BS - mean of k (M - k) / (M^2 (M - 1)).  M = 1: ``table`` (..., observed, forecast) and ``pod``, ``far``, ``csi``,
    ``ets``, ``frequency_bias``.  With neighbourhoods: ``fss`` (time, channel, threshold, scale).  Undefined ratios are NaN."""

    POINT = ("base_rate", "brier", "reliability", "resolution", "uncertainty", "auc")

    def __init__(self, n_members, times, channels, thresholds, counts, frequency, neighbourhoods_km=(), fss_terms=None):
        from .labeled import DataArray
        M = self.n_members = int(n_members)
        self.times, self.channels = list(times), list(channels)
        self.thresholds = {c: [float(v) for v in thresholds[c]] for c in self.channels}
        self.neighbourhoods_km = [float(r) for r in neighbourhoods_km]
        T, E = len(self.times), len(self.channels)
        coords = dict(time=self.times, channel=self.channels, threshold=np.arange(MAX_THRESHOLDS))
        joint = dict(observed=np.arange(2), members=np.arange(M + 1), **coords)
        dims = ["time", "channel", "threshold"]
        self.counts = DataArray(np.asarray(counts, np.int64).reshape(T, E, MAX_THRESHOLDS, 2, M + 1), dims + ["observed", "members"], joint)
        p = np.asarray(frequency, np.float64).reshape(T, E, MAX_THRESHOLDS, 2, M + 1)
        self.frequency = DataArray(p, dims + ["observed", "members"], joint)
        absent = np.ones((T, E, MAX_THRESHOLDS), bool)                  # thresholds a channel does not have
        for e, c in enumerate(self.channels):
            absent[:, e, :len(self.thresholds[c])] = False

        def put(name, a, extra=(), extra_coords=None):
            a = np.where(absent.reshape(absent.shape + (1,) * (a.ndim - 3)), np.nan, a)
            setattr(self, name, DataArray(a, dims + list(extra), dict(coords, **(extra_coords or {}))))

        p0, p1, f = p[..., 0, :], p[..., 1, :], np.arange(M + 1) / M
        with np.errstate(invalid="ignore", divide="ignore"):
            base = p1.sum(-1)
            n = p0 + p1
            obs = p1 / n                                                # NaN where no point has that k
            put("base_rate", base)
            put("brier", (p0 * f ** 2 + p1 * (f - 1) ** 2).sum(-1))
            put("reliability", np.where(n > 0, n * (f - obs) ** 2, 0.0).sum(-1))
            put("resolution", np.where(n > 0, n * (obs - base[..., None]) ** 2, 0.0).sum(-1))
            put("uncertainty", base * (1 - base))
            self.reliability_curve = dict(forecast_probability=f)
            for name, a in (("observed_frequency", obs), ("weight", n)):
                a = np.where(absent[..., None], np.nan, a)
                self.reliability_curve[name] = DataArray(a, dims + ["members"], dict(coords, members=np.arange(M + 1)))
            # "at least i members", i = 0 .. M + 1: from (1, 1) down to (0, 0)
            tail = lambda q: np.concatenate([np.cumsum(q[..., ::-1], axis=-1)[..., ::-1], np.zeros(q.shape[:-1] + (1,))], axis=-1)  # noqa: E731
            pod, pofd = tail(p1) / base[..., None], tail(p0) / p0.sum(-1)[..., None]
            put("roc", np.stack([pofd, pod], axis=-1), ["point", "rate"], dict(point=np.arange(M + 2), rate=["pofd", "pod"]))
            put("auc", ((pofd[..., :-1] - pofd[..., 1:]) * (pod[..., :-1] + pod[..., 1:]) / 2).sum(-1))
            names = list(self.POINT)
            if M > 1:
                k = np.arange(M + 1)
                put("brier_fair", self.brier.values - (n * (k * (M - k) / (M * M * (M - 1)))).sum(-1))
                names.append("brier_fair")
            else:
                a, b, c = p1[..., 1], p0[..., 1], p1[..., 0]            # hits, false alarms, misses
                put("table", p, ["observed", "forecast"], dict(observed=np.arange(2), forecast=np.arange(2)))
                chance = (a + b) * (a + c)                              # hits of a random forecast with the same margins
                for name, v in (("pod", a / (a + c)), ("far", b / (a + b)), ("csi", a / (a + b + c)),
                                ("ets", (a - chance) / (a + b + c - chance)), ("frequency_bias", (a + b) / (a + c))):
                    put(name, v)
                    names.append(name)
            self.fss_terms = self.fss = None
            if self.neighbourhoods_km:
                scale = dict(scale=np.asarray(self.neighbourhoods_km))
                t = np.asarray(fss_terms, np.float64).reshape(T, E, MAX_THRESHOLDS, len(self.neighbourhoods_km), 3)
                self.fss_terms = DataArray(t, dims + ["scale", "term"], dict(coords, term=["diff2", "pf2", "po2"], **scale))
                put("fss", 1 - t[..., 0] / (t[..., 1] + t[..., 2]), ["scale"], scale)
                names.append("fss")
        self.names = names

    @classmethod
    def from_rows(cls, n_members, times, channels, thresholds, rows, weights, W, neighbourhoods_km=(), sums=None, points=None):
        """From what the kernels deliver: ``rows`` (time, channel, 4, H, 2, M + 1) joint counts per latitude row, ``sums`` (time, channel,
        4, scale, H, 3) neighbourhood row sums, ``points`` (scale, H) the n_j; ``weights``: ``verify.area_weights`` of the H rows."""
        M = int(n_members)
        rows, w = np.asarray(rows, np.int64), np.asarray(weights, np.float64)
        denom = W * w.sum()
        freq = np.einsum("j,tecjok->tecok", w, rows.astype(np.float64)) / denom
        terms = None
        if len(neighbourhoods_km):
            per_row = w[None, :] / (M * np.asarray(points, np.float64)) ** 2                    # (scale, H)
            terms = np.einsum("sj,tecsjq->tecsq", per_row, np.asarray(sums, np.int64).astype(np.float64)) / denom
        return cls(M, times, channels, thresholds, rows.sum(axis=3), freq, neighbourhoods_km, terms)

    def to_doc(self) -> dict:
        doc = dict(channels=self.channels, thresholds=self.thresholds, neighbourhoods_km=self.neighbourhoods_km,
                   counts=self.counts.values.tolist(), frequency=self.frequency.values.tolist(),
                   scores={k: _clean(getattr(self, k).values.tolist()) for k in self.names},
                   roc=_clean(self.roc.values.tolist()),
                   reliability_curve=dict(forecast_probability=self.reliability_curve["forecast_probability"].tolist(),
                                          observed_frequency=_clean(self.reliability_curve["observed_frequency"].values.tolist()),
                                          weight=_clean(self.reliability_curve["weight"].values.tolist())))
        if self.fss_terms is not None:
            doc["fss_terms"] = self.fss_terms.values.tolist()
        return doc

    @classmethod
    def from_doc(cls, doc: dict, n_members: int, times) -> "EventScores":
        return cls(n_members, times, doc["channels"], doc["thresholds"], np.array(doc["counts"], np.int64), np.array(doc["frequency"], np.float64),
                   doc.get("neighbourhoods_km", ()), None if "fss_terms" not in doc else np.array(doc["fss_terms"], np.float64))


# ---- the driver ----------------------------------------------------------------------------------------------------------------------- #
class LeadEvents:
    """Counts the events of one lead time after the other on the device and gathers the integers.  ``names``: the forecast's channels in
    the order of its (C, H, W) states; ``events``: {channel: [thresholds]} among them (``check_request``); ``radii``: the
    neighbourhoods in km, which need the global grid of ``windows``."""

    def __init__(self, names, lat, lon, n_members, events: dict, radii=(), device="cuda:0"):
        self.names, self.M = list(names), int(n_members)
        self.events, self.radii = check_request(self.names, events, radii, self.M, "a channel of the forecast")
        self.channels = list(self.events)
        self.H, self.W = len(lat), len(lon)
        self.device = torch.device(device)
        self.hy, hx = [], []
        for r in self.radii:
            y, x = windows(lat, lon, r)
            self.hy.append(y)
            hx.append(x)
        if self.radii and self.W > MAX_WIDTH:
            raise ValueError(f"neighbourhoods need a grid of at most {MAX_WIDTH} columns (SKEVENT_MAX_WIDTH), this one has {self.W}")
        self.hx = np.stack(hx) if hx else None
        self.points = np.stack([window_points(y, x, self.H, self.W) for y, x in zip(self.hy, hx)]) if hx else None
        self.rows, self.sums = [], []
        self._dev = None

    def add(self, states, table, truth: torch.Tensor) -> None:
        """The M device states (C, H, W) of one valid time against the device ``truth`` of the same shape."""
        E, S, H, W, dev = len(self.channels), len(self.radii), self.H, self.W, self.device
        if self._dev is None:                                           # (zeros: entries the kernel does not write read as no points)
            self._dev = dict(counts=torch.zeros((E, MAX_THRESHOLDS, H, 2, self.M + 1), dtype=torch.int32, device=dev),
                             hx=torch.from_numpy(self.hx).to(dev) if S else None,
                             sums=torch.zeros((E, MAX_THRESHOLDS, S, H, 3), dtype=torch.int64, device=dev) if S else None,
                             ws=torch.empty(E * MAX_THRESHOLDS * 2 * H * W, dtype=torch.uint8, device=dev) if S else None)
        b = self._dev
        run(states, table, truth, [self.names.index(c) for c in self.channels], [self.events[c] for c in self.channels], b["counts"],
            self.hy, b["hx"], b["sums"], b["ws"])
        self.rows.append(b["counts"].cpu().numpy())
        if S:
            self.sums.append(b["sums"].cpu().numpy())

    def result(self, times, weights) -> EventScores:
        E, S = len(self.channels), len(self.radii)
        rows = np.stack(self.rows) if self.rows else np.zeros((0, E, MAX_THRESHOLDS, self.H, 2, self.M + 1), np.int64)
        sums = (np.stack(self.sums) if self.sums else np.zeros((0, E, MAX_THRESHOLDS, S, self.H, 3), np.int64)) if S else None
        return EventScores.from_rows(self.M, times, self.channels, self.events, rows, weights, self.W, self.radii, sums, self.points)
