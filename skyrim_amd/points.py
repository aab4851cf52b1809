"""Point forecasts on the device (include/skyrim_point.h): forecast states on a model's latitude-longitude grid are sampled
at scattered points -- stations, cities, wind farms -- where they lie in HBM, so that a 50-member plume at a few thousand places costs a
few thousand numbers per member and lead time on PCIe instead of the members themselves.

Layers:

* the binding of libskyrim_point.so (``SPEC``, ``load_library``, ``run``, ``validate_records``); the same call is
  ``torch.ops.skyrim_hip.point_gather``.  Point extraction has no CPU fallback;
* the points and their records: ``Points`` parses what a user names, ``records`` makes one ``skpoint_rec`` per point from the functions
  that make ``regrid.tables``' bilinear and nearest tables, so a point on a node of a regrid target gets exactly that node's taps;
* the drivers: ``PointExtractor`` (what ``ensemble.run`` calls at every saved lead time with ``points=...``), ``point_model``
  (``GlobalModel.point_forecast``) and ``extract_prediction`` for forecasts that are already on disk;
* ``PointForecast``: the sampled values (member, time, channel, point), their ensemble statistics and their scores against station
  observations, on the host in float64.
"""
from __future__ import annotations

import csv
import ctypes
import datetime
import json
import math
import os
from pathlib import Path

import numpy as np

from . import native
from .common import finish as _finish, world_size as _world_size
from .leads import open_saved, require_gpu, run_model
from .members import fill_channels, member_count, member_set

MAX_MEMBERS, MAX_CHANNELS, MAX_POINTS, CHUNK = 64, 256, 1 << 20, 8          # include/skyrim_point.h SKPOINT_MAX_*, SKPOINT_CHUNK
METHODS = ("bilinear", "nearest")
_P = ctypes.c_void_p
# skpoint_rec: 32 bytes
REC = np.dtype([("row", "<i4"), ("col", "<i4"), ("nr", "<i4"), ("ncol", "<i4"), ("wr0", "<f4"), ("wr1", "<f4"), ("wc0", "<f4"), ("wc1", "<f4")])


class PointDesc(ctypes.Structure):
    """skpoint_desc."""
    _fields_ = [("members", _P), ("M", ctypes.c_int), ("C", ctypes.c_int), ("H", ctypes.c_int), ("W", ctypes.c_int), ("nc", ctypes.c_int),
                ("channels", ctypes.c_int32 * MAX_CHANNELS), ("records", _P), ("P", ctypes.c_int), ("out", _P),
                ("member_stride", ctypes.c_size_t)]


SPEC = native.Spec("skyrim_point", "SKYRIM_POINT_LIB", "skpoint", 1, {           # include/skyrim_point.h SKPOINT_ABI_VERSION
    "skpoint_abi_version": (ctypes.c_int, []),
    "skpoint_gather": (ctypes.c_int, [ctypes.POINTER(PointDesc), _P]),
    "skpoint_validate": (ctypes.c_int, [_P, ctypes.c_int, ctypes.c_int, ctypes.c_int]),
}, " -- point extraction has no torch fallback")
EXPORTS, ABI_VERSION = SPEC.exports, SPEC.abi

_lib = None


def load_library() -> ctypes.CDLL:
    """libskyrim_point.so (built in-tree by ``__graft_entry__.build()`` / ``make -C skyrim_amd/csrc``)."""
    global _lib
    if _lib is None:
        _lib = native.load(SPEC)
    return _lib


# ---- the binding ------------------------------------------------------------------------------------------------------------------------- #
def validate_records(rec: np.ndarray, H: int, W: int) -> None:
    """``skpoint_validate`` on the host copy of the records: ValueError when the library refuses it."""
    rec = np.ascontiguousarray(rec)
    if rec.dtype != REC or rec.ndim != 1 or rec.size < 1 or load_library().skpoint_validate(rec.ctypes.data, rec.size, int(H), int(W)) != 0:
        raise ValueError("points: a record is refused by skpoint_validate (row, column, count or a weight outside its range)")


def describe(M, C, H, W, channels, P, member_stride) -> PointDesc:
    """The descriptor of a call, its pointers still NULL."""
    d = PointDesc()
    d.M, d.C, d.H, d.W, d.P, d.member_stride = M, C, H, W, P, member_stride
    fill_channels(d, channels, MAX_CHANNELS)
    return d


def run(members, table, channels, records, out) -> None:
    """One ``skpoint_gather``: the channels ``channels`` of the M ``members`` (equal-shaped contiguous float32 (C, H, W) device tensors;
    ``table`` = ``ensemble.member_table(members)``) at the P points of ``records`` -- int32 (P, 8) on the device, the bytes of P
    ``skpoint_rec`` (``device_records``) -- into ``out``, float32 (M, nc, P), or (M, stride) with stride >= nc P of which each member's
    first nc P elements are written.  Queued on torch's current stream.  As in ``regrid.run``, the contents of ``table`` are trusted to be
    the addresses of ``members``; the kernel clamps what it reads from the records, so their contents cannot cause an access out of range."""
    import torch
    channels = [int(c) for c in channels]
    member_count(members, "point_gather", MAX_MEMBERS)
    if not 1 <= len(channels) <= MAX_CHANNELS:
        raise ValueError(f"point_gather: {len(channels)} channels; 1 to {MAX_CHANNELS} are supported")
    M, dev, _ = member_set(members, table, "point_gather", MAX_MEMBERS)
    C, H, W = members[0].shape
    pr = native.tensor_ptr(records, "point_gather: records", torch.int32, dev)
    if records.dim() != 2 or records.shape[1] != 8 or not 1 <= records.shape[0] <= MAX_POINTS:
        raise ValueError(f"point_gather: records are int32 (P, 8), the bytes of P skpoint_rec, 1 <= P <= {MAX_POINTS}")
    P, nc = int(records.shape[0]), len(channels)
    po = native.tensor_ptr(out, "point_gather: out", torch.float32, dev)
    if out.dim() == 3 and tuple(out.shape) == (M, nc, P):
        stride = nc * P
    elif out.dim() == 2 and out.shape[0] == M and out.shape[1] >= nc * P:
        stride = int(out.shape[1])
    else:
        raise ValueError(f"point_gather: out must be ({M}, {nc}, {P}) or ({M}, stride >= {nc * P})")
    d = describe(M, C, H, W, channels, P, stride)
    d.members, d.records, d.out = table.data_ptr(), pr, po
    lib = load_library()
    with torch.cuda.device(dev):
        native.check(lib.skpoint_gather(ctypes.byref(d), native.stream(dev)), "skpoint_gather", lib)


def device_records(rec: np.ndarray, device):
    """The records as the int32 (P, 8) device tensor ``run`` takes."""
    import torch
    return torch.from_numpy(np.ascontiguousarray(rec).view(np.int32).reshape(-1, 8).copy()).to(device)


# ---- the points -------------------------------------------------------------------------------------------------------------------------- #
class Points:
    """Named places.  Built from ``{name: (lat, lon)}``, a list of ``(name, lat, lon)``, a CSV path with the columns ``name,lat,lon``, or
    another ``Points``.  Longitudes in [-180, 360) are taken modulo 360; duplicate names, non-finite values, |lat| > 90 and a longitude
    outside [-180, 360) are ValueError."""

    def __init__(self, spec):
        if isinstance(spec, Points):
            items = list(zip(spec.names, spec.lat, spec.lon))
        elif isinstance(spec, dict):
            items = []
            for k, v in spec.items():
                if not hasattr(v, "__len__") or len(v) != 2:
                    raise ValueError(f"points: {k!r} needs (lat, lon)")
                items.append((k, v[0], v[1]))
        elif isinstance(spec, (str, os.PathLike)):
            items = self._read_csv(os.fspath(spec))
        elif isinstance(spec, (list, tuple)):
            items = []
            for it in spec:
                if not hasattr(it, "__len__") or isinstance(it, str) or len(it) != 3:
                    raise ValueError("points: a list holds (name, lat, lon) entries")
                items.append(tuple(it))
        else:
            raise ValueError("points: {name: (lat, lon)}, a list of (name, lat, lon) or the path of a CSV file with the columns name,lat,lon")
        if not items:
            raise ValueError("points: at least one point")
        if len(items) > MAX_POINTS:
            raise ValueError(f"points: {len(items)} points; one call samples at most {MAX_POINTS} (SKPOINT_MAX_POINTS)")
        names, lat, lon, seen = [], [], [], set()
        for name, la, lo in items:
            name = str(name)
            try:
                la, lo = float(la), float(lo)
            except (TypeError, ValueError):
                raise ValueError(f"points: {name!r}: latitude and longitude are numbers") from None
            if name in seen:
                raise ValueError(f"points: the name {name!r} appears twice")
            if not (math.isfinite(la) and math.isfinite(lo)):
                raise ValueError(f"points: {name!r} has a non-finite coordinate")
            if abs(la) > 90:
                raise ValueError(f"points: {name!r} has latitude {la:g}; |lat| <= 90")
            if not -180.0 <= lo < 360.0:
                raise ValueError(f"points: {name!r} has longitude {lo:g}; longitudes lie in [-180, 360)")
            seen.add(name)
            names.append(name)
            lat.append(la)
            lon.append(lo % 360.0)
        self.names, self.lat, self.lon = names, np.asarray(lat, np.float64), np.asarray(lon, np.float64)

    @staticmethod
    def _read_csv(path: str) -> list:
        with open(path, newline="") as f:
            rows = list(csv.reader(f))
        rows = [[c.strip() for c in r] for r in rows if r and any(c.strip() for c in r)]
        if not rows or [c.lower() for c in rows[0][:3]] != ["name", "lat", "lon"]:
            raise ValueError(f"points: {path} must start with the header name,lat,lon")
        for r in rows[1:]:
            if len(r) < 3:
                raise ValueError(f"points: {path}: the line {','.join(r)!r} lacks a column")
        return [(r[0], r[1], r[2]) for r in rows[1:]]

    def __len__(self):
        return len(self.names)

    def key(self) -> tuple:
        return (tuple(self.names), self.lat.tobytes(), self.lon.tobytes())


_record_cache: dict = {}


def records(points, src_lat, src_lon, method: str = "bilinear") -> np.ndarray:
    """One ``skpoint_rec`` per point, in the order of the points (structured array of dtype ``REC``); cached per (grid, points, method).
    The taps and fp32 weights are those ``regrid.tables`` gives a target node at the same place: ``bilinear`` two taps (1 - t, t) per axis,
    the longitude periodic, ONE tap of weight 1 where the point lies on a source row or column; ``nearest`` one tap per axis, a tie to the
    lower index, a latitude beyond the last row clamped to it.  A bilinear point outside the source's latitudes is refused with a
    ValueError that names it (interpolation does not extrapolate: a 720-row grid has no south pole).

    Cost: the makers of ``regrid`` are reused as they are, for bit equality with its tables.  They loop over the points in Python (nearest
    takes an ``argmin`` over the source axis per point) and ``_axis`` carries the at most two taps in a (P, 32) fp32 table per axis: about
    a second and 8 MB for 30 000 points, minutes and some 270 MB of temporaries at the limit of 2^20 points.  Made once per (grid, points,
    method)."""
    from . import regrid
    if method not in METHODS:
        raise ValueError(f"points: unknown method {method!r}; choose from {METHODS}")
    pts = points if isinstance(points, Points) else Points(points)
    src = regrid._lat_axis(src_lat, "source")
    key = (src.tobytes(), np.asarray(src_lon, np.float64).tobytes(), pts.key(), method)
    hit = _record_cache.get(key)
    if hit is not None:
        return hit
    su = regrid._src_lon(src_lon)
    if method == "bilinear":
        outside = np.nonzero((pts.lat < src.min() - 1e-9) | (pts.lat > src.max() + 1e-9))[0]
        if outside.size:
            p = int(outside[0])
            raise ValueError(f"points: {pts.names[p]!r} (latitude {pts.lat[p]:g}) lies outside the source latitudes [{src.min():g}, {src.max():g}]: "
                             "bilinear interpolation does not extrapolate; method='nearest' takes the last row")
        rows, cols = regrid._bilinear_rows(src, pts.lat), regrid._bilinear_cols(su, pts.lon)
    else:
        rows, cols = regrid._nearest_rows(src, pts.lat), regrid._nearest_cols(su, pts.lon)
    ra = regrid._axis(rows, src.size, False, "row", float(np.mean(np.abs(np.diff(src)))))
    ca = regrid._axis(cols, su.size, True, "column", 360.0 / su.size)
    rec = np.zeros(len(pts), REC)
    rec["row"], rec["nr"], rec["wr0"], rec["wr1"] = ra.start, ra.count, ra.weight[:, 0], ra.weight[:, 1]
    rec["col"], rec["ncol"], rec["wc0"], rec["wc1"] = ca.start, ca.count, ca.weight[:, 0], ca.weight[:, 1]
    validate_records(rec, src.size, su.size)
    _record_cache[key] = rec
    return rec


def host_limit(n_members: int, n_times: int, n_channels: int, n_points: int) -> None:
    """The sampled values are held on the host like kept members: refused beyond the limit ``keep_members`` is checked against."""
    from .core.models.utils import _PINNED_LIMIT
    need = int(n_members) * int(n_times) * int(n_channels) * int(n_points) * 4
    if need > _PINNED_LIMIT:
        raise ValueError(f"points: {n_members} members x {n_times} times x {n_channels} channels x {n_points} points would hold "
                         f"{need / 2 ** 30:.1f} GiB on the host (limit {_PINNED_LIMIT / 2 ** 30:.0f} GiB): fewer points, channels or times")


def check_request(names, lat, lon, n_members, points, channels=None, method="bilinear", n_times=1) -> tuple:
    """Every refusal that needs no device; returns (Points, channels, records)."""
    if _world_size() > 1:
        raise NotImplementedError("points are sampled on one GPU from members that all lie there; members sharded over the ranks of a "
                                  "process group are out of scope (DESIGN.md 25)")
    if not 1 <= int(n_members) <= MAX_MEMBERS:
        raise ValueError(f"n_members = {n_members}: 1 to {MAX_MEMBERS} members are sampled (SKPOINT_MAX_MEMBERS)")
    if method not in METHODS:
        raise ValueError(f"points: unknown method {method!r}; choose from {METHODS}")
    names = list(names)
    picked = names if channels is None else list(channels)
    missing = [c for c in picked if c not in names]
    if missing:
        raise ValueError(f"points: channels {missing} are not channels of this forecast")
    if not 1 <= len(picked) <= MAX_CHANNELS:
        raise ValueError(f"points: {len(picked)} channels; one call samples 1 to {MAX_CHANNELS} (SKPOINT_MAX_CHANNELS)")
    pts = points if isinstance(points, Points) else Points(points)
    if len(names) * len(lat) * len(lon) > 2 ** 30 or len(picked) * len(pts) > 2 ** 30:
        raise ValueError("points: a state and its sampled channels hold at most 2^30 elements each")
    host_limit(n_members, n_times, len(picked), len(pts))
    return pts, picked, records(pts, lat, lon, method)


# ---- the drivers ------------------------------------------------------------------------------------------------------------------------- #
class PointExtractor:
    """Samples one lead time after the other.  ``names``: the channels of the (C, H, W) states in their order -- raw states, the views of a
    ``LeadDeriver``'s buffer or those of an aggregator's accumulator alike; ``channels``: those to sample (None: all).  It owns the uploaded
    records, sorted by (row, col) so that neighbouring lanes touch neighbouring lines, a device buffer (M, nc, P) and ONE page-locked host
    buffer (n_times, M, nc, P), allocated with the device buffers before the first lead time (``n_times``: the ``extract`` calls to
    come; more calls than that take a further block).  ``extract`` queues one launch and one copy into its slice of the host buffer and
    returns at once; ``result`` waits for the copies and undoes the sort."""

    def __init__(self, names, lat, lon, n_members, points, channels=None, method="bilinear", device="cuda:0", sort=True, n_times=1):
        self.points, self.channels, rec = check_request(names, lat, lon, n_members, points, channels, method, n_times)
        self.n_times = max(int(n_times), 1)
        self.names, self.M, self.method, self.device = list(names), int(n_members), method, device
        self.index = [self.names.index(c) for c in self.channels]
        self.order = np.lexsort((rec["col"], rec["row"])) if sort else np.arange(rec.size)
        self.records = rec[self.order]
        self.inverse = np.empty_like(self.order)
        self.inverse[self.order] = np.arange(self.order.size)
        self._dev, self._host, self._count = None, [], 0

    def _buffers(self):
        if self._dev is None:
            import torch
            dev = torch.device(self.device)
            self._dev = dict(rec=device_records(self.records, dev),
                             out=torch.empty((self.M, len(self.channels), len(self.points)), dtype=torch.float32, device=dev),
                             done=torch.cuda.Event())
            self._host.append(torch.empty((self.n_times, *self._dev["out"].shape), dtype=torch.float32, pin_memory=True))
        return self._dev

    def _slot(self, shape):
        """The host slice of the next call: a view of the page-locked block, nothing allocated per call within ``n_times``."""
        import torch
        block, at = divmod(self._count, self.n_times)
        if block == len(self._host):
            self._host.append(torch.empty((self.n_times, *shape), dtype=torch.float32, pin_memory=True))
        self._count += 1
        return self._host[block][at]

    def extract(self, members, table=None) -> None:
        """ONE gather launch over the M device states and one asynchronous copy of its (M, nc, P) result; nothing waits for the GPU."""
        import torch
        from .ensemble import member_table
        if len(members) != self.M:
            raise ValueError(f"{len(members)} states for an extractor of {self.M} members")
        b = self._buffers()
        run(members, member_table(members) if table is None else table, self.index, b["rec"], b["out"])
        self._slot(b["out"].shape).copy_(b["out"], non_blocking=True)      # stream-ordered: before the next launch overwrites the buffer
        b["done"].record(torch.cuda.current_stream(b["out"].device))       # (one event, recorded again: result waits for the last copy)

    def result(self) -> np.ndarray:
        """(M, T, nc, P) float32 of all ``extract`` calls so far, the points in the order they were given."""
        if not self._count:
            return np.empty((self.M, 0, len(self.channels), len(self.points)), np.float32)
        self._dev["done"].synchronize()
        host = np.concatenate([h.numpy() for h in self._host], axis=0)[:self._count]       # (T, M, nc, P)
        return np.ascontiguousarray(np.transpose(host, (1, 0, 2, 3))[:, :, :, self.inverse])


def _iso(t) -> str:
    return np.datetime64(t, "s").astype(datetime.datetime).isoformat()


class PointForecast:
    """Sampled values of a forecast.  ``values``: DataArray(member, time, channel, point) float32 with the coordinates ``lat`` / ``lon`` of
    the points and ``method``.  The statistics follow include/skyrim_ens.h and the scores DESIGN.md 18 (skyrim_score.h), evaluated on the
    host in float64 over points of equal weight."""

    def __init__(self, values, model_name: str = "", forecast_id: str = ""):
        self.values, self.model_name, self.forecast_id = values, model_name, forecast_id
        self.path = None

    @classmethod
    def build(cls, arr, times, channels, points: Points, method: str, model_name: str = "", forecast_id: str = "", **coords):
        from .labeled import DataArray
        arr = np.asarray(arr, np.float32)
        da = DataArray(arr, ["member", "time", "channel", "point"],
                       dict(member=np.arange(arr.shape[0]), time=list(times), channel=list(channels), point=list(points.names),
                            lat=points.lat, lon=points.lon, method=method, **coords))
        return cls(da, model_name, forecast_id)

    # -- coordinates
    @property
    def channels(self) -> list:
        return self.values.channel.values.tolist()

    @property
    def names(self) -> list:
        return self.values.point.values.tolist()

    @property
    def times(self) -> list:
        return [t.astype(datetime.datetime) for t in np.asarray(self.values._coords["time"]).astype("datetime64[s]")]

    @property
    def n_members(self) -> int:
        return int(self.values.shape[0])

    def _x(self) -> np.ndarray:
        return np.asarray(self.values.values, np.float32).astype(np.float64)

    def _labelled(self, arr, dim=None, labels=None):
        from .labeled import DataArray
        c = self.values._coords
        dims = ["time", "channel", "point"] if dim is None else [dim, "time", "channel", "point"]
        coords = dict(time=c["time"], channel=c["channel"], point=c["point"], lat=c["lat"], lon=c["lon"])
        if dim is not None:
            coords[dim] = labels
        return DataArray(arr, dims, coords)

    # -- ensemble statistics (include/skyrim_ens.h)
    def mean(self):
        return self._labelled(self._x().mean(axis=0))

    def spread(self):
        x = self._x()
        return self._labelled(np.sqrt(((x - x.mean(axis=0)) ** 2).mean(axis=0)))

    def quantile(self, levels):
        """The "linear" quantiles of the sorted members: DataArray(quantile, time, channel, point)."""
        levels = [float(q) for q in levels]
        s = np.sort(self._x(), axis=0)
        M = s.shape[0]
        out = []
        for lev in levels:
            if not 0.0 <= lev <= 1.0:
                raise ValueError(f"quantile level {lev} is outside [0, 1]")
            h = (M - 1) * lev
            k = min(int(math.floor(h)), M - 1)
            k1 = min(k + 1, M - 1)
            out.append(s[k] + (h - k) * (s[k1] - s[k]))
        return self._labelled(np.stack(out), "quantile", np.asarray(levels, np.float64))

    def exceedance(self, channel: str, thresholds):
        """The fraction of members above each threshold (compared in float32): DataArray(threshold, time, point)."""
        from .labeled import DataArray
        c = self.channels.index(channel) if channel in self.channels else None
        if c is None:
            raise ValueError(f"exceedance: {channel!r} is not a sampled channel ({self.channels})")
        x = np.asarray(self.values.values, np.float32)[:, :, c]
        thr = np.asarray([np.float32(t) for t in thresholds], np.float32)
        arr = np.stack([(x > t).sum(axis=0) / float(x.shape[0]) for t in thr])
        k = self.values._coords
        return DataArray(arr, ["threshold", "time", "point"], dict(threshold=thr, time=k["time"], point=k["point"], lat=k["lat"], lon=k["lon"]))

    def plume(self, channel: str, point: str, levels=(0.1, 0.25, 0.5, 0.75, 0.9)) -> dict:
        """What a plume plot of one channel at one place needs: ``times``, ``members`` (M, T), ``mean``, ``spread`` and ``quantiles`` {level: (T,)}."""
        if channel not in self.channels or point not in self.names:
            raise ValueError(f"plume: channel {channel!r} / point {point!r} is not in this forecast")
        c, p = self.channels.index(channel), self.names.index(point)
        x = self._x()[:, :, c, p]
        q = self.quantile(levels).values[:, :, c, p]
        return dict(times=self.times, members=x, mean=x.mean(axis=0), spread=np.sqrt(((x - x.mean(axis=0)) ** 2).mean(axis=0)),
                    quantiles={float(lev): q[i] for i, lev in enumerate(levels)})

    # -- station scores (DESIGN.md 18 over points of equal weight)
    def verify(self, observations) -> dict:
        """Scores against station observations: a ``DataArray(time, channel, point)`` (its channels and points picked by name, its times
        matched) or ``{channel: array(time, point)}``; NaN means missing.  Per channel and lead time, over the points whose observation is
        finite, each with equal weight: ``n``, ``bias``, ``mae``, ``rmse`` (of the ensemble mean), ``crps`` (fair), ``spread`` (root of the
        mean unbiased member variance), ``ssr`` (sqrt((M + 1) / M) spread / rmse) as (time, channel) float64 arrays, and ``rank_histogram``
        (time, channel, M + 1) counts of the members below the observation.  A (time, channel) without a valid observation has n = 0 and
        NaN scores.  The dict also holds ``channels`` and ``times``."""
        x = self._x()                                         # (M, T, C, P)
        M, T, _, P = x.shape
        if hasattr(observations, "dims"):
            if tuple(observations.dims) != ("time", "channel", "point"):
                raise ValueError("verify: observations are a DataArray(time, channel, point) or {channel: array(time, point)}")
            och, opt = observations.channel.values.tolist(), observations.point.values.tolist()
            otimes = [np.datetime64(t, "s") for t in np.asarray(observations._coords["time"])]
            mine = [np.datetime64(t, "s") for t in np.asarray(self.values._coords["time"])]
            missing = [n for n in self.names if n not in opt]
            if missing or any(t not in otimes for t in mine):
                raise ValueError(f"verify: the observations lack the points {missing[:5]} or a time of the forecast")
            ov = np.asarray(observations.values, np.float64)[[otimes.index(t) for t in mine]][:, :, [opt.index(n) for n in self.names]]
            obs = {c: ov[:, och.index(c)] for c in och if c in self.channels}
        elif isinstance(observations, dict):
            obs = {c: np.asarray(v, np.float64) for c, v in observations.items()}
        else:
            raise ValueError("verify: observations are a DataArray(time, channel, point) or {channel: array(time, point)}")
        unknown = [c for c in obs if c not in self.channels]
        if unknown or not obs:
            raise ValueError(f"verify: the channels {unknown} are not sampled channels ({self.channels})")
        scored = [c for c in self.channels if c in obs]
        for c in scored:
            if obs[c].shape != (T, P):
                raise ValueError(f"verify: observations of {c!r} have shape {obs[c].shape}, expected (time, point) = {(T, P)}")
        keys = ("bias", "mae", "rmse", "crps", "spread", "ssr")
        out = {k: np.full((T, len(scored)), np.nan) for k in keys}
        out["n"] = np.zeros((T, len(scored)), np.int64)
        out["rank_histogram"] = np.zeros((T, len(scored), M + 1), np.int64)
        for ci, c in enumerate(scored):
            k = self.channels.index(c)
            for t in range(T):
                y = obs[c][t]
                ok = np.isfinite(y)
                n = int(ok.sum())
                out["n"][t, ci] = n
                if n == 0:
                    continue
                xm, ym = x[:, t, k][:, ok], y[ok]
                e = xm - ym
                eb = xm.mean(axis=0) - ym                   # the error of the ensemble mean
                s = np.sort(xm, axis=0)
                B = np.zeros(n)
                for i in range(M - 1):
                    B += (i + 1) * (M - 1 - i) * (s[i + 1] - s[i])
                B = B / (M * (M - 1)) if M > 1 else B
                var = xm.var(axis=0, ddof=1) if M > 1 else np.zeros(n)
                mean = lambda a: math.fsum(a.tolist()) / n      # noqa: E731  (the sum over the points exactly rounded: a bias near 0 keeps its digits)
                out["bias"][t, ci], out["mae"][t, ci] = mean(eb), mean(np.abs(eb))
                out["rmse"][t, ci] = math.sqrt(mean(eb ** 2))
                out["crps"][t, ci] = mean(np.abs(e).mean(axis=0) - B)
                if M > 1:
                    out["spread"][t, ci] = math.sqrt(mean(var))
                    with np.errstate(divide="ignore", invalid="ignore"):
                        out["ssr"][t, ci] = np.float64(math.sqrt((M + 1) / M) * out["spread"][t, ci]) / np.float64(out["rmse"][t, ci])
                out["rank_histogram"][t, ci] = np.bincount((xm < ym).sum(axis=0), minlength=M + 1)
        out["channels"], out["times"] = scored, self.times
        return out

    # -- files
    def to_json(self) -> str:
        def clean(a):
            return [clean(v) for v in a] if isinstance(a, list) else (None if isinstance(a, float) and not math.isfinite(a) else a)
        c = self.values._coords
        doc = dict(model=self.model_name, forecast_id=self.forecast_id, n_members=self.n_members, method=str(np.asarray(c["method"]).item()),
                   times=[_iso(t) for t in np.asarray(c["time"])], channels=self.channels, points=self.names,
                   lat=np.asarray(c["lat"], np.float64).tolist(), lon=np.asarray(c["lon"], np.float64).tolist(),
                   values=clean(np.asarray(self.values.values, np.float64).tolist()))
        return json.dumps(doc)

    def to_csv(self, path) -> str:
        """Long form: one line ``time,member,channel,point,value`` per number (``%.9g``: every float32 survives)."""
        v = np.asarray(self.values.values, np.float32)
        times = [_iso(t) for t in np.asarray(self.values._coords["time"])]
        with open(path, "w", newline="") as f:
            w = csv.writer(f)
            w.writerow(["time", "member", "channel", "point", "value"])
            for ti, t in enumerate(times):
                for m in range(v.shape[0]):
                    for ci, ch in enumerate(self.channels):
                        for pi, name in enumerate(self.names):
                            w.writerow([t, m, ch, name, f"{v[m, ti, ci, pi]:.9g}"])
        return str(path)

    def file_name(self) -> str:
        return f"{self.model_name}-points.json"

    def save(self, output_dir) -> str:
        """``{output_dir}/{forecast id}/{model}-points.json``; returns the path."""
        d = Path(output_dir) / self.forecast_id if self.forecast_id else Path(output_dir)
        d.mkdir(parents=True, exist_ok=True)
        path = d / self.file_name()
        path.write_text(self.to_json())
        self.path = str(path)
        return self.path


def read_observations(path, channels, times, names) -> dict:
    """``{channel: array(time, point)}`` from a long-form CSV ``time,channel,point,value``; what the file lacks is NaN."""
    tkey = [np.datetime64(t, "s") for t in times]
    obs = {c: np.full((len(tkey), len(names)), np.nan) for c in channels}
    with open(path, newline="") as f:
        rows = list(csv.reader(f))
    if not rows or [c.strip().lower() for c in rows[0][:4]] != ["time", "channel", "point", "value"]:
        raise ValueError(f"observations: {path} must start with the header time,channel,point,value")
    pos = {n: i for i, n in enumerate(names)}
    for r in rows[1:]:
        if len(r) < 4:
            continue
        t, c, p = np.datetime64(r[0].strip(), "s"), r[1].strip(), r[2].strip()
        if c in obs and p in pos and t in tkey:
            obs[c][tkey.index(t), pos[p]] = float(r[3])
    return obs


def _sources(names, derived, channels):
    """Split the sampled channels over the two source buffers: (all, raw, derived names) in the order asked for."""
    names, dnames = list(names), list(derived or [])
    picked = list(channels) if channels is not None else names + dnames
    missing = [c for c in picked if c not in names and c not in dnames]
    if missing:
        raise ValueError(f"points: channels {missing} are neither output channels of this model nor derived fields named in derived=")
    if len(set(picked)) != len(picked):
        raise ValueError("points: a channel is named twice")
    return picked, [c for c in picked if c in names], [c for c in picked if c not in names]


class LeadPoints:
    """The extractors of one rollout: raw channels from the states and, in a second call, derived fields from the derived buffer -- as
    aggregation does with its two sources.  ``add`` queues the launches of one lead time, ``result`` assembles the ``PointForecast``."""

    def __init__(self, names, lat, lon, n_members, points, channels=None, method="bilinear", device="cuda:0", derived=(), n_times=1):
        self.points = points if isinstance(points, Points) else Points(points)
        self.channels, raw, der = _sources(names, derived, channels)
        host_limit(n_members, n_times, len(self.channels), len(self.points))
        mk = lambda nm, ch: PointExtractor(nm, lat, lon, n_members, self.points, ch, method, device, n_times=n_times)      # noqa: E731
        self.raw = mk(list(names), raw) if raw else None
        self.der = mk(list(derived), der) if der else None
        self.method, self.times = method, []

    @property
    def needs_derived(self) -> bool:
        return self.der is not None

    def add(self, time, states, table=None, derived=None) -> None:
        if self.raw is not None:
            self.raw.extract(states, table)
        if self.der is not None:
            if derived is None:
                raise ValueError("point channels name derived fields: add() needs derived=(states, table) of the deriver")
            self.der.extract(derived[0], derived[1])
        self.times.append(time)

    def result(self, model_name="", forecast_id="", **coords) -> PointForecast:
        parts, order = [], []
        for ex in (self.raw, self.der):
            if ex is not None:
                parts.append(ex.result())
                order += ex.channels
        arr = np.concatenate(parts, axis=2)[:, :, [order.index(c) for c in self.channels]]
        return PointForecast.build(arr, self.times, self.channels, self.points, self.method, model_name, forecast_id, **coords)


def point_model(gm, start_time: datetime.datetime, n_steps: int, points, channels=None, derived=None, method: str = "bilinear",
                save: bool = False, save_config: dict | None = None) -> PointForecast:
    """``GlobalModel.point_forecast`` (core/models/base.py has the user-facing description)."""
    model = gm.model
    names = list(model.out_channel_names)
    if n_steps < 0:
        raise ValueError("n_steps >= 0")
    deriver = None
    if derived is not None:
        from . import derived as deriving
        deriving.check_request(names, list(derived), model.grid.lat, model.grid.lon, 1)
    if _world_size() > 1:
        raise NotImplementedError("points are sampled on one GPU; a process group of more than one rank is out of scope (DESIGN.md 25)")
    lp = LeadPoints(names, model.grid.lat, model.grid.lon, 1, points, channels, method, model.device, list(derived or []), n_steps + 1)      # before the device
    require_gpu(model.device, "point_forecast samples with HIP kernels where the forecast lies: the model must be on a GPU")
    if lp.needs_derived:
        deriver = deriving.LeadDeriver(names, model.grid.lat, model.grid.lon, 1, list(derived), device=model.device)
    run_model(gm, start_time, n_steps,
              lambda k, time, state: lp.add(time, [state], None, deriver.add([state]) if deriver is not None else None))
    return _finish(lp.result(gm.model_name), save, save_config)


def extract_prediction(pred, points, channels=None, method: str = "bilinear", device="cuda:0") -> PointForecast:
    """Point values of a forecast that already exists: a ``GlobalPrediction``, a (time, channel, lat, lon) DataArray, a saved netCDF file
    or zarr store, or a list of such files (their time entries in order, duplicates of a valid time sampled once).  Each time entry is
    uploaded, sampled by the same kernel as ``point_forecast`` and dropped.  Returns a ``PointForecast`` with one member."""
    saved = open_saved(pred, "extract_prediction")
    lp = LeadPoints(saved.names, saved.lat, saved.lon, 1, points, channels, method, device, (), len(saved.entries))
    require_gpu(device, "extract_prediction samples with HIP kernels: it needs a GPU", present=True)
    for _, time, state in saved.states(device):
        lp.add(time, [state])
    return lp.result()
