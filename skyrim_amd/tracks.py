"""Cyclone tracking (include/skyrim_track.h): candidate centres are detected on the device, where the states lie in HBM,
and only their 32-byte records cross to the host, which links them into tracks.

Layers:

* the binding of libskyrim_track.so (``SPEC``, ``load_library``, ``detect``); the same call is ``torch.ops.skyrim_hip.track_detect``.
  Detection has no CPU fallback;
* ``TrackerConfig``, ``channel_plan`` and ``geometry`` -- what is detected, on which channels, and the integer window tables and row
  coefficients the kernels read, made in float64 on the host;
* ``link`` (the host's deterministic linker), ``Tracks`` (the result, its strike probability and its JSON file);
* the drivers: ``LeadTracker`` (what ``ensemble.run`` calls at every lead time with ``tracks=True``), ``track_model``
  (``GlobalModel.track_cyclones``) and ``track_prediction`` for forecasts that are already on disk.
"""
from __future__ import annotations

import ctypes
import datetime
import json
import math
from dataclasses import asdict, dataclass
from pathlib import Path

import numpy as np

from . import native
from .common import finish as _finish, iso as _iso, world_size as _world_size
from .leads import open_saved, require_gpu, run_model
from .members import member_set

MAX_MEMBERS = 64                                                # include/skyrim_track.h SKTRACK_MAX_MEMBERS
EARTH_RADIUS_KM = 6371.0
CRITERIA = ("msl", "vort", "wind", "core")
REQUIRED = ("msl", "u10m", "v10m", "u850", "v850")
RECORD = np.dtype([("member", "<i4"), ("j", "<i4"), ("i", "<i4"), ("msl", "<f4"), ("vort", "<f4"), ("wind", "<f4"), ("core", "<f4"),
                   ("pad", "<i4")])                             # sktrack_record
_P = ctypes.c_void_p


class TrackDesc(ctypes.Structure):
    """sktrack_desc."""
    _fields_ = [("members", _P), ("M", ctypes.c_int), ("C", ctypes.c_int), ("H", ctypes.c_int), ("W", ctypes.c_int),
                ("ch_msl", ctypes.c_int), ("ch_u10", ctypes.c_int), ("ch_v10", ctypes.c_int), ("ch_u850", ctypes.c_int),
                ("ch_v850", ctypes.c_int), ("ch_zup", ctypes.c_int), ("ch_zlo", ctypes.c_int), ("j0", ctypes.c_int), ("j1", ctypes.c_int),
                ("thr_msl", ctypes.c_float), ("thr_vort", ctypes.c_float), ("thr_wind", ctypes.c_float), ("thr_core", ctypes.c_float),
                ("h_msl", _P), ("h_vort", _P), ("h_wind", _P), ("h_core", _P),
                ("d_msl", ctypes.c_int), ("d_vort", ctypes.c_int), ("d_wind", ctypes.c_int), ("d_core", ctypes.c_int),
                ("rowc", _P), ("records", _P), ("capacity", ctypes.c_int), ("count", _P), ("workspace", _P),
                ("workspace_bytes", ctypes.c_size_t)]


SPEC = native.Spec("skyrim_track", "SKYRIM_TRACK_LIB", "sktrack", 1, {          # include/skyrim_track.h SKTRACK_ABI_VERSION
    "sktrack_abi_version": (ctypes.c_int, []),
    "sktrack_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "sktrack_detect": (ctypes.c_int, [ctypes.POINTER(TrackDesc), _P]),
}, " -- cyclone detection has no torch fallback")
EXPORTS, ABI_VERSION = SPEC.exports, SPEC.abi

_lib = None


def load_library() -> ctypes.CDLL:
    """libskyrim_track.so (built in-tree by ``__graft_entry__.build()`` / ``make -C skyrim_amd/csrc``)."""
    global _lib
    if _lib is None:
        _lib = native.load(SPEC)
    return _lib


# ---- what is detected ------------------------------------------------------------------------------------------------------------------ #
@dataclass(frozen=True)
class TrackerConfig:
    """Centres are sought at |lat| <= ``lat_max``; the radii are those of the four windows; the thresholds those of the criteria
    (``thr_msl``: an upper limit on the central pressure, off by default); ``core_levels``: (upper, lower) geopotential channels of the
    warm-core thickness; ``max_speed_kmh`` and ``min_points`` belong to the linker; ``capacity``: records per member and lead time."""
    lat_max: float = 60.0
    r_msl_km: float = 445.0
    r_vort_km: float = 278.0
    r_wind_km: float = 278.0
    r_core_km: float = 278.0
    thr_msl: float = math.inf
    thr_vort: float = 5e-5
    thr_wind: float = 8.0
    thr_core: float = 0.0
    core_levels: tuple = ("z200", "z850")
    max_speed_kmh: float = 90.0
    min_points: int = 2
    capacity: int = 4096

    def radii(self) -> tuple:
        return (float(self.r_msl_km), float(self.r_vort_km), float(self.r_wind_km), float(self.r_core_km))


_DEFAULT_CORE = TrackerConfig().core_levels


def as_config(config) -> TrackerConfig:
    if config is None:
        return TrackerConfig()
    if isinstance(config, TrackerConfig):
        return config
    if isinstance(config, dict):
        cfg = dict(config)
        if "core_levels" in cfg and cfg["core_levels"] is not None:
            cfg["core_levels"] = tuple(cfg["core_levels"])
        return TrackerConfig(**cfg)
    raise ValueError(f"a tracker configuration is a TrackerConfig or a dict of its fields, not {type(config).__name__}")


@dataclass(frozen=True)
class ChannelPlan:
    msl: int
    u10: int
    v10: int
    u850: int
    v850: int
    z_up: int = -1
    z_lo: int = -1
    warm_core: bool = False
    note: str = ""


def channel_plan(names, cfg: TrackerConfig | None = None, model_name: str = "forecast") -> ChannelPlan:
    """Where the channels of the criteria lie in a (C, H, W) state with the channels ``names``.  The five required channels missing is
    a ValueError naming the model and the channel; the DEFAULT warm-core levels missing drops that criterion (and the plan says so);
    levels asked for explicitly and missing are a ValueError."""
    cfg = as_config(cfg)
    names = list(names)
    missing = [c for c in REQUIRED if c not in names]
    if missing:
        raise ValueError(f"{model_name} cannot be tracked: its output has no channel {', '.join(repr(c) for c in missing)} "
                         f"(cyclone detection needs {', '.join(REQUIRED)})")
    idx = [names.index(c) for c in REQUIRED]
    levels = cfg.core_levels
    if not levels:
        return ChannelPlan(*idx, note="no warm-core criterion was asked for")
    if len(levels) != 2:
        raise ValueError("core_levels: (upper, lower) geopotential channels, or None")
    absent = [c for c in levels if c not in names]
    if absent:
        if tuple(levels) != tuple(_DEFAULT_CORE):
            raise ValueError(f"{model_name} has no channel {', '.join(repr(c) for c in absent)} for the warm-core criterion that was asked for")
        return ChannelPlan(*idx, note=f"warm-core criterion dropped: {model_name} has no channel {', '.join(repr(c) for c in absent)}")
    return ChannelPlan(*idx, names.index(levels[0]), names.index(levels[1]), True)


# ---- geometry ---------------------------------------------------------------------------------------------------------------------------- #
@dataclass
class Geometry:
    """``h[r]``: int32 (Hb, 2 ``d[r]`` + 1) half-widths of criterion r's window per band row and row offset; ``rowc``: float32 (H, 4)
    = A, B+, B-, sgn(lat); the band is the rows [j0, j1)."""
    j0: int
    j1: int
    h: dict
    d: dict
    rowc: np.ndarray
    lat: np.ndarray
    lon: np.ndarray


def _uniform_lon(lon) -> float:
    lon = np.asarray(lon, np.float64)
    W = lon.size
    if W < 3:
        raise ValueError("tracking needs a periodic longitude axis of at least 3 points")
    step = 360.0 / W
    if not np.allclose(np.diff(lon), step, rtol=0, atol=1e-6 * step):
        raise ValueError("tracking needs uniform longitudes that cover the circle")
    return math.radians(step)


def half_widths(lat, lon, j0: int, j1: int, radius_km: float):
    """(table, D) of one radius: table[j - j0][dj + D] = the largest k >= 0 with haversine((lat_j, 0), (lat_{j+dj}, k dlon)) <= radius,
    -1 where row j + dj is outside the grid or out of reach; D = the largest row offset any band row reaches."""
    phi = np.radians(np.asarray(lat, np.float64))
    H, W = phi.size, len(lon)
    dlam = _uniform_lon(lon)
    band = np.arange(j0, j1)
    merid = EARTH_RADIUS_KM * np.abs(phi[band][:, None] - phi[None, :]) <= radius_km              # (Hb, H)
    off = np.abs(np.arange(H)[None, :] - band[:, None])
    D = int(np.where(merid, off, 0).max())
    k = np.arange(W // 2 + 1)
    sk = np.sin(k * dlam / 2) ** 2
    table = np.full((band.size, 2 * D + 1), -1, np.int32)
    for dj in range(-D, D + 1):
        rows = band + dj
        ok = (rows >= 0) & (rows < H)
        p1, p2 = phi[band[ok]], phi[rows[ok]]
        hav = np.sin((p2 - p1) / 2)[:, None] ** 2 + (np.cos(p1) * np.cos(p2))[:, None] * sk[None, :]
        dist = 2 * EARTH_RADIUS_KM * np.arcsin(np.sqrt(np.minimum(hav, 1.0)))
        table[ok, dj + D] = (dist <= radius_km).sum(axis=1) - 1           # the distance grows with k up to half the circle
    return table, D


def row_coefficients(lat, lon) -> np.ndarray:
    phi = np.radians(np.asarray(lat, np.float64))
    dlam = _uniform_lon(lon)
    a = EARTH_RADIUS_KM * 1e3
    rowc = np.zeros((phi.size, 4), np.float64)
    c, cn, cs = np.cos(phi[1:-1]), np.cos(phi[2:]), np.cos(phi[:-2])
    dphi = phi[2:] - phi[:-2]
    rowc[1:-1, 0] = 1.0 / (2 * a * c * dlam)
    rowc[1:-1, 1] = cn / (a * c * dphi)
    rowc[1:-1, 2] = cs / (a * c * dphi)
    rowc[1:-1, 3] = np.sign(phi[1:-1])
    return rowc.astype(np.float32)


_geometry_cache: dict = {}


def geometry(lat, lon, cfg: TrackerConfig | None = None, warm_core: bool = True) -> Geometry:
    """The tables of include/skyrim_track.h for a grid and a configuration, in float64 on the host; cached per (grid, radii, band).
    ValueError when a half-width reaches W / 2, a window holds the first or the last row of the grid, or the 3 x 3 neighbourhood of a
    band row is not inside its msl window."""
    cfg = as_config(cfg)
    lat, lon = np.asarray(lat, np.float64), np.asarray(lon, np.float64)
    key = (lat.tobytes(), lon.tobytes(), cfg.radii(), float(cfg.lat_max), bool(warm_core))
    hit = _geometry_cache.get(key)
    if hit is not None:
        return hit
    H, W = lat.size, lon.size
    step = np.diff(lat)
    if H < 3 or not (np.all(step > 0) or np.all(step < 0)) or np.any(np.abs(lat) > 90):
        raise ValueError("tracking needs a strictly monotonic latitude axis in degrees of at least 3 rows")
    inside = np.nonzero(np.abs(lat) <= cfg.lat_max)[0]
    if inside.size == 0:
        raise ValueError(f"no grid row lies within lat_max = {cfg.lat_max}")
    j0, j1 = int(inside[0]), int(inside[-1]) + 1
    h, d = {}, {}
    for name, radius in zip(CRITERIA, cfg.radii()):
        if name == "core" and not warm_core:
            continue
        if not radius > 0:
            raise ValueError(f"r_{name}_km = {radius}: a radius is positive")
        table, D = half_widths(lat, lon, j0, j1, radius)
        rows = np.arange(j0, j1)[:, None] + np.arange(-D, D + 1)[None, :]
        widest = int(np.where((rows > 0) & (rows < H - 1), table, -1).max())         # (at a pole every longitude is equally far)
        if widest >= W // 2:
            raise ValueError(f"r_{name}_km = {radius}: a window is {2 * widest + 1} points wide on a circle of {W}; "
                             f"lower lat_max or the radius")
        if j0 - D < 1 or j1 - 1 + D > H - 2:
            raise ValueError(f"r_{name}_km = {radius}: the window of a row within lat_max = {cfg.lat_max} reaches the first or the last row "
                             f"of the grid (a pole row); lower lat_max or the radius")
        h[name], d[name] = table, D
    D = d["msl"]
    if D < 1 or h["msl"][:, D - 1:D + 2].min() < 1:
        raise ValueError(f"r_msl_km = {cfg.r_msl_km}: the msl window of a band row does not hold its 3 x 3 neighbourhood (the grid spacing "
                         f"is coarser than the radius)")
    geo = Geometry(j0, j1, h, d, row_coefficients(lat, lon), lat, lon)
    _geometry_cache[key] = geo
    return geo


_device_cache: dict = {}


def _device_geometry(geo: Geometry, device):
    import torch
    key = (id(geo), str(device))
    hit = _device_cache.get(key)
    if hit is None:
        hit = dict(geo=geo, rowc=torch.from_numpy(geo.rowc).to(device), **{k: torch.from_numpy(v).to(device) for k, v in geo.h.items()})
        _device_cache[key] = hit                                # (holds ``geo``: its id stays taken while the entry lives)
    return hit


# ---- the op ------------------------------------------------------------------------------------------------------------------------------ #
def workspace_bytes(M: int, Hb: int, W: int) -> int:
    return int(load_library().sktrack_workspace_bytes(M, Hb, W))


def detect(members, table, channels, band, thresholds, h_msl, h_vort, h_wind, h_core, rowc, records, count, workspace) -> None:
    """One ``sktrack_detect``: the M ``members`` (equal-shaped contiguous float32 (C, H, W) device tensors; ``table`` =
    ``ensemble.member_table(members)``).  ``channels``: the seven indices msl, u10, v10, u850, v850, z_up, z_lo (the last two -1: no warm
    core, ``h_core`` may then be None); ``band`` = (j0, j1); ``thresholds`` = (thr_msl, thr_vort, thr_wind, thr_core); ``h_*``: int32
    (Hb, 2 D + 1) device tables; ``rowc``: float32 (H, 4); ``records``: uint8, 32 bytes per record (its size is the capacity);
    ``count``: one int32; ``workspace``: uint8.  Queued on torch's current stream.  As in ``verify.score``, the contents of ``table``
    are trusted to be the addresses of ``members``."""
    import torch
    M, dev, _ = member_set(members, table, "track_detect", MAX_MEMBERS)
    C, H, W = members[0].shape
    channels, thresholds = [int(c) for c in channels], [float(t) for t in thresholds]
    if len(channels) != 7 or len(thresholds) != 4 or len(band) != 2:
        raise ValueError("track_detect: seven channel indices, a band (j0, j1) and four thresholds")
    j0, j1 = int(band[0]), int(band[1])
    core = channels[5] != -1 or channels[6] != -1
    d = TrackDesc()
    d.members, d.M, d.C, d.H, d.W = table.data_ptr(), M, C, H, W
    d.ch_msl, d.ch_u10, d.ch_v10, d.ch_u850, d.ch_v850, d.ch_zup, d.ch_zlo = channels
    d.j0, d.j1 = j0, j1
    d.thr_msl, d.thr_vort, d.thr_wind, d.thr_core = thresholds
    for name, t in (("msl", h_msl), ("vort", h_vort), ("wind", h_wind), ("core", h_core)):
        if name == "core" and not core:
            continue
        native.tensor_ptr(t, f"track_detect: h_{name}", torch.int32, dev)
        if t.dim() != 2 or t.shape[0] != j1 - j0 or t.shape[1] % 2 != 1:
            raise ValueError(f"track_detect: h_{name} must be (j1 - j0, 2 D + 1)")
        setattr(d, f"h_{name}", t.data_ptr())
        setattr(d, f"d_{name}", t.shape[1] // 2)
    d.rowc = native.tensor_ptr(rowc, "track_detect: rowc", torch.float32, dev)
    if tuple(rowc.shape) != (H, 4):
        raise ValueError(f"track_detect: rowc must be ({H}, 4)")
    d.records = native.tensor_ptr(records, "track_detect: records", torch.uint8, dev)
    if records.numel() % RECORD.itemsize:
        raise ValueError(f"track_detect: the record buffer holds whole records of {RECORD.itemsize} bytes")
    d.capacity = records.numel() // RECORD.itemsize
    d.count = native.tensor_ptr(count, "track_detect: count", torch.int32, dev)
    d.workspace, d.workspace_bytes = native.tensor_ptr(workspace, "track_detect: workspace", torch.uint8, dev), workspace.numel()
    lib = load_library()
    need = lib.sktrack_workspace_bytes(M, j1 - j0, W)
    if need and d.workspace_bytes < need:
        raise ValueError(f"track_detect: the workspace holds {d.workspace_bytes} bytes, {need} are needed")
    with torch.cuda.device(dev):
        native.check(lib.sktrack_detect(ctypes.byref(d), native.stream(dev)), "sktrack_detect", lib)


# ---- great circles on the host --------------------------------------------------------------------------------------------------------- #
def great_circle_km(lat1, lon1, lat2, lon2):
    """Haversine distance in km; degrees in, arrays broadcast."""
    p1, p2 = np.radians(np.asarray(lat1, np.float64)), np.radians(np.asarray(lat2, np.float64))
    dl = np.radians(np.asarray(lon2, np.float64) - np.asarray(lon1, np.float64))
    hav = np.sin((p2 - p1) / 2) ** 2 + np.cos(p1) * np.cos(p2) * np.sin(dl / 2) ** 2
    return 2 * EARTH_RADIUS_KM * np.arcsin(np.sqrt(np.minimum(hav, 1.0)))


# ---- linking ----------------------------------------------------------------------------------------------------------------------------- #
FIELDS = ("lat", "lon", "msl", "wind", "vort", "core")


def _hours(t0, t1) -> float:
    return float((np.datetime64(t1, "s") - np.datetime64(t0, "s")) / np.timedelta64(1, "s")) / 3600.0


def link(times, candidates, max_speed_kmh: float = 90.0, min_points: int = 2) -> list:
    """Tracks of ONE member.  ``candidates[t]``: the candidates of ``times[t]`` as a list of dicts with the keys of ``FIELDS``, in the
    order (j, i).  A live track predicts its last point plus, once it has two, its last displacement (longitude wraps); every
    (track, candidate) pair within ``max_speed_kmh`` x dt of the prediction is a possible match; matches are taken greedily by
    increasing distance, ties by (track id, candidate index).  An unmatched candidate starts a track, an unmatched track ends (no gap
    is bridged); tracks of fewer than ``min_points`` points are dropped.  Returns dicts {times, lat, lon, msl, wind, vort, core} in
    the order the tracks started."""
    tracks, live = [], []
    for t, (time, cands) in enumerate(zip(times, candidates)):
        taken, matched = set(), {}
        if live and cands:
            reach = float(max_speed_kmh) * _hours(times[t - 1], time)
            pairs = []
            for tid in live:
                tr = tracks[tid]
                plat, plon = tr["lat"][-1], tr["lon"][-1]
                if len(tr["lat"]) >= 2:
                    plat = min(90.0, max(-90.0, plat + (tr["lat"][-1] - tr["lat"][-2])))
                    plon = (plon + ((tr["lon"][-1] - tr["lon"][-2] + 180.0) % 360.0 - 180.0)) % 360.0
                for k, c in enumerate(cands):
                    dist = float(great_circle_km(plat, plon, c["lat"], c["lon"]))
                    if dist <= reach:
                        pairs.append((dist, tid, k))
            for dist, tid, k in sorted(pairs):
                if tid not in matched and k not in taken:
                    matched[tid] = k
                    taken.add(k)
        nxt = []
        for tid in live:
            if tid in matched:
                c = cands[matched[tid]]
                tracks[tid]["times"].append(time)
                for f in FIELDS:
                    tracks[tid][f].append(float(c[f]))
                nxt.append(tid)
        for k, c in enumerate(cands):
            if k not in taken:
                tracks.append(dict(times=[time], **{f: [float(c[f])] for f in FIELDS}))
                nxt.append(len(tracks) - 1)
        live = sorted(nxt)
    return [tr for tr in tracks if len(tr["times"]) >= int(min_points)]


# ---- the result -------------------------------------------------------------------------------------------------------------------------- #
class Tracks:
    """What tracking returns.  ``tracks``: a list of dicts {member, times, lat, lon, msl, wind, vort, core} (lists of equal length,
    longitudes in [0, 360)); ``criteria``: the criteria in effect (radii, thresholds, band, whether the warm core was applied and why
    not); ``times``: every lead time that was searched."""

    def __init__(self, model_name, n_members, times, lat, lon, tracks, criteria, forecast_id=""):
        self.model_name, self.n_members, self.forecast_id = model_name, int(n_members), forecast_id
        self.times, self.tracks, self.criteria = list(times), list(tracks), dict(criteria)
        self.lat, self.lon = np.asarray(lat, np.float64), np.asarray(lon, np.float64)

    def __len__(self):
        return len(self.tracks)

    def __iter__(self):
        return iter(self.tracks)

    def strike_probability(self, radius_km: float = 120.0):
        """DataArray(lat, lon): the fraction of members with at least one track point within ``radius_km`` of the grid point."""
        from .labeled import DataArray
        hit = np.zeros((self.n_members, self.lat.size, self.lon.size), bool)
        for tr in self.tracks:
            for plat, plon in zip(tr["lat"], tr["lon"]):
                rows = np.nonzero(EARTH_RADIUS_KM * np.abs(np.radians(self.lat - plat)) <= radius_km)[0]
                if rows.size:
                    hit[tr["member"], rows] |= great_circle_km(plat, plon, self.lat[rows][:, None], self.lon[None, :]) <= radius_km
        return DataArray(hit.sum(axis=0) / float(self.n_members), ["lat", "lon"], dict(lat=self.lat, lon=self.lon))

    def file_name(self) -> str:
        return f"{self.model_name}-tracks.json" if self.n_members == 1 else f"{self.model_name}-ens{self.n_members}-tracks.json"

    def to_json(self) -> str:
        def clean(v):                                           # JSON has no inf / NaN
            if isinstance(v, (list, tuple)):
                return [clean(x) for x in v]
            return None if isinstance(v, float) and not math.isfinite(v) else v
        doc = dict(model=self.model_name, n_members=self.n_members, forecast_id=self.forecast_id, times=[_iso(t) for t in self.times],
                   lat=self.lat.tolist(), lon=self.lon.tolist(), criteria={k: clean(v) for k, v in self.criteria.items()},
                   tracks=[dict(member=int(tr["member"]), times=[_iso(t) for t in tr["times"]], **{f: clean(list(tr[f])) for f in FIELDS})
                           for tr in self.tracks])
        return json.dumps(doc)

    def save(self, output_dir) -> str:
        """``{output_dir}/{forecast id}/{model}-tracks.json`` (``{model}-ens{M}-tracks.json`` for an ensemble); returns the path."""
        d = Path(output_dir) / self.forecast_id if self.forecast_id else Path(output_dir)
        d.mkdir(parents=True, exist_ok=True)
        path = d / self.file_name()
        path.write_text(self.to_json())
        return str(path)

    @classmethod
    def from_json(cls, text: str) -> "Tracks":
        doc = json.loads(text)
        when = datetime.datetime.fromisoformat
        nan = lambda a: [math.nan if v is None else float(v) for v in a]      # noqa: E731
        tracks = [dict(member=tr["member"], times=[when(t) for t in tr["times"]], **{f: nan(tr[f]) for f in FIELDS}) for tr in doc["tracks"]]
        crit = {k: (tuple(v) if isinstance(v, list) else v) for k, v in doc["criteria"].items()}
        if crit.get("thr_msl", 0.0) is None:
            crit["thr_msl"] = math.inf                          # (written as null: JSON has no inf)
        return cls(doc["model"], doc["n_members"], [when(t) for t in doc["times"]], doc["lat"], doc["lon"], tracks, crit,
                   doc.get("forecast_id", ""))

    @classmethod
    def load(cls, path) -> "Tracks":
        return cls.from_json(Path(path).read_text())


# ---- the drivers ------------------------------------------------------------------------------------------------------------------------- #
def check_request(model_name: str, names, lat, lon, n_members: int, cfg) -> tuple:
    """Every refusal that needs no device; returns (config, channel plan, geometry)."""
    if _world_size() > 1:
        raise NotImplementedError("cyclones are detected on one GPU from members that all lie there; members sharded over the ranks of "
                                  "a process group are out of scope (DESIGN.md 20)")
    if not 1 <= int(n_members) <= MAX_MEMBERS:
        raise ValueError(f"n_members = {n_members}: 1 to {MAX_MEMBERS} members can be tracked (SKTRACK_MAX_MEMBERS)")
    cfg = as_config(cfg)
    if cfg.capacity < 1 or cfg.min_points < 1 or not cfg.max_speed_kmh > 0:
        raise ValueError("capacity >= 1, min_points >= 1 and max_speed_kmh > 0")
    plan = channel_plan(names, cfg, model_name)
    return cfg, plan, geometry(lat, lon, cfg, plan.warm_core)


class LeadTracker:
    """Detects one lead time after the other on the device and gathers the candidate records; ``result()`` links them per member.
    ``names``: the forecast's channels in the order of its (C, H, W) states."""

    def __init__(self, model_name, names, lat, lon, n_members, config=None, device="cuda:0", forecast_id=""):
        self.cfg, self.plan, self.geo = check_request(model_name, names, lat, lon, n_members, config)
        self.model_name, self.names, self.M, self.forecast_id = model_name, list(names), int(n_members), forecast_id
        self.device = device
        self.times, self.records = [], []
        self._dev = None

    def _buffers(self):
        if self._dev is None:
            import torch
            dev = torch.device(self.device)
            g = _device_geometry(self.geo, dev)
            need = workspace_bytes(self.M, self.geo.j1 - self.geo.j0, len(self.geo.lon))
            self._dev = dict(g=g, records=torch.zeros(self.M * self.cfg.capacity * RECORD.itemsize, dtype=torch.uint8, device=dev),
                             count=torch.zeros(1, dtype=torch.int32, device=dev), ws=torch.empty(need, dtype=torch.uint8, device=dev))
        return self._dev

    def add(self, time, states, table=None) -> None:
        """Detect on the M device states (C, H, W) of valid time ``time``: ONE detect launch, then the counter and that many records
        cross to the host."""
        from .ensemble import member_table
        if len(states) != self.M:
            raise ValueError(f"{len(states)} states for a tracker of {self.M} members")
        b, p, c = self._buffers(), self.plan, self.cfg
        g = b["g"]
        table = member_table(states) if table is None else table
        detect(states, table, (p.msl, p.u10, p.v10, p.u850, p.v850, p.z_up, p.z_lo), (self.geo.j0, self.geo.j1),
               (c.thr_msl, c.thr_vort, c.thr_wind, c.thr_core), g["msl"], g["vort"], g["wind"], g.get("core"), g["rowc"], b["records"],
               b["count"], b["ws"])
        count, capacity = int(b["count"].item()), self.M * c.capacity
        if count > capacity:
            raise RuntimeError(f"cyclone detection found {count} candidates at {_iso(time)}, the record buffer holds {capacity} "
                               f"({c.capacity} per member): raise TrackerConfig.capacity or the thresholds")
        rec = b["records"][:count * RECORD.itemsize].cpu().numpy().view(RECORD)
        self.times.append(time)
        self.records.append(np.sort(rec, order=("member", "j", "i")))

    def candidates(self, t: int, member: int) -> list:
        """The candidates of lead time ``t`` and one member as the linker's dicts, in (j, i) order."""
        rec = self.records[t]
        return [dict(lat=float(self.geo.lat[r["j"]]), lon=float(self.geo.lon[r["i"]]) % 360.0, msl=float(r["msl"]), wind=float(r["wind"]),
                     vort=float(r["vort"]), core=float(r["core"])) for r in rec[rec["member"] == member]]

    def criteria(self) -> dict:
        crit = asdict(self.cfg)
        crit.update(band=(self.geo.j0, self.geo.j1), warm_core=self.plan.warm_core, note=self.plan.note)
        return crit

    def result(self) -> Tracks:
        tracks = []
        for m in range(self.M):
            for tr in link(self.times, [self.candidates(t, m) for t in range(len(self.times))], self.cfg.max_speed_kmh, self.cfg.min_points):
                tracks.append(dict(member=m, **tr))
        return Tracks(self.model_name, self.M, self.times, self.geo.lat, self.geo.lon, tracks, self.criteria(), self.forecast_id)


def track_model(gm, start_time: datetime.datetime, n_steps: int = 4, config=None, save: bool = False, save_config: dict | None = None) -> Tracks:
    """``GlobalModel.track_cyclones`` (core/models/base.py has the user-facing description)."""
    model = gm.model
    if n_steps < 0:
        raise ValueError("n_steps >= 0")
    check_request(gm.model_name, model.out_channel_names, model.grid.lat, model.grid.lon, 1, config)      # before anything of the device
    tracker = LeadTracker(gm.model_name, model.out_channel_names, model.grid.lat, model.grid.lon, 1, config, device=model.device)
    require_gpu(model.device, "track_cyclones detects with HIP kernels where the forecast lies: the model must be on a GPU")
    run_model(gm, start_time, n_steps, lambda k, time, state: tracker.add(time, [state]))
    return _finish(tracker.result(), save, save_config)


def track_prediction(pred, config=None, device="cuda:0", model_name: str = "") -> Tracks:
    """Tracks of a forecast that already exists: a ``GlobalPrediction``, a (time, channel, lat, lon) DataArray, a saved netCDF file or
    zarr store, or a list of such files (their time entries in order, duplicates of a valid time searched once).  Each time entry is
    uploaded on its own and goes through the same kernels as ``track_cyclones``."""
    saved = open_saved(pred, "track_prediction")
    tracker = LeadTracker(model_name or saved.model_name or "forecast", saved.names, saved.lat, saved.lon, 1, config, device=device)
    require_gpu(device, "track_prediction detects with HIP kernels: it needs a GPU", present=True)
    for _, time, state in saved.states(tracker.device):
        tracker.add(time, [state])
    return tracker.result()
