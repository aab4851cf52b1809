"""Weather objects (include/skyrim_object.h): the contiguous regions where a field is beyond a threshold -- an atmospheric
river, a gale area, a CAPE pool, a cold pool -- are labelled, numbered and measured on the device, where the members lie in HBM.  Only
128-byte records and one int32 count plane per request plane cross to the host.

Layers:

* the binding of libskyrim_object.so (``SPEC``, ``load_library``, ``label``, ``attributes``, ``probability``); the same calls are
  ``torch.ops.skyrim_hip.object_label`` / ``object_attributes`` / ``object_probability``.  None of them has a CPU fallback;
* ``parse_request`` (what is sought: planes, connectivity, ``min_pixels``, ``capacity`` and the host's filters), ``value_scale`` and
  ``tables`` (the float64 geometry tables the kernels turn into integers);
* ``properties`` (records -> area, centroid, axes, mean, extreme, in float64 on the host) and ``keep_mask`` (the filters);
* ``Objects`` (the result, its probability planes, its verification against a truth and its files);
* the drivers: ``LeadObjects`` (what ``ensemble.run`` calls at every saved lead time with ``objects=``), ``objects_model``
  (``GlobalModel.object_forecast``) and ``objects_prediction`` for forecasts that are already on disk.

Rows are not joined across the poles, and with a global longitude circle column W - 1 neighbours column 0 (the header has the details).
"""
from __future__ import annotations

import ctypes
import datetime
import json
import math
import warnings
from dataclasses import dataclass
from pathlib import Path

import numpy as np

from . import native
from .common import finish as _finish, iso as _iso, world_size as _world_size
from .leads import open_saved, require_gpu, run_model
from .members import member_set

MAX_MEMBERS, MAX_PLANES, MAX_CAPACITY = 64, 8, 1 << 20          # include/skyrim_object.h SKOBJ_MAX_MEMBERS, SKOBJ_MAX_PLANES
CLAMP = 4096.0                                                  # SKOBJ_CLAMP
EARTH_RADIUS_KM = 6371.0
SCALE = 2.0 ** 52
SUMS = ("area", "sx", "sy", "sz", "sxx", "sxy", "sxz", "syy", "syz", "szz", "sum_v")
RECORD = np.dtype([(k, "<i4") for k in ("member", "plane", "id", "root", "n_pixels", "jmin", "jmax", "saturated")]
                  + [(k, "<i8") for k in SUMS] + [("ext_value", "<f4"), ("ext_index", "<i4")])          # skobj_record, 128 bytes
PROPS = np.dtype([("id", "<i4"), ("n_pixels", "<i4"), ("saturated", "<i4"), ("area_km2", "<f8"), ("lat", "<f8"), ("lon", "<f8"),
                  ("length_km", "<f8"), ("width_km", "<f8"), ("orientation_deg", "<f8"), ("mean", "<f8"), ("extreme", "<f8"),
                  ("extreme_lat", "<f8"), ("extreme_lon", "<f8"), ("keep", "?")])
FILTERS = ("min_area_km2", "min_length_km", "min_elongation")
OPTIONS = dict(connectivity=8, min_pixels=1, capacity=1024)
_P = ctypes.c_void_p


class PlaneC(ctypes.Structure):
    """skobj_plane."""
    _fields_ = [("channel", ctypes.c_int32), ("threshold", ctypes.c_float), ("direction", ctypes.c_int32), ("connectivity", ctypes.c_int32),
                ("value_scale", ctypes.c_float), ("pad", ctypes.c_int32)]


class ObjDesc(ctypes.Structure):
    """skobj_desc."""
    _fields_ = [("members", _P), ("M", ctypes.c_int), ("C", ctypes.c_int), ("H", ctypes.c_int), ("W", ctypes.c_int), ("P", ctypes.c_int),
                ("planes", PlaneC * MAX_PLANES), ("periodic", ctypes.c_int), ("min_pixels", ctypes.c_int), ("capacity", ctypes.c_int),
                ("labels", _P), ("ids", _P), ("n_found", _P), ("workspace", _P), ("workspace_bytes", ctypes.c_size_t),
                ("row_tables", _P), ("col_tables", _P), ("records", _P), ("keep", _P), ("counts", _P)]


_CALL = (ctypes.c_int, [ctypes.POINTER(ObjDesc), _P])
SPEC = native.Spec("skyrim_object", "SKYRIM_OBJECT_LIB", "skobj", 1, {          # include/skyrim_object.h SKOBJ_ABI_VERSION
    "skobj_abi_version": (ctypes.c_int, []),
    "skobj_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "skobj_label": _CALL,
    "skobj_attributes": _CALL,
    "skobj_probability": _CALL,
}, " -- weather objects have no torch fallback")
EXPORTS, ABI_VERSION = SPEC.exports, SPEC.abi

_lib = None


def load_library() -> ctypes.CDLL:
    """libskyrim_object.so (built in-tree by ``__graft_entry__.build()`` / ``make -C skyrim_amd/csrc``)."""
    global _lib
    if _lib is None:
        _lib = native.load(SPEC)
    return _lib


# ---- what is sought -------------------------------------------------------------------------------------------------------------------- #
def value_scale(threshold: float) -> float:
    """The power of two at or above |threshold| (1 for a threshold of 0): what ``sum_v`` divides the values by."""
    t = abs(float(threshold))
    if t == 0.0:
        return 1.0
    m, e = math.frexp(t)                                        # t = m 2^e, 0.5 <= m < 1
    return min(max(math.ldexp(1.0, e - 1 if m == 0.5 else e), 2.0 ** -126), 2.0 ** 127)          # (a normal fp32 number)


@dataclass(frozen=True)
class Plane:
    """One thresholded field: the objects of ``name`` at or above (``direction`` +1) or at or below (-1) ``threshold``; the filters are the
    host's (an object that fails one is not kept: it is in the records, but not in the probability)."""
    name: str
    direction: int
    threshold: float
    value_scale: float
    min_area_km2: float = 0.0
    min_length_km: float = 0.0
    min_elongation: float = 0.0

    @property
    def label(self) -> str:
        return f"{self.name}{'>=' if self.direction > 0 else '<='}{self.threshold:g}"


@dataclass(frozen=True)
class Request:
    planes: tuple
    connectivity: int = 8
    min_pixels: int = 1
    capacity: int = 1024

    def as_dict(self) -> dict:
        return dict(planes=[dict(p.__dict__, label=p.label) for p in self.planes], connectivity=self.connectivity, min_pixels=self.min_pixels,
                    capacity=self.capacity)


def parse_request(objects, known, n_members: int = 1) -> Request:
    """The normalised request of ``objects={channel: {"above": [...], "below": [...], <filters>}, <options>}``.  ``known``: the channels
    (and derived fields) that may be named.  Refused before anything touches the device: unknown channels, keys and options, no plane
    or more than 8, more than 64 members, a threshold that is not finite in fp32."""
    if isinstance(objects, Request):
        req = objects
    else:
        if not isinstance(objects, dict):
            raise ValueError(f"objects: a dict {{channel: {{'above': [...], 'below': [...]}}, ...}}, not {type(objects).__name__}")
        opts = {k: int(objects.get(k, v)) for k, v in OPTIONS.items()}
        planes = []
        for name, spec in objects.items():
            if name in OPTIONS:
                continue
            if not isinstance(spec, dict):
                raise ValueError(f"objects[{name!r}]: a dict with 'above' and / or 'below' thresholds")
            odd = [k for k in spec if k not in ("above", "below") + FILTERS]
            if odd:
                raise ValueError(f"objects[{name!r}]: unknown keys {odd}; 'above', 'below' and the filters {list(FILTERS)} are understood")
            filt = {k: float(spec.get(k, 0.0)) for k in FILTERS}
            if any(not v >= 0 for v in filt.values()):
                raise ValueError(f"objects[{name!r}]: the filters are >= 0")
            n0 = len(planes)
            for key, direction in (("above", 1), ("below", -1)):
                vals = spec.get(key, [])
                for thr in ([vals] if np.isscalar(vals) else list(vals)):
                    thr = float(np.float32(thr))
                    if not math.isfinite(thr):
                        raise ValueError(f"objects[{name!r}]: the threshold {thr} is not finite in fp32")
                    planes.append(Plane(str(name), direction, thr, value_scale(thr), **filt))
            if len(planes) == n0:
                raise ValueError(f"objects[{name!r}]: no threshold under 'above' or 'below'")
        req = Request(tuple(planes), **opts)
    unknown = sorted({p.name for p in req.planes if p.name not in list(known)})
    if unknown:
        raise ValueError(f"objects: {unknown} are neither output channels of this forecast nor derived fields named in derived=")
    if not 1 <= len(req.planes) <= MAX_PLANES:
        raise ValueError(f"objects: {len(req.planes)} planes (channel x threshold); 1 to {MAX_PLANES} are supported (SKOBJ_MAX_PLANES)")
    if len({p.label for p in req.planes}) != len(req.planes):
        raise ValueError("objects: a plane is named twice")
    if not 1 <= int(n_members) <= MAX_MEMBERS:
        raise ValueError(f"n_members = {n_members}: objects are found in 1 to {MAX_MEMBERS} members (SKOBJ_MAX_MEMBERS)")
    if req.connectivity not in (4, 8):
        raise ValueError(f"objects: connectivity is 4 or 8, not {req.connectivity}")
    if req.min_pixels < 1 or not 1 <= req.capacity <= MAX_CAPACITY:
        raise ValueError(f"objects: min_pixels >= 1 and 1 <= capacity <= {MAX_CAPACITY}")
    return req


# ---- geometry -------------------------------------------------------------------------------------------------------------------------- #
@dataclass
class Geometry:
    """``row``: float64 (6, H) = a, a cos, a sin, a cos^2, a cos sin, a sin^2 of the latitude, times 2^52, with ``a`` the fraction of
    the sphere's area of one cell of the row; ``col``: float64 (5, W) = cos, sin, cos^2, cos sin, sin^2 of the longitude; ``periodic``:
    the longitudes are a full circle."""
    row: np.ndarray
    col: np.ndarray
    periodic: bool
    lat: np.ndarray
    lon: np.ndarray


def is_periodic(lon) -> bool:
    """Uniform longitudes that cover the circle (what ``tracks._uniform_lon`` demands), as opposed to a regional box."""
    lon = np.asarray(lon, np.float64)
    if lon.size < 3:
        return False
    step = 360.0 / lon.size
    return bool(np.allclose(np.diff(lon), step, rtol=0, atol=1e-6 * step))


def cell_fractions(lat, lon) -> np.ndarray:
    """a_j (H,): a cell reaches half-way to its neighbours; a first or last row AT a pole is a half cell, one short of it reaches on by
    half a row (at most to the pole).  Over a global grid W sum(a_j) = 1."""
    lat, lon = np.asarray(lat, np.float64), np.asarray(lon, np.float64)
    H, W = lat.size, lon.size
    step = np.diff(lat)
    if H < 2 or W < 2 or not (np.all(step > 0) or np.all(step < 0)) or np.any(np.abs(lat) > 90):
        raise ValueError("objects need a strictly monotonic latitude axis in degrees of at least 2 rows and at least 2 longitudes")
    dlon = np.diff(lon)
    if not np.allclose(dlon, dlon[0], rtol=0, atol=1e-6 * abs(dlon[0])) or dlon[0] == 0:
        raise ValueError("objects need uniform longitudes")
    edges = np.empty(H + 1)
    edges[1:-1] = 0.5 * (lat[1:] + lat[:-1])
    edges[0], edges[-1] = lat[0] - 0.5 * step[0], lat[-1] + 0.5 * step[-1]
    edges = np.clip(edges, -90.0, 90.0)
    band = np.abs(np.diff(np.sin(np.radians(edges)))) / 2.0     # the row's share of the sphere
    return band * (abs(dlon[0]) / 360.0)


_geometry_cache: dict = {}


def tables(lat, lon) -> Geometry:
    """The tables of include/skyrim_object.h for a grid, made in float64; cached per grid."""
    lat, lon = np.asarray(lat, np.float64), np.asarray(lon, np.float64)
    key = (lat.tobytes(), lon.tobytes())
    hit = _geometry_cache.get(key)
    if hit is None:
        a = cell_fractions(lat, lon) * SCALE
        phi, lam = np.radians(lat), np.radians(lon)
        c, s, cl, sl = np.cos(phi), np.sin(phi), np.cos(lam), np.sin(lam)
        row = np.ascontiguousarray(np.stack([a, a * c, a * s, a * (c * c), a * (c * s), a * (s * s)]))
        col = np.ascontiguousarray(np.stack([cl, sl, cl * cl, cl * sl, sl * sl]))
        hit = _geometry_cache[key] = Geometry(row, col, is_periodic(lon), lat, lon)
    return hit


# ---- the ops --------------------------------------------------------------------------------------------------------------------------- #
def workspace_bytes(M: int, P: int, H: int, W: int) -> int:
    return int(load_library().skobj_workspace_bytes(M, P, H, W))


def _shape(d: ObjDesc, M, C, H, W, planes, capacity) -> None:
    d.M, d.C, d.H, d.W, d.P, d.capacity = int(M), int(C), int(H), int(W), len(planes), int(capacity)
    for k, pl in enumerate(planes[:MAX_PLANES]):
        channel, threshold, direction, connectivity, scale = pl
        d.planes[k] = PlaneC(int(channel), float(threshold), int(direction), int(connectivity), float(scale), 0)


def _plane_tensor(t, what, dev, M, P, H, W):
    import torch
    ptr = native.tensor_ptr(t, what, torch.int32, dev)
    if t.numel() != M * P * H * W:
        raise ValueError(f"{what} must hold (M, P, H, W) = ({M}, {P}, {H}, {W}) int32")
    return ptr


def label(members, table, planes, periodic, min_pixels, capacity, labels, ids, n_found, workspace) -> None:
    """One ``skobj_label``: the M ``members`` (equal-shaped contiguous float32 (C, H, W) device tensors, ``table`` =
    ``member_table(members)``); ``planes``: up to 8 tuples (channel, threshold, direction, connectivity, value_scale); ``labels`` and
    ``ids``: int32 (M, P, H, W); ``n_found``: int32 (M, P); ``workspace``: uint8.  Queued on torch's current stream."""
    import torch
    M, dev, _ = member_set(members, table, "object_label", MAX_MEMBERS)
    C, H, W = members[0].shape
    planes = [tuple(p) for p in planes]
    d = ObjDesc()
    _shape(d, M, C, H, W, planes, capacity)
    P = len(planes)
    d.members, d.periodic, d.min_pixels = table.data_ptr(), int(bool(periodic)), int(min_pixels)
    d.labels = _plane_tensor(labels, "object_label: labels", dev, M, P, H, W)
    d.ids = _plane_tensor(ids, "object_label: ids", dev, M, P, H, W)
    d.n_found = native.tensor_ptr(n_found, "object_label: n_found", torch.int32, dev)
    if n_found.numel() != M * P:
        raise ValueError(f"object_label: n_found must hold (M, P) = ({M}, {P}) int32")
    d.workspace, d.workspace_bytes = native.tensor_ptr(workspace, "object_label: workspace", torch.uint8, dev), workspace.numel()
    lib = load_library()
    need = lib.skobj_workspace_bytes(M, P, H, W)
    if need and d.workspace_bytes < need:
        raise ValueError(f"object_label: the workspace holds {d.workspace_bytes} bytes, {need} are needed")
    with torch.cuda.device(dev):
        native.check(lib.skobj_label(ctypes.byref(d), native.stream(dev)), "skobj_label", lib)


def attributes(members, table, planes, capacity, labels, ids, n_found, row_tables, col_tables, records) -> None:
    """One ``skobj_attributes`` on the planes ``label`` made: ``row_tables`` float64 (6, H), ``col_tables`` float64 (5, W), ``records``:
    uint8, 128 bytes per record, (M, P, capacity) records."""
    import torch
    M, dev, _ = member_set(members, table, "object_attributes", MAX_MEMBERS)
    C, H, W = members[0].shape
    planes = [tuple(p) for p in planes]
    d = ObjDesc()
    _shape(d, M, C, H, W, planes, capacity)
    P = len(planes)
    d.members = table.data_ptr()
    d.labels = _plane_tensor(labels, "object_attributes: labels", dev, M, P, H, W)
    d.ids = _plane_tensor(ids, "object_attributes: ids", dev, M, P, H, W)
    d.n_found = native.tensor_ptr(n_found, "object_attributes: n_found", torch.int32, dev)
    d.row_tables = native.tensor_ptr(row_tables, "object_attributes: row_tables", torch.float64, dev)
    d.col_tables = native.tensor_ptr(col_tables, "object_attributes: col_tables", torch.float64, dev)
    if n_found.numel() != M * P or tuple(row_tables.shape) != (6, H) or tuple(col_tables.shape) != (5, W):
        raise ValueError(f"object_attributes: n_found is (M, P), row_tables (6, {H}) and col_tables (5, {W})")
    d.records = native.tensor_ptr(records, "object_attributes: records", torch.uint8, dev)
    if records.numel() != M * P * int(capacity) * RECORD.itemsize:
        raise ValueError(f"object_attributes: the record buffer holds M P capacity records of {RECORD.itemsize} bytes")
    lib = load_library()
    with torch.cuda.device(dev):
        native.check(lib.skobj_attributes(ctypes.byref(d), native.stream(dev)), "skobj_attributes", lib)


def probability(ids, keep, counts) -> None:
    """One ``skobj_probability``: ``ids`` int32 (M, P, H, W), ``keep`` uint8 (M, P, capacity + 1) with entry 0 of every row 0,
    ``counts`` int32 (P, H, W) = the members whose kept object covers the point."""
    import torch
    if not isinstance(ids, torch.Tensor) or ids.dim() != 4 or not isinstance(keep, torch.Tensor) or keep.dim() != 3:
        raise ValueError("object_probability: ids are (M, P, H, W), keep is (M, P, capacity + 1)")
    M, P, H, W = ids.shape
    dev = ids.device
    d = ObjDesc()
    d.M, d.C, d.H, d.W, d.P, d.capacity = M, 1, H, W, P, keep.shape[2] - 1
    d.ids = native.tensor_ptr(ids, "object_probability: ids", torch.int32, dev)
    d.keep = native.tensor_ptr(keep, "object_probability: keep", torch.uint8, dev)
    d.counts = native.tensor_ptr(counts, "object_probability: counts", torch.int32, dev)
    if tuple(keep.shape[:2]) != (M, P) or counts.numel() != P * H * W:
        raise ValueError(f"object_probability: keep is ({M}, {P}, capacity + 1) and counts ({P}, {H}, {W})")
    lib = load_library()
    with torch.cuda.device(dev):
        native.check(lib.skobj_probability(ctypes.byref(d), native.stream(dev)), "skobj_probability", lib)


# ---- records -> properties, in float64 on the host ---------------------------------------------------------------------------------------- #
def great_circle_km(lat1, lon1, lat2, lon2):
    from .tracks import great_circle_km as gc
    return gc(lat1, lon1, lat2, lon2)


def properties(records, lat, lon, scale: float) -> np.ndarray:
    """The ``PROPS`` array of the ``RECORD`` array of ONE plane (``scale``: its value_scale).  Area: the integer sum over 2^52 of the
    sphere.  Centroid: the direction of the mean unit vector, so the date line needs no special case.  Axes: the 3 x 3 second-moment
    matrix about the mean vector is decomposed; the eigenvector nearest the centroid's direction is the radial one (the sagitta of a
    curved object), the other two give ``length_km`` >= ``width_km`` = 4 R sqrt(eigenvalue), the axes of a uniform ellipse with those
    variances; ``orientation_deg`` in [0, 180) is the major axis' angle from local east, counter-clockwise."""
    lat, lon = np.asarray(lat, np.float64), np.asarray(lon, np.float64)
    W = lon.size
    out = np.zeros(len(records), PROPS)
    for k, r in enumerate(records):
        area = float(r["area"])
        o = out[k]
        o["id"], o["n_pixels"], o["saturated"], o["keep"] = r["id"], r["n_pixels"], r["saturated"], True
        o["area_km2"] = 4.0 * math.pi * EARTH_RADIUS_KM ** 2 * (area / SCALE)
        mu = np.array([float(r["sx"]), float(r["sy"]), float(r["sz"])]) / area
        norm = float(np.linalg.norm(mu))
        c = mu / norm if norm > 0 else np.array([1.0, 0.0, 0.0])
        o["lat"] = math.degrees(math.asin(max(-1.0, min(1.0, c[2]))))
        o["lon"] = math.degrees(math.atan2(c[1], c[0])) % 360.0
        S = np.array([[r["sxx"], r["sxy"], r["sxz"]], [r["sxy"], r["syy"], r["syz"]], [r["sxz"], r["syz"], r["szz"]]], np.float64) / area
        ev, vec = np.linalg.eigh(S - np.outer(mu, mu))
        radial = int(np.argmax(np.abs(vec.T @ c)))
        rest = sorted((i for i in range(3) if i != radial), key=lambda i: -ev[i])
        o["length_km"], o["width_km"] = (4.0 * EARTH_RADIUS_KM * math.sqrt(max(ev[i], 0.0)) for i in rest)
        lam, phi = math.atan2(c[1], c[0]), math.asin(max(-1.0, min(1.0, c[2])))
        east = np.array([-math.sin(lam), math.cos(lam), 0.0])
        north = np.array([-math.sin(phi) * math.cos(lam), -math.sin(phi) * math.sin(lam), math.cos(phi)])
        major = vec[:, rest[0]]
        o["orientation_deg"] = math.degrees(math.atan2(float(major @ north), float(major @ east))) % 180.0
        o["mean"] = float(scale) * float(r["sum_v"]) / (area / 4096.0)
        o["extreme"] = float(r["ext_value"])
        o["extreme_lat"], o["extreme_lon"] = lat[int(r["ext_index"]) // W], lon[int(r["ext_index"]) % W]
    return out


def keep_mask(props: np.ndarray, plane: Plane) -> np.ndarray:
    """The objects that pass the plane's filters (elongation = length / width; a width of 0 passes)."""
    keep = (props["area_km2"] >= plane.min_area_km2) & (props["length_km"] >= plane.min_length_km)
    if plane.min_elongation > 0:
        keep &= props["length_km"] >= plane.min_elongation * props["width_km"]
    return keep


# ---- the result ------------------------------------------------------------------------------------------------------------------------ #
class Objects:
    """What the object routes return.  ``objects[t][m][p]``: the ``PROPS`` array of lead time t, member m and plane p, in the order of the
    ids; ``counts[t][p]``: int32 (lat, lon), the members whose kept object covers the point; ``n_found``: int (time, member, plane), all
    qualifying components, also beyond ``capacity``; ``truth[t][p]``: the truth's ``PROPS`` array (None without a truth) and
    ``truth_probability[t][p]``: per truth object the mean of the probability plane over its points."""

    def __init__(self, model_name, n_members, times, lat, lon, request: Request, objects, counts, n_found, truth=None, truth_probability=None,
                 forecast_id=""):
        self.model_name, self.n_members, self.forecast_id = model_name, int(n_members), forecast_id
        self.times, self.request = list(times), request
        self.lat, self.lon = np.asarray(lat, np.float64), np.asarray(lon, np.float64)
        self.objects, self.counts = objects, counts
        self.n_found = np.asarray(n_found, np.int64).reshape(len(self.times), self.n_members, len(request.planes))
        self.truth, self.truth_probability = truth, truth_probability
        self.truncated = self.n_found > request.capacity
        if self.truncated.any():
            warnings.warn(f"objects: {int(self.truncated.sum())} (lead time, member, plane) entries found more than capacity = "
                          f"{request.capacity} objects; those beyond it are in neither the records nor the probability", stacklevel=2)

    @property
    def planes(self) -> list:
        return [p.label for p in self.request.planes]

    def plane_index(self, plane) -> int:
        if isinstance(plane, (int, np.integer)) and 0 <= int(plane) < len(self.request.planes):
            return int(plane)
        if plane in self.planes:
            return self.planes.index(plane)
        raise ValueError(f"no plane {plane!r}; the planes are {self.planes} (or their indices)")

    def probability(self, plane):
        """DataArray(time, lat, lon): the fraction of members in which a kept object of ``plane`` (its label or index) covers the point."""
        from .labeled import DataArray
        p = self.plane_index(plane)
        vals = np.stack([c[p] for c in self.counts]).astype(np.float64) / self.n_members if self.counts else np.zeros((0, self.lat.size, self.lon.size))
        return DataArray(vals, ["time", "lat", "lon"], dict(time=np.array(self.times, "datetime64[s]"), lat=self.lat, lon=self.lon))

    def count(self, plane) -> np.ndarray:
        """int (time, member): the kept objects of ``plane``."""
        p = self.plane_index(plane)
        return np.array([[int(per_m[p]["keep"].sum()) for per_m in per_t] for per_t in self.objects], np.int64).reshape(len(self.times), self.n_members)

    def verify(self, max_km: float = 1000.0) -> list:
        """Against the truth's objects (made by the same kernels from the truth state as a one-member set): per lead time and plane a dict
        {time, plane, n_truth, n_forecast, hit_rate, false_alarm_ratio, centroid_error_km, area_ratio, probability}.  Every kept truth
        object is matched, member by member, to the nearest kept forecast centroid of the plane within ``max_km`` (a forecast object may
        be the nearest of several truth objects): ``hit_rate`` = matched
        (truth object, member) pairs over all such pairs, ``false_alarm_ratio`` = forecast objects no truth object was matched to over all
        forecast objects, ``centroid_error_km`` and ``area_ratio`` (forecast / truth) are medians over the matched pairs, ``probability``
        is the mean over the truth's objects of the probability plane averaged over the object's points.  NaN where a ratio has no terms."""
        if self.truth is None:
            raise ValueError("verify needs the truth's objects: run with scores=True (ensemble) or truth= (single-forecast routes)")
        rows = []
        for t, time in enumerate(self.times):
            for p, label_ in enumerate(self.planes):
                tr = self.truth[t][p]
                if tr is None:
                    continue
                tr_keep = tr[tr["keep"]]
                hits = total = n_fc = n_false = 0
                errs, ratios = [], []
                for m in range(self.n_members):
                    fc = self.objects[t][m][p]
                    fc = fc[fc["keep"]]
                    used = np.zeros(len(fc), bool)
                    for o in tr_keep:
                        total += 1
                        if len(fc) == 0:
                            continue
                        dist = great_circle_km(o["lat"], o["lon"], fc["lat"], fc["lon"])
                        k = int(np.lexsort((used, dist))[0])        # the nearest; of several equally near (centroids at a pole) a free one
                        if dist[k] <= max_km:
                            hits += 1
                            used[k] = True
                            errs.append(float(dist[k]))
                            ratios.append(float(fc["area_km2"][k] / o["area_km2"]))
                    n_fc += len(fc)
                    n_false += int((~used).sum())
                prob = self.truth_probability[t][p]
                prob = prob[tr["keep"]] if prob is not None else np.zeros(0)
                nan = math.nan
                rows.append(dict(time=time, plane=label_, n_truth=len(tr_keep), n_forecast=n_fc,
                                 hit_rate=hits / total if total else nan, false_alarm_ratio=n_false / n_fc if n_fc else nan,
                                 centroid_error_km=float(np.median(errs)) if errs else nan, area_ratio=float(np.median(ratios)) if ratios else nan,
                                 probability=float(prob.mean()) if prob.size else nan))
        return rows

    # -- files: the records as JSON, the count planes beside them as .npz
    def file_name(self) -> str:
        return f"{self.model_name}-objects.json" if self.n_members == 1 else f"{self.model_name}-ens{self.n_members}-objects.json"

    @staticmethod
    def _rows(a):
        return None if a is None else {k: a[k].tolist() for k in PROPS.names}

    def to_json(self) -> str:
        doc = dict(model=self.model_name, n_members=self.n_members, forecast_id=self.forecast_id, times=[_iso(t) for t in self.times],
                   lat=self.lat.tolist(), lon=self.lon.tolist(), request=self.request.as_dict(), n_found=self.n_found.tolist(),
                   objects=[[[self._rows(a) for a in per_m] for per_m in per_t] for per_t in self.objects],
                   truth=None if self.truth is None else [[self._rows(a) for a in per_t] for per_t in self.truth],
                   truth_probability=None if self.truth_probability is None else
                   [[None if a is None else np.asarray(a).tolist() for a in per_t] for per_t in self.truth_probability])
        return json.dumps(doc)

    def save(self, output_dir) -> str:
        """``{output_dir}/{forecast id}/{model}-objects.json`` (``{model}-ens{M}-objects.json`` for an ensemble) and, beside it with the
        suffix ``.npz``, the int32 count planes (time, plane, lat, lon); returns the path of the JSON file."""
        d = Path(output_dir) / self.forecast_id if self.forecast_id else Path(output_dir)
        d.mkdir(parents=True, exist_ok=True)
        path = d / self.file_name()
        path.write_text(self.to_json())
        np.savez_compressed(path.with_suffix(".npz"), counts=self._count_array())
        return str(path)

    def _count_array(self) -> np.ndarray:
        P = len(self.request.planes)
        return np.stack([np.stack(c) for c in self.counts]).astype(np.int32) if self.counts else np.zeros((0, P, self.lat.size, self.lon.size), np.int32)

    @classmethod
    def from_json(cls, text: str, counts=None) -> "Objects":
        doc = json.loads(text)
        when = datetime.datetime.fromisoformat

        def arr(rows):
            if rows is None:
                return None
            a = np.zeros(len(rows["id"]), PROPS)
            for k in PROPS.names:
                a[k] = np.array([math.nan if v is None else v for v in rows[k]], PROPS[k]) if len(rows[k]) else a[k]
            return a
        r = doc["request"]
        names = [f for f in Plane.__dataclass_fields__]
        req = Request(tuple(Plane(**{k: p[k] for k in names}) for p in r["planes"]), r["connectivity"], r["min_pixels"], r["capacity"])
        T, P, H, W = len(doc["times"]), len(req.planes), len(doc["lat"]), len(doc["lon"])
        if counts is None:
            counts = np.zeros((T, P, H, W), np.int32)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")                     # (the warning was given when the result was made)
            return cls(doc["model"], doc["n_members"], [when(t) for t in doc["times"]], doc["lat"], doc["lon"], req,
                       [[[arr(a) for a in per_m] for per_m in per_t] for per_t in doc["objects"]], [list(c) for c in counts], doc["n_found"],
                       None if doc["truth"] is None else [[arr(a) for a in per_t] for per_t in doc["truth"]],
                       None if doc["truth_probability"] is None else
                       [[None if a is None else np.asarray(a, np.float64) for a in per_t] for per_t in doc["truth_probability"]],
                       doc.get("forecast_id", ""))

    @classmethod
    def load(cls, path) -> "Objects":
        path = Path(path)
        side = path.with_suffix(".npz")
        return cls.from_json(path.read_text(), np.load(side)["counts"] if side.exists() else None)


# ---- the drivers ----------------------------------------------------------------------------------------------------------------------- #
def check_request(names, lat, lon, n_members: int, objects, derived_names=()) -> tuple:
    """Every refusal that needs no device; returns (request, geometry)."""
    if _world_size() > 1:
        raise NotImplementedError("objects are found on one GPU from members that all lie there; members sharded over the ranks of a "
                                  "process group are out of scope (DESIGN.md 31)")
    req = parse_request(objects, list(names) + list(derived_names), n_members)
    return req, tables(lat, lon)


class _Source:
    """The planes that read one member set (the states, or the deriver's buffer) and their device buffers for M members."""

    def __init__(self, names, planes, index, req: Request, geo: Geometry, M: int, device):
        self.names, self.planes, self.index, self.req, self.geo, self.M, self.device = list(names), planes, index, req, geo, M, device
        self.spec = [(self.names.index(p.name), p.threshold, p.direction, req.connectivity, p.value_scale) for p in planes]
        self._dev = None

    def buffers(self):
        if self._dev is None:
            import torch
            dev = torch.device(self.device)
            H, W, P, M, cap = self.geo.lat.size, self.geo.lon.size, len(self.planes), self.M, self.req.capacity
            i32 = lambda *s: torch.zeros(s, dtype=torch.int32, device=dev)      # noqa: E731
            self._dev = dict(labels=i32(M, P, H, W), ids=i32(M, P, H, W), n_found=i32(M, P), counts=i32(P, H, W),
                             ws=torch.empty(workspace_bytes(M, P, H, W), dtype=torch.uint8, device=dev),
                             records=torch.zeros(M * P * cap * RECORD.itemsize, dtype=torch.uint8, device=dev),
                             row=torch.from_numpy(self.geo.row).to(dev), col=torch.from_numpy(self.geo.col).to(dev))
        return self._dev

    def run(self, states, table):
        """(props[m][p], n_found (M, P), keep table on the device): label, attributes, then the records to the host and the filters."""
        import torch
        b, req, P, M, cap = self.buffers(), self.req, len(self.planes), self.M, self.req.capacity
        label(states, table, self.spec, self.geo.periodic, req.min_pixels, cap, b["labels"], b["ids"], b["n_found"], b["ws"])
        attributes(states, table, self.spec, cap, b["labels"], b["ids"], b["n_found"], b["row"], b["col"], b["records"])
        n_found = b["n_found"].cpu().numpy().astype(np.int64)
        most = int(min(n_found.max(), cap))
        rec = b["records"].view(M, P, cap * RECORD.itemsize)[:, :, :most * RECORD.itemsize].cpu().numpy()
        rec = np.ascontiguousarray(rec).view(RECORD).reshape(M, P, most) if most else np.zeros((M, P, 0), RECORD)
        keep = np.zeros((M, P, cap + 1), np.uint8)
        props = []
        for m in range(M):
            per_p = []
            for p, plane in enumerate(self.planes):
                n = int(min(n_found[m, p], cap))
                pr = properties(rec[m, p, :n], self.geo.lat, self.geo.lon, plane.value_scale)
                pr["keep"] = keep_mask(pr, plane)
                keep[m, p, 1:n + 1] = pr["keep"]
                per_p.append(pr)
            props.append(per_p)
        return props, n_found, torch.from_numpy(keep).to(b["ids"].device)


class LeadObjects:
    """Finds the objects of one lead time after the other.  ``names``: the forecast's channels in the order of its (C, H, W) states;
    ``derived_names``: the fields of the deriver's buffer, which planes may name as well.  Planes of raw channels read the states, planes
    of derived fields the deriver's (dstates, dtable), as ``points.LeadPoints`` does; a truth state goes through the same kernels as a
    one-member set."""

    def __init__(self, names, lat, lon, n_members, request, device="cuda:0", derived_names=(), model_name="forecast", forecast_id=""):
        names, derived_names = list(names), list(derived_names)
        self.req, self.geo = check_request(names, lat, lon, n_members, request, derived_names)
        self.model_name, self.M, self.device, self.forecast_id = model_name, int(n_members), device, forecast_id
        self.sources, self.truth_sources = {}, {}
        for kind, nm in (("raw", names), ("derived", derived_names)):
            index = [k for k, p in enumerate(self.req.planes) if (p.name in names) == (kind == "raw")]
            if index:
                planes = [self.req.planes[k] for k in index]
                self.sources[kind] = _Source(nm, planes, index, self.req, self.geo, self.M, device)
                self.truth_sources[kind] = _Source(nm, planes, index, self.req, self.geo, 1, device)
        self.times, self.objects, self.counts, self.n_found, self.truth, self.truth_prob = [], [], [], [], [], []
        self.any_truth = False

    @property
    def needs_derived(self) -> bool:
        return "derived" in self.sources

    def add(self, time, states, table=None, derived=None, truth=None, derived_truth=None, truth_names=None) -> None:
        """The objects of the M device states of valid time ``time``.  ``derived``: (states, table) of the deriver when planes name
        derived fields.  ``truth`` / ``derived_truth``: the (C, H, W) device state of the truth in the forecast's (derived) channels;
        ``truth_names``: the channels whose rows of it are valid (None: all) -- planes of other channels get no truth objects."""
        import torch
        from .members import member_table
        if len(states) != self.M:
            raise ValueError(f"{len(states)} states for an object finder of {self.M} members")
        if self.needs_derived and derived is None:
            raise ValueError("object planes name derived fields: add() needs derived=(states, table) of the deriver")
        P = len(self.req.planes)
        objects = [[None] * P for _ in range(self.M)]
        counts, n_found, tr, tp = [None] * P, np.zeros((self.M, P), np.int64), [None] * P, [None] * P
        for kind, src in self.sources.items():
            st, tb = (states, member_table(states) if table is None else table) if kind == "raw" else derived
            props, nf, keep = src.run(list(st), tb)
            b = src.buffers()
            probability(b["ids"], keep, b["counts"])
            host = b["counts"].cpu().numpy()
            for q, k in enumerate(src.index):
                counts[k], n_found[:, k] = host[q].copy(), nf[:, q]
                for m in range(self.M):
                    objects[m][k] = props[m][q]
            tstate = truth if kind == "raw" else derived_truth
            if tstate is None:
                continue
            self.any_truth = True
            tsrc = self.truth_sources[kind]
            tprops, _, _ = tsrc.run([tstate], member_table([tstate]))
            tids = tsrc.buffers()["ids"][0]
            for q, k in enumerate(src.index):
                if truth_names is not None and src.planes[q].name not in truth_names:
                    continue
                n = len(tprops[0][q])                           # the mean of the count plane over each truth object's points
                sums = torch.bincount(tids[q].flatten(), weights=b["counts"][q].flatten().double(), minlength=n + 1)[1:n + 1]
                tr[k] = tprops[0][q]
                tp[k] = sums.cpu().numpy() / np.maximum(tr[k]["n_pixels"], 1) / self.M
        self.times.append(time)
        self.objects.append(objects)
        self.counts.append(counts)
        self.n_found.append(n_found)
        self.truth.append(tr)
        self.truth_prob.append(tp)

    def result(self) -> Objects:
        return Objects(self.model_name, self.M, self.times, self.geo.lat, self.geo.lon, self.req, self.objects, self.counts,
                       np.stack(self.n_found) if self.n_found else np.zeros((0, self.M, len(self.req.planes))),
                       self.truth if self.any_truth else None, self.truth_prob if self.any_truth else None, self.forecast_id)


class _Truth:
    """The truth of the single-forecast routes: any form ``verify`` accepts, uploaded lead by lead into a (C, H, W) state in the
    forecast's channels; ``names``: the channels it holds."""

    def __init__(self, truth, names, lat, lon, device):
        from .verify import _Fields
        self.fields = _Fields(truth, "truth", lat, lon)
        self.all, self.device = list(names), device
        self.names = [n for n in self.all if n in self.fields.names]
        if not self.names:
            raise ValueError("the forecast and the truth share no channel")
        self.state = None

    def at(self, time):
        import torch
        if self.state is None:
            self.state = torch.zeros((len(self.all), len(self.fields.lat), len(self.fields.lon)), dtype=torch.float32, device=self.device)
        self.state[[self.all.index(n) for n in self.names]] = torch.from_numpy(self.fields.at(time, self.names)).to(self.device)
        return self.state


def _single(model_name, names, lat, lon, objects, derived, truth, device, leads) -> Objects:
    """The single-forecast routes: ``leads(each)`` calls ``each(k, time, state)`` per lead time."""
    dnames = list(derived or [])
    if dnames:
        from . import derived as deriving
        deriving.check_request(list(names), dnames, lat, lon, 1)
    lo = LeadObjects(names, lat, lon, 1, objects, device, dnames, model_name)      # before the device
    tr = None if truth is None else _Truth(truth, names, lat, lon, device)
    deriver = tderiver = None

    def each(k, time, state):
        nonlocal deriver, tderiver
        der = dtruth = None
        tstate = None if tr is None else tr.at(time)
        if lo.needs_derived:
            if deriver is None:
                deriver = deriving.LeadDeriver(list(names), lat, lon, 1, dnames, device=device)
            der = deriver.add([state])
            if tr is not None and len(tr.names) == len(names):      # the truth of a derived field: derived from a truth that holds every channel
                if tderiver is None:
                    tderiver = deriving.LeadDeriver(list(names), lat, lon, 1, dnames, device=device)
                dtruth = tderiver.add([tstate])[0][0]
        lo.add(time, [state], None, der, tstate, dtruth, None if tr is None else tr.names + (dnames if dtruth is not None else []))
    leads(each)
    return lo.result()


def objects_model(gm, start_time: datetime.datetime, n_steps: int = 4, objects=None, derived=None, truth=None, save: bool = False,
                  save_config: dict | None = None) -> Objects:
    """``GlobalModel.object_forecast`` (core/models/base.py has the user-facing description)."""
    model = gm.model
    if n_steps < 0:
        raise ValueError("n_steps >= 0")
    check_request(model.out_channel_names, model.grid.lat, model.grid.lon, 1, objects, list(derived or []))      # before anything of the device
    require_gpu(model.device, "object_forecast finds objects with HIP kernels where the forecast lies: the model must be on a GPU")
    res = _single(gm.model_name, list(model.out_channel_names), model.grid.lat, model.grid.lon, objects, derived, truth, model.device,
                  lambda each: run_model(gm, start_time, n_steps, each))
    return _finish(res, save, save_config)


def objects_prediction(pred, objects, derived=None, truth=None, device="cuda:0", model_name: str = "") -> Objects:
    """Objects of a forecast that already exists: a ``GlobalPrediction``, a (time, channel, lat, lon) DataArray, a saved netCDF file or
    zarr store, or a list of such files (their time entries in order, duplicates of a valid time searched once).  Each time entry is
    uploaded on its own and goes through the same kernels as ``object_forecast``."""
    saved = open_saved(pred, "objects_prediction")
    check_request(saved.names, saved.lat, saved.lon, 1, objects, list(derived or []))
    require_gpu(device, "objects_prediction finds objects with HIP kernels: it needs a GPU", present=True)

    def leads(each):
        for k, time, state in saved.states(device):
            each(k, time, state)
    return _single(model_name or saved.model_name or "forecast", saved.names, saved.lat, saved.lon, objects, derived, truth, device, leads)
