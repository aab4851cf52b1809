"""Regridding on the device (include/skyrim_regrid.h): forecast states on a model's latitude-longitude grid are put on
another one -- coarser (first-order conservative), finer (bilinear) or a regional box -- where they lie in HBM, as compact channels per
member, so that the ensemble statistics and the scorer read them like raw channels.

On such grids every method is a separable, banded linear map; the kernel applies two small tables, one per axis.  Layers:

* the binding of libskyrim_regrid.so (``SPEC``, ``load_library``, ``run``, ``validate_axis``); the same call is
  ``torch.ops.skyrim_hip.regrid``.  Regridding has no CPU fallback;
* the grids and the weights: ``target_grid`` resolves what a user asks for ("1.5deg", arrays, a region) against the source grid,
  ``tables`` makes the taps and weights of a method in float64 and rounds them to fp32 once;
* the drivers: ``LeadRegridder`` (what ``ensemble.run`` calls at every lead time with ``grid=...``), ``TruthRegridder`` (the hook that
  lets ``verify.LeadScorer`` score on the target grid against a truth on the source grid), ``regrid_model``
  (``GlobalModel.regrid_forecast``) and ``regrid_prediction`` for forecasts that are already on disk.
"""
from __future__ import annotations

import ctypes
import datetime
from dataclasses import dataclass, field

import numpy as np

from . import native
from .common import world_size as _world_size
from .leads import open_saved, require_gpu, run_model
from .members import fill_channels, member_count, member_set

MAX_MEMBERS, MAX_CHANNELS, MAX_TAPS, MAX_W = 64, 256, 32, 8192          # include/skyrim_regrid.h SKREGRID_MAX_*
METHODS = ("conservative", "bilinear", "nearest")
_P = ctypes.c_void_p
_EPS = 1e-12                                                            # overlaps and fractions below this share of a cell are round-off


class TableDesc(ctypes.Structure):
    """skregrid_table."""
    _fields_ = [("start", _P), ("count", _P), ("weight", _P)]


class RegridDesc(ctypes.Structure):
    """skregrid_desc."""
    _fields_ = [("members", _P), ("M", ctypes.c_int), ("member_align", ctypes.c_int), ("C", ctypes.c_int), ("H", ctypes.c_int),
                ("W", ctypes.c_int), ("Ho", ctypes.c_int), ("Wo", ctypes.c_int), ("nc", ctypes.c_int),
                ("channels", ctypes.c_int32 * MAX_CHANNELS), ("rows", TableDesc), ("cols", TableDesc), ("out", _P),
                ("member_stride", ctypes.c_size_t)]


SPEC = native.Spec("skyrim_regrid", "SKYRIM_REGRID_LIB", "skregrid", 1, {       # include/skyrim_regrid.h SKREGRID_ABI_VERSION
    "skregrid_abi_version": (ctypes.c_int, []),
    "skregrid_run": (ctypes.c_int, [ctypes.POINTER(RegridDesc), _P]),
    "skregrid_validate": (ctypes.c_int, [_P, _P, _P, ctypes.c_int, ctypes.c_int, ctypes.c_int]),
}, " -- regridding has no torch fallback")
EXPORTS, ABI_VERSION = SPEC.exports, SPEC.abi

_lib = None


def load_library() -> ctypes.CDLL:
    """libskyrim_regrid.so (built in-tree by ``__graft_entry__.build()`` / ``make -C skyrim_amd/csrc``)."""
    global _lib
    if _lib is None:
        _lib = native.load(SPEC)
    return _lib


# ---- the tables -------------------------------------------------------------------------------------------------------------------------- #
@dataclass
class Axis:
    """One table of include/skyrim_regrid.h on the host: output o reads the ``count[o]`` source points ``start[o] + t`` (modulo ``n_src``
    when ``periodic``) with the fp32 weights ``weight[o, t]``; the entries beyond ``count`` are 0."""
    start: np.ndarray
    count: np.ndarray
    weight: np.ndarray
    n_src: int
    periodic: bool

    def dense(self) -> np.ndarray:
        """The float64 (n_out, n_src) matrix of the fp32 weights."""
        A = np.zeros((self.start.size, self.n_src))
        for o in range(self.start.size):
            for t in range(int(self.count[o])):
                A[o, (int(self.start[o]) + t) % self.n_src] += float(self.weight[o, t])
        return A


@dataclass
class Tables:
    """Both axes of one (source grid, target grid, method)."""
    rows: Axis
    cols: Axis
    method: str
    lat: np.ndarray
    lon: np.ndarray
    _dev: dict = field(default_factory=dict, repr=False)

    def on(self, device):
        """The six device arrays, uploaded once per device: (rows start, count, weight, cols start, count, weight)."""
        import torch
        dev = torch.device(device)
        hit = self._dev.get(dev)
        if hit is None:
            hit = tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev)
                        for ax in (self.rows, self.cols) for a in (ax.start, ax.count, ax.weight))
            self._dev[dev] = hit
        return hit


def validate_axis(ax: Axis) -> None:
    """``skregrid_validate`` on the host copy of one table: ValueError when the library refuses it."""
    start, count, weight = (np.ascontiguousarray(a) for a in (ax.start, ax.count, ax.weight))
    ok = (start.dtype == np.int32 and count.dtype == np.int32 and weight.dtype == np.float32 and start.ndim == 1 and start.size >= 1
          and count.shape == start.shape and weight.shape == (start.size, MAX_TAPS))
    if not ok or load_library().skregrid_validate(start.ctypes.data, count.ctypes.data, weight.ctypes.data, start.size, int(ax.n_src),
                                                  int(bool(ax.periodic))) != 0:
        raise ValueError("regrid: a table is refused by skregrid_validate (start, count or a weight outside its range)")


def _axis(taps, n_src: int, periodic: bool, what: str, spacing: float) -> Axis:
    """``taps``: per output (start, float64 weights).  Rounds to fp32 once, drops nothing (the makers emit no zero weight)."""
    n = len(taps)
    start, count, weight = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros((n, MAX_TAPS), np.float32)
    for o, (s, w) in enumerate(taps):
        if len(w) > MAX_TAPS:
            raise ValueError(f"regrid: {what} {o} of the target reads {len(w)} source {what}s; one output reads at most {MAX_TAPS} "
                             f"(SKREGRID_MAX_TAPS).  The coarsest target resolution that fits this source is {(MAX_TAPS - 2) * spacing:g} degrees")
        start[o], count[o] = s, len(w)
        weight[o, :len(w)] = np.asarray(w, np.float64).astype(np.float32)
    ax = Axis(start, count, weight, int(n_src), bool(periodic))
    validate_axis(ax)
    return ax


def _lat_axis(lat, what: str) -> np.ndarray:
    lat = np.asarray(lat, np.float64)
    step = np.diff(lat)
    if lat.ndim != 1 or lat.size < 2 or not np.all(np.isfinite(lat)) or np.any(np.abs(lat) > 90) or not (np.all(step > 0) or np.all(step < 0)):
        raise ValueError(f"regrid: {what} latitudes must be a strictly monotonic axis in degrees of at least 2 rows")
    return lat


def _unwrapped(lon) -> np.ndarray:
    """A longitude axis as an ascending sequence: 360 is added wherever it falls (a box across the date line)."""
    lon = np.asarray(lon, np.float64)
    if lon.ndim != 1 or lon.size < 1 or not np.all(np.isfinite(lon)):
        raise ValueError("regrid: longitudes must be a one-dimensional axis in degrees")
    out = np.mod(lon, 360.0)
    out = out + 360.0 * np.concatenate([[0], np.cumsum(np.diff(out) < 0)])
    if np.any(np.diff(out) <= 0) or (out.size > 1 and out[-1] - out[0] >= 360.0):
        raise ValueError("regrid: longitudes must run eastward without repeating a point")
    return out


def _src_lon(lon) -> np.ndarray:
    u = _unwrapped(lon)
    if u.size < 4:
        raise ValueError("regrid: the source needs a periodic longitude axis of at least 4 points")
    return u


def _lon_bounds(u: np.ndarray, periodic: bool) -> np.ndarray:
    """n + 1 cell bounds of an unwrapped longitude axis: midway between neighbours; the outer ones close the circle (source) or lie half
    a spacing beyond the axis (target)."""
    if u.size == 1:
        raise ValueError("regrid: a conservative target needs at least 2 columns to have cell bounds")
    mid = (u[:-1] + u[1:]) / 2
    if periodic:
        first = (u[-1] - 360.0 + u[0]) / 2
        return np.concatenate([[first], mid, [first + 360.0]])
    return np.concatenate([[u[0] - (u[1] - u[0]) / 2], mid, [u[-1] + (u[-1] - u[-2]) / 2]])


def _conservative_rows(src, dst):
    from .verify import cell_bounds
    sb, db = np.sin(np.deg2rad(cell_bounds(src, "regrid"))), np.sin(np.deg2rad(cell_bounds(dst, "regrid")))
    s_lo, s_hi = np.minimum(sb[:-1], sb[1:]), np.maximum(sb[:-1], sb[1:])
    taps = []
    for J in range(dst.size):
        lo, hi = min(db[J], db[J + 1]), max(db[J], db[J + 1])
        ov = np.clip(np.minimum(hi, s_hi) - np.maximum(lo, s_lo), 0.0, None)
        ov[ov < _EPS * (hi - lo)] = 0.0
        idx = np.nonzero(ov)[0]
        covered = ov.sum()
        if idx.size == 0 or covered < 0.5 * (hi - lo):
            raise ValueError(f"regrid: target row {J} (latitude {dst[J]:g}) is less than half covered by the source grid "
                             f"({100 * covered / (hi - lo):.0f} %): a conservative mean of it is refused")
        taps.append((int(idx[0]), ov[idx[0]:idx[-1] + 1] / covered))
    return taps


def _conservative_cols(src_u, dst_u):
    W = src_u.size
    sb, db = _lon_bounds(src_u, True), _lon_bounds(dst_u, False)
    taps = []
    for I in range(dst_u.size):
        a, b = db[I], db[I + 1]
        ov = np.zeros(W)
        for shift in (-720.0, -360.0, 0.0, 360.0, 720.0):
            ov += np.clip(np.minimum(b, sb[1:] + shift) - np.maximum(a, sb[:-1] + shift), 0.0, None)
        ov[ov < _EPS * (b - a)] = 0.0
        covered = ov.sum()
        if covered < 0.5 * (b - a):
            raise ValueError(f"regrid: target column {I} is less than half covered by the source grid")
        nz = ov > 0
        if nz.all():
            s, n = 0, W
        else:
            s = next(i for i in range(W) if nz[i] and not nz[i - 1])
            n = int(nz.sum())
        w = ov[(s + np.arange(n)) % W]
        if np.any(w == 0):
            raise ValueError(f"regrid: target column {I} overlaps source columns that are not neighbours")
        taps.append((s, w / covered))
    return taps


def _two_taps(j: int, t: float, n: int, periodic: bool):
    if t < _EPS:
        return (j, [1.0])
    if t > 1.0 - _EPS:
        return ((j + 1) % n if periodic else j + 1, [1.0])
    return (j, [1.0 - t, t])


def _bilinear_rows(src, dst):
    sgn = 1.0 if src[1] > src[0] else -1.0
    a = sgn * src
    taps = []
    for J, phi in enumerate(sgn * dst):
        if phi < a[0] - 1e-9 or phi > a[-1] + 1e-9:
            raise ValueError(f"regrid: target row {J} (latitude {dst[J]:g}) lies outside the source latitudes "
                             f"[{src.min():g}, {src.max():g}]: bilinear interpolation does not extrapolate")
        j = int(np.clip(np.searchsorted(a, phi, side="right") - 1, 0, a.size - 2))
        taps.append(_two_taps(j, float(np.clip((phi - a[j]) / (a[j + 1] - a[j]), 0.0, 1.0)), a.size, False))
    return taps


def _bilinear_cols(src_u, dst_u):
    W = src_u.size
    ext = np.concatenate([src_u, [src_u[0] + 360.0]])
    taps = []
    for lam in dst_u:
        x = src_u[0] + np.mod(lam - src_u[0], 360.0)
        i = int(np.clip(np.searchsorted(ext, x, side="right") - 1, 0, W - 1))
        taps.append(_two_taps(i, float(np.clip((x - ext[i]) / (ext[i + 1] - ext[i]), 0.0, 1.0)), W, True))
    return taps


def _nearest_rows(src, dst):
    return [(int(np.argmin(np.abs(src - phi))), [1.0]) for phi in dst]                   # (argmin: a tie goes to the lower index)


def _nearest_cols(src_u, dst_u):
    taps = []
    for lam in dst_u:
        d = np.abs(np.mod(src_u - lam + 180.0, 360.0) - 180.0)
        taps.append((int(np.argmin(d)), [1.0]))
    return taps


_table_cache: dict = {}


def tables(src_lat, src_lon, dst_lat, dst_lon, method: str = "conservative") -> Tables:
    """The two tables of ``method`` from the source grid to the target grid, made in float64 and rounded to fp32 once; cached per (grids,
    method).  Every refusal is a ValueError: an unknown method, more than ``MAX_TAPS`` taps on an axis, a conservative target cell less
    than half covered, a bilinear target row outside the source latitudes.

    ``conservative`` (first order): cell bounds midway between neighbours (``verify.cell_bounds``, those of ``area_weights``); a row weight
    is the overlap in sin(lat), a column weight the overlap length on the circle, each divided by the covered part of the target cell.
    ``bilinear``: two taps (1 - t, t) per axis, longitude periodic, ONE tap of weight 1 where a target point lies on a source point.
    ``nearest``: one tap per axis, a tie to the lower index."""
    if method not in METHODS:
        raise ValueError(f"regrid: unknown method {method!r}; choose from {METHODS}")
    src_lat, dst_lat = _lat_axis(src_lat, "source"), _lat_axis(dst_lat, "target") if np.size(dst_lat) > 1 else np.asarray(dst_lat, np.float64).reshape(-1)
    if dst_lat.size < 1 or not np.all(np.isfinite(dst_lat)) or np.any(np.abs(dst_lat) > 90):
        raise ValueError("regrid: target latitudes must be a strictly monotonic axis in degrees")
    key = (src_lat.tobytes(), np.asarray(src_lon, np.float64).tobytes(), dst_lat.tobytes(), np.asarray(dst_lon, np.float64).tobytes(), method)
    hit = _table_cache.get(key)
    if hit is not None:
        return hit
    src_u, dst_u = _src_lon(src_lon), _unwrapped(dst_lon)
    if src_u.size > MAX_W:
        raise ValueError(f"regrid: the source has {src_u.size} columns; at most {MAX_W} are supported (SKREGRID_MAX_W)")
    if method == "conservative":
        if dst_lat.size < 2:
            raise ValueError("regrid: a conservative target needs at least 2 rows to have cell bounds")
        rows, cols = _conservative_rows(src_lat, dst_lat), _conservative_cols(src_u, dst_u)
    elif method == "bilinear":
        rows, cols = _bilinear_rows(src_lat, dst_lat), _bilinear_cols(src_u, dst_u)
    else:
        rows, cols = _nearest_rows(src_lat, dst_lat), _nearest_cols(src_u, dst_u)
    hit = Tables(_axis(rows, src_lat.size, False, "row", float(np.mean(np.abs(np.diff(src_lat))))),
                 _axis(cols, src_u.size, True, "column", 360.0 / src_u.size), method, dst_lat.copy(), np.asarray(dst_lon, np.float64).copy())
    _table_cache[key] = hit
    return hit


# ---- the target grid --------------------------------------------------------------------------------------------------------------------- #
def _resolution(res) -> float:
    if isinstance(res, str):
        text = res.strip().lower()
        text = text[:-3] if text.endswith("deg") else text
        try:
            res = float(text)
        except ValueError:
            raise ValueError(f"regrid: {res!r} is not a resolution; write it as '1.5deg' or a number of degrees") from None
    res = float(res)
    if not np.isfinite(res) or res <= 0:
        raise ValueError(f"regrid: a resolution is a positive number of degrees, not {res}")
    return res


def _whole(x: float) -> bool:
    return abs(x - round(x)) < 1e-9 and round(x) >= 1


def target_grid(spec, src_lat, src_lon) -> tuple:
    """(lat, lon) float64 of the target ``spec`` asks for, oriented like the source:

    * a resolution, ``"1.5deg"`` or a float: the pole-to-pole equiangular grid of 180 / res + 1 rows and 360 / res columns that starts at
      the source's first longitude; 180 / res must be an integer;
    * explicit ``(lat, lon)`` arrays, taken as they are;
    * ``dict(region=(lat_s, lat_n, lon_w, lon_e), res=...)``: the points of a box; ``res`` defaults to the source's, and then the points
      are the source's own inside the box; ``lon_w > lon_e``: the box crosses the date line."""
    src_lat, src_u = _lat_axis(src_lat, "source"), _src_lon(src_lon)
    descending = src_lat[0] > src_lat[-1]
    if isinstance(spec, dict):
        extra = set(spec) - {"region", "res"}
        if "region" not in spec or extra:
            raise ValueError("regrid: a regional grid is dict(region=(lat_s, lat_n, lon_w, lon_e), res=...)")
        lat_s, lat_n, lon_w, lon_e = (float(v) for v in spec["region"])
        if not (-90 <= lat_s < lat_n <= 90):
            raise ValueError("regrid: a region needs -90 <= lat_s < lat_n <= 90")
        lon_w, lon_e = lon_w % 360.0, lon_e % 360.0
        span = (lon_e - lon_w) % 360.0
        if spec.get("res") is None:
            lat = src_lat[(src_lat >= lat_s - 1e-9) & (src_lat <= lat_n + 1e-9)]
            off = np.mod(np.mod(src_u, 360.0) - lon_w, 360.0)
            inside = np.nonzero(off <= span + 1e-9)[0]
            lon = np.mod(src_u, 360.0)[inside[np.argsort(off[inside], kind="stable")]]
        else:
            res = _resolution(spec["res"])
            lat = lat_s + res * np.arange(int(np.floor((lat_n - lat_s) / res + 1e-9)) + 1)
            lat = lat[::-1] if descending else lat
            lon = np.mod(lon_w + res * np.arange(int(np.floor(span / res + 1e-9)) + 1), 360.0)
        if lat.size < 1 or lon.size < 1:
            raise ValueError("regrid: the region holds no grid point")
        return np.asarray(lat, np.float64), np.asarray(lon, np.float64)
    if isinstance(spec, (str, int, float)) and not isinstance(spec, bool):
        res = _resolution(spec)
        if not _whole(180.0 / res):
            raise ValueError(f"regrid: 180 / {res:g} is not an integer: a pole-to-pole equiangular grid needs a resolution that divides 180 degrees")
        n = int(round(180.0 / res))
        lat = 90.0 - res * np.arange(n + 1)
        lat[-1] = -90.0
        lon = np.mod(src_u[0] + res * np.arange(2 * n), 360.0)
        return (lat if descending else lat[::-1].copy()), lon
    if isinstance(spec, (tuple, list)) and len(spec) == 2:
        lat, lon = np.asarray(spec[0], np.float64).reshape(-1), np.asarray(spec[1], np.float64).reshape(-1)
        if lat.size > 1:
            _lat_axis(lat, "target")
        _unwrapped(lon)
        return lat, lon
    raise ValueError("regrid: a grid is a resolution ('1.5deg' or a float), (lat, lon) arrays or dict(region=..., res=...)")


def grid_label(spec) -> str:
    """A short text for file names and the scores' JSON."""
    if isinstance(spec, dict):
        return "region" + "_".join(f"{float(v):g}" for v in spec["region"]) + ("" if spec.get("res") is None else f"@{_resolution(spec['res']):g}deg")
    if isinstance(spec, (str, int, float)):
        return f"{_resolution(spec):g}deg"
    return f"{len(spec[0])}x{len(spec[1])}"


# ---- the binding ------------------------------------------------------------------------------------------------------------------------- #
def describe(M, C, H, W, Ho, Wo, channels, member_stride, member_align=16) -> RegridDesc:
    """The descriptor of a call, its pointers still NULL."""
    d = RegridDesc()
    d.M, d.member_align, d.C, d.H, d.W, d.Ho, d.Wo, d.member_stride = M, member_align, C, H, W, Ho, Wo, member_stride
    fill_channels(d, channels, MAX_CHANNELS)
    return d


def run(members, table, channels, row_table, col_table, out) -> None:
    """One ``skregrid_run``: the channels ``channels`` of the M ``members`` (equal-shaped contiguous float32 (C, H, W) device tensors;
    ``table`` = ``ensemble.member_table(members)``) into ``out``, float32 (M, nc, Ho, Wo).  ``row_table`` / ``col_table``: (start int32
    (n_out,), count int32 (n_out,), weight float32 (n_out, 32)) on the device (``Tables.on``).  Queued on torch's current stream.  As in
    ``verify.score``, the contents of ``table`` are trusted to be the addresses of ``members``; the kernel clamps what it reads from the
    tables, so their contents cannot cause an access out of range."""
    import torch
    channels = [int(c) for c in channels]
    member_count(members, "regrid", MAX_MEMBERS)
    if not 1 <= len(channels) <= MAX_CHANNELS:
        raise ValueError(f"regrid: {len(channels)} channels; 1 to {MAX_CHANNELS} are supported")
    M, dev, align = member_set(members, table, "regrid", MAX_MEMBERS)
    C, H, W = members[0].shape
    po = native.tensor_ptr(out, "regrid: out", torch.float32, dev)
    if out.dim() != 4 or out.shape[0] != M or out.shape[1] != len(channels):
        raise ValueError(f"regrid: out must be ({M}, {len(channels)}, Ho, Wo)")
    Ho, Wo = int(out.shape[2]), int(out.shape[3])
    d = describe(M, C, H, W, Ho, Wo, channels, len(channels) * Ho * Wo, align)
    d.members, d.out = table.data_ptr(), po
    for what, tab, dst, n in (("row", row_table, d.rows, Ho), ("column", col_table, d.cols, Wo)):
        start, count, weight = tab
        if start.numel() != n or count.numel() != n or tuple(weight.shape) != (n, MAX_TAPS):
            raise ValueError(f"regrid: the {what} table must hold {n} starts, {n} counts and ({n}, {MAX_TAPS}) weights")
        dst.start, dst.count = native.tensor_ptr(start, f"regrid: {what} start", torch.int32, dev), native.tensor_ptr(count, f"regrid: {what} count", torch.int32, dev)
        dst.weight = native.tensor_ptr(weight, f"regrid: {what} weight", torch.float32, dev)
    lib = load_library()
    with torch.cuda.device(dev):
        native.check(lib.skregrid_run(ctypes.byref(d), native.stream(dev)), "skregrid_run", lib)


# ---- the drivers ------------------------------------------------------------------------------------------------------------------------- #
def check_request(names, lat, lon, n_members, grid, method="conservative", channels=None) -> Tables:
    """Every refusal that needs no device; returns the tables (``.lat`` / ``.lon``: the target grid)."""
    if _world_size() > 1:
        raise NotImplementedError("regridding is done on one GPU from members that all lie there; members sharded over the ranks of a "
                                  "process group are out of scope (DESIGN.md 22)")
    if not 1 <= int(n_members) <= MAX_MEMBERS:
        raise ValueError(f"n_members = {n_members}: 1 to {MAX_MEMBERS} members are regridded (SKREGRID_MAX_MEMBERS)")
    if method not in METHODS:
        raise ValueError(f"regrid: unknown method {method!r}; choose from {METHODS}")
    names = list(names)
    picked = names if channels is None else list(channels)
    missing = [c for c in picked if c not in names]
    if missing:
        raise ValueError(f"regrid: channels {missing} are not channels of this forecast")
    if not 1 <= len(picked) <= MAX_CHANNELS:
        raise ValueError(f"regrid: {len(picked)} channels; one call regrids 1 to {MAX_CHANNELS} (SKREGRID_MAX_CHANNELS)")
    dst_lat, dst_lon = target_grid(grid, lat, lon)
    tabs = tables(lat, lon, dst_lat, dst_lon, method)
    if len(names) * len(lat) * len(lon) > 2 ** 30 or len(picked) * dst_lat.size * dst_lon.size > 2 ** 30:
        raise ValueError("regrid: a state and its regridded channels hold at most 2^30 elements each")
    return tabs


class LeadRegridder:
    """Regrids one lead time after the other into its own (M, nc, Ho, Wo) buffer.  ``names``: the forecast's channels in the order of its
    (C, H, W) states; ``channels``: those to regrid, channel k of the buffer is channels[k] (None: all, in order); ``grid``: what
    ``target_grid`` accepts.  ``lat_out`` / ``lon_out``: the target grid."""

    def __init__(self, names, lat, lon, n_members, grid, method="conservative", channels=None, device="cuda:0"):
        self.tables = check_request(names, lat, lon, n_members, grid, method, channels)
        self.names, self.M, self.method, self.device = list(names), int(n_members), method, device
        self.channels = list(names) if channels is None else list(channels)
        self.index = [self.names.index(c) for c in self.channels]
        self.lat, self.lon = np.asarray(lat, np.float64), np.asarray(lon, np.float64)
        self.lat_out, self.lon_out = self.tables.lat, self.tables.lon
        self._dev = None

    def _buffers(self):
        if self._dev is None:
            import torch
            from .ensemble import member_table
            dev = torch.device(self.device)
            out = torch.empty((self.M, len(self.channels), self.lat_out.size, self.lon_out.size), dtype=torch.float32, device=dev)
            states = [out[m] for m in range(self.M)]
            tabs = self.tables.on(dev)
            self._dev = dict(out=out, states=states, table=member_table(states), rows=tabs[:3], cols=tabs[3:])
        return self._dev

    def add(self, states, table=None) -> tuple:
        """ONE regrid launch over the M device states (C, H, W); returns (regridded_states, regridded_table): M (nc, Ho, Wo) views of the
        buffer and their ``ensemble.member_table``, ready for ``ensemble.stats`` and ``LeadScorer.add``.  The next ``add`` overwrites
        them."""
        from .ensemble import member_table
        if len(states) != self.M:
            raise ValueError(f"{len(states)} states for a regridder of {self.M} members")
        b = self._buffers()
        run(states, member_table(states) if table is None else table, self.index, b["rows"], b["cols"], b["out"])
        return b["states"], b["table"]


class TruthRegridder:
    """The hook ``verify.LeadScorer(adapt=...)`` calls so that a truth (or climatology) on the SOURCE grid scores a forecast on the target
    grid: the scored channels of a valid time are uploaded on the source grid and regridded by the same kernel with M = 1, so forecast
    and truth pass through identical arithmetic.  ``truth_grid`` tells the scorer which grid its truth is read on."""

    def __init__(self, lat, lon, grid, method="conservative", device="cuda:0"):
        self.lat, self.lon, self.grid, self.method, self.device = np.asarray(lat, np.float64), np.asarray(lon, np.float64), grid, method, device
        self.truth_grid = (self.lat, self.lon)
        self._regridders: dict = {}

    def names(self, fields) -> list:
        return list(fields.names)

    def upload(self, fields, time, scored, dst, idx_dev) -> None:
        """Fill the rows ``idx_dev`` of ``dst`` (the scorer's (C, Ho, Wo) truth buffer) with the channels ``scored`` at ``time``."""
        import torch
        key = tuple(scored)
        rg = self._regridders.get(key)
        if rg is None:
            rg = self._regridders[key] = LeadRegridder(list(scored), self.lat, self.lon, 1, self.grid, self.method, device=self.device)
        state = torch.from_numpy(fields.at(time, list(scored))).to(rg.device)
        states, _ = rg.add([state])
        dst[idx_dev] = states[0]


@dataclass
class RegriddedProducts:
    """``EnsembleForecast.regridded``: the attributes of the raw products on the target grid ``lat`` x ``lon``."""
    lat: np.ndarray
    lon: np.ndarray
    method: str
    mean: object = None
    spread: object = None
    min: object = None
    max: object = None
    exceedance: dict = field(default_factory=dict)
    quantile: dict = field(default_factory=dict)
    members: object = None
    scores: object = None


def regrid_model(gm, start_time: datetime.datetime, n_steps: int, grid, method: str = "conservative", channels=None, save: bool = False,
                 save_config: dict | None = None):
    """``GlobalModel.regrid_forecast`` (core/models/base.py has the user-facing description)."""
    from .labeled import DataArray
    model = gm.model
    if n_steps < 0:
        raise ValueError("n_steps >= 0")
    rg = LeadRegridder(model.out_channel_names, model.grid.lat, model.grid.lon, 1, grid, method, channels, device=model.device)      # before anything of the device
    require_gpu(model.device, "regrid_forecast regrids with HIP kernels where the forecast lies: the model must be on a GPU")
    times, host = [], []

    def each(k, time, state):
        states, _ = rg.add([state])
        times.append(time)
        host.append(states[0].cpu().numpy())
    run_model(gm, start_time, n_steps, each)
    da = DataArray(np.stack(host), ["time", "channel", "lat", "lon"], dict(time=times, channel=list(rg.channels), lat=rg.lat_out, lon=rg.lon_out))
    if save:
        from .common import save_config_with_id, save_forecast
        cfg = save_config_with_id(save_config)
        da.path = save_forecast(da, f"{gm.model_name}-regrid", times[0], times[-1], gm.source_label, config=cfg)
    return da


def regrid_prediction(pred, grid, method: str = "conservative", device="cuda:0", channels=None):
    """A forecast that already exists, on the target grid: a ``GlobalPrediction``, a (time, channel, lat, lon) DataArray, a saved netCDF
    file or zarr store, or a list of such files (their time entries in order, duplicates of a valid time regridded once).  Each time entry
    is uploaded on its own and goes through the same kernel as ``regrid_forecast``.  Returns DataArray(time, channel, lat, lon)."""
    from .labeled import DataArray
    saved = open_saved(pred, "regrid_prediction")
    rg = LeadRegridder(saved.names, saved.lat, saved.lon, 1, grid, method, channels, device=device)
    require_gpu(device, "regrid_prediction regrids with HIP kernels: it needs a GPU", present=True)
    times, host = [], []
    for _, time, state in saved.states(rg.device):
        states, _ = rg.add([state])
        times.append(time)
        host.append(states[0].cpu().numpy())
    return DataArray(np.stack(host), ["time", "channel", "lat", "lon"], dict(time=times, channel=list(rg.channels), lat=rg.lat_out, lon=rg.lon_out))
