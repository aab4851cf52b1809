"""Quantile climates on the device (include/skyrim_clim.h): what a forecast is compared with when the question is not
"how many members are above 15 m/s" but "is this unusual for this place and this time of year".

Layers:

* the binding of libskyrim_clim.so (``SPEC``, ``load_library``, ``run_extremes``, ``run_quantiles``); the same calls are
  ``torch.ops.skyrim_hip.clim_extremes`` and ``torch.ops.skyrim_hip.clim_quantiles``.  Neither has a CPU fallback;
* the host tables of the index (``tables``) and the positions of the levels in N sorted samples (``positions``), formed in double;
* ``Climate``: levels, field names, grid and one or more slices (Q, F, H, W) keyed by (month, day, hour), with ``at(valid_time)``,
  ``save`` and ``open``;
* ``build`` (samples -> a one-slice climate, the sort on the device) and ``build_from_files`` (saved forecasts or analyses, grouped by
  calendar key and window).
"""
from __future__ import annotations

import ctypes
import datetime
import math
from pathlib import Path

import numpy as np

from . import native
from .members import member_count, member_set

# include/skyrim_clim.h SKCLIM_MAX_*
MAX_MEMBERS, MAX_FIELDS, MAX_LEVELS, MAX_SOT, MAX_PROB, MAX_SAMPLES = 64, 16, 128, 4, 8, 2048
_P = ctypes.c_void_p
DEFAULT_LEVELS = np.linspace(0.0, 1.0, 101)


class SotReq(ctypes.Structure):
    """skclim_sot."""
    _fields_ = [("q_index", ctypes.c_int32), ("q_frac", ctypes.c_float), ("k_ref", ctypes.c_int32), ("k_base", ctypes.c_int32)]


class ProbReq(ctypes.Structure):
    """skclim_prob."""
    _fields_ = [("k", ctypes.c_int32), ("below", ctypes.c_int32)]


class ExtremesDesc(ctypes.Structure):
    """skclim_extremes_desc."""
    _fields_ = [("members", _P), ("M", ctypes.c_int), ("member_align", ctypes.c_int), ("C", ctypes.c_int), ("H", ctypes.c_int),
                ("W", ctypes.c_int), ("nf", ctypes.c_int), ("channels", ctypes.c_int32 * MAX_FIELDS), ("clim", _P), ("Q", ctypes.c_int),
                ("p", ctypes.c_float * MAX_LEVELS), ("A", ctypes.c_float * MAX_LEVELS), ("B", ctypes.c_float * MAX_LEVELS),
                ("rdp", ctypes.c_float * MAX_LEVELS), ("floor", ctypes.c_float * MAX_FIELDS), ("n_sot", ctypes.c_int),
                ("sot_req", SotReq * MAX_SOT), ("n_prob", ctypes.c_int), ("prob_req", ProbReq * MAX_PROB), ("efi", _P), ("sot", _P),
                ("prob", _P)]


class QuantilesDesc(ctypes.Structure):
    """skclim_quantiles_desc."""
    _fields_ = [("samples", _P), ("N", ctypes.c_int), ("C", ctypes.c_int), ("H", ctypes.c_int), ("W", ctypes.c_int), ("nf", ctypes.c_int),
                ("channels", ctypes.c_int32 * MAX_FIELDS), ("Q", ctypes.c_int), ("q_index", ctypes.c_int32 * MAX_LEVELS),
                ("q_frac", ctypes.c_float * MAX_LEVELS), ("clim", _P)]


SPEC = native.Spec("skyrim_clim", "SKYRIM_CLIM_LIB", "skclim", 1, {              # include/skyrim_clim.h SKCLIM_ABI_VERSION
    "skclim_abi_version": (ctypes.c_int, []),
    "skclim_extremes": (ctypes.c_int, [ctypes.POINTER(ExtremesDesc), _P]),
    "skclim_quantiles": (ctypes.c_int, [ctypes.POINTER(QuantilesDesc), _P]),
    "skclim_extremes_check": (ctypes.c_int, [ctypes.POINTER(ExtremesDesc)]),
    "skclim_quantiles_check": (ctypes.c_int, [ctypes.POINTER(QuantilesDesc)]),
    "skclim_tile_points": (ctypes.c_int, [ctypes.c_int]),
}, " -- climate-relative extremes have no torch fallback")
EXPORTS, ABI_VERSION = SPEC.exports, SPEC.abi

_lib = None


def load_library() -> ctypes.CDLL:
    """libskyrim_clim.so (built in-tree by ``__graft_entry__.build()`` / ``make -C skyrim_amd/csrc``)."""
    global _lib
    if _lib is None:
        _lib = native.load(SPEC)
    return _lib


# ---- the host tables --------------------------------------------------------------------------------------------------------------------- #
def check_levels(levels) -> np.ndarray:
    """The levels as float64, strictly increasing in [0, 1]; ValueError otherwise."""
    p = np.asarray(levels, np.float64).reshape(-1)
    if p.size < 1 or not np.all(np.isfinite(p)) or p[0] < 0.0 or p[-1] > 1.0 or np.any(np.diff(p) <= 0.0):
        raise ValueError("climate: the levels must be strictly increasing in [0, 1]")
    return p


def tables(levels) -> dict:
    """p[Q], A[Q-1], B[Q-1], rdp[Q-1] of the header, in double: the integrals of 1 / sqrt(p (1 - p)) and p / sqrt(p (1 - p)) over each
    interval (G and K of the header) and the reciprocal widths.  The descriptor takes them rounded once to fp32."""
    p = check_levels(levels)
    s = np.sqrt(p)
    G = -2.0 * np.arccos(s)
    K = -np.sqrt(p * (1.0 - p)) - np.arccos(s)
    return dict(p=p, A=np.diff(G), B=np.diff(K), rdp=1.0 / np.diff(p))


def _position(h, last: int) -> tuple:
    """(index, fraction) of the position ``h`` (array, double) among ``last + 1`` sorted values, such that the fraction is below 1 AS
    FP32, which is what the descriptors carry: a product like 100 * 0.29 = 28.999999999999996 has the fraction 1 - 4e-15, which rounds
    to 1.0f; it is the next index with fraction 0 (the same value to rounding, and what the level means)."""
    h = np.asarray(h, np.float64)
    k = np.minimum(np.floor(h).astype(np.int64), last)
    f = h - k
    up = (f.astype(np.float32) >= np.float32(1.0)) & (k < last)
    return np.where(up, k + 1, k), np.where(up | (k >= last), 0.0, f)


def positions(levels, N: int) -> tuple:
    """(q_index, q_frac) of numpy's "linear" method in N sorted values: h = (N - 1) level in double, 0 <= q_frac < 1 also once
    rounded to fp32 (``_position``)."""
    k, f = _position((int(N) - 1) * check_levels(levels), int(N) - 1)
    return k.astype(np.int32), f.astype(np.float64)


def level_index(levels, q: float, what: str) -> int:
    """The index of level ``q`` in ``levels`` (matched to 1e-9); a ValueError naming the level when the climate does not hold it."""
    d = np.abs(np.asarray(levels, np.float64) - float(q))
    k = int(np.argmin(d))
    if not d[k] <= 1e-9:
        raise ValueError(f"{what}: the climate has no level {float(q):.10g}")
    return k


def sot_levels(q: float) -> tuple:
    """(base, ref) levels of the SOT of tail ``q``: the 0.9 request reads 0.9 and 0.99, the 0.1 request 0.1 and 0.01."""
    q = float(q)
    if not 0.0 < q < 1.0:
        raise ValueError(f"extremes: a SOT tail lies in (0, 1), got {q:g}")
    return q, (1.0 - (1.0 - q) / 10.0 if q >= 0.5 else q / 10.0)


def sot_request(levels, q: float, M: int) -> tuple:
    """(q_index, q_frac, k_ref, k_base) of the header for tail ``q`` of M members."""
    base, ref = sot_levels(q)
    k, f = _position([(int(M) - 1) * base], int(M) - 1)
    return int(k[0]), float(f[0]), level_index(levels, ref, "extremes: sot"), level_index(levels, base, "extremes: sot")


# ---- the binding ------------------------------------------------------------------------------------------------------------------------- #
def describe_extremes(M, align, C, H, W, channels, levels, floor=None, sot=(), prob=()) -> ExtremesDesc:
    """The descriptor of a call, its pointers still NULL.  ``sot``: (q_index, q_frac, k_ref, k_base) tuples; ``prob``: (k, below)."""
    d = ExtremesDesc()
    d.M, d.member_align, d.C, d.H, d.W = int(M), int(align), int(C), int(H), int(W)
    channels = [int(c) for c in channels]
    d.nf = len(channels)
    for k, c in enumerate(channels[:MAX_FIELDS]):
        d.channels[k] = c
        d.floor[k] = -math.inf if floor is None else float(floor[k])
    t = tables(levels)
    d.Q = int(t["p"].size)
    for i, v in enumerate(t["p"][:MAX_LEVELS]):
        d.p[i] = v
    for name in ("A", "B", "rdp"):
        for i, v in enumerate(t[name][:MAX_LEVELS]):
            getattr(d, name)[i] = v
    d.n_sot, d.n_prob = len(sot), len(prob)
    for s, r in enumerate(list(sot)[:MAX_SOT]):
        d.sot_req[s] = SotReq(int(r[0]), float(r[1]), int(r[2]), int(r[3]))
    for s, r in enumerate(list(prob)[:MAX_PROB]):
        d.prob_req[s] = ProbReq(int(r[0]), int(bool(r[1])))
    return d


def describe_quantiles(N, C, H, W, channels, levels) -> QuantilesDesc:
    d = QuantilesDesc()
    d.N, d.C, d.H, d.W = int(N), int(C), int(H), int(W)
    channels = [int(c) for c in channels]
    d.nf = len(channels)
    for k, c in enumerate(channels[:MAX_FIELDS]):
        d.channels[k] = c
    qi, qf = positions(levels, max(int(N), 1))
    d.Q = int(qi.size)
    for i in range(min(d.Q, MAX_LEVELS)):
        d.q_index[i], d.q_frac[i] = int(qi[i]), float(qf[i])
    return d


def _counts(what, nf, Q, lo_q, H, W, C):
    if not 1 <= nf <= MAX_FIELDS:
        raise ValueError(f"{what}: {nf} fields; 1 to {MAX_FIELDS} per call (SKCLIM_MAX_FIELDS)")
    if not lo_q <= Q <= MAX_LEVELS:
        raise ValueError(f"{what}: {Q} levels; {lo_q} to {MAX_LEVELS} are supported (SKCLIM_MAX_LEVELS)")
    if C * H * W > 2 ** 30 or nf * Q * H * W > 2 ** 30:
        raise ValueError(f"{what}: a state holds at most 2^30 elements, and so do the nf Q planes of a call")


def run_extremes(members, table, channels, clim, levels, floor=None, sot=(), prob=(), efi=None, sot_out=None, prob_out=None) -> None:
    """One ``skclim_extremes``: the listed ``channels`` of the M ``members`` (equal-shaped contiguous float32 (C, H, W) device tensors;
    ``table`` = ``member_table(members)``) against ``clim`` (nf, Q, H, W) at the probability ``levels``.  ``sot``: (q_index, q_frac,
    k_ref, k_base) per request (``sot_request``), ``prob``: (level index, below) per request; ``efi`` (nf, H, W), ``sot_out`` (n_sot, nf,
    H, W), ``prob_out`` (n_prob, nf, H, W) or None: not computed.  Queued on torch's current stream."""
    import torch
    what = "clim_extremes"
    channels, sot, prob = [int(c) for c in channels], list(sot), list(prob)
    member_count(members, what, MAX_MEMBERS)
    M, dev, align = member_set(members, table, what, MAX_MEMBERS)
    C, H, W = members[0].shape
    p = check_levels(levels)
    _counts(what, len(channels), p.size, 2, H, W, C)
    if len(sot) > MAX_SOT or len(prob) > MAX_PROB:
        raise ValueError(f"{what}: at most {MAX_SOT} SOT requests and {MAX_PROB} tail-odds requests per call")
    nf = len(channels)
    pc = native.tensor_ptr(clim, f"{what}: clim", torch.float32, dev)
    if tuple(clim.shape) != (nf, p.size, H, W):
        raise ValueError(f"{what}: clim must be ({nf}, {p.size}, {H}, {W})")
    d = describe_extremes(M, align, C, H, W, channels, p, floor, sot, prob)
    d.members, d.clim = table.data_ptr(), pc
    for name, t, shape in (("efi", efi, (nf, H, W)), ("sot", sot_out, (len(sot), nf, H, W)), ("prob", prob_out, (len(prob), nf, H, W))):
        if t is not None:
            ptr = native.tensor_ptr(t, f"{what}: {name}", torch.float32, dev)
            if tuple(t.shape) != shape:
                raise ValueError(f"{what}: {name} must be {shape}")
            setattr(d, name, ptr)
    lib = load_library()
    with torch.cuda.device(dev):
        native.check(lib.skclim_extremes(ctypes.byref(d), native.stream(dev)), "skclim_extremes", lib)


def run_quantiles(samples, table, channels, levels, clim) -> None:
    """One ``skclim_quantiles``: the ``levels`` (numpy's "linear" method) of the listed ``channels`` over the N ``samples`` (equal-shaped
    contiguous float32 (C, H, W) device tensors; ``table`` = ``member_table(samples)``) into ``clim`` (nf, Q, H, W)."""
    import torch
    what = "clim_quantiles"
    channels = [int(c) for c in channels]
    N, dev, _ = member_set(samples, table, what, MAX_SAMPLES)
    C, H, W = samples[0].shape
    p = check_levels(levels)
    _counts(what, len(channels), p.size, 1, H, W, C)
    pc = native.tensor_ptr(clim, f"{what}: clim", torch.float32, dev)
    if tuple(clim.shape) != (len(channels), p.size, H, W):
        raise ValueError(f"{what}: clim must be ({len(channels)}, {p.size}, {H}, {W})")
    d = describe_quantiles(N, C, H, W, channels, p)
    d.samples, d.clim = table.data_ptr(), pc
    lib = load_library()
    with torch.cuda.device(dev):
        native.check(lib.skclim_quantiles(ctypes.byref(d), native.stream(dev)), "skclim_quantiles", lib)


def tile_points(N: int) -> int:
    """The points of a workgroup's tile in ``skclim_quantiles`` for N samples."""
    return int(load_library().skclim_tile_points(int(N)))


# ---- the climate ------------------------------------------------------------------------------------------------------------------------- #
def _doy(month: int, day: int) -> int:
    return datetime.date(2000, int(month), int(day)).timetuple().tm_yday          # a leap year: the 366-day circle


def _norm_key(key):
    if key is None:
        return None
    month, day, hour = (tuple(key) + (None,))[:3]
    _doy(month, day)
    if hour is not None and not 0 <= int(hour) < 24:
        raise ValueError(f"climate: the hour of key {key} is outside 0..23")
    return int(month), int(day), None if hour is None else int(hour)


class Climate:
    """A quantile climate: ``levels`` (Q,) strictly increasing in [0, 1], ``fields`` (F names), ``lat`` / ``lon`` and ``slices``
    ``{(month, day, hour): (Q, F, H, W) float32}`` -- ``hour`` may be None -- or a single array, the unkeyed slice that serves every
    time.  Checked on construction and on ``open``: the levels, the shapes, and that the planes are non-decreasing in the level wherever
    they are finite."""

    def __init__(self, levels, fields, lat, lon, slices, n_samples=0, half_window_days=0, max_gap_days=15):
        self.levels = check_levels(levels)
        self.fields = [str(f) for f in fields]
        if not self.fields or len(set(self.fields)) != len(self.fields):
            raise ValueError("climate: the fields need distinct names, at least one")
        self.lat, self.lon = np.asarray(lat, np.float64), np.asarray(lon, np.float64)
        if not isinstance(slices, dict):
            slices = {None: slices}
        if not slices or (None in slices and len(slices) > 1):
            raise ValueError("climate: one unkeyed slice, or slices keyed by (month, day, hour)")
        self.slices = {}
        shape = (self.levels.size, len(self.fields), self.lat.size, self.lon.size)
        for key, arr in slices.items():
            arr = np.ascontiguousarray(arr, np.float32)
            if arr.shape != shape:
                raise ValueError(f"climate: the slice {key} has shape {arr.shape}, expected (level, field, lat, lon) = {shape}")
            with np.errstate(invalid="ignore"):
                d = np.diff(arr, axis=0)
                if np.any(d[np.isfinite(d)] < 0):
                    raise ValueError(f"climate: the planes of slice {key} decrease with the level somewhere")
            self.slices[_norm_key(key)] = arr
        hours = {k[2] is None for k in self.slices if k is not None}
        if len(hours) > 1:
            raise ValueError("climate: either every slice carries an hour or none does")
        self.n_samples, self.half_window_days, self.max_gap_days = int(n_samples), int(half_window_days), float(max_gap_days)

    def at(self, valid_time) -> tuple:
        """(key, slice) for ``valid_time``: among the slices of the same hour of day (where they carry hours) the nearest day of year on
        the 366-day circle; a ValueError naming the gap when that is more than ``max_gap_days`` away."""
        if None in self.slices:
            return None, self.slices[None]
        t = np.datetime64(valid_time, "s").astype(datetime.datetime)
        keys = list(self.slices)
        if keys[0][2] is not None:
            keys = [k for k in keys if k[2] == t.hour]
            if not keys:
                raise ValueError(f"climate: no slice for hour {t.hour:02d} (valid time {t.isoformat()}); the slices hold the hours "
                                 f"{sorted({k[2] for k in self.slices})}")
        d0 = _doy(t.month, t.day)
        gap = lambda k: min(abs(_doy(k[0], k[1]) - d0), 366 - abs(_doy(k[0], k[1]) - d0))      # noqa: E731
        best = min(keys, key=lambda k: (gap(k), k))
        if gap(best) > self.max_gap_days:
            raise ValueError(f"climate: the nearest slice to {t.isoformat()} is {best[0]:02d}-{best[1]:02d}, {gap(best)} days away "
                             f"(max_gap_days = {self.max_gap_days:g})")
        return best, self.slices[best]

    def check_grid(self, lat, lon) -> None:
        if not (np.array_equal(self.lat, np.asarray(lat, np.float64)) and np.array_equal(self.lon, np.asarray(lon, np.float64))):
            raise ValueError("climate: its latitudes and longitudes are not the forecast's grid (climates on other grids are out of scope)")

    # -- files: one netCDF file per slice
    @staticmethod
    def _file(key) -> str:
        if key is None:
            return "climate.nc"
        return f"climate_{key[0]:02d}{key[1]:02d}" + ("" if key[2] is None else f"_{key[2]:02d}") + ".nc"

    def save(self, directory) -> list:
        """One file per slice under ``directory`` (levels, field names, lat, lon, the key, ``n_samples``, ``half_window_days``)."""
        from .labeled import DataArray
        from .ncio import write_dataarray_netcdf3
        d = Path(directory)
        d.mkdir(parents=True, exist_ok=True)
        paths = []
        for key, arr in self.slices.items():
            m, dd, h = (-1, -1, -1) if key is None else (key[0], key[1], -1 if key[2] is None else key[2])
            da = DataArray(arr, ["level", "field", "lat", "lon"],
                           dict(level=self.levels, field=self.fields, lat=self.lat, lon=self.lon, month=np.int32(m), day=np.int32(dd),
                                hour=np.int32(h), n_samples=np.int32(self.n_samples), half_window_days=np.int32(self.half_window_days)),
                           "climate")
            write_dataarray_netcdf3(da, d / self._file(key))
            paths.append(str(d / self._file(key)))
        return paths

    @classmethod
    def open(cls, directory, max_gap_days=15) -> "Climate":
        from .ncio import read_dataarray_netcdf3
        files = sorted(Path(directory).glob("climate*.nc"))
        if not files:
            raise ValueError(f"climate: no climate*.nc file under {directory}")
        slices, first = {}, None
        for f in files:
            da = read_dataarray_netcdf3(f)
            c = da._coords
            if tuple(da.dims) != ("level", "field", "lat", "lon"):
                raise ValueError(f"climate: {f} is not a climate slice (level, field, lat, lon)")
            m, dd, h = (int(np.asarray(c[k]).reshape(-1)[0]) for k in ("month", "day", "hour"))
            key = None if m < 0 else (m, dd, None if h < 0 else h)
            if first is None:
                first = c
            elif not all(np.array_equal(np.asarray(first[k]), np.asarray(c[k])) for k in ("level", "field", "lat", "lon")):
                raise ValueError(f"climate: {f} differs from {files[0]} in levels, fields or grid")
            slices[key] = np.asarray(da.values, np.float32)
        ns, hw = (int(np.asarray(first[k]).reshape(-1)[0]) for k in ("n_samples", "half_window_days"))
        return cls(np.asarray(first["level"], np.float64), [str(s) for s in np.asarray(first["field"]).tolist()], first["lat"], first["lon"],
                   slices, ns, hw, max_gap_days)


def as_climate(c) -> Climate:
    """A ``Climate`` as it is, a path opened."""
    return c if isinstance(c, Climate) else Climate.open(c)


# ---- making one -------------------------------------------------------------------------------------------------------------------------- #
def field_groups(n_fields: int, Q: int, hw: int) -> list:
    """The fields of a request split over calls: at most SKCLIM_MAX_FIELDS each and nf Q H W <= 2^30."""
    per = max(1, min(MAX_FIELDS, (2 ** 30) // max(Q * hw, 1)))
    return [list(range(i, min(i + per, n_fields))) for i in range(0, n_fields, per)]


def build(samples, fields, levels=DEFAULT_LEVELS, lat=None, lon=None, device="cuda:0", key=None, half_window_days=0) -> Climate:
    """A one-slice ``Climate`` of ``fields`` from ``samples``, an iterable of ``(names, state)`` with ``state`` a (C, H, W) array or
    device tensor whose channels are ``names``: only ``fields`` of each sample are kept on the device, then ONE ``skclim_quantiles``
    launch per field group sorts the N values of every point.  More than 2048 samples are refused, not thinned."""
    import torch
    from .leads import require_gpu
    from .members import member_table
    fields, p = [str(f) for f in fields], check_levels(levels)
    if not 1 <= p.size <= MAX_LEVELS:
        raise ValueError(f"climate: {p.size} levels; 1 to {MAX_LEVELS} are supported (SKCLIM_MAX_LEVELS)")
    require_gpu(device, "climate.build sorts the samples with a HIP kernel: it needs a GPU", present=True)
    dev, kept = torch.device(device), []
    for names, state in samples:
        names = list(names)
        missing = [f for f in fields if f not in names]
        if missing:
            raise ValueError(f"climate: a sample lacks the fields {missing}")
        if len(kept) == MAX_SAMPLES:
            raise ValueError(f"climate: more than {MAX_SAMPLES} samples (SKCLIM_MAX_SAMPLES); a climate is not thinned silently: "
                             "narrow the window or the years")
        idx = [names.index(f) for f in fields]
        t = state if isinstance(state, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(state)[idx], np.float32))
        t = t[idx] if isinstance(state, torch.Tensor) else t
        kept.append(t.to(dev, torch.float32).contiguous())
    if not kept:
        raise ValueError("climate: no samples")
    _, H, W = kept[0].shape
    lat = np.arange(H, dtype=np.float64) if lat is None else lat
    lon = np.arange(W, dtype=np.float64) if lon is None else lon
    table = member_table(kept)
    out = np.empty((p.size, len(fields), H, W), np.float32)
    for group in field_groups(len(fields), p.size, H * W):
        clim = torch.empty((len(group), p.size, H, W), dtype=torch.float32, device=dev)
        run_quantiles(kept, table, group, p, clim)
        out[:, group] = clim.cpu().numpy().transpose(1, 0, 2, 3)
    return Climate(p, fields, lat, lon, {key: out}, len(kept), half_window_days)


def calendar_groups(times, half_window_days=15, hours=None, keys=None) -> dict:
    """``{(month, day, hour): [indices into times]}``: every valid time goes to each key whose day of year lies within
    ``half_window_days`` of its own on the 366-day circle and whose hour is its own.  ``keys``: the (month, day) pairs to make (None: the
    days the times themselves fall on); ``hours``: the hours of day to make (None: one slice per day without an hour)."""
    ts = [np.datetime64(t, "s").astype(datetime.datetime) for t in times]
    days = sorted({(t.month, t.day) for t in ts}) if keys is None else [tuple(k)[:2] for k in keys]
    out = {}
    for m, d in days:
        for h in ([None] if hours is None else list(hours)):
            d0 = _doy(m, d)
            idx = [i for i, t in enumerate(ts) if (h is None or t.hour == h)
                   and min(abs(_doy(t.month, t.day) - d0), 366 - abs(_doy(t.month, t.day) - d0)) <= half_window_days]
            if idx:
                out[(m, d, h)] = idx
    return out


def build_from_files(files, fields, derived=None, half_window_days=15, hours=None, levels=DEFAULT_LEVELS, keys=None, device="cuda:0") -> Climate:
    """A keyed ``Climate`` from saved forecasts or analyses (``leads.open_saved``: netCDF files, zarr stores, predictions): ``fields``
    are raw channels of the files or fields of ``derived``, which the deriver of ``derived=`` makes on the device.  The valid times are
    grouped by ``calendar_groups`` and each group is one ``build``.  A group of more than 2048 samples is refused by name.  The slices
    are made one after the other: the device holds the samples of ONE slice, only their ``fields`` (at most 2048 F planes, 8.5 GB per
    field at 721 x 1440), whatever the length of the record; an entry that lies in the windows of several slices is uploaded (and
    derived from) once per slice.  Aggregated
    fields such as ``ws10m_max_24h`` do not come from here: pass the arrays ``aggregate_prediction`` gives to ``build``."""
    import torch
    from .leads import open_saved, require_gpu
    saved = open_saved(files, "climate.build_from_files")
    dnames = list(derived or [])
    missing = [f for f in fields if f not in saved.names and f not in dnames]
    if missing:
        raise ValueError(f"climate: the fields {missing} are neither channels of the files nor derived fields named in derived=")
    groups = calendar_groups([e[0] for e in saved.entries], half_window_days, hours, keys)
    for key, idx in groups.items():
        if len(idx) > MAX_SAMPLES:
            raise ValueError(f"climate: the slice {key} would take {len(idx)} samples; at most {MAX_SAMPLES} (SKCLIM_MAX_SAMPLES): "
                             "narrow half_window_days or the years")
    require_gpu(device, "climate.build_from_files sorts the samples with a HIP kernel: it needs a GPU", present=True)
    deriver = None
    if dnames:
        from . import derived as deriving
        deriving.check_request(saved.names, dnames, saved.lat, saved.lon, 1)
        deriver = deriving.LeadDeriver(saved.names, saved.lat, saved.lon, 1, dnames, device=device)
    raw = [f for f in fields if f in saved.names]

    def sample(i):
        """Entry i uploaded, derived from and cut to ``fields``: (F, H, W) on the device."""
        _, da, at = saved.entries[i]
        state = torch.from_numpy(np.array(da.values[at], dtype=np.float32, order="C")).to(device)
        parts = {f: state[saved.names.index(f)] for f in raw}
        if deriver is not None:
            dst, _ = deriver.add([state])
            parts.update({f: dst[0][dnames.index(f)] for f in fields if f not in saved.names})
        return torch.stack([parts[f] for f in fields]).contiguous()
    slices, n = {}, 0
    for key, idx in groups.items():                            # slice by slice: only one slice's samples lie on the device at a time
        c = build(((fields, sample(i)) for i in idx), fields, levels, saved.lat, saved.lon, device, key, half_window_days)
        slices[key], n = c.slices[_norm_key(key)], max(n, len(idx))
    return Climate(levels, fields, saved.lat, saved.lon, slices, n, half_window_days)
