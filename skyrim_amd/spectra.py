"""Zonal power spectra on the device (include/skyrim_spec.h): the power per zonal wavenumber of a forecast, of an ensemble's
members, mean and spread and, with a truth, of the truth and of the errors -- along latitude circles, averaged over latitude bands with
area weights, as WeatherBench 2 defines its zonal energy spectra (except that the Nyquist bin is not doubled here, so that the bins sum
to the mean square).  One HIP pass makes them where the states lie in HBM; nc x nb x 6 x K doubles per lead time go to the host.

Layers:

* the binding of libskyrim_spec.so (``SPEC``, ``load_library``, ``twiddles``, ``bound_factor``, ``describe``, ``workspace_bytes``,
  ``zonal``); the same call is ``torch.ops.skyrim_hip.zonal_spectra``.  It has no CPU fallback;
* the request: ``band_rows``, ``check_request``;
* the drivers: ``LeadSpectra`` (what ``ensemble.run`` calls at every saved lead time with ``spectra=...``), ``spectrum_model`` (the
  deterministic route, ``GlobalModel.spectrum_forecast``), ``spectra_prediction`` for forecasts on disk and ``from_members`` for member
  tensors that are already on the device;
* ``Spectra``: the result and its float64 host algebra.

Raw channels on the model's own grid, and in ``ensemble_forecast`` the fields of ``derived=[...]`` (the deriver's buffer is M (D, H, W)
states with a member table of their own: the same thing to the kernel).  Regridded and aggregated channels are refused by name.
"""
from __future__ import annotations

import ctypes
import datetime
import json
import math
from pathlib import Path

import numpy as np

from . import native
from .common import finish as _finish
from .leads import open_saved, require_gpu, run_model
from .members import fill_channels, member_set

# include/skyrim_spec.h SKSPEC_*
MAX_MEMBERS, MAX_CHANNELS, MAX_BANDS, MIN_W, MAX_W, MAX_H, CHUNK, SLOTS = 64, 32, 8, 2, 4096, 4096, 8, 6
KINDS = ("member", "mean", "spread", "truth", "error_mean", "error_member")          # the slots in their order
DEFAULT_BANDS = {"nh_mid": (30.0, 60.0), "tropics": (-20.0, 20.0), "sh_mid": (-60.0, -30.0), "globe": None}
EARTH_RADIUS_KM = 6371.0
U = 2.0 ** -24
_P = ctypes.c_void_p


class SpecDesc(ctypes.Structure):
    """skspec_desc."""
    _fields_ = [("members", _P), ("M", ctypes.c_int), ("truth", _P), ("C", ctypes.c_int), ("H", ctypes.c_int), ("W", ctypes.c_int),
                ("nc", ctypes.c_int), ("channels", ctypes.c_int32 * MAX_CHANNELS), ("nb", ctypes.c_int), ("j0", ctypes.c_int32 * MAX_BANDS),
                ("j1", ctypes.c_int32 * MAX_BANDS), ("lat_weight", _P), ("twiddles", _P), ("out", _P), ("workspace", _P),
                ("workspace_bytes", ctypes.c_size_t)]


SPEC = native.Spec("skyrim_spec", "SKYRIM_SPEC_LIB", "skspec", 1, {              # include/skyrim_spec.h SKSPEC_ABI_VERSION
    "skspec_abi_version": (ctypes.c_int, []),
    "skspec_twiddles": (ctypes.c_int, [ctypes.c_int, _P]),
    "skspec_bound_factor": (ctypes.c_double, [ctypes.c_int]),
    "skspec_workspace_bytes": (ctypes.c_size_t, [ctypes.POINTER(SpecDesc)]),
    "skspec_run": (ctypes.c_int, [ctypes.POINTER(SpecDesc), _P]),
}, " -- zonal spectra have no torch fallback")
EXPORTS, ABI_VERSION = SPEC.exports, SPEC.abi

_lib = None
_twiddles = {}                                              # (W, device) -> the uploaded table


def load_library() -> ctypes.CDLL:
    """libskyrim_spec.so (built in-tree by ``__graft_entry__.build()`` / ``make -C skyrim_amd/csrc``)."""
    global _lib
    if _lib is None:
        _lib = native.load(SPEC)
    return _lib


# ---- the binding ------------------------------------------------------------------------------------------------------------------------- #
def factor(W: int) -> list:
    """The radices of the transform of length ``W`` in the order the kernel applies them (4s, a 2, 3s, 5s); [] when W has another prime
    factor or lies outside [MIN_W, MAX_W]."""
    W, out = int(W), []
    if not MIN_W <= W <= MAX_W:
        return []
    while W % 4 == 0:
        out.append(4)
        W //= 4
    if W % 2 == 0:
        out.append(2)
        W //= 2
    for r in (3, 5):
        while W % r == 0:
            out.append(r)
            W //= r
    return out if W == 1 else []


def bound_factor(W: int) -> float:
    """c_W of the header's bound: a complex transform of the pair (a, b) errs by at most c_W u sqrt(rms(a)^2 + rms(b)^2) per coefficient."""
    rho = {2: 1.0, 4: 2.0, 3: 5.25, 5: 7.25}
    return 1.02 * sum(3.25 + math.sqrt(r) * rho[r] for r in factor(W))


def bound(W: int, rms_a, rms_b=0.0):
    """The header's bound on every coefficient of the transforms of a pair of rows with root mean squares ``rms_a`` and ``rms_b``."""
    return bound_factor(W) * U * np.sqrt(np.asarray(rms_a, np.float64) ** 2 + np.asarray(rms_b, np.float64) ** 2)


def twiddles(W: int) -> np.ndarray:
    """``skspec_twiddles``: the (W, 2) float32 table cos, -sin of 2 pi n / W, the bits the kernel is given."""
    tw = np.empty((int(W), 2), np.float32)
    lib = load_library()
    native.check(lib.skspec_twiddles(int(W), tw.ctypes.data_as(_P)), "skspec_twiddles", lib)
    return tw


def describe(M, C, H, W, channels, bands, truth: bool = False) -> SpecDesc:
    """The descriptor of a ``skspec_run`` call, its pointers still NULL (``truth``: a placeholder that only says there is one).
    ``bands``: row ranges (j0, j1)."""
    d = SpecDesc()
    d.M, d.C, d.H, d.W = int(M), int(C), int(H), int(W)
    fill_channels(d, channels, MAX_CHANNELS)
    bands = [(int(a), int(b)) for a, b in bands]
    d.nb = len(bands)
    for k, (a, b) in enumerate(bands[:MAX_BANDS]):
        d.j0[k], d.j1[k] = a, b
    if truth:
        d.truth = 4
    return d


def workspace_bytes(M, H, W, nc, bands, truth: bool = False) -> int:
    """``skspec_workspace_bytes``: 0 for arguments ``skspec_run`` would refuse."""
    d = describe(M, 1, H, W, [0] * int(nc), bands, truth)
    return int(load_library().skspec_workspace_bytes(ctypes.byref(d)))


def n_bins(W: int) -> int:
    return int(W) // 2 + 1


def device_twiddles(W: int, dev):
    """The twiddle table of ``W`` on ``dev``, uploaded once."""
    import torch
    key = (int(W), str(dev))
    if key not in _twiddles:
        _twiddles[key] = torch.from_numpy(twiddles(W)).to(dev)
    return _twiddles[key]


def zonal(members, table, truth, channels, bands, lat_weight, out, workspace) -> None:
    """One ``skspec_run``: the band spectra of the channels ``channels`` of the M ``members`` (equal-shaped contiguous float32 (C, H, W)
    device tensors; ``table`` = ``ensemble.member_table(members)``) and, when ``truth`` (C, H, W) is given, of the truth and the errors,
    over the row ranges ``bands`` = [(j0, j1), ...] with the H float64 weights ``lat_weight``, into ``out``, float64
    (nc, nb, 3 or 6, W // 2 + 1).  ``workspace``: a device tensor of at least ``workspace_bytes(...)`` bytes.  Queued on torch's current
    stream."""
    import torch
    M, dev, _ = member_set(members, table, "zonal_spectra", MAX_MEMBERS)
    C, H, W = members[0].shape
    channels = [int(c) for c in channels]
    bands = [(int(a), int(b)) for a, b in bands]
    if not 1 <= len(channels) <= MAX_CHANNELS:
        raise ValueError(f"zonal_spectra: {len(channels)} channels; 1 to {MAX_CHANNELS} are supported")
    if not 1 <= len(bands) <= MAX_BANDS:
        raise ValueError(f"zonal_spectra: {len(bands)} bands; 1 to {MAX_BANDS} are supported")
    if not factor(W):
        raise ValueError(f"zonal_spectra: W = {W}; the transform takes W = 2^a 3^b 5^c in [{MIN_W}, {MAX_W}]")
    d = describe(M, C, H, W, channels, bands)
    if truth is not None:
        d.truth = native.tensor_ptr(truth, "zonal_spectra: truth", torch.float32, dev)
        if truth.shape != members[0].shape:
            raise ValueError("zonal_spectra: the truth differs from the members in shape")
    d.members, d.lat_weight = table.data_ptr(), native.tensor_ptr(lat_weight, "zonal_spectra: lat_weight", torch.float64, dev)
    if lat_weight.numel() != H:
        raise ValueError(f"zonal_spectra: {lat_weight.numel()} weights for {H} rows")
    slots = SLOTS if truth is not None else 3
    d.out = native.tensor_ptr(out, "zonal_spectra: out", torch.float64, dev)
    if tuple(out.shape) != (len(channels), len(bands), slots, n_bins(W)):
        raise ValueError(f"zonal_spectra: out must be ({len(channels)}, {len(bands)}, {slots}, {n_bins(W)})")
    if not isinstance(workspace, torch.Tensor) or not workspace.is_cuda or workspace.device != dev or not workspace.is_contiguous():
        raise ValueError("zonal_spectra: workspace must be a contiguous device tensor")
    d.workspace, d.workspace_bytes = workspace.data_ptr(), workspace.numel() * workspace.element_size()
    d.twiddles = device_twiddles(W, dev).data_ptr()
    lib = load_library()
    with torch.cuda.device(dev):
        native.check(lib.skspec_run(ctypes.byref(d), native.stream(dev)), "skspec_run", lib)


# ---- the request ------------------------------------------------------------------------------------------------------------------------- #
def band_rows(lat, band, name: str = "band") -> tuple:
    """(j0, j1) of the latitude band ``band`` = (lat_s, lat_n) in degrees on the axis ``lat``: the rows with lat_s <= lat <= lat_n, the
    convention of ``scenarios.region_index``; None is every row.  An empty band and bounds outside [-90, 90] are ValueError."""
    lat = np.asarray(lat, np.float64)
    if band is None:
        return 0, int(lat.size)
    if not hasattr(band, "__len__") or len(band) != 2:
        raise ValueError(f"spectra: band {name!r} is (lat_s, lat_n) in degrees or None")
    lat_s, lat_n = (float(v) for v in band)
    if not (np.isfinite(lat_s) and np.isfinite(lat_n)) or lat_s < -90 or lat_n > 90:
        raise ValueError(f"spectra: band {name!r} = {tuple(band)} lies outside the grid: latitudes are in [-90, 90]")
    if lat_s > lat_n:
        raise ValueError(f"spectra: band {name!r} = {tuple(band)} is empty: lat_s > lat_n")
    rows = np.nonzero((lat >= lat_s) & (lat <= lat_n))[0]
    if rows.size == 0:
        raise ValueError(f"spectra: band {name!r} = {tuple(band)} holds no row of the grid (it lies outside the grid's latitudes or between "
                         "two rows)")
    return int(rows[0]), int(rows[-1]) + 1


def check_request(names, lat, lon, n_members: int, spec, other=()) -> dict:
    """Every refusal that needs no device; returns the request normalised: ``channels``, ``index``, ``bands`` (names), ``rows``
    [(j0, j1)].  ``spec``: a dict with ``channels`` and, optionally, ``bands`` {name: (lat_s, lat_n) or None}.  ``other``: names of
    regridded or aggregated channels of the same forecast (and of derived fields where the caller has no deriver), which this version
    refuses by name."""
    if not isinstance(spec, dict):
        raise ValueError("spectra: a dict with channels and bands")
    unknown = [k for k in spec if k not in ("channels", "bands")]
    if unknown:
        raise ValueError(f"spectra: unknown keys {unknown}")
    names, M = list(names), int(n_members)
    channels = list(spec.get("channels") or [])
    if not 1 <= len(channels) <= MAX_CHANNELS:
        raise ValueError(f"spectra: {len(channels)} channels; name 1 to {MAX_CHANNELS} (SKSPEC_MAX_CHANNELS)")
    for c in channels:
        if c in other and c not in names:
            raise ValueError(f"spectra: {c!r} is a regridded or aggregated channel; this version takes raw channels and derived fields on "
                             "the model's own grid only")
        if c not in names:
            raise ValueError(f"spectra: channel {c!r} is not an output channel of this model")
    if len(set(channels)) != len(channels):
        raise ValueError("spectra: a channel is named twice")
    if not 1 <= M <= MAX_MEMBERS:
        raise ValueError(f"spectra: n_members = {M}; 1 to {MAX_MEMBERS} (SKSPEC_MAX_MEMBERS)")
    bands = spec.get("bands")
    bands = dict(DEFAULT_BANDS) if bands is None else bands
    if not isinstance(bands, dict) or not 1 <= len(bands) <= MAX_BANDS:
        raise ValueError(f"spectra: bands is a dict of 1 to {MAX_BANDS} named latitude ranges (SKSPEC_MAX_BANDS)")
    H, W = len(lat), len(lon)
    if not factor(W):
        raise ValueError(f"spectra: {W} longitudes; the transform takes W = 2^a 3^b 5^c in [{MIN_W}, {MAX_W}]")
    if H > MAX_H:
        raise ValueError(f"spectra: {H} latitude rows; at most {MAX_H} (SKSPEC_MAX_H)")
    if len(names) * H * W > 2 ** 30:
        raise ValueError("spectra: a state holds at most 2^30 elements")
    rows = [band_rows(lat, b, str(k)) for k, b in bands.items()]
    return dict(channels=channels, index=[names.index(c) for c in channels], bands=[str(k) for k in bands], rows=rows)


def check_scored(channels, scored) -> None:
    """With a truth the truth must hold every spectrum channel: they must be among the channels the scorer holds a truth for."""
    unscored = [c for c in channels if c not in list(scored)]
    if unscored:
        raise ValueError(f"spectra: the channels {unscored} are not among the scored channels (the truth must hold them)")


# ---- the result -------------------------------------------------------------------------------------------------------------------------- #
def _iso(t) -> str:
    return t.isoformat() if hasattr(t, "isoformat") else str(t)


class Spectra:
    """What ``LeadSpectra.result`` returns.  ``power``: DataArray(time, channel, band, kind, wavenumber), float64; the kinds are
    ``KINDS`` (the first three without a truth).  Summed over the wavenumbers a value is the band's area-mean square of the field of
    that kind.  Everything below is float64 host algebra on ``power``."""

    def __init__(self, times, channels, bands, rows, lat, n_lon, n_members, power, model_name: str = "", forecast_id: str = ""):
        from .labeled import DataArray
        self.times, self.channels, self.bands = list(times), list(channels), list(bands)
        self.rows, self.lat, self.n_lon, self.n_members = [tuple(int(v) for v in r) for r in rows], np.asarray(lat, np.float64), int(n_lon), int(n_members)
        self.model_name, self.forecast_id = model_name, forecast_id
        power = np.asarray(power, np.float64)
        self.kinds = list(KINDS[:power.shape[3]]) if power.ndim == 5 else list(KINDS[:3])
        K = n_bins(self.n_lon)
        power = power.reshape(len(self.times), len(self.channels), len(self.bands), len(self.kinds), K)
        self.power = DataArray(power, ["time", "channel", "band", "kind", "wavenumber"],
                               dict(time=self.times, channel=self.channels, band=self.bands, kind=self.kinds, wavenumber=np.arange(K)))

    # -- access --
    def _kind(self, kind: str) -> np.ndarray:
        if kind not in self.kinds:
            raise ValueError(f"spectra: no {kind!r} spectrum" + (" (it needs a truth)" if kind in KINDS else f"; choose from {self.kinds}"))
        return self.power.values[:, :, :, self.kinds.index(kind), :]              # (time, channel, band, wavenumber)

    def _at(self, kind: str, channel: str, band: str) -> np.ndarray:
        if channel not in self.channels:
            raise ValueError(f"spectra: channel {channel!r} was not requested")
        if band not in self.bands:
            raise ValueError(f"spectra: band {band!r} was not requested")
        return self._kind(kind)[:, self.channels.index(channel), self.bands.index(band), :]

    def band_latitude(self, band: str) -> float:
        """The area-weighted mean latitude of the band's rows, in degrees."""
        from .verify import area_weights
        if band not in self.bands:
            raise ValueError(f"spectra: band {band!r} was not requested")
        j0, j1 = self.rows[self.bands.index(band)]
        w = area_weights(self.lat)[j0:j1]
        return float((w * self.lat[j0:j1]).sum() / w.sum())

    def wavelength_km(self, band: str) -> np.ndarray:
        """The wavelength of every wavenumber: the circumference of the latitude circle at the band's area-weighted mean latitude
        divided by k (k = 0: inf)."""
        circ = 2.0 * math.pi * EARTH_RADIUS_KM * math.cos(math.radians(self.band_latitude(band)))
        k = np.arange(n_bins(self.n_lon), dtype=np.float64)
        with np.errstate(divide="ignore"):
            return np.where(k > 0, circ / np.where(k > 0, k, 1.0), np.inf)

    def kinetic_energy(self, level, kind: str = "member") -> np.ndarray:
        """(time, band, wavenumber): (P[u<level>] + P[v<level>]) / 2 of the kind ``kind``; both channels must have been requested."""
        u, v = f"u{level}", f"v{level}"
        missing = [c for c in (u, v) if c not in self.channels]
        if missing:
            raise ValueError(f"spectra: kinetic_energy({level!r}) needs the channels {missing} to have been requested")
        p = self._kind(kind)
        return 0.5 * (p[:, self.channels.index(u)] + p[:, self.channels.index(v)])

    def ratio(self, kind_a: str, kind_b: str) -> np.ndarray:
        """(time, channel, band, wavenumber): the power of ``kind_a`` over that of ``kind_b`` (0 / 0 is NaN)."""
        with np.errstate(divide="ignore", invalid="ignore"):
            return self._kind(kind_a) / self._kind(kind_b)

    def effective_resolution(self, channel: str, band: str, ratio: float = 0.5) -> np.ndarray:
        """(time,): per lead time the shortest wavelength in km down to which the ``member`` power stays >= ``ratio`` times the ``truth``
        power at every larger scale (k = 1 upwards); inf when already wavenumber 1 falls short."""
        mem, tru = self._at("member", channel, band), self._at("truth", channel, band)
        lam = self.wavelength_km(band)
        out = np.empty(len(self.times))
        for t in range(len(self.times)):
            ok = mem[t, 1:] >= ratio * tru[t, 1:]
            last = int(ok.size if ok.all() else np.argmin(ok))                    # wavenumbers 1 .. last hold
            out[t] = lam[last]
        return out

    def spread_skill(self, channel: str, band: str) -> np.ndarray:
        """(time, wavenumber): sqrt((M + 1) / M * spread / error_mean), the spread/skill ratio of ``verify`` resolved by scale."""
        M = self.n_members
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.sqrt((M + 1.0) / M * self._at("spread", channel, band) / self._at("error_mean", channel, band))

    # -- files --
    def file_name(self) -> str:
        return f"{self.model_name or 'forecast'}-spectra.json"

    def to_json(self) -> str:
        def clean(a):                                           # JSON has no NaN: non-finite values are written as null
            return [clean(v) for v in a] if isinstance(a, list) else (a if math.isfinite(a) else None)
        return json.dumps(dict(model=self.model_name, n_members=self.n_members, forecast_id=self.forecast_id, times=[_iso(t) for t in self.times],
                               channels=self.channels, bands=self.bands, rows=[list(r) for r in self.rows], lat=self.lat.tolist(), n_lon=self.n_lon,
                               kinds=self.kinds, power=clean(self.power.values.tolist())))

    def save(self, path) -> str:
        """Write the JSON document; ``path``: a ``.json`` file, or a directory, in which the file is ``{dir}/{forecast id}/{model}-spectra.json``."""
        path = Path(path)
        if path.suffix.lower() != ".json":
            path = (path / self.forecast_id if self.forecast_id else path) / self.file_name()
        path.parent.mkdir(parents=True, exist_ok=True)
        path.write_text(self.to_json())
        return str(path)

    @classmethod
    def from_json(cls, text: str) -> "Spectra":
        doc = json.loads(text)
        power = np.array([np.nan if v is None else v for v in _flatten(doc["power"])], np.float64)
        times = [datetime.datetime.fromisoformat(t) if isinstance(t, str) and "T" in t else t for t in doc["times"]]
        power = power.reshape(len(times), len(doc["channels"]), len(doc["bands"]), len(doc["kinds"]), -1)
        return cls(times, doc["channels"], doc["bands"], doc["rows"], doc["lat"], doc["n_lon"], doc["n_members"], power, doc.get("model", ""),
                   doc.get("forecast_id", ""))

    @classmethod
    def load(cls, path) -> "Spectra":
        return cls.from_json(Path(path).read_text())


def _flatten(a):
    for v in a:
        if isinstance(v, list):
            yield from _flatten(v)
        else:
            yield v


def merge(parts, channels) -> Spectra:
    """One ``Spectra`` of several that share times, bands and kinds (the raw channels' and the derived fields' of one forecast), its
    channels in the order ``channels``."""
    parts = list(parts)
    first = parts[0]
    if len(parts) == 1 and first.channels == list(channels):
        return first
    for p in parts[1:]:
        if p.times != first.times or p.bands != first.bands or p.kinds != first.kinds:
            raise ValueError("spectra: only spectra of the same times, bands and kinds can be merged")
    have = [c for p in parts for c in p.channels]
    power = np.concatenate([p.power.values for p in parts], axis=1)[:, [have.index(c) for c in channels]]
    return Spectra(first.times, list(channels), first.bands, first.rows, first.lat, first.n_lon, first.n_members, power, first.model_name,
                   first.forecast_id)


# ---- the drivers ------------------------------------------------------------------------------------------------------------------------- #
class LeadSpectra:
    """The spectra of one lead time after the other.  ``names``: the channels of the (C, H, W) states in their order; ``spec``: the dict of
    ``ensemble_forecast(spectra=...)``.  ``add`` makes ONE ``zonal`` call and copies its (nc, nb, kinds, K) doubles to the host.
    ``truth=True``: ``add`` is given the truth state of the valid time."""

    def __init__(self, names, lat, lon, n_members, spec, device="cuda:0", truth: bool = False):
        self.req = check_request(names, lat, lon, n_members, spec)
        self.names, self.M, self.device, self.truth = list(names), int(n_members), device, bool(truth)
        self.lat, self.lon = np.asarray(lat, np.float64), np.asarray(lon, np.float64)
        from .verify import area_weights
        self.weights = area_weights(self.lat)
        self.times, self.parts = [], []
        self._dev = None

    def _buffers(self):
        if self._dev is None:
            import torch
            dev = torch.device(self.device)
            nc, nb, H, W = len(self.req["index"]), len(self.req["rows"]), self.lat.size, self.lon.size
            need = workspace_bytes(self.M, H, W, nc, self.req["rows"], self.truth)
            self._dev = dict(w=torch.from_numpy(self.weights).to(dev),
                             out=torch.empty((nc, nb, SLOTS if self.truth else 3, n_bins(W)), dtype=torch.float64, device=dev),
                             ws=torch.empty(max(need // 8, 1), dtype=torch.float64, device=dev))
        return self._dev

    def add(self, time, states, table=None, truth=None) -> None:
        from . import ensemble as E
        if len(states) != self.M:
            raise ValueError(f"{len(states)} states for spectra of {self.M} members")
        if self.truth != (truth is not None):
            raise ValueError("spectra: the truth state is given exactly when truth=True")
        b, r = self._buffers(), self.req
        table = E.member_table(states) if table is None else table
        zonal(states, table, truth, r["index"], r["rows"], b["w"], b["out"], b["ws"])
        self.times.append(time)
        self.parts.append(b["out"].cpu().numpy())

    def result(self, model_name: str = "", forecast_id: str = "") -> Spectra:
        r = self.req
        kinds = SLOTS if self.truth else 3
        power = np.stack(self.parts) if self.parts else np.zeros((0, len(r["channels"]), len(r["bands"]), kinds, n_bins(self.lon.size)))
        return Spectra(self.times, r["channels"], r["bands"], r["rows"], self.lat, self.lon.size, self.M, power, model_name, forecast_id)


class TruthStates:
    """The truth of a valid time as a (C, H, W) device state in the forecast's channel order: the channels ``channels`` are filled from
    ``truth`` (a data source, a DataArray or a saved forecast, as ``verify`` takes them), the others stay zero."""

    def __init__(self, truth, names, channels, lat, lon, device):
        import torch
        from .verify import _Fields
        self.fields = _Fields(truth, "truth", lat, lon)
        missing = [c for c in channels if c not in self.fields.names]
        if missing:
            raise ValueError(f"spectra: the truth does not hold the channels {missing}")
        self.channels, self.device = list(channels), torch.device(device)
        self.index = [list(names).index(c) for c in channels]
        self.shape = (len(names), len(lat), len(lon))
        self.state = None

    def at(self, time):
        import torch
        if self.state is None:
            self.state = torch.zeros(self.shape, dtype=torch.float32, device=self.device)
            self._idx = torch.tensor(self.index, device=self.device)
        self.state[self._idx] = torch.from_numpy(self.fields.at(time, self.channels)).to(self.device)
        return self.state


def spectrum_model(gm, start_time, n_steps: int = 4, spectra=None, truth=None, save: bool = False, save_config: dict | None = None) -> Spectra:
    """``GlobalModel.spectrum_forecast`` (core/models/base.py has the user-facing description): the deterministic route, M = 1, driven
    like ``verify``; no state goes to the host."""
    model = gm.model
    if spectra is None:
        raise ValueError("spectrum_forecast: spectra={'channels': [...], 'bands': {...}}")
    if n_steps < 0:
        raise ValueError("n_steps >= 0")
    names = list(model.out_channel_names)
    ls = LeadSpectra(names, model.grid.lat, model.grid.lon, 1, spectra, device=model.device, truth=truth is not None)
    require_gpu(model.device, "spectrum_forecast makes the spectra with HIP kernels where the states lie: the model must be on a GPU")
    truths = None if truth is None else TruthStates(truth, names, ls.req["channels"], model.grid.lat, model.grid.lon, model.device)
    run_model(gm, start_time, n_steps, lambda k, time, state: ls.add(time, [state], None, None if truths is None else truths.at(time)))
    return _finish(ls.result(gm.model_name), save, save_config)


def spectra_prediction(pred, truth=None, channels=None, bands=None, device="cuda:0", model_name: str = "") -> Spectra:
    """The spectra of a forecast that already exists: a ``GlobalPrediction``, a (time, channel, lat, lon) DataArray, a saved netCDF file
    or zarr store, or a list of such files (their time entries in order, duplicates of a valid time taken once) -- the route for GraphCast,
    as ``verify.score_prediction``.  Each time entry is uploaded on its own and goes through the same kernel as ``spectrum_forecast``."""
    saved = open_saved(pred, "spectra_prediction")
    names, lat, lon = saved.names, saved.lat, saved.lon
    spec = dict(channels=list(channels) if channels is not None else names)
    if bands is not None:
        spec["bands"] = bands
    ls = LeadSpectra(names, lat, lon, 1, spec, device=device, truth=truth is not None)
    require_gpu(device, "spectra_prediction makes the spectra with HIP kernels: it needs a GPU", present=True)
    truths = None if truth is None else TruthStates(truth, names, ls.req["channels"], lat, lon, device)
    for _, time, state in saved.states(device):
        ls.add(time, [state], None, None if truths is None else truths.at(time))
    return ls.result(model_name or saved.model_name or "forecast")


def from_members(members, lat, lon, names=None, channels=None, bands=None, truth=None, times=None) -> Spectra:
    """The spectra of member tensors that are already on the device.  ``members``: M float32 device tensors, each (C, H, W) for one
    valid time or (T, C, H, W) for T of them; ``names``: their C channel names (default "0", "1", ...); ``channels``: the names the
    spectra are made of (default: all); ``bands``: {name: (lat_s, lat_n) or None} (default: ``DEFAULT_BANDS``); ``truth``: a tensor of a
    member's shape; ``times``: the T labels."""
    import torch
    members = list(members)
    if not members or not all(isinstance(t, torch.Tensor) for t in members) or members[0].dim() not in (3, 4):
        raise ValueError("from_members: members are (C, H, W) or (T, C, H, W) tensors")
    if members[0].dim() == 3:
        members = [t[None] for t in members]
        truth = None if truth is None else truth[None]
    T, C = members[0].shape[0], members[0].shape[1]
    names = [str(k) for k in range(C)] if names is None else list(names)
    if len(names) != C:
        raise ValueError(f"from_members: {len(names)} names for {C} channels")
    spec = dict(channels=list(channels) if channels is not None else names)
    if bands is not None:
        spec["bands"] = bands
    ls = LeadSpectra(names, lat, lon, len(members), spec, device=members[0].device, truth=truth is not None)
    if not members[0].is_cuda:
        raise RuntimeError("from_members makes the spectra with HIP kernels: the members must be on a GPU")
    times = list(range(T)) if times is None else list(times)
    for t in range(T):
        ls.add(times[t], [m[t].contiguous() for m in members], None, None if truth is None else truth[t].contiguous())
    return ls.result()
