"""Perturbed-initial-condition ensembles of ONE model (include/skyrim_ens.h).

Four layers:

* the binding of libskyrim_ens.so (``SPEC``, ``load_library``, ``perturb``, ``stats``, ``member_table``); the same calls are
  ``torch.ops.skyrim_hip.ens_perturb / ens_stats`` (skyrim_amd/ops.py);
* ``ProductSet`` -- the products of one family of fields (raw, derived, regridded, one window group of aggregates): their buffers,
  the ``stats`` launches and copies of an entry, its files, its labelled arrays;
* ``run`` -- what ``GlobalModel.ensemble_forecast`` does: the initial condition once, M members from ``ens_perturb`` (white noise) or
  ``noise.Perturber`` (``perturbation="spherical"``: correlated fields, skyrim_amd/noise.py), with ``breeding=`` bred from those seeds
  through the model itself (skyrim_amd/breeding.py), ONE TimeLoop
  generator per member advanced step-major (all members one step, then the statistics of that lead time), so only the members'
  current states are alive on the GPU; with ``stochastic=`` the members are held as states instead and every step of every member
  but the control is perturbed (SPPT, additive noise: skyrim_amd/stochastic.py);
* ``EnsembleForecast`` -- the labelled products, and their files in the layout of every other forecast of this package.

Members sharded over ranks stay with ``skyrim_amd/pangu/ensemble.py``; multi-MODEL ensembles are ``core/models/ensemble.py``.
"""
from __future__ import annotations

import ctypes
import datetime
import functools
import math
from dataclasses import dataclass, field

import numpy as np
import torch

from . import native
from .common import world_size as _world_size
from .members import member_set, member_table          # noqa: F401 (member_table: this module's callers build the table with it)

MAX_MEMBERS, MAX_THRESHOLDS, MAX_QUANTILES = 64, 4, 4          # include/skyrim_ens.h SKENS_MAX_*
PRODUCTS = ("mean", "spread", "min", "max")
_P = ctypes.c_void_p


class StatsDesc(ctypes.Structure):
    """skens_stats_desc."""
    _fields_ = [("members", _P), ("M", ctypes.c_int), ("member_align", ctypes.c_int), ("offset", ctypes.c_size_t), ("n", ctypes.c_size_t),
                ("mean", _P), ("spread", _P), ("min", _P), ("max", _P), ("exceed", _P), ("n_thr", ctypes.c_int),
                ("thr", ctypes.c_float * MAX_THRESHOLDS), ("quant", _P), ("n_quant", ctypes.c_int),
                ("q_index", ctypes.c_int * MAX_QUANTILES), ("q_frac", ctypes.c_float * MAX_QUANTILES)]


SPEC = native.Spec("skyrim_ens", "SKYRIM_ENS_LIB", "skens", 1, {               # include/skyrim_ens.h SKENS_ABI_VERSION
    "skens_abi_version": (ctypes.c_int, []),
    "skens_perturb": (ctypes.c_int, [_P, _P, _P, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_int, ctypes.c_float, ctypes.c_uint32,
                                     ctypes.c_uint32, ctypes.c_int, _P]),
    "skens_stats": (ctypes.c_int, [ctypes.POINTER(StatsDesc), _P]),
}, " -- ensemble members and statistics have no torch fallback")
EXPORTS, ABI_VERSION = SPEC.exports, SPEC.abi

_lib = None


def load_library() -> ctypes.CDLL:
    """libskyrim_ens.so (built in-tree by ``__graft_entry__.build()`` / ``make -C skyrim_amd/csrc``)."""
    global _lib
    if _lib is None:
        _lib = native.load(SPEC)
    return _lib


def quantile_position(level: float, M: int) -> tuple[int, float]:
    """(index, fraction) of numpy's "linear" quantile of M sorted values: h = (M - 1) * level in double; the fraction is what the kernel
    multiplies with in fp32, so a fraction that rounds up to 1 there becomes the next index."""
    if not (0.0 <= level <= 1.0):
        raise ValueError(f"quantile level {level} is outside [0, 1]")
    h = (M - 1) * float(level)
    k = min(int(math.floor(h)), M - 1)
    f = float(np.float32(h - k))
    if f >= 1.0:
        k, f = k + 1, 0.0
    if k >= M - 1:
        k, f = M - 1, 0.0
    return k, f


def perturb(x0: torch.Tensor, std: torch.Tensor, out: torch.Tensor, chan_stride: int, scale: float, seed: int, member_first: int) -> None:
    """``out`` (``k * x0.numel()`` elements: members ``member_first .. member_first + k - 1``, one after the other) from the flat
    (L, C, H, W) state ``x0`` and the C per-channel sigmas ``std``; ``chan_stride`` = H * W.  Queued on torch's current stream."""
    dev = x0.device
    px = native.tensor_ptr(x0, "ens_perturb: x0", torch.float32)
    ps, po = (native.tensor_ptr(t, f"ens_perturb: {w}", torch.float32, dev) for t, w in ((std, "std"), (out, "out")))
    n = x0.numel()
    if n == 0 or out.numel() % n or out.numel() == 0:
        raise ValueError(f"ens_perturb: out holds {out.numel()} elements, not a multiple of the state's {n}")
    if not (0 <= seed < 2 ** 32 and 0 <= member_first < 2 ** 32):
        raise ValueError("ens_perturb: seed and member are 32-bit (the generator's key)")
    lib = load_library()
    with torch.cuda.device(dev):
        native.check(lib.skens_perturb(px, ps, po, n, chan_stride, std.numel(), scale, seed, member_first, out.numel() // n, native.stream(dev)),
                     "skens_perturb", lib)


def stats(members, table: torch.Tensor, offset: int, n: int, mean=None, spread=None, min=None, max=None, exceed=None, thresholds=(),
          quant=None, levels=()) -> None:
    """One pass over the flat range [offset, offset + n) of the M ``members`` (equal-sized contiguous float32 device tensors; ``table`` =
    ``member_table(members)``): the outputs that are not None are written at range-relative positions -- ``mean / spread / min / max``: n
    elements, ``exceed``: len(thresholds) x n, ``quant``: len(levels) x n.  Queued on torch's current stream."""
    M, dev, align = member_set(members, table, "ens_stats", MAX_MEMBERS, ndim=None, same="numel")
    if members[0].numel() < offset + n:
        raise ValueError(f"ens_stats: a member holds {members[0].numel()} elements, the range ends at {offset + n}")
    if offset < 0 or n < 0 or len(thresholds) > MAX_THRESHOLDS or len(levels) > MAX_QUANTILES:
        raise ValueError(f"ens_stats: at most {MAX_THRESHOLDS} thresholds and {MAX_QUANTILES} quantile levels, a non-negative range")
    if (exceed is None) != (len(thresholds) == 0) or (quant is None) != (len(levels) == 0):
        raise ValueError("ens_stats: exceed goes with thresholds, quant with levels")
    d = StatsDesc()
    d.members, d.M, d.member_align, d.offset, d.n = table.data_ptr(), M, align, offset, n
    for name, t, rows in (("mean", mean, 1), ("spread", spread, 1), ("min", min, 1), ("max", max, 1), ("exceed", exceed, len(thresholds)),
                          ("quant", quant, len(levels))):
        if t is not None:
            if native.tensor_ptr(t, f"ens_stats: {name}", torch.float32, dev) and t.numel() != rows * n:
                raise ValueError(f"ens_stats: {name} holds {t.numel()} elements, expected {rows * n}")
            setattr(d, name, t.data_ptr())
    d.n_thr, d.n_quant = len(thresholds), len(levels)
    for k, v in enumerate(thresholds):
        d.thr[k] = float(v)
    for k, v in enumerate(levels):
        d.q_index[k], d.q_frac[k] = quantile_position(v, M)
    lib = load_library()
    with torch.cuda.device(dev):
        native.check(lib.skens_stats(ctypes.byref(d), native.stream(dev)), "skens_stats", lib)


# ---- the products of one family of fields ------------------------------------------------------------------------------------------- #
class ProductSet:
    """The statistics of ONE family of fields on one grid, entry by entry: the raw channels, the derived fields, the regridded channels
    or the aggregates of one window group (DESIGN.md 17 has the launch rule).  ``entries``: the saved leads, or the group's windows;
    ``exceed`` / ``quantiles``: the tables of this family's fields; ``prefix``: what stands before the product in a file's model name
    (``""``, ``"derived-"``, ``"regrid-"``, ``"agg{label}-"``); ``always``: the outputs every ``reduce`` computes, stored or not."""

    def __init__(self, model_name, M, products, device, fields, lat, lon, entries, exceed, quantiles, keep_members, prefix="", always=()):
        self.model_name, self.M, self.products, self.prefix, self.always = model_name, M, products, prefix, always
        self.fields, self.lat, self.lon, self.exceed, self.quantiles = list(fields), np.asarray(lat), np.asarray(lon), exceed, quantiles
        F, grid = len(self.fields), (len(self.lat), len(self.lon))
        self.hw = grid[0] * grid[1]

        def host(rows):
            return np.empty((entries, rows, *grid), np.float32)

        def dev(rows):
            return torch.empty((rows, *grid), dtype=torch.float32, device=device)
        self.host = {p: host(F) for p in products}
        self.host_ex = {ch: host(len(v)) for ch, v in exceed.items()}
        self.host_q = {ch: host(len(v)) for ch, v in quantiles.items()}
        self.members = np.empty((M, entries, F, *grid), np.float32) if keep_members else None
        self.dev = {p: dev(F) for p in dict.fromkeys((*products, *always))}
        self.dev_ex = {ch: dev(len(v)) for ch, v in exceed.items()}
        self.dev_q = {ch: dev(len(v)) for ch, v in quantiles.items()}

    def reduce(self, states, table, slot) -> None:
        """Entry ``slot`` from the M ``states`` of this family's fields: one launch over all fields for the products, one per exceed
        channel and one per quantile channel, each result to the host, then the states themselves with ``keep_members``.
        ``slot=None``: the ``always`` outputs only, left on the device (``dev``)."""
        n = self.hw
        out = {p: self.dev[p] for p in (*(self.products if slot is not None else ()), *self.always)}
        if out:
            stats(states, table, 0, len(self.fields) * n, **out)
        if slot is None:
            return
        for p in self.products:
            self.host[p][slot] = self.dev[p].cpu().numpy()
        for ch, thr in self.exceed.items():
            stats(states, table, self.fields.index(ch) * n, n, exceed=self.dev_ex[ch], thresholds=thr)
            self.host_ex[ch][slot] = self.dev_ex[ch].cpu().numpy()
        for ch, lev in self.quantiles.items():
            stats(states, table, self.fields.index(ch) * n, n, quant=self.dev_q[ch], levels=lev)
            self.host_q[ch][slot] = self.dev_q[ch].cpu().numpy()
        if self.members is not None:
            for m, st in enumerate(states):
                self.members[m, slot] = st.cpu().numpy()

    def save(self, first, times, start, source, cfg) -> list:
        """One file per product with the entries ``first ..`` valid at ``times``, named from ``start`` to ``times[-1]``; returns the
        paths.  zarr: one store per product under the forecast id, appended along time."""
        from .common import save_forecast
        from .labeled import DataArray
        paths = []
        for p in self.products:
            da = DataArray(self.host[p][first:first + len(times)], ["time", "channel", "lat", "lon"],
                           dict(time=times, channel=self.fields, lat=self.lat, lon=self.lon))
            name = product_model_name(self.model_name, self.M, self.prefix + p)
            pcfg = dict(cfg, forecast_id=f"{cfg['forecast_id']}/{name}") if (cfg.get("file_type") or "netcdf") == "zarr" else cfg
            paths.append(save_forecast(da, name, start, times[-1], source, config=pcfg))
        return paths

    def fill(self, result, times, channels=None, window_start=None) -> None:
        """The labelled arrays as attributes of ``result``: the products, ``exceedance``, ``quantile`` and, when kept, ``members``.
        ``channels``: the selection on the channel dimension of products and members; ``window_start``: the coordinate that goes with
        ``times`` when those are window ends."""
        from .labeled import DataArray
        coords = dict({} if window_start is None else dict(window_start=window_start), lat=self.lat, lon=self.lon)

        def labelled(arr, dim, labels):
            da = DataArray(arr, ["time", dim, "lat", "lon"], dict(time=times, **{dim: labels}, **coords))
            return da.sel(channel=list(channels)) if channels and dim == "channel" else da
        for p in self.products:
            setattr(result, p, labelled(self.host[p], "channel", self.fields))
        result.exceedance = {ch: labelled(self.host_ex[ch], "threshold", np.asarray(v, np.float32)) for ch, v in self.exceed.items()}
        result.quantile = {ch: labelled(self.host_q[ch], "quantile", np.asarray(v, np.float64)) for ch, v in self.quantiles.items()}
        if self.members is not None:
            da = DataArray(self.members, ["member", "time", "channel", "lat", "lon"],
                           dict(member=np.arange(self.M), time=times, channel=self.fields, **coords))
            result.members = da.sel(channel=list(channels)) if channels else da


def split_table(table, fields) -> tuple[dict, dict]:
    """(the entries of the ``{field: values}`` table that name one of ``fields``, the other entries)."""
    return {k: v for k, v in table.items() if k in fields}, {k: v for k, v in table.items() if k not in fields}


def _stamped(maker, fid):
    """``maker.result()`` with the forecast id on it."""
    res = maker.result()
    res.forecast_id = fid
    return res


def _save_result(res, cfg, paths) -> None:
    """Write a result object under the forecast's output directory and note its path."""
    from .common import OUTPUT_DIR
    paths.append(res.save(cfg.get("output_dir") or OUTPUT_DIR))


# ---- the driver ---------------------------------------------------------------------------------------------------------------------- #
@dataclass
class EnsembleForecast:
    """What ``ensemble_forecast`` returns.  ``mean / spread / min / max``: DataArray(time, channel, lat, lon) or None when not asked
    for; ``exceedance[channel]``: (time, threshold, lat, lon) -- the fraction of members above each threshold; ``quantile[channel]``:
    (time, quantile, lat, lon); ``members``: (member, time, channel, lat, lon) with ``keep_members=True``; ``paths``: the files written."""
    model_name: str
    n_members: int
    seed: int
    perturb_scale: float
    mean: object = None
    spread: object = None
    min: object = None
    max: object = None
    exceedance: dict = field(default_factory=dict)
    quantile: dict = field(default_factory=dict)
    members: object = None
    paths: list = field(default_factory=list)
    forecast_id: str = ""
    scores: object = None        # verify.Scores with ``scores=True``
    perturbation: str = "white"  # "white" (skens_perturb) or "spherical" (skyrim_amd/noise.py)
    length_scale_km: float = 500.0
    alpha: float = 2.0
    lmax: object = None          # the truncation used, spherical only
    tracks: object = None        # tracks.Tracks with ``tracks=True``
    derived: object = None       # derived.DerivedProducts with ``derived=[...]``
    regridded: object = None     # regrid.RegriddedProducts with ``grid=...``
    aggregated: dict = field(default_factory=dict)      # {window label: aggregate.AggregatedProducts} with ``aggregates=[...]``
    points: object = None        # points.PointForecast with ``points=...``
    scenarios: object = None     # scenarios.Scenarios with ``scenarios={...}``
    spectra: object = None       # spectra.Spectra with ``spectra={...}``
    breeding: object = None      # the normalised ``breeding=`` request (cycles, norm, paired) or None
    breeding_growth: object = None      # (cycles, member, channel) float64 with ``breeding=``: breeding.Breeder.growth
    stochastic: object = None    # the normalised ``stochastic=`` request (stochastic.Plan.as_dict) or None
    objects: object = None       # objects.Objects with ``objects={...}``


def product_model_name(model_name: str, n_members: int, product: str) -> str:
    """The model field of a product's file name: ``{model}-ens{M}-{product}`` (no ``__``, so the name still splits into its four parts)."""
    return f"{model_name}-ens{n_members}-{product}"


def channel_std(model) -> torch.Tensor:
    """The per-channel sigma of ``model``'s input channels that scales the perturbation: the TimeLoop's ``channel_std``."""
    std = getattr(model, "channel_std", None)
    if std is None:
        raise NotImplementedError(f"{type(model).__name__} has no channel_std: perturbed members need the model's per-channel scale")
    return std.to(model.device, torch.float32).reshape(-1).contiguous()


def scenario_std(model, names) -> np.ndarray:
    """The sigma of each OUTPUT channel for ``scenarios={"normalise": "std"}``: ``channel_std`` when the model's output channels are its
    input channels (one sigma each), refused otherwise."""
    std = channel_std(model).cpu().numpy().astype(np.float64)
    if std.size != len(names):
        raise NotImplementedError(f"{type(model).__name__}: channel_std holds {std.size} values for {len(names)} output channels; "
                                  "normalise='std' needs one per output channel")
    return std


def validate(model, n_steps, n_members, seed, products, exceed, quantiles, channels, save_every, keep_members, events=None,
             neighbourhoods_km=(), scores=False, points=None, point_channels=None, point_method="bilinear", scenarios=None, spectra=None, objects=None, breeding=None,
             stochastic=None, aggregates=None, derived_surface=None, derived=None, grid=None, regrid_method="conservative", perturbation="white", length_scale_km=500.0, alpha=2.0, lmax=None,
             perturb_channels=None):
    """Every refusal that needs no device; returns (products, exceed, quantiles, saved step numbers) normalised.  ``derived``: the
    derived fields asked for (skyrim_amd/derived.py); ``exceed`` and ``quantiles`` may then name them alongside the raw channels.
    ``aggregates``: the time-window aggregates asked for (skyrim_amd/aggregate.py), of raw channels and derived fields on the model's own
    grid; ``exceed``, ``quantiles`` and ``events`` may name them (``ws10m_max_24h``) as well.  ``grid`` / ``regrid_method``: the target grid of skyrim_amd/regrid.py the products are also made on.  ``events`` /
    ``neighbourhoods_km``: the threshold events verified with the ``scores`` (skyrim_amd/events.py; ``event_request`` normalises them).
    ``points`` / ``point_channels`` / ``point_method``: the places every member is sampled at (skyrim_amd/points.py), the raw channels and
    derived fields sampled there (default: ``channels``, or all raw channels) and the interpolation.  ``scenarios``: the dict of
    skyrim_amd/scenarios.py (channels, region, n_clusters, n_eofs, normalise): raw channels on the model's own grid only.  ``breeding``:
    the dict of skyrim_amd/breeding.py (cycles, norm, paired); ``perturbation`` then names the seed.  ``stochastic``: the dict of
    skyrim_amd/stochastic.py (kind, amplitude, clip, additive_scale, tau_h, length_scale_km, alpha, lmax, channels).  ``spectra``: the dict
    of skyrim_amd/spectra.py (channels, bands): raw channels and fields of ``derived`` on the model's own grid.  ``objects``: the dict
    of skyrim_amd/objects.py (thresholded channels or derived fields, their filters, connectivity, min_pixels, capacity)."""
    from . import noise
    from .core.models.utils import _PINNED_LIMIT
    if _world_size() > 1:
        raise NotImplementedError("ensemble_forecast runs all members on one GPU; under a process group of more than one rank use "
                                  "skyrim_amd.pangu.ensemble.MemberParallelEnsemble (members sharded over ranks)")
    if not 1 <= int(n_members) <= MAX_MEMBERS:
        raise ValueError(f"n_members = {n_members}: 1 to {MAX_MEMBERS} members are supported (SKENS_MAX_MEMBERS)")
    if n_steps < 0 or save_every < 1:
        raise ValueError("n_steps >= 0 and save_every >= 1")
    if not 0 <= int(seed) < 2 ** 32:
        raise ValueError("seed is a 32-bit unsigned integer (the generator's key)")
    products = tuple(products)
    unknown = [p for p in products if p not in PRODUCTS]
    if unknown:
        raise ValueError(f"unknown products {unknown}; choose from {PRODUCTS}")
    names = list(model.out_channel_names)
    if derived is not None:
        from . import derived as deriving
        deriving.check_request(names, list(derived), model.grid.lat, model.grid.lon, n_members, surface=derived_surface is not None)
    known = names + list(derived or [])
    aplan = None
    if aggregates is not None:
        from . import aggregate
        aplan = aggregate.check_request(known, aggregates, model.time_step, n_steps, model.grid.lat, model.grid.lon, n_members)
        clash = [f for g in aplan.groups for f in g.fields if f in known]
        if clash:
            raise ValueError(f"aggregates: {clash} are already channels of this forecast")
        known = known + [f for g in aplan.groups for f in g.fields]
    tabs = None
    if grid is not None:
        from . import regrid
        if derived is not None:
            raise ValueError("grid= together with derived= is not supported: derived fields are made on the model's own grid only "
                             "(DESIGN.md 22, out of scope)")
        tabs = regrid.check_request(names, model.grid.lat, model.grid.lon, n_members, grid, regrid_method)
    for what, table, cap in (("exceed", exceed, MAX_THRESHOLDS), ("quantiles", quantiles, MAX_QUANTILES)):
        for ch, vals in (table or {}).items():
            if ch not in known:
                raise ValueError(f"{what}: channel {ch!r} is not an output channel of this model"
                                 + ("" if derived is None else " or one of the derived fields")
                                 + ("" if aplan is None else " or one of the aggregates"))
            if not 1 <= len(vals) <= cap:
                raise ValueError(f"{what}[{ch!r}]: 1 to {cap} values per channel, got {len(vals)}")
    for ch, vals in (quantiles or {}).items():
        for q in vals:
            quantile_position(q, int(n_members))
    if events is not None:
        event_request(events, neighbourhoods_km, exceed, known, n_members, scores)
    missing = [c for c in (channels or []) if c not in names]
    if missing:
        raise ValueError(f"channels {missing} are not output channels of this model")
    noise.plan(model, perturbation, length_scale_km, alpha, lmax, perturb_channels)      # kind, length scale, lmax, grid, channels
    if breeding is not None:                                # cycles, norm, keys; one history level, the same channels in and out
        from . import breeding as breed
        breed.plan(model, breeding)
    if stochastic is not None:                              # kind, amplitudes, the pattern's spectrum and grid, a model that steps from one state
        from . import stochastic as stoch
        stoch.plan(model, stochastic)
    saved = list(range(0, n_steps + 1, save_every))
    if points is not None:                                  # the points, their channels, a bilinear point outside the source rows, the host limit
        from . import points as pointing
        pts = pointing.Points(points)
        picked, raw, der = pointing._sources(names, derived, point_channels if point_channels is not None else (list(channels) if channels else None))
        for nm, ch in ((names, raw), (list(derived or []), der)):
            if ch:
                pointing.check_request(nm, model.grid.lat, model.grid.lon, n_members, pts, ch, point_method, len(saved))
        pointing.host_limit(n_members, len(saved), len(picked), len(pts))
        for g in (aplan.groups if aplan is not None else []):
            pointing.check_request(g.fields, model.grid.lat, model.grid.lon, n_members, pts, None, point_method, max(g.n_windows, 1))
    if scenarios is not None:                               # raw channels of the model's grid only; names of other products are refused by name
        from . import scenarios as scen
        other = list(derived or []) + ([f for g in aplan.groups for f in g.fields] if aplan is not None else [])
        req = scen.check_request(names, model.grid.lat, model.grid.lon, n_members, scenarios, scores, other)
        if req["normalise"] == "std":
            channel_std(model)                              # NotImplementedError for a model without per-channel sigmas
    if spectra is not None:                                 # raw channels and derived fields of the model's grid; aggregates are refused by name
        from . import spectra as spec
        other = [f for g in aplan.groups for f in g.fields] if aplan is not None else []
        spec.check_request(names + list(derived or []), model.grid.lat, model.grid.lon, n_members, spectra, other)
    if objects is not None:                                 # planes, members, the grid's axes; raw channels and derived fields of the model's grid
        from . import objects as objecting
        objecting.check_request(names, model.grid.lat, model.grid.lon, n_members, objects, list(derived or []))
    if keep_members not in (False, True, "regridded") or (keep_members == "regridded" and grid is None):
        raise ValueError('keep_members is False, True or, with grid=, "regridded" (only the regridded members are kept)')
    if keep_members:
        planes = len(saved) * (len(names) + len(derived or [])) + (0 if aplan is None else sum(g.n_windows * len(g.fields) for g in aplan.groups))
        need = 0 if keep_members == "regridded" else int(n_members) * planes * len(model.grid.lat) * len(model.grid.lon) * 4
        if tabs is not None:                                # the regridded members are checked at the size they have
            need += int(n_members) * len(saved) * len(names) * tabs.lat.size * tabs.lon.size * 4
        if need > _PINNED_LIMIT:
            raise ValueError(f"keep_members=True would hold {need / 2 ** 30:.1f} GiB of member states on the host (limit "
                             f"{_PINNED_LIMIT / 2 ** 30:.0f} GiB): fewer members, fewer steps or a larger save_every")
    return (products, {k: [float(np.float32(v)) for v in vs] for k, vs in (exceed or {}).items()},
            {k: [float(v) for v in vs] for k, vs in (quantiles or {}).items()}, saved)


def event_request(events, neighbourhoods_km, exceed, known, n_members, scores) -> tuple[dict, list]:
    """({channel: [thresholds]}, [radii in km]) of ``ensemble_forecast(events=, neighbourhoods_km=)``; ``events=True`` means the
    thresholds of ``exceed``.  Events are verified against a truth, so they need ``scores=True``."""
    from . import events as eventing
    if not scores:
        raise ValueError("events= verifies the exceedance events against a truth: it needs scores=True")
    if events is True:
        if not exceed:
            raise ValueError("events=True means the thresholds of exceed=, which is empty")
        events = dict(exceed)
    return eventing.check_request(known, events, neighbourhoods_km, n_members, "an output channel of this model or one of the derived fields")


def run(gm, start_time: datetime.datetime, n_steps: int = 4, n_members: int = 10, perturb_scale: float = 1e-3, seed: int = 0,
        products=("mean", "spread"), exceed=None, quantiles=None, channels=None, save_every: int = 1, keep_members: bool = False,
        save: bool = False, save_config: dict | None = None, truth=None, climatology=None, scores: bool = False,
        tracks: bool = False, track_config=None, events=None, neighbourhoods_km=(), points=None, point_channels=None,
        point_method: str = "bilinear", scenarios=None, spectra=None, objects=None, breeding=None, stochastic=None, aggregates=None, derived_surface=None,
        derived=None, grid=None, regrid_method: str = "conservative", perturbation: str = "white", length_scale_km: float = 500.0, alpha: float = 2.0, lmax: int | None = None,
        perturb_channels=None) -> EnsembleForecast:
    """``GlobalModel.ensemble_forecast`` (core/models/base.py has the user-facing description)."""
    from . import noise
    from .common import save_config_with_id
    from .datasource import get_initial_condition_for_model
    from .leads import forget_resident
    model = gm.model
    products, exceed, quantiles, saved = validate(model, n_steps, n_members, seed, products, exceed, quantiles, channels, save_every,
                                                  keep_members, events=events, neighbourhoods_km=neighbourhoods_km, scores=scores, points=points,
                                                  point_channels=point_channels, point_method=point_method, scenarios=scenarios, spectra=spectra,
                                                  breeding=breeding, stochastic=stochastic, aggregates=aggregates, derived_surface=derived_surface,
                                                  derived=derived, grid=grid, regrid_method=regrid_method, perturbation=perturbation,
                                                  length_scale_km=length_scale_km, alpha=alpha, lmax=lmax, perturb_channels=perturb_channels,
                                                  objects=objects)
    keep_regridded, keep_members = bool(keep_members) and grid is not None, bool(keep_members) and keep_members != "regridded"
    plan = noise.plan(model, perturbation, length_scale_km, alpha, lmax, perturb_channels)
    bplan = None
    if breeding is not None:
        from . import breeding as breed
        bplan = breed.plan(model, breeding)
    splan = None
    if stochastic is not None:
        from . import stochastic as stoch
        splan = stoch.plan(model, stochastic, perturb_scale)
    M = int(n_members)
    names = list(model.out_channel_names)
    n_lat, n_lon = len(model.grid.lat), len(model.grid.lon)
    scorer = None
    ev = d_ev = {}                                         # keyword arguments of the raw / regridded and of the derived scorer
    aggregator, a_events, a_radii = None, {}, []
    if aggregates is not None:                             # time-window aggregates (skyrim_amd/aggregate.py): names of aggregates in
        from . import aggregate                            # ``exceed``, ``quantiles`` and ``events`` go to their window group
        aggregator = aggregate.LeadAggregator(names, model.grid.lat, model.grid.lon, M, aggregates, start_time, model.time_step,
                                              device=model.device, n_steps=n_steps, derived=list(derived or []))
        a_fields = [f for g in aggregator.plan.groups for f in g.fields]
        (a_exceed, exceed), (a_quant, quantiles) = split_table(exceed, a_fields), split_table(quantiles, a_fields)
    if events is not None:                                 # names of derived fields go to the derived scorer, as those of ``exceed`` do
        known = names + list(derived or []) + (a_fields if aggregator is not None else [])
        events, radii = event_request(events, neighbourhoods_km, dict(exceed, **a_exceed) if aggregator is not None else exceed, known, M, scores)
        if aggregator is not None:
            (a_events, events), a_radii = split_table(events, a_fields), radii
        raw, der = split_table(events, names)
        ev = dict(events=raw, neighbourhoods_km=radii) if raw else {}
        d_ev = dict(events=der, neighbourhoods_km=radii) if der else {}
    if scores:                                             # (refusals of the request come before anything touches the device)
        from . import verify
        scorer = verify.LeadScorer(gm.model_name, names, model.grid.lat, model.grid.lon, M, verify.default_truth(gm) if truth is None else truth,
                                   climatology, channels, device=model.device, **ev)
        if scenarios is not None:                          # the truth is a column of the Gram matrix: it must hold the scenario channels
            from . import scenarios as scen
            scen.check_scored(scenarios.get("channels") or [], scorer.scored)
        if spectra is not None:                            # truth, error_mean and error_member need the truth of every spectrum channel
            from . import spectra as spec
            spec.check_scored([c for c in spectra.get("channels") or [] if c in names], scorer.scored)
    tracker = None
    if tracks:
        from . import tracks as tracking
        tracker = tracking.LeadTracker(gm.model_name, names, model.grid.lat, model.grid.lon, M, track_config, device=model.device)
    deriver = dscorer = adapt = None
    if derived is not None:                                # derived fields (skyrim_amd/derived.py): their own products, labelled with their names
        from . import derived as deriving
        dnames = list(derived)
        deriver = deriving.LeadDeriver(names, model.grid.lat, model.grid.lon, M, dnames, device=model.device, surface=derived_surface)
        # what every truth of these fields shares with the forecast: its thermodynamic columns, its kind of humidity and its surface mask
        thermal = dict(column=deriver.plan.column or None, moisture=deriver.plan.moisture, surface=derived_surface)
        (d_exceed, exceed), (d_quant, quantiles) = split_table(exceed, dnames), split_table(quantiles, dnames)
        if scores:
            adapt = deriving.TruthDeriver(dnames, model.grid.lat, model.grid.lon, device=model.device, levels=deriver.plan.levels or None,
                                          **thermal)
            dscorer = verify.LeadScorer(gm.model_name, dnames, model.grid.lat, model.grid.lon, M, scorer.truth.src, climatology, None,
                                        device=model.device, adapt=adapt, **d_ev)
            if spectra is not None:
                spec.check_scored([c for c in spectra.get("channels") or [] if c in dnames], dscorer.scored)
    ascorers = {}
    if aggregator is not None and scores:                  # one scorer per window group, against the same aggregates of the truth
        for g in aggregator.plan.groups:
            inner = None if derived is None else deriving.TruthDeriver(dnames, model.grid.lat, model.grid.lon, device=model.device,
                                                                       levels=deriver.plan.levels or None, **thermal)
            hook = aggregate.TruthAggregator(g.requests, model.grid.lat, model.grid.lon, start_time, model.time_step, device=model.device,
                                             inner=inner)
            g_ev = split_table(a_events, g.fields)[0]
            ascorers[g.label] = (hook, verify.LeadScorer(gm.model_name, g.fields, model.grid.lat, model.grid.lon, M, scorer.truth.src, climatology,
                                                         None, device=model.device, adapt=hook,
                                                         **(dict(events=g_ev, neighbourhoods_km=a_radii) if g_ev else {})))
    regridder = rscorer = None
    if grid is not None:                                   # the same products on the target grid (skyrim_amd/regrid.py)
        from . import regrid
        regridder = regrid.LeadRegridder(names, model.grid.lat, model.grid.lon, M, grid, regrid_method, device=model.device)
        grid_label = regrid.grid_label(grid)
        if scores:
            rscorer = verify.LeadScorer(gm.model_name, names, regridder.lat_out, regridder.lon_out, M, scorer.truth.src, climatology, channels,
                                        device=model.device,
                                        adapt=regrid.TruthRegridder(model.grid.lat, model.grid.lon, grid, regrid_method, device=model.device),
                                        **ev)
    pointer, apointers = None, {}
    if points is not None:                                 # every member at the points (skyrim_amd/points.py): raw channels and derived fields
        from . import points as pointing                   # at each saved lead time, each aggregate group when a window closes
        pts = pointing.Points(points)
        pointer = pointing.LeadPoints(names, model.grid.lat, model.grid.lon, M, pts, point_channels if point_channels is not None else
                                      (list(channels) if channels else None), point_method, model.device, list(derived or []), len(saved))
        if aggregator is not None:
            apointers = {g.label: pointing.LeadPoints(g.fields, model.grid.lat, model.grid.lon, M, pts, None, point_method, model.device, (),
                                                      max(g.n_windows, 1)) for g in aggregator.plan.groups}
    scenarist = None
    if scenarios is not None:                              # clusters, EOFs and the energy score of the members (skyrim_amd/scenarios.py)
        from . import scenarios as scen
        sigma = None
        if scenarios.get("normalise") == "std":
            sigma = scenario_std(model, names)
        scenarist = scen.LeadScenarios(names, model.grid.lat, model.grid.lon, M, scenarios, device=model.device, truth=scorer is not None,
                                       std=sigma)
    spectrist = dspectrist = None
    if spectra is not None:                                # zonal power spectra of members, mean, spread and errors (skyrim_amd/spectra.py):
        from . import spectra as spec                      # raw channels from the states, derived fields from the deriver's buffer
        raw, der = ([c for c in spectra["channels"] if (c in names) == own] for own in (True, False))
        if raw:
            spectrist = spec.LeadSpectra(names, model.grid.lat, model.grid.lon, M, dict(spectra, channels=raw), device=model.device,
                                         truth=scorer is not None)
        if der:
            dspectrist = spec.LeadSpectra(dnames, model.grid.lat, model.grid.lon, M, dict(spectra, channels=der), device=model.device,
                                          truth=dscorer is not None)
    objecter = None
    if objects is not None:                                # labelled threshold regions of every member (skyrim_amd/objects.py): raw channels
        from . import objects as objecting                 # from the states, derived fields from the deriver's buffer
        objecter = objecting.LeadObjects(names, model.grid.lat, model.grid.lon, M, objects, model.device, list(derived or []),
                                         model_name=gm.model_name)
    hw = n_lat * n_lon
    x0 = get_initial_condition_for_model(model, gm.data_source, start_time).to(model.device, torch.float32).contiguous()
    dev = x0.device
    if dev.type != "cuda":
        raise RuntimeError("ensemble_forecast makes and reduces its members with HIP kernels: the model must be on a GPU")
    forget_resident(model, closed=False)                   # the interleaved loops below are not a state a later rollout continues from
    std = channel_std(model)
    if std.numel() != x0.shape[2]:
        raise ValueError(f"channel_std holds {std.numel()} values for {x0.shape[2]} input channels")
    cfg = save_config_with_id(save_config)
    fid = cfg["forecast_id"]

    sigma_all = std                                        # (breeding normalises with every channel's own sigma)
    if plan.channel_mask is not None and plan.kind == "white":
        std = torch.where(torch.from_numpy(plan.channel_mask).to(dev), std, torch.zeros_like(std))        # amplitude exactly 0 elsewhere
    spherical = noise.Perturber(plan, x0, std, float(perturb_scale), int(seed)) if plan.kind == "spherical" else None

    def seed_member(m, xm):
        if spherical is not None:
            spherical.member(m, xm)
        else:
            perturb(x0, std, xm, hw, float(perturb_scale), int(seed), m)

    breeder = None
    if bplan is not None:                                  # the seeds bred through the model (skyrim_amd/breeding.py): they replace the seeds
        breeder = breed.Breeder(model, bplan, x0, sigma_all, float(perturb_scale), int(seed), start_time, seed_member, mask=plan.channel_mask)
        breeder.run(M)
        forget_resident(model, closed=False)
    loops, current, stepper = [], [], None
    if splan is not None:                                  # per-step perturbations (skyrim_amd/stochastic.py): the members are held as states,
        from .breeding import step_once                    # each lead is the model's own lead 1 from the perturbed state before it
        stepper = stoch.Stepper(splan, dev, x0.shape[2:], sigma_all, M, int(seed), float(perturb_scale))
    for m in range(M):
        if breeder is not None:
            xm = breeder.member(m)
        else:
            xm = torch.empty_like(x0)
            seed_member(m, xm)
        if stepper is not None:
            current.append(xm)
        else:
            loops.append(model(start_time, xm))
        del xm
    breeding_growth = None if breeder is None else breeder.growth
    del x0, spherical, breeder, sigma_all                  # (with them the work buffers of one member's synthesis and of the cycle)
    times, paths, source = [], [], gm.source_label
    lat, lon, n_saved = model.grid.lat, model.grid.lon, len(saved)
    family = functools.partial(ProductSet, gm.model_name, M, products, dev)
    raw_set = family(names, lat, lon, n_saved, exceed, quantiles, keep_members, always=("mean",))
    derived_set = regrid_set = None
    agg_sets = {}                                          # {window label: (its set, the ends of its closed windows, their starts)}
    if deriver is not None:
        derived_set = family(dnames, lat, lon, n_saved, d_exceed, d_quant, keep_members, "derived-")
    if aggregator is not None:                             # per window group: one entry per complete window
        for g in aggregator.plan.groups:
            own = [split_table(t, g.fields)[0] for t in (a_exceed, a_quant)]
            agg_sets[g.label] = (family(g.fields, lat, lon, g.n_windows, *own, keep_members, f"agg{g.label}-"), [], [])
        agg_derived = any(r.channel in (derived or []) for r in aggregator.plan.requests)
    if regridder is not None:
        regrid_set = family(names, regridder.lat_out, regridder.lon_out, n_saved, exceed, quantiles, keep_regridded, "regrid-")
    try:
        for k in range(n_steps + 1):
            states, time = [], None
            for m, loop in enumerate(loops):
                try:
                    time, out, _ = next(loop)
                except FloatingPointError as e:
                    raise FloatingPointError(f"ensemble member {m}, step {k}: {e}") from e
                states.append((out[0] if out.dim() == 4 else out).contiguous())
            if stepper is not None:
                time = start_time + k * model.time_step
                for m in range(M):
                    if k >= 1:
                        xp = current[m]
                        xn = step_once(model, time - model.time_step, xp, f"ensemble member {m}, step {k}")
                        stepper.advance(k, m, xp[0, 0], xn)           # in place on xn; member 0 is left as the model made it
                        current[m] = xn.reshape(xp.shape)
                        del xp, xn
                    states.append(current[m][0, 0])
            table = member_table(states)
            keep = k in saved
            s = saved.index(k) if keep else None
            raw_set.reduce(states, table, s)               # every step: a non-finite member makes the mean non-finite, one flag to read
            if not bool(torch.isfinite(raw_set.dev["mean"]).all().item()):
                bad = [m for m, st in enumerate(states) if not bool(torch.isfinite(st).all().item())]
                raise FloatingPointError(f"non-finite values in ensemble member(s) {bad} after step {k}")
            if keep:
                times.append(time)
            if scorer is not None:
                scorer.add(time, states, table)            # the same states and table: one more read of the members, one of the truth
            if tracker is not None:
                tracker.add(time, states, table)           # cyclone candidates of this lead time: only their records leave the device
            fold_derived = aggregator is not None and agg_derived and k >= 1
            if deriver is not None and (keep or dscorer is not None or fold_derived):      # (``objecter`` reads the derived planes of saved leads)
                dstates, dtable = deriver.add(states, table)      # ONE launch: D derived planes per member, read below like raw channels
                if dscorer is not None:
                    dscorer.add(time, dstates, dtable)
                if dspectrist is not None and keep:        # the derived planes are (D, H, W) states with a member table of their own
                    dspectrist.add(time, dstates, dtable, dscorer.truth_state() if dscorer is not None else None)
                if keep:
                    derived_set.reduce(dstates, dtable, s)
            if scenarist is not None and keep:             # one Gram launch, its M' x M' doubles to the host, cluster means, EOF patterns
                scenarist.add(time, states, table, scorer.truth_state() if scorer is not None else None)
            if spectrist is not None and keep:             # one launch, nc x nb x kinds x K doubles to the host
                spectrist.add(time, states, table, scorer.truth_state() if scorer is not None else None)
            if objecter is not None and keep:              # label, attributes, probability: records and count planes leave the device
                objecter.add(time, states, table, (dstates, dtable) if objecter.needs_derived else None,
                             scorer.truth_state() if scorer is not None else None,
                             dscorer.truth_state() if dscorer is not None else None,
                             None if scorer is None else list(scorer.scored) + (list(dscorer.scored) if dscorer is not None else []))
            if pointer is not None and keep:               # the members where they lie: one launch per source buffer, only the values leave
                pointer.add(time, states, table, (dstates, dtable) if pointer.needs_derived else None)
            if aggregator is not None and k >= 1:          # (step 0, the initial state, belongs to no window)
                for c in aggregator.add(k, time, states, table, (dstates, dtable) if fold_derived else None):
                    agg_set, ends, starts = agg_sets[c.label]
                    ends.append(c.end)                     # windows close independently of ``save_every``
                    starts.append(c.start)
                    agg_set.reduce(c.states, c.table, c.window)
                    if c.label in apointers:
                        apointers[c.label].add(c.end, c.states, c.table)
                    if c.label in ascorers:
                        hook, asc = ascorers[c.label]
                        hook.window(c.times)               # the truth is aggregated over the same valid times
                        asc.add(c.end, c.states, c.table)
                    if save:                               # one file per closed window, without the ``window_start`` coordinate
                        paths += agg_set.save(c.window, [c.end], c.start, gm.source_label, cfg)
            if regridder is not None and (keep or rscorer is not None):
                rstates, rtable = regridder.add(states, table)    # ONE launch: every channel of every member on the target grid
                if rscorer is not None:
                    rscorer.add(time, rstates, rtable)
                if keep:
                    regrid_set.reduce(rstates, rtable, s)
            if keep and save and s >= 1:                   # files of two entries: the step saved before and this one
                for family_set in (raw_set, derived_set, regrid_set):
                    if family_set is not None:
                        paths += family_set.save(s - 1, times[s - 1:s + 1], times[s - 1], source, cfg)
                source = "file"
            del states, table
    finally:
        for loop in loops:
            try:
                loop.close()
            except FloatingPointError:
                pass                                       # every delivered step was checked above, by member
        forget_resident(model)

    ens = EnsembleForecast(gm.model_name, M, int(seed), float(perturb_scale), paths=paths, forecast_id=fid, perturbation=plan.kind,
                           length_scale_km=float(length_scale_km), alpha=float(alpha), lmax=plan.lmax if plan.kind == "spherical" else None,
                           breeding=None if bplan is None else bplan.as_dict(), breeding_growth=breeding_growth,
                           stochastic=None if splan is None else splan.as_dict())
    if scorer is not None:
        ens.scores = _stamped(scorer, fid)
        if save:
            _save_result(ens.scores, cfg, paths)
    if tracker is not None:
        ens.tracks = _stamped(tracker, fid)
        if save:
            _save_result(ens.tracks, cfg, paths)
    raw_set.fill(ens, times, channels)
    if deriver is not None:
        ens.derived = deriving.DerivedProducts(dnames)
        derived_set.fill(ens.derived, times)
        if dscorer is not None:
            ens.derived.scores = _stamped(dscorer, fid)
            ens.derived.dropped = dict(adapt.dropped)
    if regridder is not None:
        ens.regridded = regrid.RegriddedProducts(regridder.lat_out, regridder.lon_out, regrid_method)
        regrid_set.fill(ens.regridded, times, channels)
        if rscorer is not None:
            ens.regridded.scores = _stamped(rscorer, fid)
            ens.regridded.scores.grid = grid_label
    if aggregator is not None:
        for g in aggregator.plan.groups:
            agg_set, ends, starts = agg_sets[g.label]
            prod = aggregate.AggregatedProducts(g.label, list(g.fields))
            agg_set.fill(prod, ends, window_start=starts)
            prod.incomplete = aggregator.incomplete.get(g.label)
            if g.label in apointers:
                prod.points = apointers[g.label].result(f"{gm.model_name}-ens{M}-agg{g.label}", fid, window_start=starts)
            if g.label in ascorers:
                hook, asc = ascorers[g.label]
                prod.scores = _stamped(asc, fid)
                prod.dropped = dict(hook.dropped)
            ens.aggregated[g.label] = prod
    if scenarist is not None:
        ens.scenarios = scenarist.result(f"{gm.model_name}-ens{M}", fid)
    if spectrist is not None or dspectrist is not None:
        parts = [s.result(f"{gm.model_name}-ens{M}", fid) for s in (spectrist, dspectrist) if s is not None]
        ens.spectra = spec.merge(parts, spectra["channels"])
    if objecter is not None:
        ens.objects = _stamped(objecter, fid)
        if save:
            _save_result(ens.objects, cfg, paths)
    if pointer is not None:
        ens.points = pointer.result(f"{gm.model_name}-ens{M}", fid)
        if save:
            _save_result(ens.points, cfg, paths)
    return ens
