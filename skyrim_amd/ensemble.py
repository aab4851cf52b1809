"""Perturbed-initial-condition ensembles of ONE model (include/skyrim_ens.h).

Four layers:

* the binding of libskyrim_ens.so (``SPEC``, ``load_library``, ``perturb``, ``stats``, ``member_table``); the same calls are
  ``torch.ops.skyrim_hip.ens_perturb / ens_stats`` (skyrim_amd/ops.py);
* ``ProductSet`` -- the products of one family of fields (raw, derived, regridded, one window group of aggregates): their buffers,
  the ``stats`` launches and copies of an entry, its files, its labelled arrays;
* ``run`` -- what ``GlobalModel.ensemble_forecast`` does.  ``plan_request``: the refusals that need no device, the request normalised
  once.  ``seed_members``: the initial condition once, M members from ``ens_perturb`` (white noise) or ``noise.Perturber``
  (``perturbation="spherical"``, skyrim_amd/noise.py), with ``breeding=`` bred from those seeds through the model itself
  (skyrim_amd/breeding.py).  ``Members``: ONE TimeLoop generator per member advanced step-major (all members one step, then that lead
  time's statistics), so only the members' current states are alive on the GPU; with ``stochastic=`` the members are held as states
  and every step of every member but the control is perturbed (skyrim_amd/stochastic.py).  ``stages``: what a lead time sets off;
  ``drive``: the leads of any member source with ``advance(k)`` and ``close()`` -- ``Members``, or the files of a forecast that was
  written down (``archive.ArchiveMembers``, skyrim_amd/archive.py);
* ``EnsembleForecast`` -- the labelled products, and their files in the layout of every other forecast of this package.

Members sharded over ranks stay with ``skyrim_amd/pangu/ensemble.py``; multi-MODEL ensembles are ``core/models/ensemble.py``.
"""
from __future__ import annotations

import collections
import ctypes
import datetime
import functools
import math
from dataclasses import dataclass, field, make_dataclass
from types import SimpleNamespace

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


def _per_family(table, fields_of) -> dict:
    """``{family: its entries of table}`` for the ``{family: fields}`` of ``fields_of``; ``"raw"`` takes what none of them names."""
    out = {}
    for fam, fields in fields_of.items():
        out[fam], table = split_table(table, fields)
    return dict(out, raw=table)


def _hang(res, fid, sink=None):
    """``res`` with the forecast id on it; a ``sink`` = (save config, paths): written under the forecast's output directory, its path noted."""
    res.forecast_id = fid
    if sink is not None:
        from .common import OUTPUT_DIR
        sink[1].append(res.save(sink[0].get("output_dir") or OUTPUT_DIR))
    return res


def _put(obj, name, value):
    setattr(obj, name, value)
    return value


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
    neighbourhood: object = None # neighbourhood.NeighbourhoodProducts with ``neighbourhood=[...]``
    points: object = None        # points.PointForecast with ``points=...``
    scenarios: object = None     # scenarios.Scenarios with ``scenarios={...}``
    spectra: object = None       # spectra.Spectra with ``spectra={...}``
    breeding: object = None      # the normalised ``breeding=`` request (cycles, norm, paired) or None
    breeding_growth: object = None      # (cycles, member, channel) float64 with ``breeding=``: breeding.Breeder.growth
    stochastic: object = None    # the normalised ``stochastic=`` request (stochastic.Plan.as_dict) or None
    objects: object = None       # objects.Objects with ``objects={...}``
    extremes: object = None      # extremes.Extremes with ``extremes={...}``: raw channels and derived fields at the saved leads
    archive: object = None       # archive.MemberArchive with ``archive={...}``: the members themselves, one file per (member, saved lead)


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


# ---- the request --------------------------------------------------------------------------------------------------------------------- #
# A checked ``ensemble_forecast`` request (``plan_request``): everything ``run`` needs from it that the host can decide.  ``asked``: the
# keywords as given, by name -- what a ``Lead*`` object normalises itself reaches it as it came; ``saved``: the saved step numbers;
# ``names`` / ``derived``: the model's output channels and the derived fields ([]: none); ``exceed`` / ``quantiles`` / ``events``:
# ``{family: {field: values}}`` with the families ``"raw"`` (the regridded channels share it), ``"derived"`` and ``"agg{label}"`` per window
# group and ``"nbr"`` (the neighbourhood fields); ``radii``: the events' neighbourhoods, km; ``keep_members``: the raw, derived and aggregated ones; ``noise`` / ``breeding`` /
# ``stochastic`` / ``aggregate``: the plans of those modules, or None; ``regrid``: ``regrid.Tables`` or None; ``points``: ``points.Points`` or
# None; ``point_channels``: what is sampled there (``point_channels``, else ``channels``, else None = every raw channel); ``extremes``: the
# checked ``extremes.Request`` or None; ``archive``: the checked ``archive=`` request (``archive.check_request``) or None; ``neighbourhood``:
# ``neighbourhood.Plan`` or None -- its fields are the family ``"nbr"``.
Plan = make_dataclass("Plan", "asked M products saved names derived exceed quantiles events radii keep_members keep_regridded noise breeding "
                      "stochastic aggregate regrid points point_channels extremes archive neighbourhood".split())


def plan_request(model, n_steps, n_members, seed, products, exceed, quantiles, channels, save_every, keep_members, events=None,
                 neighbourhoods_km=(), scores=False, points=None, point_channels=None, point_method="bilinear", scenarios=None, spectra=None, objects=None,
                 extremes=None, archive=None, save=False, breeding=None, stochastic=None, aggregates=None, neighbourhood=None, vertical=None, derived_surface=None, derived=None, grid=None,
                 regrid_method="conservative", perturbation="white", length_scale_km=500.0, alpha=2.0, lmax=None, perturb_channels=None,
                 perturb_scale=None) -> Plan:
    """Every refusal that needs no device, in one fixed order, and the request normalised once: the ``Plan``.  The keywords are those of
    ``GlobalModel.ensemble_forecast`` (core/models/base.py describes them).  ``exceed`` and ``quantiles`` may name raw channels, fields
    of ``derived`` and aggregates (``ws10m_max_24h``), ``events`` too; ``scenarios`` takes raw channels, ``spectra`` and ``objects`` raw
    channels and derived fields, all on the model's own grid.  ``perturb_scale``: the default of ``stochastic``'s ``additive_scale``,
    which ``run`` passes and ``validate`` has not."""
    asked = SimpleNamespace(**locals())
    from . import aggregate, archive as archiving, breeding as breed, derived as deriving, extremes as extreming, noise, objects as objecting
    from . import neighbourhood as nbr, points as pointing, regrid, scenarios as scen, spectra as spec, stochastic as stoch
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
    names, dnames = list(model.out_channel_names), list(derived or [])
    if derived is not None:
        deriving.check_request(names, dnames, model.grid.lat, model.grid.lon, n_members, surface=derived_surface is not None, vertical=vertical)
    known = names + dnames
    aplan, groups = None, []
    n_asked = [nbr.parse_request(r).name for r in neighbourhood] if isinstance(neighbourhood, (list, tuple)) else []
    if n_asked:                                             # neighbourhood fields feed the statistics, the scorer, the events and the points, no other product
        for what, req in (("aggregates", [getattr(r, "channel", str(r).split(":")[0].strip()) for r in aggregates or []]), ("extremes", extremes),
                          ("objects", objects), ("spectra", spectra), ("scenarios", scenarios)):
            asked_there = list(req) if isinstance(req, (dict, list, tuple)) else []
            if isinstance(req, dict):
                asked_there += [c for k in ("channels", "fields") if isinstance(req.get(k), (list, tuple)) for c in req[k]]
            named = [f for f in n_asked if f in asked_there]
            if named:
                raise ValueError(f"{what}: {named} are neighbourhood fields; neighbourhood fields as input to {what}= are out of scope "
                                 "(DESIGN.md 35)")
    if aggregates is not None:
        aplan = aggregate.check_request(known, aggregates, model.time_step, n_steps, model.grid.lat, model.grid.lon, n_members)
        groups = aplan.groups
        clash = [f for g in groups for f in g.fields if f in known]
        if clash:
            raise ValueError(f"aggregates: {clash} are already channels of this forecast")
        known = known + [f for g in groups for f in g.fields]
    nbplan = None
    if neighbourhood is not None:
        if grid is not None:
            raise ValueError("neighbourhood= together with grid= is not supported: neighbourhood fields are made on the model's own global "
                             "grid only (DESIGN.md 35, out of scope)")
        nbplan = nbr.check_request(names, neighbourhood, model.grid.lat, model.grid.lon, n_members, dnames, [f for g in groups for f in g.fields])
        known = known + nbplan.fields
    n_fields = nbplan.fields if nbplan is not None else []
    tabs = None
    if grid is not None:
        if derived is not None:
            raise ValueError("grid= together with derived= is not supported: derived fields are made on the model's own grid only "
                             "(DESIGN.md 22, out of scope)")
        tabs = regrid.check_request(names, model.grid.lat, model.grid.lon, n_members, grid, regrid_method)
    for what, table, cap in (("exceed", exceed, MAX_THRESHOLDS), ("quantiles", quantiles, MAX_QUANTILES)):
        for ch, vals in (table or {}).items():
            if ch not in known:
                raise ValueError(f"{what}: channel {ch!r} is not an output channel of this model"
                                 + ("" if derived is None else " or one of the derived fields")
                                 + ("" if aplan is None else " or one of the aggregates")
                                 + ("" if nbplan is None else " or one of the neighbourhood fields"))
            if not 1 <= len(vals) <= cap:
                raise ValueError(f"{what}[{ch!r}]: 1 to {cap} values per channel, got {len(vals)}")
    for ch, vals in (quantiles or {}).items():
        for q in vals:
            quantile_position(q, int(n_members))
    # (``event_request`` rounds the thresholds of ``exceed`` to fp32 itself)
    ev, radii = event_request(events, neighbourhoods_km, exceed, known, n_members, scores) if events is not None else ({}, [])
    missing = [c for c in (channels or []) if c not in names]
    if missing:
        raise ValueError(f"channels {missing} are not output channels of this model")
    nplan = noise.plan(model, perturbation, length_scale_km, alpha, lmax, perturb_channels)      # kind, length scale, lmax, grid, channels
    bplan = breed.plan(model, breeding)                     # cycles, norm, keys; one history level, the same channels in and out
    splan = stoch.plan(model, stochastic, perturb_scale)    # kind, amplitudes, the pattern's spectrum and grid, a model that steps from one state
    saved = list(range(0, n_steps + 1, save_every))
    pts = None
    point_channels = point_channels if point_channels is not None else (list(channels) if channels else None)
    if points is not None:                                  # the points, their channels, a bilinear point outside the source rows, the host limit
        pts = pointing.Points(points)
        picked, raw, der = pointing._sources(names, derived, point_channels)
        for nm, ch in ((names, raw), (dnames, der)):
            if ch:
                pointing.check_request(nm, model.grid.lat, model.grid.lon, n_members, pts, ch, point_method, len(saved))
        pointing.host_limit(n_members, len(saved), len(picked), len(pts))
        for g in groups:
            pointing.check_request(g.fields, model.grid.lat, model.grid.lon, n_members, pts, None, point_method, max(g.n_windows, 1))
        if n_fields:
            pointing.check_request(n_fields, model.grid.lat, model.grid.lon, n_members, pts, None, point_method, len(saved))
    a_fields = [f for g in groups for f in g.fields]
    if scenarios is not None:                               # raw channels of the model's grid only; names of other products are refused by name
        if scen.check_request(names, model.grid.lat, model.grid.lon, n_members, scenarios, scores, dnames + a_fields)["normalise"] == "std":
            channel_std(model)                              # NotImplementedError for a model without per-channel sigmas
    if spectra is not None:                                 # raw channels and derived fields of the model's grid; aggregates are refused by name
        spec.check_request(names + dnames, model.grid.lat, model.grid.lon, n_members, spectra, a_fields)
    if objects is not None:                                 # planes, members, the grid's axes; raw channels and derived fields of the model's grid
        objecting.check_request(names, model.grid.lat, model.grid.lon, n_members, objects, dnames)
    xreq = None
    if extremes is not None:                                # the climate, its fields and levels; raw channels, derived fields and aggregates of the model's grid
        xreq = extreming.check_request(names, model.grid.lat, model.grid.lon, n_members, extremes, dnames, a_fields)
    areq = archiving.check_request(names, archive, save) if archive is not None else None      # the packing, its channels, somewhere to write
    if keep_members not in (False, True, "regridded") or (keep_members == "regridded" and grid is None):
        raise ValueError('keep_members is False, True or, with grid=, "regridded" (only the regridded members are kept)')
    if keep_members:
        planes = len(saved) * (len(names) + len(dnames) + len(n_fields)) + sum(g.n_windows * len(g.fields) for g in groups)
        need = 0 if keep_members == "regridded" else int(n_members) * planes * len(model.grid.lat) * len(model.grid.lon) * 4
        if tabs is not None:                                # the regridded members are checked at the size they have
            need += int(n_members) * len(saved) * len(names) * tabs.lat.size * tabs.lon.size * 4
        if need > _PINNED_LIMIT:
            raise ValueError(f"keep_members=True would hold {need / 2 ** 30:.1f} GiB of member states on the host (limit "
                             f"{_PINNED_LIMIT / 2 ** 30:.0f} GiB): fewer members, fewer steps or a larger save_every -- or archive={{...}}, which writes "
                             "the members to files as they are made and replays them later (skyrim_amd/archive.py)")
    fields_of = dict({"derived": dnames} if dnames else {}, **{f"agg{g.label}": g.fields for g in groups}, **({"nbr": n_fields} if n_fields else {}))
    exceed = {k: [float(np.float32(v)) for v in vs] for k, vs in (exceed or {}).items()}
    quantiles = {k: [float(v) for v in vs] for k, vs in (quantiles or {}).items()}
    return Plan(asked, int(n_members), products, saved, names, dnames, _per_family(exceed, fields_of), _per_family(quantiles, fields_of),
                _per_family(ev, fields_of), radii, bool(keep_members) and keep_members != "regridded", bool(keep_members) and grid is not None,
                nplan, bplan, splan, aplan, tabs, pts, point_channels, xreq, areq, nbplan)


def validate(model, n_steps, n_members, seed, products, exceed, quantiles, channels, save_every, keep_members, events=None,
             neighbourhoods_km=(), scores=False, points=None, point_channels=None, point_method="bilinear", scenarios=None, spectra=None, objects=None, extremes=None, archive=None,
             save=False, breeding=None, stochastic=None, aggregates=None, neighbourhood=None, vertical=None, derived_surface=None, derived=None, grid=None, regrid_method="conservative", perturbation="white", length_scale_km=500.0, alpha=2.0, lmax=None,
             perturb_channels=None):
    """Every refusal that needs no device (``plan_request``); returns (products, exceed, quantiles, saved step numbers) normalised."""
    p = plan_request(**locals())
    return (p.products, *({k: v for part in t.values() for k, v in part.items()} for t in (p.exceed, p.quantiles)), p.saved)


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


# ---- the members --------------------------------------------------------------------------------------------------------------------- #
def seed_members(model, p: Plan, x0, std, perturb_scale, start_time) -> tuple[list, object]:
    """(the M member states seeded from the initial condition ``x0``, ``Breeder.growth`` or None): white noise (``perturb``) or spherical
    fields (``noise.Perturber``), with ``breeding=`` bred through the model (skyrim_amd/breeding.py).  ``std``: ``channel_std(model)``."""
    from . import breeding as breed, noise
    from .leads import forget_resident
    hw, seed, sigma_all = len(model.grid.lat) * len(model.grid.lon), int(p.asked.seed), std      # (breeding normalises with every channel's own sigma)
    if p.noise.channel_mask is not None and p.noise.kind == "white":
        std = torch.where(torch.from_numpy(p.noise.channel_mask).to(x0.device), std, torch.zeros_like(std))       # amplitude exactly 0 elsewhere
    spherical = noise.Perturber(p.noise, x0, std, perturb_scale, seed) if p.noise.kind == "spherical" else None

    def seed_member(m, xm):
        if spherical is not None:
            spherical.member(m, xm)
        else:
            perturb(x0, std, xm, hw, perturb_scale, seed, m)
    if p.breeding is not None:
        breeder = breed.Breeder(model, p.breeding, x0, sigma_all, perturb_scale, seed, start_time, seed_member, mask=p.noise.channel_mask)
        breeder.run(p.M)
        forget_resident(model, closed=False)
        return [breeder.member(m) for m in range(p.M)], breeder.growth
    states = [torch.empty_like(x0) for _ in range(p.M)]
    for m, xm in enumerate(states):
        seed_member(m, xm)
    return states, None


class Members:
    """The M members of one forecast behind ``advance(k) -> (valid time, their states (C, H, W) of lead k)``, the leads in order from 0.
    Without a ``stepper`` every member is its own TimeLoop generator ``model(start_time, x_m)`` and a lead is one ``next`` of each, in
    member order; with one (``stochastic.Stepper``) the members are held as states, and lead k >= 1 of a member is the model's own lead 1
    from its state before (``breeding.step_once``), perturbed in place by ``stepper.advance``.  Only the members' current states are kept."""

    def __init__(self, model, start_time, seeds, stepper=None):
        self.model, self.start_time, self.stepper = model, start_time, stepper
        self.loops = [model(start_time, x) for x in seeds] if stepper is None else []
        self.current = [] if stepper is None else list(seeds)

    def advance(self, k: int) -> tuple:
        if self.stepper is None:
            states = []
            for m, loop in enumerate(self.loops):
                try:
                    time, out, _ = next(loop)
                except FloatingPointError as e:
                    raise FloatingPointError(f"ensemble member {m}, step {k}: {e}") from e
                states.append((out[0] if out.dim() == 4 else out).contiguous())
            return time, states
        from .breeding import step_once
        time = self.start_time + k * self.model.time_step
        for m, xp in enumerate(self.current if k >= 1 else ()):
            xn = step_once(self.model, time - self.model.time_step, xp, f"ensemble member {m}, step {k}")
            self.stepper.advance(k, m, xp[0, 0], xn)       # in place on xn; member 0 is left as the model made it
            self.current[m] = xn.reshape(xp.shape)
        return time, [x[0, 0] for x in self.current]

    def close(self) -> None:
        """Close every generator, also after one of them raises: a ``FloatingPointError`` of a loop's own guard is dropped (every delivered
        step was checked, by member), the first other error is raised once all are closed."""
        first = None
        for loop in self.loops:
            try:
                loop.close()
            except FloatingPointError:
                pass
            except Exception as e:
                first = first or e
        if first is not None:
            raise first


# ---- families and stages ------------------------------------------------------------------------------------------------------------- #
class Family:
    """One family of fields in the driver: raw channels, derived fields, regridded channels or the aggregates of one window group.
    ``make()``: its ``ProductSet`` (``products``), made once the members are seeded; ``hang(ens)``: the object its results go on (``ens``,
    ``DerivedProducts``, ``RegriddedProducts``, ``AggregatedProducts``), put in its place; ``scorer``: its ``LeadScorer`` or None, the truth
    adapter in it; ``points``: a window group's ``LeadPoints``; ``select``: the channels to cut to; ``grid``: the target grid's label."""

    def __init__(self, make, hang, scorer=None, points=None, select=None, grid=None, windows=False):
        self.make, self.hang, self.scorer, self.points, self.select, self.grid = make, hang, scorer, points, select, grid
        self.extremes = None                                # a window group's ``LeadExtremes``
        self.products, self.times, self.starts = None, [], [] if windows else None

    def score(self, time, states, table, window=None):
        """The scores of this lead; returns the truth they were made against as a device state, None without scores.  ``window``: the
        valid times of the window that closes, which the truth is aggregated over."""
        if self.scorer is None:
            return None
        if window is not None:
            self.scorer.adapt.window(window)
        self.scorer.add(time, states, table)               # the same states and table: one more read of the members, one of the truth
        return self.scorer.truth_state()

    def reduce(self, time, states, table, slot, start=None) -> None:
        """Entry ``slot`` of the products (None: only what the set computes at every lead), then a window group's points."""
        if slot is not None:
            self.times.append(time)
            if start is not None:
                self.starts.append(start)
        self.products.reduce(states, table, slot)
        if self.points is not None:
            self.points.add(time, states, table)
        if self.extremes is not None and slot is not None:  # the slice of the climate is chosen by ``time``, a window's end
            self.extremes.add(time, states, table)

    def lead(self, time, states, table, slot):
        """What a lead time is to a family whose states are made for it: the scores, then the products."""
        self.score(time, states, table)
        self.reduce(time, states, table, slot)

    def fill(self, ens, fid, sink=None, xsink=None) -> None:
        """The labelled arrays, ``points``, ``scores``, the scores' ``grid`` and ``dropped`` on the family's object, where they apply."""
        target, ps = self.hang(ens), self.products
        ps.fill(target, self.times, self.select, window_start=self.starts)
        if self.points is not None:
            target.points = self.points.result(product_model_name(ps.model_name, ps.M, ps.prefix[:-1]), fid,
                                               **({} if self.starts is None else dict(window_start=self.starts)))
        if self.extremes is not None:
            target.extremes = _hang(self.extremes.result(product_model_name(ps.model_name, ps.M, ps.prefix[:-1]), fid, window_start=self.starts),
                                    fid, xsink)
        if self.scorer is not None:
            target.scores = _hang(self.scorer.result(), fid, sink)
            if self.grid is not None:
                target.scores.grid = self.grid
            if hasattr(self.scorer.adapt, "dropped"):
                target.dropped = dict(self.scorer.adapt.dropped)


_saved = lambda L: L.slot is not None                      # noqa: E731
Stage = collections.namedtuple("Stage", "add due finish close", defaults=(None, _saved, None, None))


def stages(gm, p: Plan, start_time, truth=None, climatology=None, scores=False, tracks=False, track_config=None) -> tuple[list, list]:
    """(the stages of a lead time, the families: raw, derived, regridded, neighbourhood, then the window groups).  THE place a product is wired in: its
    ``Lead*`` object is made here, in the order the refusals of these objects have, with the checks that need the truth, and it gets one
    ``Stage`` in the list at the end, whose order is the order of the launches of a lead (DESIGN.md 17 has the rules it keeps):
    ``add(L)`` is called where ``due(L)`` (default: at saved leads), ``finish(ens, fid, sink)`` once after the last lead, ``close()`` when
    the leads are over, also after an error (a stage with threads or files of its own).  ``L``, the record of
    a lead: ``k``, ``time``, ``slot`` (the entry of a saved lead, else None), ``states``, ``table``, ``sink`` (where files go) and, set by the
    stages before, ``truth`` (the raw scorer's truth state), ``derived`` = (states, table) of the deriver, ``dtruth``."""
    from . import aggregate, archive as archiving, derived as deriving, extremes as extreming, objects as objecting, points as pointing, regrid
    from . import neighbourhood as nbr
    from . import scenarios as scen
    from . import spectra as spec
    from . import tracks as tracking, verify
    model, a, M, names, dnames, dev, n_saved = gm.model, p.asked, p.M, p.names, p.derived, gm.model.device, len(p.saved)
    lat, lon, label = model.grid.lat, model.grid.lon, f"{gm.model_name}-ens{M}"
    groups = p.aggregate.groups if p.aggregate is not None else []
    wants = lambda asked, family: [c for c in asked.get("channels") or [] if (c in names) == (family == "raw")]      # noqa: E731

    def products(fields, la, lo, entries, family, keep, prefix="", always=()):
        return functools.partial(ProductSet, gm.model_name, M, p.products, dev, fields, la, lo, entries, p.exceed.get(family, {}),
                                 p.quantiles.get(family, {}), keep, prefix, always)

    def scorer(fields, la, lo, src, channels, family, adapt=None):
        ev = p.events.get(family)                          # names of derived fields and aggregates go to their family's scorer
        return verify.LeadScorer(gm.model_name, fields, la, lo, M, src, climatology, channels, device=dev, adapt=adapt,
                                 **(dict(events=ev, neighbourhoods_km=p.radii) if ev else {})) if scores else None
    aggregator = aggregate.LeadAggregator(names, lat, lon, M, p.aggregate.requests, start_time, model.time_step, device=dev,
                                          n_steps=a.n_steps, derived=dnames) if groups else None
    raw = Family(products(names, lat, lon, n_saved, "raw", p.keep_members, always=("mean",)), lambda ens: ens,
                 scorer(names, lat, lon, verify.default_truth(gm) if truth is None and scores else truth, a.channels, "raw"), select=a.channels)
    if scores:                                             # (refusals of the request come before anything touches the device)
        truth = raw.scorer.truth.src
        if a.scenarios is not None:                        # the truth is a column of the Gram matrix: it must hold the scenario channels
            scen.check_scored(a.scenarios.get("channels") or [], raw.scorer.scored)
        if a.spectra is not None:                          # truth, error_mean and error_member need the truth of every spectrum channel
            spec.check_scored(wants(a.spectra, "raw"), raw.scorer.scored)
    tracker = tracking.LeadTracker(gm.model_name, names, lat, lon, M, track_config, device=dev) if tracks else None
    deriver = derived = truth_deriver = None
    if dnames:                                             # derived fields (skyrim_amd/derived.py): their own products, labelled with their names
        deriver = deriving.LeadDeriver(names, lat, lon, M, dnames, device=dev, surface=a.derived_surface, vertical=a.vertical)
        # what every truth of these fields shares with the forecast: its levels, its thermodynamic columns, its kind of humidity, its surface mask
        truth_deriver = functools.partial(deriving.TruthDeriver, dnames, lat, lon, device=dev, levels=deriver.plan.levels or None,
                                          column=deriver.plan.column or None, moisture=deriver.plan.moisture, surface=a.derived_surface, vertical=a.vertical)
        derived = Family(products(dnames, lat, lon, n_saved, "derived", p.keep_members, "derived-"),
                         lambda ens: _put(ens, "derived", deriving.DerivedProducts(dnames)),
                         scorer(dnames, lat, lon, truth, None, "derived", truth_deriver() if scores else None))
        if scores and a.spectra is not None:
            spec.check_scored(wants(a.spectra, "derived"), derived.scorer.scored)
    windowed = {}                                          # per window group: one entry per complete window, scored against the same
    for g in groups:                                       # aggregates of the truth
        hook = aggregate.TruthAggregator(g.requests, lat, lon, start_time, model.time_step, device=dev,
                                         inner=truth_deriver and truth_deriver()) if scores else None
        windowed[g.label] = Family(products(g.fields, lat, lon, g.n_windows, f"agg{g.label}", p.keep_members, f"agg{g.label}-"),
                                   lambda ens, g=g: ens.aggregated.setdefault(g.label, aggregate.AggregatedProducts(
                                       g.label, list(g.fields), incomplete=p.aggregate.incomplete.get(g.label))),
                                   scorer(g.fields, lat, lon, truth, None, f"agg{g.label}", hook), windows=True)
    neighbour = neighbours = None
    if p.neighbourhood is not None:                        # neighbourhood fields (skyrim_amd/neighbourhood.py): their own products, read like raw channels
        nfields = p.neighbourhood.fields
        neighbour = nbr.LeadNeighbourhood(names, lat, lon, M, p.neighbourhood.requests, dev, dnames)
        hook = nbr.TruthNeighbourhood(p.neighbourhood.requests, lat, lon, dev, inner=truth_deriver and truth_deriver()) if scores else None
        neighbours = Family(products(nfields, lat, lon, n_saved, "nbr", p.keep_members, "nbr-"),
                            lambda ens: _put(ens, "neighbourhood", nbr.NeighbourhoodProducts(list(nfields))),
                            scorer(nfields, lat, lon, truth, None, "nbr", hook))
    regridder = regridded = None
    if a.grid is not None:                                 # the same products on the target grid (skyrim_amd/regrid.py)
        regridder = regrid.LeadRegridder(names, lat, lon, M, a.grid, a.regrid_method, device=dev)
        hook = regrid.TruthRegridder(lat, lon, a.grid, a.regrid_method, device=dev) if scores else None
        regridded = Family(products(names, regridder.lat_out, regridder.lon_out, n_saved, "raw", p.keep_regridded, "regrid-"),
                           lambda ens: _put(ens, "regridded", regrid.RegriddedProducts(regridder.lat_out, regridder.lon_out, a.regrid_method)),
                           scorer(names, regridder.lat_out, regridder.lon_out, truth, a.channels, "raw", hook), select=a.channels,
                           grid=regrid.grid_label(a.grid))
    # every member at the points (skyrim_amd/points.py): raw channels and derived fields at each saved lead, a window group when a window closes
    pointer = pointing.LeadPoints(names, lat, lon, M, p.points, p.point_channels, a.point_method, dev, dnames, n_saved) if p.points is not None else None
    for g in groups if p.points is not None else ():
        windowed[g.label].points = pointing.LeadPoints(g.fields, lat, lon, M, p.points, None, a.point_method, dev, (), max(g.n_windows, 1))
    if neighbours is not None and p.points is not None:
        neighbours.points = pointing.LeadPoints(nfields, lat, lon, M, p.points, None, a.point_method, dev, (), n_saved)
    # EFI, SOT and tail odds against a quantile climate (skyrim_amd/extremes.py): raw channels and derived fields at each saved lead, a window
    # group's fields when a window closes
    x = p.extremes
    extremist = extreming.LeadExtremes(names, lat, lon, M, x, dev, dnames) if x is not None and any(f in names + dnames for f in x.fields) else None
    for g in groups if x is not None else ():
        mine = [f for f in x.fields if f in g.fields]
        if mine:
            windowed[g.label].extremes = extreming.LeadExtremes(g.fields, lat, lon, M, x, dev, (), mine)
    # clusters, EOFs and the energy score of the members (skyrim_amd/scenarios.py)
    scenarist = scen.LeadScenarios(names, lat, lon, M, a.scenarios, device=dev, truth=scores, std=scenario_std(model, names) if a.scenarios.get(
        "normalise") == "std" else None) if a.scenarios is not None else None
    spectrists = {}                                        # zonal power spectra of members, mean, spread and errors (skyrim_amd/spectra.py):
    for family, own in (("raw", names), ("derived", dnames)) if a.spectra is not None else ():      # raw channels from the states, derived
        if wants(a.spectra, family):                       # fields from the deriver's buffer
            spectrists[family] = spec.LeadSpectra(own, lat, lon, M, dict(a.spectra, channels=wants(a.spectra, family)), device=dev, truth=scores)
    # labelled threshold regions of every member (skyrim_amd/objects.py): raw channels from the states, derived fields from the deriver's buffer
    objecter = objecting.LeadObjects(names, lat, lon, M, a.objects, dev, dnames, model_name=gm.model_name) if a.objects is not None else None
    truth_names = list(raw.scorer.scored) + (list(derived.scorer.scored) if derived is not None else []) if scores else None
    # the members themselves, packed on the device and written by threads of their own (skyrim_amd/archive.py)
    archiver = archiving.LeadArchive(gm, p, start_time) if p.archive is not None else None

    def raw_lead(L):                                       # first at every lead: a non-finite member makes the mean non-finite, one flag to read
        raw.reduce(L.time, L.states, L.table, L.slot)
        if not bool(torch.isfinite(raw.products.dev["mean"]).all().item()):
            bad = [m for m, st in enumerate(L.states) if not bool(torch.isfinite(st).all().item())]
            raise FloatingPointError(f"non-finite values in ensemble member(s) {bad} after step {L.k}")
        L.truth = raw.score(L.time, L.states, L.table)

    def derive(L):                                         # ONE launch: D derived planes per member, read below like raw channels
        L.derived = deriver.add(L.states, L.table)
        L.dtruth = derived.score(L.time, *L.derived)

    def neighbourhoods(L):                                 # one launch for the ops on the states, one for those on the deriver's buffer
        fields = neighbour.add(L.states, L.table, L.derived)
        neighbours.score(L.time, *fields)
        if L.slot is not None:
            neighbours.reduce(L.time, *fields, L.slot)

    def close_windows(L):                                  # windows close independently of ``save_every``
        for c in aggregator.add(L.k, L.time, L.states, L.table, L.derived):
            windowed[c.label].reduce(c.end, c.states, c.table, c.window, c.start)
            windowed[c.label].score(c.end, c.states, c.table, c.times)
            if L.sink is not None:                         # one file per closed window, without the ``window_start`` coordinate
                L.sink[1].extend(windowed[c.label].products.save(c.window, [c.end], c.start, gm.source_label, L.sink[0]))

    def hung(name, result, saved=True):                    # a ``finish``: the result on ``ens`` and, where it always was, in a file
        return lambda ens, fid, sink: _put(ens, name, _hang(result(fid), fid, sink if saved else None))
    folds_derived = bool(groups) and any(r.channel in dnames for r in p.aggregate.requests)
    every = lambda L: True                                 # noqa: E731
    todo = [                                               # (wanted?, the stage) in the order of a lead time
        (True, Stage(raw_lead, every, raw.fill)),
        (archiver, Stage(lambda L: archiver.add(L), finish=lambda ens, fid, sink: archiver.finish(ens), close=lambda: archiver.close())),
        (tracker, Stage(lambda L: tracker.add(L.time, L.states, L.table), every, hung("tracks", lambda fid: tracker.result()))),      # (a track needs every lead)
        (deriver, Stage(derive, lambda L: _saved(L) or derived.scorer is not None or (folds_derived and L.k >= 1))),
        (spectrists.get("derived"), Stage(lambda L: spectrists["derived"].add(L.time, *L.derived, L.dtruth))),
        (deriver, Stage(lambda L: derived.reduce(L.time, *L.derived, L.slot), finish=lambda ens, fid, sink: derived.fill(ens, fid))),
        (neighbour, Stage(neighbourhoods, lambda L: _saved(L) or neighbours.scorer is not None, lambda ens, fid, sink: neighbours.fill(ens, fid))),
        (scenarist, Stage(lambda L: scenarist.add(L.time, L.states, L.table, L.truth),
                          finish=hung("scenarios", lambda fid: scenarist.result(label, fid), False))),
        (spectrists.get("raw"), Stage(lambda L: spectrists["raw"].add(L.time, L.states, L.table, L.truth))),
        (spectrists, Stage(finish=hung("spectra", lambda fid: spec.merge([s.result(label, fid) for s in spectrists.values()], a.spectra["channels"]),
                                       False))),
        (objecter, Stage(lambda L: objecter.add(L.time, L.states, L.table, L.derived, L.truth, L.dtruth, truth_names),
                         finish=hung("objects", lambda fid: objecter.result()))),
        (pointer, Stage(lambda L: pointer.add(L.time, L.states, L.table, L.derived), finish=hung("points", lambda fid: pointer.result(label, fid)))),
        (extremist, Stage(lambda L: extremist.add(L.time, L.states, L.table, L.derived), finish=hung("extremes", lambda fid: extremist.result(label, fid)))),
        (aggregator, Stage(close_windows, lambda L: L.k >= 1,                  # (step 0, the initial state, belongs to no window)
                           lambda ens, fid, sink: [group.fill(ens, fid, xsink=sink) for group in windowed.values()])),
        (regridder, Stage(lambda L: regridded.lead(L.time, *regridder.add(L.states, L.table), L.slot),     # ONE launch: all channels, all members
                          lambda L: _saved(L) or regridded.scorer is not None, lambda ens, fid, sink: regridded.fill(ens, fid))),
    ]
    return [stage for wanted, stage in todo if wanted], [f for f in (raw, derived, regridded, neighbours) if f is not None] + list(windowed.values())


def run(gm, start_time: datetime.datetime, n_steps: int = 4, n_members: int = 10, perturb_scale: float = 1e-3, seed: int = 0,
        products=("mean", "spread"), exceed=None, quantiles=None, channels=None, save_every: int = 1, keep_members: bool = False,
        save: bool = False, save_config: dict | None = None, truth=None, climatology=None, scores: bool = False,
        tracks: bool = False, track_config=None, events=None, neighbourhoods_km=(), points=None, point_channels=None,
        point_method: str = "bilinear", scenarios=None, spectra=None, objects=None, extremes=None, archive=None, breeding=None, stochastic=None, aggregates=None, neighbourhood=None, vertical=None, derived_surface=None,
        derived=None, grid=None, regrid_method: str = "conservative", perturbation: str = "white", length_scale_km: float = 500.0, alpha: float = 2.0, lmax: int | None = None,
        perturb_channels=None) -> EnsembleForecast:
    """``GlobalModel.ensemble_forecast`` (core/models/base.py has the user-facing description): the plan of the request, the stages of a
    lead time, the seeded members (the member source), then ``drive``: lead by lead every stage that is due."""
    from .datasource import get_initial_condition_for_model
    from .leads import forget_resident
    from .stochastic import Stepper
    model = gm.model
    p = plan_request(model, n_steps, n_members, seed, products, exceed, quantiles, channels, save_every, keep_members, events=events,
                     neighbourhoods_km=neighbourhoods_km, scores=scores, points=points, point_channels=point_channels, point_method=point_method,
                     scenarios=scenarios, spectra=spectra, objects=objects, extremes=extremes, archive=archive, save=save, breeding=breeding, stochastic=stochastic,
                     aggregates=aggregates, neighbourhood=neighbourhood, vertical=vertical, derived_surface=derived_surface, derived=derived, grid=grid, regrid_method=regrid_method, perturbation=perturbation,
                     length_scale_km=length_scale_km, alpha=alpha, lmax=lmax, perturb_channels=perturb_channels, perturb_scale=perturb_scale)
    todo, families = stages(gm, p, start_time, truth, climatology, scores, tracks, track_config)
    x0 = get_initial_condition_for_model(model, gm.data_source, start_time).to(model.device, torch.float32).contiguous()
    if x0.device.type != "cuda":
        raise RuntimeError("ensemble_forecast makes and reduces its members with HIP kernels: the model must be on a GPU")
    forget_resident(model, closed=False)                   # the interleaved loops below are not a state a later rollout continues from
    std = channel_std(model)
    if std.numel() != x0.shape[2]:
        raise ValueError(f"channel_std holds {std.numel()} values for {x0.shape[2]} input channels")
    seeds, growth = seed_members(model, p, x0, std, float(perturb_scale), start_time)
    # per-step perturbations (skyrim_amd/stochastic.py): the members are held as states, each lead the model's own lead 1 from the perturbed one before
    stepper = Stepper(p.stochastic, x0.device, x0.shape[2:], std, p.M, int(seed), float(perturb_scale)) if p.stochastic is not None else None
    members = Members(model, start_time, seeds, stepper)
    del x0, seeds                                          # (only the members' current states stay alive on the GPU)
    return drive(gm, p, todo, families, members, n_steps, save, save_config, float(perturb_scale), growth)


def drive(gm, p: Plan, todo, families, members, n_steps, save, save_config, perturb_scale, growth=None) -> EnsembleForecast:
    """The leads of a forecast from a member source: ``members.advance(k) -> (valid time, M states)`` in order from 0 and
    ``members.close()`` -- the stepping ``Members`` of ``run``, or the files of a forecast that was written down
    (``archive.ArchiveMembers``).  Lead by lead every stage of ``todo`` that is due, the files of ``save``, then what the stages hang on
    the ``EnsembleForecast``."""
    from .common import save_config_with_id
    from .leads import forget_resident
    model, seed = gm.model, p.asked.seed
    cfg = save_config_with_id(save_config)
    fid, paths, source = cfg["forecast_id"], [], gm.source_label
    sink = (cfg, paths) if save else None                  # where the stages write
    for family in families:
        family.products = family.make()
    stored = [f for f in families if f.starts is None]     # raw, derived, regridded: their entries are the saved leads
    try:
        for k in range(n_steps + 1):
            time, states = members.advance(k)
            s = p.saved.index(k) if k in p.saved else None
            lead = SimpleNamespace(k=k, time=time, slot=s, states=states, table=member_table(states), sink=sink, truth=None, derived=None, dtruth=None)
            for stage in todo:
                if stage.add is not None and stage.due(lead):
                    stage.add(lead)
            if save and s:                                 # from the second saved step on: files of two entries, the step saved before and this one
                for family in stored:
                    paths += family.products.save(s - 1, family.times[s - 1:s + 1], family.times[s - 1], source, cfg)
                source = "file"
            del lead, states
    finally:
        try:
            members.close()
        finally:
            try:
                for stage in todo:
                    if stage.close is not None:
                        stage.close()
            finally:
                forget_resident(model)

    ens = EnsembleForecast(gm.model_name, p.M, int(seed), float(perturb_scale), paths=paths, forecast_id=fid, perturbation=p.noise.kind,
                           length_scale_km=float(p.asked.length_scale_km), alpha=float(p.asked.alpha), lmax=p.noise.lmax if p.noise.kind == "spherical" else None,
                           breeding=None if p.breeding is None else p.breeding.as_dict(), breeding_growth=growth,
                           stochastic=None if p.stochastic is None else p.stochastic.as_dict())
    for stage in todo:
        if stage.finish is not None:
            stage.finish(ens, fid, sink)
    return ens
