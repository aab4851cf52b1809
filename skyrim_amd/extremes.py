"""Climate-relative extremes of forecasts (include/skyrim_clim.h): the Extreme Forecast Index, the Shift of Tails and the
fraction of members beyond a climate percentile, made on the device from the members where they lie in HBM and a quantile climate
(skyrim_amd/climate.py).

Layers:

* ``check_request``: every refusal of ``extremes={...}`` that needs no device, in one fixed order;
* ``LeadExtremes``: what ``ensemble.run`` calls at every saved lead (raw channels from the states, derived fields from the deriver's
  buffer) and, with its own instance, when a window of a group closes; the climate's slice of the valid time is uploaded only when it
  differs from the resident one;
* ``Extremes``: the labelled (time, field, lat, lon) results and their files;
* ``extremes_model`` (``GlobalModel.extremes_forecast``: one state is an ensemble of one) and ``extremes_prediction`` for forecasts on disk.
"""
from __future__ import annotations

import datetime
import math
from dataclasses import dataclass, field
from pathlib import Path

import numpy as np

from . import climate as climating
from .common import finish as _finish, world_size as _world_size
from .leads import open_saved, require_gpu, run_model

KEYS = ("climate", "fields", "efi", "sot", "above", "below", "floor")
MAX_MEMBERS, MAX_SOT, MAX_PROB = climating.MAX_MEMBERS, climating.MAX_SOT, climating.MAX_PROB


@dataclass
class Request:
    """A checked ``extremes=`` request: the opened climate, the fields in the order asked for, ``efi``, the SOT tails, the percentiles
    ``(direction, level)`` -- the ``above`` ones first -- and ``floor`` per field (-inf: none)."""
    climate: object
    fields: list
    efi: bool
    sot: list
    prob: list
    floor: dict = field(default_factory=dict)


def check_request(names, lat, lon, n_members, extremes, derived=(), aggregates=()) -> Request:
    """Every refusal that needs no device, in this order: members sharded over ranks; not a dict, or without a climate; unknown keys;
    fields that are neither raw channels (``names``), derived fields nor aggregates of the request; fields the climate lacks; a SOT tail
    or a percentile whose levels the climate does not hold (matched to 1e-9, the level named); more than 4 SOT tails or 8 percentiles; a
    ``floor`` for a field not asked for; then the member count, a SOT of one member, nothing asked for, and the climate's grid."""
    if _world_size() > 1:
        raise NotImplementedError("extremes are made on one GPU from members that all lie there; members sharded over the ranks of a "
                                  "process group are out of scope (DESIGN.md 32)")
    if isinstance(extremes, Request):
        return extremes
    if not isinstance(extremes, dict) or extremes.get("climate") is None:
        raise ValueError('extremes: a dict {"climate": Climate or path, "fields": [...], "efi": True, "sot": [...], "above": [...], '
                         '"below": [...], "floor": {...}}')
    unknown = [k for k in extremes if k not in KEYS]
    if unknown:
        raise ValueError(f"extremes: unknown keys {unknown}; choose from {list(KEYS)}")
    clim = climating.as_climate(extremes["climate"])
    fields = [str(f) for f in (extremes.get("fields") or clim.fields)]
    known = list(names) + list(derived) + list(aggregates)
    missing = [f for f in fields if f not in known]
    if missing:
        raise ValueError(f"extremes: fields {missing} are neither output channels of this forecast nor derived fields nor aggregates of the request")
    if len(set(fields)) != len(fields):
        raise ValueError("extremes: a field is named twice")
    lacking = [f for f in fields if f not in clim.fields]
    if lacking:
        raise ValueError(f"extremes: the climate has no field {lacking}; it holds {clim.fields}")
    sot = [float(q) for q in extremes.get("sot") or []]
    for q in sot:
        base, ref = climating.sot_levels(q)
        climating.level_index(clim.levels, base, "extremes: sot")
        climating.level_index(clim.levels, ref, "extremes: sot")
    prob = [("above", float(v)) for v in extremes.get("above") or []] + [("below", float(v)) for v in extremes.get("below") or []]
    for direction, v in prob:
        climating.level_index(clim.levels, v, f"extremes: {direction}")
    if len(sot) > MAX_SOT or len(prob) > MAX_PROB:
        raise ValueError(f"extremes: {len(sot)} SOT tails and {len(prob)} percentiles; at most {MAX_SOT} and {MAX_PROB} "
                         "(SKCLIM_MAX_SOT, SKCLIM_MAX_PROB)")
    floor = {str(k): float(v) for k, v in (extremes.get("floor") or {}).items()}
    stray = [k for k in floor if k not in fields]
    if stray:
        raise ValueError(f"extremes: floor names {stray}, which are not among the fields asked for")
    if any(math.isnan(v) for v in floor.values()):
        raise ValueError("extremes: a floor is a number or -inf")
    if not 1 <= int(n_members) <= MAX_MEMBERS:
        raise ValueError(f"n_members = {n_members}: 1 to {MAX_MEMBERS} members are compared with a climate (SKCLIM_MAX_MEMBERS)")
    if sot and int(n_members) == 1:
        raise ValueError("extremes: the Shift of Tails is a quantile of the members; one state has none (ask for efi or percentiles)")
    efi = bool(extremes.get("efi", True))
    if not (efi or sot or prob):
        raise ValueError("extremes: nothing asked for (efi, sot, above, below)")
    if clim.levels.size < 2:
        raise ValueError("extremes: the climate needs at least 2 levels")
    clim.check_grid(lat, lon)
    return Request(clim, fields, efi, sot, prob, floor)


class Extremes:
    """The results: ``efi`` DataArray(time, field, lat, lon) or None; ``sot[q]`` the same per tail; ``probability(field, "above" |
    "below", level)`` DataArray(time, lat, lon), the fraction of members beyond the climate's ``level``; ``keys``: the climate slice each
    time was compared with."""

    def __init__(self, efi, sot, prob, keys, model_name="", forecast_id="", n_members=1):
        self.efi, self.sot, self.prob, self.keys = efi, sot, prob, keys
        self.model_name, self.forecast_id, self.n_members, self.path = model_name, forecast_id, n_members, None

    @property
    def fields(self) -> list:
        da = self.efi if self.efi is not None else next(iter({**self.sot, **self.prob}.values()))
        return da._coords["field"].tolist() if hasattr(da._coords["field"], "tolist") else list(da._coords["field"])

    def probability(self, fld: str, direction: str, level: float):
        for (d, v), da in self.prob.items():
            if d == direction and abs(v - float(level)) <= 1e-9:
                if fld not in self.fields:
                    raise ValueError(f"probability: {fld!r} is not among {self.fields}")
                return da.isel(field=self.fields.index(fld))
        raise ValueError(f"probability: {direction} {level} was not asked for ({list(self.prob)})")

    def arrays(self) -> dict:
        """``{file stem: DataArray}`` of everything held."""
        out = {} if self.efi is None else {"efi": self.efi}
        out.update({f"sot{q:g}": da for q, da in self.sot.items()})
        out.update({f"p{d}{v:g}": da for (d, v), da in self.prob.items()})
        return out

    def to_netcdf(self, directory) -> list:
        """One file ``{model}-{efi | sot<q> | p<above|below><level>}.nc`` per array under ``directory`` (time, field, lat, lon with the
        coordinates of these dimensions); returns the paths."""
        d = Path(directory)
        d.mkdir(parents=True, exist_ok=True)
        paths = []
        from .labeled import DataArray
        for stem, da in self.arrays().items():
            p = d / f"{self.model_name + '-' if self.model_name else ''}{stem}.nc"
            # (a window group's ``window_start`` runs along time without being a dimension: the file keeps the dimensions' coordinates)
            coords = {k: v for k, v in da._coords.items() if k in da.dims or np.ndim(v) == 0}
            DataArray(np.asarray(da.values), da.dims, coords, stem).to_netcdf(p)
            paths.append(str(p))
        return paths

    def save(self, output_dir) -> str:
        """The files of ``to_netcdf`` under ``{output_dir}/{forecast id}/extremes``; returns that directory."""
        d = (Path(output_dir) / self.forecast_id if self.forecast_id else Path(output_dir)) / "extremes"
        self.to_netcdf(d)
        self.path = str(d)
        return self.path


def merge(parts, fields) -> Extremes:
    """One ``Extremes`` of several over the same times (raw and derived fields), its fields in the order ``fields``."""
    from .labeled import DataArray
    parts = [p for p in parts if p is not None]
    if len(parts) == 1 and parts[0].fields == list(fields):
        return parts[0]
    order = [f for p in parts for f in p.fields]
    pick = [order.index(f) for f in fields]

    def cat(arrs):
        first = arrs[0]
        c = dict(first._coords)
        c["field"] = np.asarray(list(fields))
        return DataArray(np.concatenate([np.asarray(a.values) for a in arrs], axis=1)[:, pick], first.dims, c)
    first = parts[0]
    return Extremes(None if first.efi is None else cat([p.efi for p in parts]), {q: cat([p.sot[q] for p in parts]) for q in first.sot},
                    {k: cat([p.prob[k] for p in parts]) for k in first.prob}, first.keys, first.model_name, first.forecast_id, first.n_members)


class _Source:
    """The extremes of the fields one buffer holds: ``names`` are the channels of the (C, H, W) states handed to ``add``."""

    def __init__(self, names, lat, lon, n_members, req: Request, fields, device):
        self.names, self.lat, self.lon, self.M, self.req, self.fields, self.device = list(names), lat, lon, int(n_members), req, list(fields), device
        c = req.climate
        self.index = [self.names.index(f) for f in self.fields]
        self.cindex = [c.fields.index(f) for f in self.fields]
        self.floor = [req.floor.get(f, -math.inf) for f in self.fields]
        self.sot_req = [climating.sot_request(c.levels, q, self.M) for q in req.sot]
        self.prob_req = [(climating.level_index(c.levels, v, "extremes"), d == "below") for d, v in req.prob]
        self.groups = climating.field_groups(len(self.fields), c.levels.size, len(lat) * len(lon))
        self.key, self.resident, self.keys, self.times = "none", None, [], []
        self.host = dict(efi=[], sot=[], prob=[])

    def _upload(self, time):
        """The slice of ``time`` on the device as (nf, Q, H, W) per field group; uploaded only when it differs from the resident one."""
        import torch
        key, arr = self.req.climate.at(time)
        if self.resident is None or key != self.key:
            self.resident = None                                              # (the old slice is freed before the new one is allocated)
            self.resident = [torch.from_numpy(np.ascontiguousarray(arr[:, [self.cindex[i] for i in g]].transpose(1, 0, 2, 3))).to(self.device)
                             for g in self.groups]
            self.key = key
        return key

    def add(self, time, states, table=None) -> None:
        import torch
        from .members import member_table
        if len(states) != self.M:
            raise ValueError(f"{len(states)} states for extremes of {self.M} members")
        key = self._upload(time)
        table = member_table(states) if table is None else table
        dev, (H, W), r = states[0].device, states[0].shape[1:], self.req
        F, S, T = len(self.fields), len(self.sot_req), len(self.prob_req)
        efi = torch.empty((F, H, W), dtype=torch.float32, device=dev) if r.efi else None
        sot = torch.empty((S, F, H, W), dtype=torch.float32, device=dev) if S else None
        prob = torch.empty((T, F, H, W), dtype=torch.float32, device=dev) if T else None
        for g, clim in zip(self.groups, self.resident):
            whole = len(g) == F
            e = efi if whole or efi is None else torch.empty((len(g), H, W), dtype=torch.float32, device=dev)
            s = sot if whole or sot is None else torch.empty((S, len(g), H, W), dtype=torch.float32, device=dev)
            p = prob if whole or prob is None else torch.empty((T, len(g), H, W), dtype=torch.float32, device=dev)
            climating.run_extremes(states, table, [self.index[i] for i in g], clim, r.climate.levels, [self.floor[i] for i in g],
                                   self.sot_req, self.prob_req, e, s, p)
            if not whole:
                for full, part, ax in ((efi, e, 0), (sot, s, 1), (prob, p, 1)):
                    if full is not None:
                        full.index_copy_(ax, torch.tensor(g, device=dev), part)
        for name, t in (("efi", efi), ("sot", sot), ("prob", prob)):
            if t is not None:
                self.host[name].append(t.cpu().numpy())
        self.keys.append(key)
        self.times.append(time)

    def result(self, model_name="", forecast_id="", **coords) -> Extremes:
        from .labeled import DataArray
        r = self.req
        H, W = len(self.lat), len(self.lon)

        def labelled(arr):
            return DataArray(arr, ["time", "field", "lat", "lon"], dict(time=list(self.times), field=list(self.fields), lat=self.lat,
                                                                         lon=self.lon, **coords))
        n = len(self.times)
        stack = lambda name, lead: (np.stack(self.host[name]) if n else np.empty((0, *lead, len(self.fields), H, W), np.float32))      # noqa: E731
        efi = labelled(stack("efi", ())) if r.efi else None
        sot = {q: labelled(stack("sot", (len(r.sot),))[:, s]) for s, q in enumerate(r.sot)}
        prob = {k: labelled(stack("prob", (len(r.prob),))[:, t]) for t, k in enumerate(r.prob)}
        return Extremes(efi, sot, prob, list(self.keys), model_name, forecast_id, self.M)


class LeadExtremes:
    """The extremes of one rollout, modelled on ``points.LeadPoints``: raw channels from the states and, in a second call, derived fields
    from the deriver's buffer.  ``fields``: those of the request this object serves (None: the raw channels and derived fields among
    them; a window group passes its own).  ``add`` queues the launches of one lead time, ``result`` assembles the ``Extremes``."""

    def __init__(self, names, lat, lon, n_members, request, device="cuda:0", derived=(), fields=None):
        self.req = request if isinstance(request, Request) else check_request(names, lat, lon, n_members, request, derived)
        names, dnames = list(names), list(derived or [])
        self.fields = [f for f in self.req.fields if f in names or f in dnames] if fields is None else list(fields)
        raw, der = [f for f in self.fields if f in names], [f for f in self.fields if f not in names]
        mk = lambda nm, fl: _Source(nm, lat, lon, n_members, self.req, fl, device)      # noqa: E731
        self.raw = mk(names, raw) if raw else None
        self.der = mk(dnames, der) if der else None

    @property
    def needs_derived(self) -> bool:
        return self.der is not None

    def add(self, time, states, table=None, derived=None) -> None:
        if self.raw is not None:
            self.raw.add(time, states, table)
        if self.der is not None:
            if derived is None:
                raise ValueError("extremes name derived fields: add() needs derived=(states, table) of the deriver")
            self.der.add(time, derived[0], derived[1])

    def result(self, model_name="", forecast_id="", **coords) -> Extremes:
        return merge([s.result(model_name, forecast_id, **coords) for s in (self.raw, self.der) if s is not None], self.fields)


def extremes_model(gm, start_time: datetime.datetime, n_steps: int, extremes, derived=None, save: bool = False,
                   save_config: dict | None = None) -> Extremes:
    """``GlobalModel.extremes_forecast`` (core/models/base.py has the user-facing description)."""
    model = gm.model
    names = list(model.out_channel_names)
    if n_steps < 0:
        raise ValueError("n_steps >= 0")
    deriver = None
    if derived is not None:
        from . import derived as deriving
        deriving.check_request(names, list(derived), model.grid.lat, model.grid.lon, 1)
    req = check_request(names, model.grid.lat, model.grid.lon, 1, extremes, list(derived or []))      # before the device
    le = LeadExtremes(names, model.grid.lat, model.grid.lon, 1, req, model.device, list(derived or []))
    require_gpu(model.device, "extremes_forecast compares with HIP kernels where the forecast lies: the model must be on a GPU")
    if le.needs_derived:
        deriver = deriving.LeadDeriver(names, model.grid.lat, model.grid.lon, 1, list(derived), device=model.device)
    run_model(gm, start_time, n_steps,
              lambda k, time, state: le.add(time, [state], None, deriver.add([state]) if deriver is not None else None))
    return _finish(le.result(gm.model_name), save, save_config)


def extremes_prediction(pred, extremes, derived=None, device="cuda:0") -> Extremes:
    """The extremes of a forecast that already exists: a ``GlobalPrediction``, a (time, channel, lat, lon) DataArray, a saved netCDF file
    or zarr store, or a list of such files.  Each time entry is uploaded, compared by the same kernel as ``extremes_forecast`` (one state
    is an ensemble of one) and dropped."""
    saved = open_saved(pred, "extremes_prediction")
    dnames, deriver = list(derived or []), None
    if dnames:
        from . import derived as deriving
        deriving.check_request(saved.names, dnames, saved.lat, saved.lon, 1)
    req = check_request(saved.names, saved.lat, saved.lon, 1, extremes, dnames)
    le = LeadExtremes(saved.names, saved.lat, saved.lon, 1, req, device, dnames)
    require_gpu(device, "extremes_prediction compares with HIP kernels: it needs a GPU", present=True)
    if le.needs_derived:
        deriver = deriving.LeadDeriver(saved.names, saved.lat, saved.lon, 1, dnames, device=device)
    for _, time, state in saved.states(device):
        le.add(time, [state], None, deriver.add([state]) if deriver is not None else None)
    return le.result(saved.model_name)
