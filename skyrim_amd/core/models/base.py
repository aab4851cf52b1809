"""GlobalModel / GlobalPrediction / GlobalPredictionRollout -- the names, arguments and results of
/root/reference/skyrim/core/models/base.py (:13-15 adjust_lead_time, :18-146 GlobalModel, :149-274
GlobalPrediction, :277-303 GlobalPredictionRollout).  The model side drives a HIP TimeLoop; the prediction side works on
``labeled.DataArray`` with regular-grid index arithmetic (lat / lon are uniform axes, so "nearest" is a division, not a search)."""
from __future__ import annotations

import datetime
import logging
import os
import time
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path
from typing import List

import numpy as np

from ...common import save_config_with_id, save_forecast
from ...datasource import IC_SOURCES, get_data_source
from ...labeled import DataArray, open_dataarray
from .utils import run_basic_inference

logger = logging.getLogger("skyrim_amd")

STEPS_AHEAD = 3           # steps ``rollout`` lets the host queue in front of the GPU
SAVE_WORKERS = 8          # per-step netCDF files written at once by ``rollout`` (SKYRIM_SAVE_WORKERS; one file is one pwrite stream of ~6 GB/s, files side by side scale: docs/experiments.md A6.5)


def adjust_lead_time(lead_time: int, step_size: int = 6):
    """Adjust lead time to the nearest multiple of step_size"""
    return max(step_size, (lead_time // step_size) * step_size)


class GlobalModel:
    def __init__(self, model_name: str, ic_source: str = "cds"):
        clock = time.time()
        if ic_source not in IC_SOURCES:
            raise ValueError(f"Invalid initial condition source: {ic_source}")
        self.model_name = model_name
        self.ic_source = ic_source
        self.model = self.build_model()
        self.data_source = self.build_datasource()
        logger.info(f"Initialized {model_name} in {time.time() - clock:.1f} seconds")

    def build_model(self):
        raise NotImplementedError

    def build_datasource(self):
        return get_data_source(self.model.in_channel_names, initial_condition_source=self.ic_source,
                               geom=getattr(self.model, "geom", None), state_fn=getattr(self.model, "synthetic_state", None))

    def release_model(self):
        """Give the model's device memory back, deterministically (the reference's TODO, base.py:50-55; what its ensemble does between
        members, ensemble.py:39-48): the TimeLoop destroys its engine contexts (``sk*_destroy``) and drops every arena / prepared tensor,
        then the caching allocator is emptied.  The wrapper is unusable afterwards (``build_model()`` again for a new one)."""
        m, self.model = getattr(self, "model", None), None
        if getattr(self, "stepper", None) is not None:
            self.stepper = None
        if m is not None and hasattr(m, "__dict__"):
            m._resident_state = None                            # the device copy of the last delivered states (utils.ResidentState)
        if m is not None and hasattr(m, "release"):
            m.release()
        del m
        import gc
        import torch
        gc.collect()
        if torch.cuda.is_available():
            torch.cuda.empty_cache()

    @property
    def time_step(self):
        raise NotImplementedError

    def time_steps(self, lead_time: int):
        lead_time = adjust_lead_time(lead_time, step_size=6)
        return int(lead_time // (self.model.time_step.total_seconds() / 3600))

    @property
    def in_channel_names(self):
        raise NotImplementedError

    @property
    def out_channel_names(self):
        raise NotImplementedError

    def __repr__(self) -> str:
        return f"{self.__class__.__name__}(model_name={self.model_name})"

    @property
    def source_label(self) -> str:
        """What saved files are stamped with: the requested source, or "synthetic" when the data source is the seeded stand-in."""
        return getattr(self.data_source, "label", None) or self.ic_source

    def predict_one_step(self, start_time: datetime.datetime, initial_condition=None) -> DataArray:
        # if initial_condition is None, it is fetched from the self.ic_source
        return self._step_delivering(start_time, initial_condition, None)

    def _mark_step(self):
        """An event behind everything queued so far on the model's GPU (None for a model that is not on one)."""
        import torch
        dev = getattr(self.model, "device", None)
        if dev is None or torch.device(dev).type != "cuda":
            return None
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(torch.device(dev)))
        return ev

    def _step_delivering(self, start_time, initial_condition, deliver, defer_check=False) -> DataArray:
        # (not ``_predict_one_step``: the GraphCast wrapper has a method of that name, as the reference's does)
        return run_basic_inference(model=self.model, n=1, data_source=self.data_source, time=start_time, x=initial_condition, deliver=deliver,
                                   defer_check=defer_check)

    def forecast(self, start_time: datetime.datetime, n_steps: int = 3, channels: List[str] = []):
        da = run_basic_inference(model=self.model, n=n_steps, data_source=self.data_source, time=start_time, x=None)
        return da.sel(channel=channels) if channels else da

    def ensemble_forecast(self, start_time: datetime.datetime, n_steps: int = 4, n_members: int = 10, perturb_scale: float = 1e-3,
                          seed: int = 0, products=("mean", "spread"), exceed: dict | None = None, quantiles: dict | None = None,
                          channels: List[str] | None = None, save_every: int = 1, keep_members: bool = False, save: bool = False,
                          save_config: dict | None = None, truth=None, climatology=None, scores: bool = False,
                          tracks: bool = False, track_config=None, events=None, neighbourhoods_km=(),
                          points=None, point_channels: List[str] | None = None, point_method: str = "bilinear",
                          scenarios: dict | None = None, spectra: dict | None = None, objects: dict | None = None, extremes: dict | None = None,
                          archive: dict | None = None, breeding: dict | None = None, stochastic: dict | None = None,
                          aggregates: List[str] | None = None, neighbourhood: List[str] | None = None, vertical: dict | None = None,
                          derived_surface=None, derived: List[str] | None = None, grid=None, regrid_method: str = "conservative", perturbation: str = "white",
                          length_scale_km: float = 500.0, alpha: float = 2.0, lmax: int | None = None,
                          perturb_channels: List[str] | None = None):
        """An ``n_members`` ensemble of THIS model from perturbed initial conditions (skyrim_amd/ensemble.py): member m
        starts from ``x0 + perturb_scale * sigma_channel * z(seed, m)`` (member 0 is the unperturbed control), every member runs through its
        own TimeLoop generator, and at each lead time one HIP pass over the members gives the ``products`` (any of mean, spread, min, max),
        the exceedance fractions ``exceed = {channel: [thresholds]}`` and the quantiles ``quantiles = {channel: [levels]}`` (at most 4
        values per channel).  Returns an ``ensemble.EnsembleForecast``; its time axis holds the initial condition and every
        ``save_every``-th step.  ``save=True`` writes one file per product and saved step, model field ``{model}-ens{M}-{product}``.
        ``scores=True`` scores every lead time against ``truth`` right after its statistics, on the members where they lie
        (``verify`` below has the forms of ``truth`` and ``climatology``); the ``verify.Scores`` land in ``EnsembleForecast.scores``.
        ``perturbation="spherical"`` replaces the grid-point white noise z by an isotropic Gaussian random field per (history level,
        channel) with unit pointwise variance, correlation length ``length_scale_km`` and spectrum
        (kappa^2 + l (l + 1))^(-alpha / 2) truncated at ``lmax`` (default min(256, n_lat_full, n_lon / 2)), synthesised on the device
        (skyrim_amd/noise.py); it needs a pole-to-pole equiangular grid or its first rows.  ``perturb_channels`` lists the
        input channels that are perturbed, for either kind; the others get amplitude exactly 0.  ``tracks=True`` detects cyclone centres in
        every member at every lead time, right after the scores and on the same states (skyrim_amd/tracks.py, DESIGN.md 20;
        ``track_config``: a ``tracks.TrackerConfig`` or a dict of its fields); the linked ``tracks.Tracks`` land in
        ``EnsembleForecast.tracks``.  ``derived=[...]`` names derived fields (``ws10m``, ``ws100m``, ``ws<level>``, ``thk<a>_<b>``, ``vo<X>``,
        ``div<X>``, ``ivt``, ``ivtu``, ``ivtv``, ``iwv``: skyrim_amd/derived.py; and the column thermodynamics ``td<level>``,
        ``thetae<level>``, ``kx``, ``tt``, ``zdeg0``, ``sbcape``, ``mucape``, ``muli`` ... of DESIGN.md 30, with ``derived_surface=`` the (lat, lon) surface
        geopotential that masks the levels below the ground -- without it they are treated as air; and the fields on chosen surfaces
        ``<field>@<surface>`` of DESIGN.md 34 -- ``ws@100magl``, ``t@1500m``, ``z@-10C``, ``u@320K``, ``ws@875hPa`` -- with ``derived_surface=`` also the
        ground of ``@<Z>magl`` and ``vertical={"outside": "nan" | "nearest"}`` what they are where the surface does not cross the column) that are formed from every member on the device at
        each lead time; the same ``products`` of them, ``exceed`` / ``quantiles`` under their names and, with ``scores=True``, their scores land
        in ``EnsembleForecast.derived``.  ``grid=`` names a target grid (``"1.5deg"`` or a float, ``(lat, lon)`` arrays, or
        ``dict(region=(lat_s, lat_n, lon_w, lon_e), res=...)``: skyrim_amd/regrid.py) every member is also put on at each lead
        time, on the device, by ``regrid_method`` (conservative, bilinear, nearest); the same ``products``, ``exceed`` and ``quantiles`` on it
        and, with ``scores=True``, the scores against the truth regridded likewise land in ``EnsembleForecast.regridded``.  With a grid,
        ``keep_members=True`` also returns the regridded members and ``keep_members="regridded"`` only those, so that the host limit is
        checked against their size.  ``events={channel: [thresholds]}`` (``True``: the thresholds of ``exceed``), with ``scores=True``,
        verifies the events "above the threshold" at each lead time (skyrim_amd/events.py): Brier score and decomposition,
        reliability curve, ROC and, over the radii ``neighbourhoods_km``, the fractions skill score land in ``scores.events`` of the raw,
        derived and regridded scores.  ``aggregates=["ws10m:max:24h", "t2m:mean:24h", "ws10m:hours_above@15:all", "msl:when_min:all"]``
        asks for time-window aggregates ``channel:stat:window`` (skyrim_amd/aggregate.py) of raw channels and of the fields in
        ``derived``: every member is reduced over the lead times of each window on the device, and the same ``products``, ``exceed`` /
        ``quantiles`` / ``events`` under the aggregates' names (``ws10m_max_24h``), the members with ``keep_members`` and the scores with
        ``scores=True`` land in ``EnsembleForecast.aggregated[window label]``, with the window ends as time axis.  ``points=`` names places
        -- ``{name: (lat, lon)}``, a list of ``(name, lat, lon)`` or a CSV file ``name,lat,lon`` (skyrim_amd/points.py) -- at
        which every member is sampled on the device at each saved lead time, by ``point_method`` (bilinear, nearest), for the channels
        ``point_channels`` (raw channels and fields of ``derived``; default ``channels``, or every raw and derived channel): the
        ``points.PointForecast`` (member, time, channel, point) lands in ``EnsembleForecast.points``, and each aggregate group's fields at
        the points, sampled when a window closes, in ``EnsembleForecast.aggregated[label].points``.
        ``neighbourhood=["ws10m:max:100km", "t2m:frac_above@303.15:50km", "msl:mean:200km"]`` asks for neighbourhood fields
        ``channel:stat:radius`` (skyrim_amd/neighbourhood.py) of raw channels and of the fields in ``derived``: every member is
        reduced over the great-circle disc around every grid point on the device (``stat``: max, min, the area-weighted mean,
        frac_above@<threshold>), and the same ``products``, ``exceed`` / ``quantiles`` / ``events`` under the fields' names
        (``ws10m_max_100km``: ``exceed`` of it is the chance of the event SOMEWHERE within 100 km), the members with ``keep_members``, the
        scores with ``scores=True`` and the points with ``points=`` land in ``EnsembleForecast.neighbourhood``.
        ``scenarios={"channels": ["z500"], "region": (lat_s, lat_n, lon_w, lon_e), "n_clusters": 3, "n_eofs": 3, "normalise": "spread"}``
        relates the members to each other as patterns (skyrim_amd/scenarios.py): at each saved lead time ONE device pass
        makes the member Gram matrix of the named raw channels over the region (None: the globe; a box may cross the date line), and from
        it the host makes the clusters by Ward's method (labels, sizes, probabilities, representative members), the leading EOFs of the
        spread and, with ``scores=True``, the fair energy score; the clusters' mean fields and the EOF patterns are made on the device.
        ``normalise``: how channels are weighed against each other (``"spread"``: by their mean member variance, ``"std"``: by the
        model's ``channel_std``, ``"none"``).  This version takes raw channels on the model's own grid only; 2 <= n_members <= 64 (63
        with ``scores=True``: the truth is one more column).  The ``scenarios.Scenarios`` land in ``EnsembleForecast.scenarios``.
        ``breeding={"cycles": 3, "norm": "total", "paired": False}`` breeds the initial perturbations through the model itself
        (skyrim_amd/breeding.py): ``perturbation`` then names the SEED; each cycle steps every member once, takes the
        difference from the control forecast, scales it back to ``perturb_scale`` (``norm="total"``: one factor per member over the
        perturbed channels, which keeps the balance between variables the model produced; ``"channel"``: every channel to its own
        amplitude) and puts it on the analysis again -- two device launches per cycle for all members.  ``paired=True`` makes the members
        2j - 1 and 2j the two signs of one bred vector.  Models with one history level and the same channels in and out (pangu,
        fourcastnet, fourcastnet_v2); ``EnsembleForecast.breeding_growth`` holds the growth record (cycle, member, channel).
        ``stochastic={"kind": "sppt", "amplitude": 0.3, "tau_h": 6.0, "length_scale_km": 500.0}`` perturbs the MODEL as it runs, at
        every step of every member but the control (skyrim_amd/stochastic.py), by a random pattern that is correlated in
        space (the spectrum of ``perturbation="spherical"``: ``length_scale_km``, ``alpha``, ``lmax``) and in time (decorrelation time
        ``tau_h`` hours; 0: a fresh pattern every step).  ``kind="sppt"`` multiplies the step's tendency x_k - x_{k-1} by 1 + w, ONE
        pattern w for all channels with standard deviation ``amplitude``, clipped to +-``clip`` (0.9); ``"additive"`` puts one field
        per channel on the state, ``additive_scale`` (default ``perturb_scale``) times the channel's sigma; ``"both"`` does both.
        ``channels`` restricts either term to some input channels.  Each lead time is then the model's own first step from the
        perturbed state before it, so the members are held as states: the same models as ``breeding``, and not a Pangu loaded with
        its 24-h network.  It combines with every ``perturbation`` and with ``breeding``; ``perturb_scale=0`` leaves the stochastic
        terms as the only source of spread.  The defaults are the first scale of ECMWF's SPPT; whether they give a calibrated spread
        with real weights is not measured (``verify --stochastic`` prints spread against skill).  The normalised request lands in
        ``EnsembleForecast.stochastic``.
        ``spectra={"channels": ["z500", "u850", "v850"], "bands": {"nh_mid": (30, 60), "tropics": (-20, 20)}}`` makes zonal power spectra
        (skyrim_amd/spectra.py) at each saved lead time in ONE device pass: per channel, latitude band (default: nh_mid,
        tropics, sh_mid, globe) and zonal wavenumber the power of the members, of their mean and of their spread and, with
        ``scores=True``, of the truth and of the errors of the mean and of the members.  Raw channels and fields of ``derived`` on the model's own grid; the
        number of longitudes must be 2^a 3^b 5^c.  The ``spectra.Spectra`` land in ``EnsembleForecast.spectra``.  ``spectra=None``
        launches nothing.
        ``objects={"ivt": {"above": [250.0], "min_area_km2": 2e5, "min_length_km": 2000.0, "min_elongation": 2.0}, "t2m": {"below":
        [253.15]}, "connectivity": 8, "min_pixels": 4, "capacity": 1024}`` finds, at each saved lead time and in every member, the contiguous
        regions where a raw channel or a field of ``derived`` is beyond a threshold (skyrim_amd/objects.py): labelled and
        measured on the device, filtered on the host, with the fraction of members whose kept object covers each point; with
        ``scores=True`` the truth goes through the same kernels and ``Objects.verify()`` compares.  The ``objects.Objects`` land in
        ``EnsembleForecast.objects``.  ``objects=None`` launches nothing.  ``extremes={"climate": Climate or path, "fields": [...], "efi": True,
        "sot": [0.9, 0.1], "above": [0.95, 0.99], "below": [0.05], "floor": {"mucape": 0.0}}`` compares the members with a quantile climate
        (skyrim_amd/climate.py) where they lie in HBM: the Extreme Forecast Index, the Shift of Tails and the fraction of members
        beyond a climate percentile of raw channels and derived fields at the saved leads (``EnsembleForecast.extremes``) and of aggregates
        when their window closes (``EnsembleForecast.aggregated[label].extremes``, the slice of the climate chosen by the window's end).
        ``extremes=None`` launches nothing.  ``archive={"packing": "int16" | "float32", "channels": [...] | None, "dir": None}`` writes the
        members themselves (skyrim_amd/archive.py): at each saved lead every member's listed channels (None: all) are
        quantised plane by plane to 16-bit codes in the file's byte order on the device (``"float32"``: byte-swapped, lossless) and written
        by threads of their own, one netCDF file per (member, lead) under ``<output_dir>/<forecast_id>/members/`` (or ``"dir"``) with a
        ``manifest.json``; it needs ``save=True`` or a ``"dir"``.  ``EnsembleForecast.archive`` is the ``archive.MemberArchive``, whose
        ``replay(**request)`` later runs every product that only reads states on the files, without the model.  ``archive=None`` launches
        nothing."""
        from ... import ensemble
        extra = dict(tracks=True, track_config=track_config) if tracks else {}
        if events is not None:
            extra.update(events=events, neighbourhoods_km=neighbourhoods_km)
        if derived is not None:
            extra["derived"] = derived
        if derived_surface is not None:
            extra["derived_surface"] = derived_surface
        if vertical is not None:
            extra["vertical"] = vertical
        if grid is not None:
            extra.update(grid=grid, regrid_method=regrid_method)
        if aggregates is not None:
            extra["aggregates"] = aggregates
        if neighbourhood is not None:
            extra["neighbourhood"] = neighbourhood
        if points is not None:
            extra.update(points=points, point_channels=point_channels, point_method=point_method)
        if scenarios is not None:
            extra["scenarios"] = scenarios
        if breeding is not None:
            extra["breeding"] = breeding
        if stochastic is not None:
            extra["stochastic"] = stochastic
        if spectra is not None:
            extra["spectra"] = spectra
        if objects is not None:
            extra["objects"] = objects
        if extremes is not None:
            extra["extremes"] = extremes
        if archive is not None:
            extra["archive"] = archive
        return ensemble.run(self, start_time, n_steps=n_steps, n_members=n_members, perturb_scale=perturb_scale, seed=seed, products=products,
                            exceed=exceed, quantiles=quantiles, channels=channels, save_every=save_every, keep_members=keep_members,
                            save=save, save_config=save_config, truth=truth, climatology=climatology, scores=scores,
                            perturbation=perturbation, length_scale_km=length_scale_km, alpha=alpha, lmax=lmax,
                            perturb_channels=perturb_channels, **extra)

    def track_cyclones(self, start_time: datetime.datetime, n_steps: int = 4, config=None, save: bool = False, save_config: dict | None = None):
        """Cyclone tracks of the deterministic forecast over the lead times 0 .. ``n_steps`` (skyrim_amd/tracks.py).  The
        model's TimeLoop is advanced and every state is searched where it lies in HBM -- a pressure minimum with cyclonic 850-hPa
        vorticity, 10-m wind and (where the model has the levels) a warm core nearby -- so that only the candidates' records cross to the
        host, which links them into tracks.  ``config``: a ``tracks.TrackerConfig`` or a dict of its fields.  Returns ``tracks.Tracks``;
        ``save=True`` writes ``{model}-tracks.json`` under the forecast id directory.  A model without msl, u10m, v10m, u850 and v850
        (DLWP) is refused with ValueError before the device is touched."""
        from ... import tracks
        return tracks.track_model(self, start_time, n_steps=n_steps, config=config, save=save, save_config=save_config)

    def object_forecast(self, start_time: datetime.datetime, n_steps: int = 4, objects: dict | None = None, derived: List[str] | None = None,
                        truth=None, save: bool = False, save_config: dict | None = None):
        """Weather objects of the deterministic forecast at the lead times 0 .. ``n_steps`` (skyrim_amd/objects.py): the
        contiguous regions where a channel, or a field of ``derived``, is at or above / at or below a threshold -- ``objects={"ivt":
        {"above": [250.0], "min_area_km2": 2e5, "min_length_km": 2000.0, "min_elongation": 2.0}, "t2m": {"below": [253.15]},
        "connectivity": 8, "min_pixels": 4, "capacity": 1024}``.  The model's TimeLoop is advanced and every state is labelled and measured
        where it lies in HBM (with a global longitude circle an object may cross the date line; rows are not joined across the poles); only
        128-byte records and one count plane per threshold cross to the host.  ``truth`` (the forms of ``verify``): its objects are found
        by the same kernels and ``Objects.verify()`` matches them.  Returns ``objects.Objects``; ``save=True`` writes
        ``{model}-objects.json`` and the count planes beside it.  A request that cannot be served is refused with ValueError before the
        device is touched."""
        from ... import objects as objecting
        return objecting.objects_model(self, start_time, n_steps, objects, derived=derived, truth=truth, save=save, save_config=save_config)

    def extremes_forecast(self, start_time: datetime.datetime, n_steps: int = 4, extremes: dict | None = None, derived: List[str] | None = None,
                          save: bool = False, save_config: dict | None = None):
        """The deterministic forecast at the lead times 0 .. ``n_steps`` against a quantile climate (skyrim_amd/extremes.py).
        ``extremes``: the dict of ``ensemble_forecast(extremes=...)``; its fields are raw channels and fields of ``derived``.  One state is an
        ensemble of one: the EFI is defined (and steps between -1 and 1 as the state crosses the climate's levels), the tail odds are 0 or 1,
        a SOT is refused.  The model's TimeLoop is advanced and every state is compared where it lies in HBM; only the index planes cross
        to the host.  Returns an ``extremes.Extremes``; ``save=True`` writes its files under the forecast id directory.  A request that
        cannot be served is refused with ValueError before the device is touched."""
        from ... import extremes as extreming
        if extremes is None:
            raise ValueError('extremes_forecast needs extremes: {"climate": Climate or path, "fields": [...], ...}')
        return extreming.extremes_model(self, start_time, n_steps, extremes, derived=derived, save=save, save_config=save_config)

    def derive_fields(self, start_time: datetime.datetime, n_steps: int = 4, fields: List[str] = (), save: bool = False,
                      save_config: dict | None = None, derived_surface=None, vertical: dict | None = None):
        """Derived fields of the deterministic forecast at the lead times 0 .. ``n_steps`` (skyrim_amd/derived.py): wind speed
        (``ws10m``, ``ws100m``, ``ws<level>``), thickness (``thk<a>_<b>``), vorticity and divergence (``vo<X>``, ``div<X>``) and the column
        integrals ``ivt``, ``ivtu``, ``ivtv``, ``iwv``, and the column thermodynamics of DESIGN.md 30 (``td<level>``, ``thetae<level>``, ``kx``,
        ``tt``, ``zdeg0``, ``sbcape``, ``mucape``, ``muli`` ...; ``derived_surface``: the (lat, lon) surface geopotential that masks the levels
        below the ground -- without it they are treated as air), and the fields on chosen surfaces of DESIGN.md 34 (``ws@100magl``, ``t@1500m``,
        ``z@-10C``, ``u@320K``, ``ws@875hPa``; ``vertical={"outside": "nan" | "nearest"}``).  The model's TimeLoop is advanced and every state is derived where it lies in HBM; only
        the derived planes cross to the host.  Returns DataArray(time, channel=fields, lat, lon); ``save=True`` writes it as the forecast of
        ``{model}-derived``.  A field whose input channels the model lacks is refused with ValueError before the device is touched."""
        from ... import derived
        return derived.derive_model(self, start_time, n_steps, list(fields), save=save, save_config=save_config, surface=derived_surface, vertical=vertical)

    def aggregate_forecast(self, start_time: datetime.datetime, n_steps: int = 4, aggregates: List[str] = (), derived: List[str] | None = None,
                           save: bool = False, save_config: dict | None = None):
        """Time-window aggregates of the deterministic forecast over the lead times 1 .. ``n_steps`` (skyrim_amd/aggregate.py).
        ``aggregates``: requests ``channel:stat:window`` -- ``stat`` one of max, min, mean, sum, hours_above@<threshold>, when_max, when_min
        (hours since ``start_time``); ``window`` ``<N>h`` (consecutive windows (w N, (w + 1) N] hours after ``start_time``; N a multiple of
        the model's step) or ``all``; ``derived``: derived fields the requests may name.  The model's TimeLoop is advanced and every state is
        folded into the windows where it lies in HBM; only the closed windows cross to the host.  Returns {window label:
        DataArray(time = window ends, channel = aggregates, lat, lon)} with the coordinate ``window_start``; ``save=True`` writes each as the
        forecast of ``{model}-agg<label>``.  A request that cannot be served is refused with ValueError before the device is touched."""
        from ... import aggregate
        return aggregate.aggregate_model(self, start_time, n_steps, list(aggregates), derived=derived, save=save, save_config=save_config)

    def neighbourhood_forecast(self, start_time: datetime.datetime, n_steps: int = 4, neighbourhood: List[str] = (),
                               derived: List[str] | None = None, save: bool = False, save_config: dict | None = None):
        """Neighbourhood fields of the deterministic forecast at the lead times 0 .. ``n_steps`` (skyrim_amd/neighbourhood.py).
        ``neighbourhood``: requests ``channel:stat:radius`` -- ``stat`` one of max, min, mean (area-weighted), frac_above@<threshold>;
        ``radius`` ``<N>km``, the radius of the great-circle disc around every grid point; ``derived``: derived fields the requests may name.
        The model's TimeLoop is advanced and every state is reduced where it lies in HBM; only the fields cross to the host.  Returns
        DataArray(time, channel = ``ws10m_max_100km`` ..., lat, lon); ``save=True`` writes it as the forecast of ``{model}-nbr``.  A request
        that cannot be served is refused with ValueError before the device is touched."""
        from ... import neighbourhood as nbr
        return nbr.neighbourhood_model(self, start_time, n_steps, list(neighbourhood), derived=derived, save=save, save_config=save_config)

    def point_forecast(self, start_time: datetime.datetime, n_steps: int = 4, points=None, channels: List[str] | None = None,
                       derived: List[str] | None = None, method: str = "bilinear", save: bool = False, save_config: dict | None = None):
        """The deterministic forecast at the lead times 0 .. ``n_steps`` at scattered places (skyrim_amd/points.py).
        ``points``: ``{name: (lat, lon)}``, a list of ``(name, lat, lon)`` or a CSV file ``name,lat,lon``; ``channels``: raw channels and
        fields of ``derived`` (default: all of both); ``method``: bilinear (two taps per axis, the longitude periodic; a point outside the
        model's latitudes is refused) or nearest.  The model's TimeLoop is advanced and every state is sampled where it lies in HBM; only
        the sampled values cross to the host.  Returns a ``points.PointForecast`` with one member; ``save=True`` writes
        ``{model}-points.json`` under the forecast id directory.  A request that cannot be served is refused with ValueError before the
        device is touched."""
        from ... import points as pointing
        if points is None:
            raise ValueError("point_forecast needs points: {name: (lat, lon)}, a list of (name, lat, lon) or a CSV file name,lat,lon")
        return pointing.point_model(self, start_time, n_steps, points, channels=channels, derived=derived, method=method, save=save,
                                    save_config=save_config)

    def regrid_forecast(self, start_time: datetime.datetime, n_steps: int = 4, grid="1.5deg", method: str = "conservative",
                        channels: List[str] | None = None, save: bool = False, save_config: dict | None = None):
        """The deterministic forecast at the lead times 0 .. ``n_steps`` on another latitude-longitude grid (skyrim_amd/regrid.py,
        DESIGN.md 22).  ``grid``: a resolution (``"1.5deg"`` or a float; 180 / res an integer), ``(lat, lon)`` arrays, or
        ``dict(region=(lat_s, lat_n, lon_w, lon_e), res=...)``; ``method``: conservative (first order), bilinear or nearest.  The model's
        TimeLoop is advanced and every state is regridded where it lies in HBM; only the regridded states cross to the host.  Returns
        DataArray(time, channel, lat, lon) on the target grid; ``save=True`` writes it as the forecast of ``{model}-regrid``.  A target
        the method cannot serve is refused with ValueError before the device is touched."""
        from ... import regrid
        return regrid.regrid_model(self, start_time, n_steps, grid, method, channels, save=save, save_config=save_config)

    def spectrum_forecast(self, start_time: datetime.datetime, n_steps: int = 4, spectra: dict | None = None, truth=None, save: bool = False,
                          save_config: dict | None = None):
        """Zonal power spectra of the deterministic forecast at the lead times 0 .. ``n_steps`` (skyrim_amd/spectra.py).
        ``spectra``: ``{"channels": [...], "bands": {name: (lat_s, lat_n) or None}}`` (default bands: nh_mid, tropics, sh_mid, globe).
        The model's TimeLoop is advanced and every state is transformed where it lies in HBM: no state goes to the host.  ``truth`` (the
        forms ``verify`` takes, but not None): also the spectra of the truth and of the error.  Returns a ``spectra.Spectra`` whose
        ``power`` is (time, channel, band, kind, wavenumber); ``save=True`` writes ``{model}-spectra.json`` under the forecast id
        directory.  A request that cannot be served is refused with ValueError before the device is touched."""
        from ... import spectra as spec
        return spec.spectrum_model(self, start_time, n_steps=n_steps, spectra=spectra, truth=truth, save=save, save_config=save_config)

    def verify(self, start_time: datetime.datetime, n_steps: int = 4, truth=None, climatology=None, channels: List[str] | None = None,
               save: bool = False, save_config: dict | None = None, grid=None, regrid_method: str = "conservative", events=None,
               neighbourhoods_km=()):
        """Scores of the deterministic forecast at every lead time 0 .. ``n_steps`` (skyrim_amd/verify.py): bias, MAE, RMSE,
        CRPS (= MAE for one member) and, with a ``climatology``, ACC, area-weighted per channel.  The model's TimeLoop is advanced, each
        valid time's truth is uploaded and the state is scored where it lies in HBM: no forecast state goes to the host.  ``truth``:
        None = the model's own kind of data source at the valid times; or any object with ``channel_names`` and ``[time]``; or a
        (time, channel, lat, lon) DataArray / saved forecast.  ``climatology``: the same forms, or one (channel, lat, lon) array for every
        lead time.  Channels present in both forecast and truth are scored.  Returns ``verify.Scores``; ``save=True`` writes
        ``{model}-scores.json`` under the forecast id directory.  ``grid=`` (the forms of ``regrid_forecast``) scores on that target
        grid: forecast and truth, both on the model's grid, are regridded by ``regrid_method`` on the device and scored with the target's
        area weights; the scores' JSON then carries the grid's label.  ``events={channel: [thresholds]}`` also verifies the events "above
        the threshold" (skyrim_amd/events.py): the 2 x 2 table with POD, FAR, CSI, ETS and frequency bias, the Brier score
        and, over the radii ``neighbourhoods_km``, the fractions skill score, in ``Scores.events``."""
        from ... import verify
        extra = {} if grid is None else dict(grid=grid, regrid_method=regrid_method)
        if events is not None:
            extra.update(events=events, neighbourhoods_km=neighbourhoods_km)
        return verify.verify_model(self, start_time, n_steps=n_steps, truth=truth, climatology=climatology, channels=channels, save=save,
                                   save_config=save_config, **extra)

    def rollout(self, start_time: datetime.datetime, n_steps: int = 3, save: bool = True, save_config: dict | None = None,
                initial_condition=None):
        """Final prediction (2 time entries) + the paths of the per-step files.

        ``initial_condition`` (the reference's base.py:127 TODO): a saved forecast path or a DataArray whose last
        ``n_history_levels`` time entries are the state at ``start_time``; default: fetched from the data source.
        A ``save_config`` dict handed in by the caller receives the forecast id drawn here, as in the reference
        (base.py:129-130); there is no shared ``{}`` default, so an id never leaks from one call into the next."""
        cfg = save_config_with_id(save_config)
        pred, pending = initial_condition, []
        source = "file" if initial_condition is not None else self.source_label
        # Step k's file is written by a worker thread while the next steps run (the reference writes 573 MB synchronously between two
        # steps, base.py:134-143).  netCDF targets are one independent file per step, so up to SAVE_WORKERS of them are written at once:
        # the page cache takes ONE file's bytes at ~6 GB/s however many threads push them (buffered writes serialise on the inode,
        # tools/predict_cost.py), different files do not share that lock.  zarr appends to one store and keeps a single worker, in step
        # order.  At most ``workers + 1`` predictions wait for the disk, so a slow target throttles the rollout instead of filling host
        # memory.  Same files, same paths, returned in step order.  Divergences from the reference's serial loop, both opt-out: a
        # user-supplied ``save_config["mapping_func"]`` runs on the save threads, several at once (SKYRIM_SAVE_WORKERS=1 restores one file
        # at a time, in step order); once a step's write has failed no further step is submitted, but writes already running finish.
        workers = 1
        netcdf_local = save and (cfg.get("file_type") or "netcdf") == "netcdf" and "://" not in str(cfg.get("output_dir", ""))
        if netcdf_local:
            workers = max(1, int(os.environ.get("SKYRIM_SAVE_WORKERS", SAVE_WORKERS)))
        pool = ThreadPoolExecutor(max_workers=workers, thread_name_prefix="skyrim-save") if save else None
        # netCDF-3 holds big-endian floats.  When the file is the prediction as delivered (no mapping_func, no channel filter) its bytes
        # are produced in HBM and copied to the host as they will lie in the file (skyrim_amd/deliver.py): the save threads only pwrite.
        # Intermediate steps bring ONLY that image over PCIe -- the next step reads the state from HBM, nobody reads their ``values``
        # (which would be filled from the image on demand); the last step, returned to the caller, brings both.
        own_step = type(self).predict_one_step is GlobalModel.predict_one_step       # (an overriding subclass is called as the reference would)
        image = netcdf_local and cfg.get("mapping_func") is None and not cfg.get("filter_vars") and own_step
        # The loop never waits for the GPU: a step's non-finite check is read with its copy to the host -- by the save thread, whose
        # exception stops the rollout below, or at the end of the rollout -- instead of between two steps, where the host would sit
        # out every step before queueing the next (17.4 -> 14.6 ms per step at 721x1440, the engine's own pace).
        ahead = []
        try:
            for n in range(n_steps):
                if own_step:
                    last = n == n_steps - 1
                    deliver = ("both" if last else "be") if image else (None if last or save else "skip")
                    pred = self._step_delivering(start_time, pred, deliver, defer_check=True)
                    ahead.append(self._mark_step())
                    if len(ahead) > STEPS_AHEAD:                   # the host queues at most STEPS_AHEAD steps in front of the GPU (each holds its output buffer)
                        mark = ahead.pop(0)
                        if mark is not None:
                            mark.synchronize()
                else:
                    pred = self.predict_one_step(start_time, initial_condition=pred)
                pred_time = start_time + self.time_step
                if save:
                    failed = next((f for f in pending if f.done() and f.exception() is not None), None)
                    if failed is not None:
                        failed.result()                            # a writer failed: stop the rollout here instead of writing later steps
                    pending.append(pool.submit(save_forecast, pred, self.model_name, start_time, pred_time, source, config=cfg))
                    if len(pending) > workers + 1:
                        pending[-(workers + 2)].result()
                start_time, source = pred_time, "file"
                logger.info(f"Rollout step {n + 1}/{n_steps} completed")
            output_paths = [f.result() for f in pending]         # re-raises a writer's exception here, in step order
            if own_step and n_steps > 0 and isinstance(pred, DataArray):
                pred.values                                      # the last state's copy and check: a rollout returns numbers that passed it
        finally:
            if pool is not None:
                pool.shutdown(wait=True)
        return pred, output_paths


class EngineModel(GlobalModel):
    """A wrapper whose model is a HIP-engine TimeLoop: ``timeloop`` names its class as ``"module:Class"`` under this package (imported
    when the model is built), the keyword arguments beyond the reference's signature go to it, and what the reference reads off the model
    is passed through."""

    model_name = ""
    timeloop = ""

    def __init__(self, *args, cfg=None, device="cuda:0", params=None, **kwargs):
        # extras beyond the reference's signature (all optional): network configuration, device, parameter dict
        self._engine_kw = dict(cfg=cfg, device=device, params=params)
        super().__init__(self.model_name, *args, **kwargs)

    def build_model(self):
        import importlib
        module, name = self.timeloop.split(":")
        return getattr(importlib.import_module(f"...{module}", __package__), name)(**self._engine_kw)

    @property
    def device(self):
        return self.model.device

    @property
    def time_step(self):
        return self.model.time_step

    @property
    def in_channel_names(self):
        return self.model.in_channel_names

    @property
    def out_channel_names(self):
        return self.model.out_channel_names


def _axis_index(axis: np.ndarray, x: float) -> tuple[int, bool]:
    """(index of the axis value nearest to x, whether it is an exact hit).  Uniform axes (lat 90..-90, lon 0..359.75) are
    inverted arithmetically; anything else falls back to a linear scan."""
    n = axis.shape[0]
    if n > 1:
        step = (float(axis[-1]) - float(axis[0])) / (n - 1)
        if step != 0.0 and np.allclose(np.diff(axis), step, rtol=0, atol=abs(step) * 1e-6):
            i = int(min(max(round((x - float(axis[0])) / step), 0), n - 1))
            return i, bool(axis[i] == x)
    i = int(np.abs(axis - x).argmin())
    return i, bool(axis[i] == x)


class GlobalPrediction:
    """A forecast result, in memory or on disk, with point / wind accessors (reference base.py:149-274)."""

    filepath = None
    prediction = None

    def __init__(self, source, model_name: str = ""):
        self.model = model_name
        if isinstance(source, DataArray):
            data, self.filepath = source, None
        elif isinstance(source, (str, Path)):
            self.filepath = Path(source)
            data = open_dataarray(self.filepath)
        else:
            raise ValueError("Invalid source type.")
        self.prediction = data.squeeze()          # size-1 dims dropped, as the reference does

    # ---- what the array carries ----------------------------------------- #
    @property
    def coords(self):
        return self.prediction.coords

    @property
    def size(self):
        return self.prediction.size

    @property
    def channels(self):
        return self.prediction.channel

    def __repr__(self) -> str:
        where = self.filepath or f"{type(self.prediction).__name__} with shape {self.prediction.shape}"
        return f"GlobalPrediction(model={self.model},source={where})"

    def _need(self, channel: str):
        assert channel in self.channels, f"Variable {channel} not found in dataset."

    # ---- sub-arrays -------------------------------------------------------- #
    def slice(self, lat=None, lon=None, channel=None, n_step=None):
        """Sub-array over whichever of (lat range, lon range, one channel, time positions) are given."""
        out = self.prediction
        if channel is not None:
            self._need(channel)
            out = out.sel(channel=channel)
        for dim, rng in (("lat", lat), ("lon", lon)):
            if rng:
                out = out.sel(**{dim: rng})
        if n_step and "time" in out.dims:
            out = out.isel(time=n_step)
        return out

    # ---- point values --------------------------------------------------------- #
    def point(self, lat: float, lon: float, channel: str, n_step=1):
        """Value of ``channel`` at the grid cell nearest to (lat, lon); negative longitudes wrap to [0, 360)."""
        lon = lon + 360 if lon < 0 else lon
        self._need(channel)
        p = self.prediction
        i, hit_lat = _axis_index(p._coords["lat"], lat)
        j, hit_lon = _axis_index(p._coords["lon"], lon)
        if not (hit_lat and hit_lon):
            logger.warning(f"Exact coordinates not found. Using nearest values: Lat {p._coords['lat'][i]}, Lon {p._coords['lon'][j]}")
        index = []
        for dim in p.dims:
            if dim == "lat":
                index.append(i)
            elif dim == "lon":
                index.append(j)
            elif dim == "channel":
                index.append(p._coords["channel"].tolist().index(channel))
            elif dim == "time":
                index.append(n_step)
            else:
                index.append(slice(None))
        return p.values[tuple(index)].item()

    def point_wind_uv(self, lat: float, lon: float, pressure_level: int = 1000, n_step=1):
        return tuple(self.point(lat=lat, lon=lon, channel=f"{c}{pressure_level}", n_step=n_step) for c in "uv")

    def wind_speed(self, lat: float, lon: float, pressure_level: int, n_step=1):
        """|(u, v)| at a pressure level in hPa."""
        u, v = self.point_wind_uv(lat, lon, pressure_level, n_step)
        return float(np.hypot(u, v))

    def surface_wind_speed(self, lat: float, lon: float, n_step=1):
        return self.wind_speed(lat, lon, pressure_level=1000, n_step=n_step)

    def wind_speed_field(self, pressure_level: int = 1000, n_step=1, device=None):
        """Whole-grid |(u, v)| of one time entry (lat, lon).  With ``device`` (e.g. the model's GPU) the reduction runs there
        through torch; the point accessors above are the reference's surface, this is the field form of the same quantity."""
        u = self.slice(channel=f"u{pressure_level}").isel(time=n_step).values
        v = self.slice(channel=f"v{pressure_level}").isel(time=n_step).values
        if device is None:
            return np.hypot(u, v)
        import torch
        return torch.hypot(torch.as_tensor(u, device=device), torch.as_tensor(v, device=device))


class GlobalPredictionRollout:
    """A list of per-step predictions (paths or arrays) queried together (reference base.py:277-303)."""

    def __init__(self, rollout: list):
        self.rollout = [GlobalPrediction(source) for source in rollout]
        self.time_steps = [r.prediction.time.values[-1] for r in self.rollout]

    def __repr__(self):
        return f"<GlobalPredictionRollout with {len(self.rollout)} predictions, last times: {self.time_steps}>"

    def wind_speed(self, lat: float, lon: float, pressure_level: int, n_step=1):
        return [pred.wind_speed(lat, lon, pressure_level, n_step) for pred in self.rollout]

    def surface_wind_speed(self, lat: float, lon: float, n_step=1):
        return self.wind_speed(lat, lon, pressure_level=1000, n_step=n_step)
