"""``Skyrim`` facade -- /root/reference/skyrim/core/skyrim.py:12-95, same constructor, ``predict``,
``forecast`` and ``list_available_models``."""
from __future__ import annotations

import datetime
import logging

from .models import MODELS
from .models.base import GlobalModel, GlobalPrediction, adjust_lead_time
from .models.ensemble import GlobalEnsemble

logger = logging.getLogger("skyrim_amd")


class Skyrim:
    def __init__(self, *model_names: str, ic_source: str = "cds"):
        missing_names = [name for name in model_names if name not in MODELS]
        if missing_names:
            raise ValueError(f"Invalid model name(s): {missing_names}")
        self.model_names = model_names
        self.ic_source = ic_source
        self.model: GlobalEnsemble | GlobalModel
        if len(model_names) > 1:
            self.model = GlobalEnsemble(model_names, ic_source=ic_source)
        else:
            self.model = MODELS[model_names[0]](ic_source=ic_source)

    def __repr__(self) -> str:
        return f"Skyrim(models={self.model_names},ic={self.ic_source})"

    @staticmethod
    def list_available_models():
        return list(MODELS.keys())

    def forecast(self, start_time: datetime.datetime, n_steps: int = 4, channels: list | None = None):
        """Full concatenated forecast (all steps from the IC on) for the channels of interest."""
        start_time = start_time.replace(second=0, microsecond=0)
        return self.model.forecast(start_time=start_time, n_steps=n_steps, channels=channels or [])

    def ensemble_forecast(self, start_time: datetime.datetime, n_steps: int = 4, n_members: int = 10, **kwargs):
        """Perturbed-initial-condition ensemble of the single model (``GlobalModel.ensemble_forecast`` has the arguments): the ensemble
        mean / spread / min / max, exceedance fractions and quantiles at every lead time, as an ``EnsembleForecast``."""
        start_time = start_time.replace(second=0, microsecond=0)
        return self.model.ensemble_forecast(start_time, n_steps=n_steps, n_members=n_members, **kwargs)

    @staticmethod
    def open_archive(directory):
        """The members ``ensemble_forecast(..., archive={...})`` wrote under ``directory`` as an ``archive.MemberArchive``: ``info()``,
        ``member(m, k)``, ``states(k, device)`` and ``replay(**request)``, which makes the products of ``ensemble_forecast`` from the
        files without running the model."""
        from .. import archive
        return archive.open(directory)

    def verify(self, start_time: datetime.datetime, n_steps: int = 4, **kwargs):
        """Scores of the single model's forecast against a truth at every lead time (``GlobalModel.verify`` has the arguments):
        bias, MAE, RMSE, CRPS and ACC per channel as a ``verify.Scores``.  ``ensemble_forecast(..., scores=True)`` scores an ensemble."""
        start_time = start_time.replace(second=0, microsecond=0)
        return self.model.verify(start_time, n_steps=n_steps, **kwargs)

    def spectrum_forecast(self, start_time: datetime.datetime, n_steps: int = 4, **kwargs):
        """Zonal power spectra of the single model's forecast at every lead time (``GlobalModel.spectrum_forecast`` has the arguments)
        as a ``spectra.Spectra``.  ``ensemble_forecast(..., spectra={...})`` makes those of an ensemble."""
        start_time = start_time.replace(second=0, microsecond=0)
        return self.model.spectrum_forecast(start_time, n_steps=n_steps, **kwargs)

    @staticmethod
    def spectra_prediction(pred, truth=None, device="cuda:0", **kwargs):
        """Zonal power spectra of a forecast that is already in memory or on disk (``spectra.spectra_prediction``)."""
        from .. import spectra
        return spectra.spectra_prediction(pred, truth=truth, device=device, **kwargs)

    @staticmethod
    def score_prediction(pred, truth, climatology=None, device="cuda:0", **kwargs):
        """Scores of a forecast that is already in memory or on disk (``verify.score_prediction``)."""
        from .. import verify
        return verify.score_prediction(pred, truth, climatology=climatology, device=device, **kwargs)

    def track_cyclones(self, start_time: datetime.datetime, n_steps: int = 4, **kwargs):
        """Cyclone tracks of the single model's forecast (``GlobalModel.track_cyclones`` has the arguments) as a ``tracks.Tracks``.
        ``ensemble_forecast(..., tracks=True)`` tracks every member of an ensemble."""
        start_time = start_time.replace(second=0, microsecond=0)
        return self.model.track_cyclones(start_time, n_steps=n_steps, **kwargs)

    def object_forecast(self, start_time: datetime.datetime, n_steps: int = 4, objects=None, **kwargs):
        """Weather objects -- the contiguous regions where a field is beyond a threshold: atmospheric rivers, gale areas, cold pools -- of
        the single model's forecast as an ``objects.Objects`` (``GlobalModel.object_forecast`` has the arguments).
        ``ensemble_forecast(..., objects={...})`` finds them in every member and gives their probability."""
        start_time = start_time.replace(second=0, microsecond=0)
        return self.model.object_forecast(start_time, n_steps=n_steps, objects=objects, **kwargs)

    @staticmethod
    def objects_prediction(pred, objects, device="cuda:0", **kwargs):
        """Weather objects of a forecast that is already in memory or on disk (``objects.objects_prediction``)."""
        from .. import objects as objecting
        return objecting.objects_prediction(pred, objects, device=device, **kwargs)

    def extremes_forecast(self, start_time: datetime.datetime, n_steps: int = 4, extremes=None, **kwargs):
        """The single model's forecast against a quantile climate -- the Extreme Forecast Index and the odds of leaving a climate
        percentile -- as an ``extremes.Extremes`` (``GlobalModel.extremes_forecast`` has the arguments).
        ``ensemble_forecast(..., extremes={...})`` compares every member and adds the Shift of Tails."""
        start_time = start_time.replace(second=0, microsecond=0)
        return self.model.extremes_forecast(start_time, n_steps=n_steps, extremes=extremes, **kwargs)

    @staticmethod
    def extremes_prediction(pred, extremes, derived=None, device="cuda:0"):
        """The same for a forecast that is already in memory or on disk (``extremes.extremes_prediction``)."""
        from .. import extremes as extreming
        return extreming.extremes_prediction(pred, extremes, derived=derived, device=device)

    def derive_fields(self, start_time: datetime.datetime, n_steps: int = 4, fields=(), **kwargs):
        """Derived fields (wind speed, thickness, vorticity, divergence, vapour transport) of the single model's forecast as a
        DataArray(time, channel=fields, lat, lon) (``GlobalModel.derive_fields`` has the arguments).
        ``ensemble_forecast(..., derived=[...])`` gives their ensemble products."""
        start_time = start_time.replace(second=0, microsecond=0)
        return self.model.derive_fields(start_time, n_steps=n_steps, fields=fields, **kwargs)

    def aggregate_forecast(self, start_time: datetime.datetime, n_steps: int = 4, aggregates=(), **kwargs):
        """Time-window aggregates (daily maximum, mean, hours above a threshold, time of the peak ...) of the single model's forecast as
        {window label: DataArray(time = window ends, channel = aggregates, lat, lon)} (``GlobalModel.aggregate_forecast`` has the
        arguments).  ``ensemble_forecast(..., aggregates=[...])`` gives their ensemble products."""
        start_time = start_time.replace(second=0, microsecond=0)
        return self.model.aggregate_forecast(start_time, n_steps=n_steps, aggregates=aggregates, **kwargs)

    @staticmethod
    def aggregate_prediction(pred, aggregates, derived=None, device="cuda:0"):
        """Time-window aggregates of a forecast that is already in memory or on disk (``aggregate.aggregate_prediction``)."""
        from .. import aggregate
        return aggregate.aggregate_prediction(pred, aggregates, derived=derived, device=device)

    def neighbourhood_forecast(self, start_time: datetime.datetime, n_steps: int = 4, neighbourhood=(), derived=None, **kwargs):
        """Neighbourhood fields (maximum, minimum, mean, fraction above a threshold within R km of every grid point) of the single model's
        forecast as a DataArray(time, channel = ``ws10m_max_100km`` ..., lat, lon) (``GlobalModel.neighbourhood_forecast`` has the
        arguments).  ``ensemble_forecast(..., neighbourhood=[...])`` gives their ensemble products."""
        start_time = start_time.replace(second=0, microsecond=0)
        return self.model.neighbourhood_forecast(start_time, n_steps=n_steps, neighbourhood=neighbourhood, derived=derived, **kwargs)

    @staticmethod
    def neighbourhood_prediction(pred, neighbourhood, derived=None, device="cuda:0"):
        """Neighbourhood fields of a forecast that is already in memory or on disk (``neighbourhood.neighbourhood_prediction``)."""
        from .. import neighbourhood as nbr
        return nbr.neighbourhood_prediction(pred, neighbourhood, derived=derived, device=device)

    def point_forecast(self, start_time: datetime.datetime, n_steps: int = 4, points=None, **kwargs):
        """The single model's forecast at scattered places -- stations, cities, wind farms -- as a ``points.PointForecast``
        (``GlobalModel.point_forecast`` has the arguments).  ``ensemble_forecast(..., points=...)`` gives every member there."""
        start_time = start_time.replace(second=0, microsecond=0)
        return self.model.point_forecast(start_time, n_steps=n_steps, points=points, **kwargs)

    def regrid_forecast(self, start_time: datetime.datetime, n_steps: int = 4, grid="1.5deg", method: str = "conservative", **kwargs):
        """The single model's forecast on another latitude-longitude grid -- "1.5deg", (lat, lon) arrays or a region -- as a
        DataArray(time, channel, lat, lon) (``GlobalModel.regrid_forecast`` has the arguments).
        ``ensemble_forecast(..., grid=...)`` gives the ensemble products on it, ``verify(..., grid=...)`` the scores."""
        start_time = start_time.replace(second=0, microsecond=0)
        return self.model.regrid_forecast(start_time, n_steps=n_steps, grid=grid, method=method, **kwargs)

    @staticmethod
    def regrid_prediction(pred, grid, method="conservative", device="cuda:0", **kwargs):
        """A forecast that is already in memory or on disk, on another grid (``regrid.regrid_prediction``)."""
        from .. import regrid
        return regrid.regrid_prediction(pred, grid, method, device=device, **kwargs)

    @staticmethod
    def derive_prediction(pred, fields, device="cuda:0", derived_surface=None, vertical=None):
        """Derived fields of a forecast that is already in memory or on disk (``derived.derive_prediction``)."""
        from .. import derived
        return derived.derive_prediction(pred, fields, device=device, surface=derived_surface, vertical=vertical)

    @staticmethod
    def track_prediction(pred, config=None, device="cuda:0", **kwargs):
        """Cyclone tracks of a forecast that is already in memory or on disk (``tracks.track_prediction``)."""
        from .. import tracks
        return tracks.track_prediction(pred, config=config, device=device, **kwargs)

    def predict(self, date: str, time: str, lead_time: int = 6, save: bool = False, save_config: dict | None = None):
        """Predict a single lead-time snapshot, optionally saving every intermediate step.
        date: YYYYMMDD, time: HHMM, lead_time in hours (clipped down to a multiple of 6, at least 6)."""
        from ..forecast import start_time_of
        start_time = start_time_of(date, time)
        lead_time = adjust_lead_time(lead_time, step_size=6)
        step_h = self.model.time_step.total_seconds() / 3600
        n_steps = int(lead_time // step_h)
        if n_steps < 1:
            raise ValueError(f"lead time {lead_time} h is shorter than one {step_h:g}-h step of {', '.join(self.model_names)}")
        pred, output_paths = self.model.rollout(start_time=start_time, n_steps=n_steps, save=save, save_config=save_config)
        return GlobalPrediction(pred, model_name=self.model_names), output_paths
