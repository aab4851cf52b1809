"""The two drivers of the single-forecast product routes: every product that reads ONE forecast lead by lead (verify, tracks, derived,
regrid, aggregate, points, spectra) gets its (C, H, W) device states from here -- ``run_model`` steps a model, ``open_saved`` reads a
forecast that already exists -- and keeps only its own request checks, its ``Lead*`` object and its result.

``run_model`` owns the invariant that protects the plain-forecast hot path: a product's loop is not a state a later ``rollout`` continues
from, so the model's resident state (core/models/utils.py ``ResidentState``) is dropped before the loop opens, and dropped again, with
the loop closed, before the driver returns or raises."""
from __future__ import annotations

import datetime
import os
from dataclasses import dataclass
from pathlib import Path

import numpy as np


def require_gpu(device, message: str, present: bool = False) -> None:
    """RuntimeError(``message``) unless ``device`` is a GPU -- ``present``: and this process sees one (a saved route's device is only a name)."""
    import torch
    if torch.device(device).type != "cuda" or (present and not torch.cuda.is_available()):
        raise RuntimeError(message)


def forget_resident(model, closed: bool = True) -> None:
    """Drop the device state ``run_basic_inference`` would continue from; ``closed`` (a loop of ``model`` has just ended): and the mark
    it leaves for the loop it opens."""
    if hasattr(model, "__dict__"):
        model._resident_state = None
        if closed:
            model.__dict__.pop("_state_is_own_output", None)


def run_model(gm, start_time: datetime.datetime, n_steps: int, each) -> None:
    """Step ``gm.model`` from its initial condition at ``start_time`` and call ``each(k, time, state)`` for the leads k = 0 .. n_steps;
    ``state`` is the contiguous (C, H, W) device tensor of that lead.  The loop is closed and the resident state forgotten when this
    returns or raises, also when ``each`` raises (a call-back, not a generator: nothing here waits for a collection)."""
    from .datasource import get_initial_condition_for_model
    model = gm.model
    x0 = get_initial_condition_for_model(model, gm.data_source, start_time)
    forget_resident(model, closed=False)                   # the loop below is not a state a later rollout continues from
    loop = model(start_time, x0)
    try:
        for k in range(n_steps + 1):
            time, out, _ = next(loop)
            each(k, time, (out[0] if out.dim() == 4 else out).contiguous())
            del out
    finally:
        loop.close()
        forget_resident(model)


@dataclass
class SavedForecast:
    """A forecast that already exists.  ``names``, ``lat``, ``lon``: of its first file; ``model_name``: of a ``GlobalPrediction``, else
    of a file named ``{model}__...``, else ""; ``entries``: (valid time, DataArray, index) of its unique valid times, in order."""
    names: list
    lat: np.ndarray
    lon: np.ndarray
    model_name: str
    entries: list

    def states(self, device):
        """(k, time, state) per entry: the (C, H, W) float32 state on ``device``, uploaded through a C-order copy (the file's array may
        be read-only, and is never aliased)."""
        import torch
        for k, (time, da, i) in enumerate(self.entries):
            yield k, time, torch.from_numpy(np.array(da.values[i], dtype=np.float32, order="C")).to(device)


def open_saved(pred, who: str) -> SavedForecast:
    """``pred``: a ``GlobalPrediction``, a (time, channel, lat, lon) DataArray, a saved netCDF file or zarr store, or a list of these
    (their time entries in order, a repeated valid time taken once).  ``who`` names the caller in the refusals."""
    from .labeled import DataArray, open_dataarray
    arrays, model_name = [], ""
    for p in list(pred) if isinstance(pred, (list, tuple)) else [pred]:
        if hasattr(p, "prediction") and isinstance(getattr(p, "prediction"), DataArray):
            model_name = model_name or (p.model if isinstance(p.model, str) else "")
            p = p.prediction
        elif isinstance(p, (str, os.PathLike)):
            model_name = model_name or Path(p).name.split("__")[0].split(".")[0]
            p = open_dataarray(os.fspath(p))
        if not isinstance(p, DataArray) or tuple(p.dims) != ("time", "channel", "lat", "lon"):
            raise ValueError(f"{who}: a forecast is a (time, channel, lat, lon) DataArray, a GlobalPrediction holding one, or a saved file / store")
        arrays.append(p)
    names = arrays[0].channel.values.tolist()
    lat, lon = np.asarray(arrays[0]._coords["lat"]), np.asarray(arrays[0]._coords["lon"])
    seen, entries = set(), []
    for da in arrays:
        if da.channel.values.tolist() != names or not np.array_equal(da._coords["lat"], lat) or not np.array_equal(da._coords["lon"], lon):
            raise ValueError(f"{who}: the files of one forecast must share channels and grid")
        for i, t in enumerate(np.asarray(da._coords["time"]).astype("datetime64[s]")):
            if t not in seen:
                seen.add(t)
                entries.append((t.astype(datetime.datetime), da, i))
    return SavedForecast(names, lat, lon, model_name, entries)
