"""Forecast verification on the device (include/skyrim_score.h): RMSE, ACC, fair CRPS, spread / skill and the rank
histogram of a forecast or an ensemble against a truth state, made where the states lie in HBM.

Three layers:

* the binding of libskyrim_score.so (``SPEC``, ``load_library``, ``score``); the same call is ``torch.ops.skyrim_hip.score_fields``;
* ``area_weights`` and ``Scores`` -- the latitude weights and the labelled table the host forms from the kernel's per-channel sums;
* threshold events (Brier, reliability, ROC, contingency scores, FSS) are skyrim_amd/events.py; ``LeadScorer(events=...)`` runs them;
* the drivers: ``verify_model`` (``GlobalModel.verify``), ``LeadScorer`` (what ``ensemble.run`` calls at every lead time with
  ``scores=True``) and ``score_prediction`` for forecasts that are already on disk.
"""
from __future__ import annotations

import ctypes
import datetime
import json
import math
import os
from pathlib import Path

import numpy as np
import torch

from . import native
from .common import finish as _finish, iso as _iso, world_size as _world_size
from .leads import open_saved, require_gpu, run_model
from .members import member_count, member_set

MAX_MEMBERS = 64                                                # include/skyrim_score.h SKSCORE_MAX_MEMBERS
DET, VAR, CRPS, ACC, RANK = 1, 2, 4, 8, 16                      # SKSCORE_DET ...
SLOTS = ("bias", "mae", "mse", "var", "crps", "abs", "pair", "fa", "ff", "aa")      # SKSCORE_BIAS ... SKSCORE_AA
PARTIALS = 9
METRICS = ("bias", "mae", "rmse", "acc", "crps", "spread", "ssr")
DEFAULT_CHANNELS = ("z500", "t850", "t2m", "u10m")
_P = ctypes.c_void_p


class ScoreDesc(ctypes.Structure):
    """skscore_desc."""
    _fields_ = [("members", _P), ("M", ctypes.c_int), ("member_align", ctypes.c_int), ("truth", _P), ("clim", _P),
                ("C", ctypes.c_int), ("H", ctypes.c_int), ("W", ctypes.c_int), ("c0", ctypes.c_int), ("nc", ctypes.c_int),
                ("lat_weight", _P), ("flags", ctypes.c_int), ("out", _P), ("counts", _P), ("workspace", _P),
                ("workspace_bytes", ctypes.c_size_t)]


SPEC = native.Spec("skyrim_score", "SKYRIM_SCORE_LIB", "skscore", 1, {          # include/skyrim_score.h SKSCORE_ABI_VERSION
    "skscore_abi_version": (ctypes.c_int, []),
    "skscore_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "skscore_run": (ctypes.c_int, [ctypes.POINTER(ScoreDesc), _P]),
}, " -- forecast scores have no torch fallback")
EXPORTS, ABI_VERSION = SPEC.exports, SPEC.abi

_lib = None


def load_library() -> ctypes.CDLL:
    """libskyrim_score.so (built in-tree by ``__graft_entry__.build()`` / ``make -C skyrim_amd/csrc``)."""
    global _lib
    if _lib is None:
        _lib = native.load(SPEC)
    return _lib


def score(members, table: torch.Tensor, truth: torch.Tensor, weights: torch.Tensor, out, workspace: torch.Tensor, flags: int,
          clim=None, counts=None, c0: int = 0, nc: int | None = None) -> None:
    """One ``skscore_run``: the M ``members`` (equal-shaped contiguous float32 (C, H, W) device tensors; ``table`` =
    ``ensemble.member_table(members)``) against ``truth`` over the channels [c0, c0 + nc).  ``weights``: H float64; ``out``: float64
    (nc, 10), slots ``SLOTS`` (only those of the groups in ``flags`` are written); ``counts``: int32 (nc, H, M + 1) with RANK;
    ``workspace``: float64, at least C * H * 9 elements.  Queued on torch's current stream.

    The members themselves are checked here; the CONTENTS of ``table`` (device memory) are not read back and are trusted to be the
    addresses of ``members`` in order, as in ``ensemble.stats``: build it with ``member_table`` from the same list."""
    member_count(members, "score_fields", MAX_MEMBERS)
    if truth.dim() != 3:
        raise ValueError("score_fields: states are (C, H, W)")
    C, H, W = truth.shape
    nc = C - c0 if nc is None else nc
    d = ScoreDesc()
    M, dev, align = member_set(members, table, "score_fields", MAX_MEMBERS, ndim=None, same="numel", dev=truth.device)
    if members[0].numel() != truth.numel():
        raise ValueError(f"score_fields: a member holds {members[0].numel()} elements, the truth {truth.numel()}")
    if not (0 <= c0 and 0 <= nc and c0 + nc <= C) or flags <= 0 or flags & ~31:
        raise ValueError("score_fields: a channel range inside the states and at least one group of outputs")
    d.members, d.M, d.member_align, d.truth = table.data_ptr(), M, align, native.tensor_ptr(truth, "score_fields: truth", torch.float32, dev)
    d.C, d.H, d.W, d.c0, d.nc, d.flags = C, H, W, c0, nc, flags
    d.lat_weight = native.tensor_ptr(weights, "score_fields: weights", torch.float64, dev)
    if weights.numel() != H:
        raise ValueError(f"score_fields: {weights.numel()} latitude weights for {H} rows")
    if flags & ACC:
        if clim is None or clim.shape != truth.shape:
            raise ValueError("score_fields: the ACC sums need a climatology of the truth's shape")
        d.clim = native.tensor_ptr(clim, "score_fields: clim", torch.float32, dev)
    if flags & RANK:
        d.counts = native.tensor_ptr(counts, "score_fields: counts", torch.int32, dev)
        if counts.numel() != nc * H * (M + 1):
            raise ValueError(f"score_fields: counts must hold nc * H * (M + 1) = {nc * H * (M + 1)} int32")
    if flags & ~RANK:
        d.out = native.tensor_ptr(out, "score_fields: out", torch.float64, dev)
        if out.numel() != nc * len(SLOTS):
            raise ValueError(f"score_fields: out must hold nc * {len(SLOTS)} float64")
    lib = load_library()
    need = lib.skscore_workspace_bytes(C, H, M, flags)
    d.workspace, d.workspace_bytes = native.tensor_ptr(workspace, "score_fields: workspace", torch.float64, dev), workspace.numel() * 8
    if d.workspace_bytes < need:
        raise ValueError(f"score_fields: the workspace holds {workspace.numel() * 8} bytes, {need} are needed")
    with torch.cuda.device(dev):
        native.check(lib.skscore_run(ctypes.byref(d), native.stream(dev)), "skscore_run", lib)


# ---- weights and the table ------------------------------------------------------------------------------------------------------------ #
def area_weights(lat) -> np.ndarray:
    """Float64 cell-area weights of a latitude axis in degrees, as WeatherBench 2 defines them: w_j = sin(ub_j) - sin(lb_j) with the
    cell bounds midway between neighbouring latitudes, the two outer bounds half a spacing beyond the axis and clipped to +-90.
    Ascending and descending axes give the same weight to the same latitude; an axis from pole to pole sums to 2."""
    lat = np.asarray(lat, np.float64)
    if lat.ndim == 1 and lat.size == 1 and np.isfinite(lat[0]) and abs(lat[0]) <= 90:
        return np.ones(1)
    return np.abs(np.diff(np.sin(np.deg2rad(cell_bounds(lat, "area_weights")))))


def cell_bounds(lat, what: str = "cell_bounds") -> np.ndarray:
    """The H + 1 float64 cell bounds, in degrees and in the order of the axis, of a latitude axis of H >= 2 rows: midway between
    neighbouring latitudes, the two outer bounds half a spacing beyond the axis and clipped to +-90.  ``area_weights`` and the
    conservative weights of skyrim_amd/regrid.py are both made from these."""
    lat = np.asarray(lat, np.float64)
    if lat.ndim != 1 or lat.size < 2 or not np.all(np.isfinite(lat)) or np.any(np.abs(lat) > 90):
        raise ValueError(f"{what}: a one-dimensional latitude axis in degrees")
    step = np.diff(lat)
    if not (np.all(step > 0) or np.all(step < 0)):
        raise ValueError(f"{what}: the latitude axis must be strictly monotonic")
    mid = (lat[:-1] + lat[1:]) / 2
    return np.clip(np.concatenate([[lat[0] - step[0] / 2], mid, [lat[-1] + step[-1] / 2]]), -90.0, 90.0)


class Scores:
    """What verification returns.  ``table``: DataArray(metric, time, channel) with the metrics of ``METRICS`` that apply (ACC needs a
    climatology; crps / spread / ssr as ensemble metrics need M > 1 -- the others are absent, not NaN-filled; at M = 1 ``crps`` is
    present and equals ``mae``).  ``sums``: DataArray(slot, time, channel), the kernel's own per-channel sums (``SLOTS``) the table is
    formed from.  ``rank_histogram``: (time, channel, rank) area-weighted frequencies that sum to 1, ``rank_counts`` the exact integers
    summed over the latitude rows; both None at M = 1.  ``events``: the ``events.EventScores`` of threshold events when they were asked
    for (``events=``), else None."""

    def __init__(self, model_name, n_members, times, channels, sums, slots, rank_counts=None, rank_histogram=None, forecast_id=""):
        from .labeled import DataArray
        self.model_name, self.n_members, self.forecast_id = model_name, int(n_members), forecast_id
        self.times, self.channels = list(times), list(channels)
        slots = list(slots)
        coords = dict(time=self.times, channel=self.channels)
        self.sums = DataArray(np.asarray(sums, np.float64), ["slot", "time", "channel"], dict(slot=slots, **coords))
        s = {k: np.asarray(sums, np.float64)[i] for i, k in enumerate(slots)}
        M, rows = self.n_members, {}
        with np.errstate(invalid="ignore", divide="ignore"):
            if "mse" in s:
                rows["bias"], rows["mae"], rows["rmse"] = s["bias"], s["mae"], np.sqrt(s["mse"])
            if "fa" in s:
                rows["acc"] = s["fa"] / np.sqrt(s["ff"] * s["aa"])
            if "crps" in s:
                rows["crps"] = s["crps"]
            if "var" in s and M > 1:
                rows["spread"] = np.sqrt(s["var"])
                if "mse" in s:
                    rows["ssr"] = math.sqrt((M + 1) / M) * rows["spread"] / rows["rmse"]
        names = [m for m in METRICS if m in rows]
        self.table = DataArray(np.stack([rows[m] for m in names]) if names else np.zeros((0, len(self.times), len(self.channels))),
                               ["metric", "time", "channel"], dict(metric=names, **coords))
        self.grid = ""                                          # the label of the target grid when the scores were made on one (regrid.py)
        self.events = None                                      # events.EventScores (skyrim_amd/events.py)
        self.rank_counts = self.rank_histogram = None
        if rank_counts is not None:
            rc = dict(rank=np.arange(M + 1), **coords)
            self.rank_counts = DataArray(np.asarray(rank_counts, np.int64), ["time", "channel", "rank"], rc)
            self.rank_histogram = DataArray(np.asarray(rank_histogram, np.float64), ["time", "channel", "rank"], rc)

    def metric(self, name: str) -> np.ndarray:
        """(time, channel) values of one metric."""
        return self.table.sel(metric=name).values

    def file_name(self) -> str:
        return f"{self.model_name}-scores.json" if self.n_members == 1 else f"{self.model_name}-ens{self.n_members}-scores.json"

    def to_json(self) -> str:
        def clean(a):                                           # JSON has no NaN: non-finite scores are written as null
            return [clean(v) for v in a] if isinstance(a, list) else (a if isinstance(a, int) or math.isfinite(a) else None)
        doc = dict(model=self.model_name, n_members=self.n_members, forecast_id=self.forecast_id, times=[_iso(t) for t in self.times],
                   channels=self.channels, slots=self.sums.slot.values.tolist(), sums=clean(self.sums.values.tolist()),
                   metrics=self.table.metric.values.tolist(), table=clean(self.table.values.tolist()))
        if self.grid:
            doc["grid"] = self.grid
        if self.rank_counts is not None:
            doc["rank_counts"] = self.rank_counts.values.tolist()
            doc["rank_histogram"] = clean(self.rank_histogram.values.tolist())
        if self.events is not None:
            doc["events"] = self.events.to_doc()
        return json.dumps(doc)

    def save(self, output_dir) -> str:
        """``{output_dir}/{forecast id}/{model}-scores.json`` (``{model}-ens{M}-scores.json`` for an ensemble); returns the path."""
        d = Path(output_dir) / self.forecast_id if self.forecast_id else Path(output_dir)
        d.mkdir(parents=True, exist_ok=True)
        path = d / self.file_name()
        path.write_text(self.to_json())
        return str(path)

    @classmethod
    def from_json(cls, text: str) -> "Scores":
        doc = json.loads(text)
        nan = lambda a: np.array([[[np.nan if v is None else v for v in r] for r in p] for p in a], np.float64)      # noqa: E731
        times = [datetime.datetime.fromisoformat(t) for t in doc["times"]]
        rc = doc.get("rank_counts")
        out = cls(doc["model"], doc["n_members"], times, doc["channels"], nan(doc["sums"]).reshape(len(doc["slots"]), len(times), -1),
                  doc["slots"], None if rc is None else np.array(rc, np.int64), None if rc is None else nan(doc["rank_histogram"]),
                  doc.get("forecast_id", ""))
        out.grid = doc.get("grid", "")
        if "events" in doc:
            from .events import EventScores
            out.events = EventScores.from_doc(doc["events"], doc["n_members"], times)
        return out

    @classmethod
    def load(cls, path) -> "Scores":
        return cls.from_json(Path(path).read_text())


# ---- truth and climatology ------------------------------------------------------------------------------------------------------------ #
class _Fields:
    """A truth or climatology in any of its accepted forms, read one valid time at a time as (channel names, (C, H, W) float32)."""

    def __init__(self, src, what: str, lat, lon):
        from .labeled import DataArray
        self.src, self.what, self.lat, self.lon = src, what, np.asarray(lat), np.asarray(lon)
        if isinstance(src, (str, os.PathLike)):
            from .labeled import open_dataarray
            self.src = src = open_dataarray(os.fspath(src))
        self.array = isinstance(src, DataArray)
        if self.array:
            if tuple(src.dims) not in (("time", "channel", "lat", "lon"), ("channel", "lat", "lon")):
                raise ValueError(f"{what}: a DataArray must have dims (time, channel, lat, lon) or (channel, lat, lon), not {tuple(src.dims)}")
            self.names = src.channel.values.tolist()
            self.flip = self._orientation(np.asarray(src._coords["lat"]), np.asarray(src._coords["lon"]))
        elif hasattr(src, "channel_names") and hasattr(src, "__getitem__"):
            self.names, self.flip = list(src.channel_names), False
        else:
            raise ValueError(f"{what}: expected a data source (channel_names, [time]), a DataArray or a saved forecast, not {type(src).__name__}")

    def _orientation(self, lat, lon) -> bool:
        """False: on the forecast's grid; True: the latitude axis runs the other way (compare core/models/ensemble._on_grid_of)."""
        if lon.shape != self.lon.shape or not np.array_equal(lon, self.lon):
            raise ValueError(f"{self.what} is on a different lon axis than the forecast")
        if lat.shape == self.lat.shape and np.array_equal(lat, self.lat):
            return False
        if lat.shape == self.lat.shape and np.array_equal(lat[::-1], self.lat):
            return True
        raise ValueError(f"{self.what} is on a different lat axis than the forecast")

    def at(self, time, names) -> np.ndarray:
        """The (len(names), H, W) float32 state at ``time``."""
        idx = [self.names.index(n) for n in names]
        if self.array:
            da = self.src
            if "time" in da.dims:
                times = np.asarray(da._coords["time"]).astype("datetime64[s]")
                hit = np.nonzero(times == np.datetime64(time, "s"))[0]
                if hit.size == 0:
                    raise ValueError(f"{self.what} holds no entry for {time}")
                a = np.asarray(da.values[int(hit[-1])])
            else:
                a = np.asarray(da.values)
        else:
            a = np.asarray(self.src[time])
            if a.shape[-2] == len(self.lat) + 1 == 721:
                a = a[..., :720, :]       # 0.25-degree source, grid without the south-pole row (datasource.get_initial_condition_for_model)
            if a.shape[-2:] != (len(self.lat), len(self.lon)):
                raise ValueError(f"{self.what} delivers {a.shape[-2:]} fields for a {len(self.lat)} x {len(self.lon)} forecast")
        a = a[idx]
        if self.flip:
            a = a[:, ::-1]
        return np.ascontiguousarray(a, dtype=np.float32)


def default_truth(gm):
    """The model's own kind of data source for its OUTPUT channels, built the way the model builds its own."""
    from .datasource import get_data_source
    return get_data_source(gm.model.out_channel_names, initial_condition_source=gm.ic_source, geom=getattr(gm.model, "geom", None),
                           state_fn=getattr(gm.model, "synthetic_state", None))


def check_request(n_members: int, out_names, channels=None) -> None:
    """The refusals that need no device."""
    if _world_size() > 1:
        raise NotImplementedError("scores are made on one GPU from members that all lie there; members sharded over the ranks of a "
                                  "process group are out of scope (DESIGN.md 18)")
    if not 1 <= int(n_members) <= MAX_MEMBERS:
        raise ValueError(f"n_members = {n_members}: 1 to {MAX_MEMBERS} members can be scored (SKSCORE_MAX_MEMBERS)")
    missing = [c for c in (channels or []) if c not in list(out_names)]
    if missing:
        raise ValueError(f"channels {missing} are not output channels of this model")


class LeadScorer:
    """Scores one lead time after the other on the device and gathers the per-channel sums.  ``names``: the forecast's channels in
    the order of its (C, H, W) states; the channels scored are those the truth (and the climatology) also holds, restricted to
    ``channels`` when given.  ``adapt``: an object with ``names(fields)`` and ``upload(fields, time, scored, dst, idx)`` that stands between the
    truth's own channels and the forecast's (``derived.TruthDeriver``: the truth of a derived field is derived from raw channels;
    ``regrid.TruthRegridder``: the truth is on another grid, named by its ``truth_grid``, and regridded to the scorer's).
    ``events``: {channel: [thresholds]} among the scored channels, and ``neighbourhoods_km``: after the scores of a lead time the events
    "above the threshold" are counted on the same states and truth (skyrim_amd/events.py) and land in ``Scores.events``."""

    def __init__(self, model_name, names, lat, lon, n_members, truth, climatology=None, channels=None, device="cuda:0", forecast_id="",
                 adapt=None, events=None, neighbourhoods_km=()):
        check_request(n_members, names, channels)
        if events is not None:
            from . import events as eventing
            events, neighbourhoods_km = eventing.check_request(names, events, neighbourhoods_km, n_members, "a channel of the forecast")
        if truth is None:
            raise ValueError("scores need a truth: a data source, a DataArray or a saved forecast")
        self.model_name, self.names, self.M, self.forecast_id = model_name, list(names), int(n_members), forecast_id
        self.lat, self.lon = np.asarray(lat, np.float64), np.asarray(lon)
        self.adapt = adapt
        tlat, tlon = getattr(adapt, "truth_grid", (lat, lon))          # (regrid.TruthRegridder reads the truth on the forecast's SOURCE grid)
        self.truth = _Fields(truth, "truth", tlat, tlon)
        self.clim = _Fields(climatology, "climatology", tlat, tlon) if climatology is not None else None
        truth_names = self.truth.names if adapt is None else adapt.names(self.truth)
        clim_names = None if self.clim is None else (self.clim.names if adapt is None else adapt.names(self.clim))
        common = [n for n in self.names if n in truth_names and (clim_names is None or n in clim_names)]
        if not common:
            raise ValueError("the forecast and the truth share no channel")
        self.scored = [n for n in common if not channels or n in channels]
        if not self.scored:
            raise ValueError(f"none of the channels {list(channels)} is in both the forecast and the truth")
        self.flags = DET | CRPS | (ACC if self.clim is not None else 0) | ((VAR | RANK) if self.M > 1 else 0)
        self.device = torch.device(device)
        self.weights_host = area_weights(self.lat)
        self.times, self.sums, self.counts = [], [], []
        self._dev = None
        self.events = None
        if events is not None:
            unscored = [c for c in events if c not in self.scored]
            if unscored:
                raise ValueError(f"events: the channels {unscored} are not among the scored channels (the truth must hold them too)")
            self.events = eventing.LeadEvents(self.names, self.lat, self.lon, self.M, events, neighbourhoods_km, device=self.device)

    def _buffers(self):
        if self._dev is None:
            C, H, W, dev = len(self.names), len(self.lat), len(self.lon), self.device
            self._dev = dict(w=torch.from_numpy(self.weights_host).to(dev), truth=torch.zeros((C, H, W), dtype=torch.float32, device=dev),
                             clim=torch.zeros((C, H, W), dtype=torch.float32, device=dev) if self.clim is not None else None,
                             out=torch.zeros((C, len(SLOTS)), dtype=torch.float64, device=dev),
                             counts=torch.zeros((C, H, self.M + 1), dtype=torch.int32, device=dev) if self.M > 1 else None,
                             ws=torch.empty(C * H * PARTIALS, dtype=torch.float64, device=dev))
            self._idx = [self.names.index(n) for n in self.scored]
            self._idx_dev = torch.tensor(self._idx, device=dev)
        return self._dev

    def truth_state(self) -> torch.Tensor:
        """The (C, H, W) device state that holds the truth of the last ``add`` in the rows of the scored channels (zeros elsewhere)."""
        return self._buffers()["truth"]

    def _upload(self, fields: _Fields, time, dst: torch.Tensor):
        if self.adapt is not None:
            return self.adapt.upload(fields, time, self.scored, dst, self._idx_dev)
        dst[self._idx_dev] = torch.from_numpy(fields.at(time, self.scored)).to(self.device)

    def add(self, time, states, table=None) -> None:
        """Score the M device states (C, H, W) of valid time ``time``: the truth (and climatology) of that time is uploaded into the
        rows of the scored channels, ONE kernel pass reads members and truth, and the per-channel sums cross to the host."""
        from .ensemble import member_table
        if len(states) != self.M:
            raise ValueError(f"{len(states)} states for a scorer of {self.M} members")
        b = self._buffers()
        self._upload(self.truth, time, b["truth"])
        if self.clim is not None:
            self._upload(self.clim, time, b["clim"])
        table = member_table(states) if table is None else table
        # one call per run of neighbouring scored channels (usually one: every channel)
        runs, start = [], 0
        for k in range(1, len(self._idx) + 1):
            if k == len(self._idx) or self._idx[k] != self._idx[k - 1] + 1:
                runs.append((self._idx[start], k - start))
                start = k
        H = len(self.lat)
        for c0, nc in runs:
            score(states, table, b["truth"], b["w"], b["out"][c0:c0 + nc], b["ws"], self.flags, clim=b["clim"],
                  counts=None if b["counts"] is None else b["counts"][c0:c0 + nc], c0=c0, nc=nc)
        self.times.append(time)
        self.sums.append(b["out"][self._idx_dev].cpu().numpy())
        if b["counts"] is not None:
            self.counts.append(b["counts"][self._idx_dev].cpu().numpy().reshape(len(self._idx), H, self.M + 1))
        if self.events is not None:
            self.events.add(states, table, b["truth"])         # one more read of the event channels of members and truth

    def result(self) -> Scores:
        wanted = [k for k, need in zip(SLOTS, (DET, DET, DET, VAR, CRPS, CRPS, CRPS, ACC, ACC, ACC)) if self.flags & need]
        sums = np.stack(self.sums) if self.sums else np.zeros((0, len(self.scored), len(SLOTS)))          # (time, channel, slot)
        sums = np.transpose(sums, (2, 0, 1))[[SLOTS.index(k) for k in wanted]]
        rc = rh = None
        if self.M > 1:
            per_row = np.stack(self.counts).astype(np.int64) if self.counts else np.zeros((0, len(self.scored), len(self.lat), self.M + 1), np.int64)
            rc = per_row.sum(axis=2)
            w = self.weights_host
            rh = np.einsum("j,tcjr->tcr", w, per_row.astype(np.float64)) / (len(self.lon) * w.sum())
        scores = Scores(self.model_name, self.M, self.times, self.scored, sums, wanted, rc, rh, self.forecast_id)
        if self.events is not None:
            scores.events = self.events.result(self.times, self.weights_host)
        return scores


def verify_model(gm, start_time: datetime.datetime, n_steps: int = 4, truth=None, climatology=None, channels=None, save: bool = False,
                 save_config: dict | None = None, grid=None, regrid_method: str = "conservative", events=None,
                 neighbourhoods_km=()) -> Scores:
    """``GlobalModel.verify`` (core/models/base.py has the user-facing description)."""
    model = gm.model
    check_request(1, model.out_channel_names, channels)
    ev = {} if events is None else dict(events=events, neighbourhoods_km=neighbourhoods_km)
    if events is not None:
        from . import events as eventing
        eventing.check_request(model.out_channel_names, events, neighbourhoods_km, 1)
    if n_steps < 0:
        raise ValueError("n_steps >= 0")
    regridder = None
    if grid is not None:                                   # score on the target grid: forecast and truth go through the same regrid kernel
        from . import regrid
        names = list(model.out_channel_names)
        regridder = regrid.LeadRegridder(names, model.grid.lat, model.grid.lon, 1, grid, regrid_method, device=model.device)
        scorer = LeadScorer(gm.model_name, names, regridder.lat_out, regridder.lon_out, 1, default_truth(gm) if truth is None else truth,
                            climatology, channels, device=model.device,
                            adapt=regrid.TruthRegridder(model.grid.lat, model.grid.lon, grid, regrid_method, device=model.device), **ev)
    else:
        scorer = LeadScorer(gm.model_name, model.out_channel_names, model.grid.lat, model.grid.lon, 1,
                            default_truth(gm) if truth is None else truth, climatology, channels, device=model.device, **ev)
    require_gpu(model.device, "verify scores the forecast with HIP kernels where it lies: the model must be on a GPU")

    def each(k, time, state):
        if regridder is None:
            scorer.add(time, [state])
        else:
            scorer.add(time, *regridder.add([state]))
    run_model(gm, start_time, n_steps, each)
    result = scorer.result()
    if regridder is not None:
        result.grid = regrid.grid_label(grid)
    return _finish(result, save, save_config)


def score_prediction(pred, truth, climatology=None, device="cuda:0", channels=None, model_name: str = "", events=None,
                     neighbourhoods_km=()) -> Scores:
    """Scores of a forecast that already exists: a ``GlobalPrediction``, a (time, channel, lat, lon) DataArray, a saved netCDF file or
    zarr store, or a list of such files (their time entries in order, duplicates of a valid time scored once).  Each time entry is
    uploaded on its own and goes through the same kernel as ``verify``; ``events`` / ``neighbourhoods_km`` as there."""
    saved = open_saved(pred, "score_prediction")
    scorer = LeadScorer(model_name or saved.model_name or "forecast", saved.names, saved.lat, saved.lon, 1, truth, climatology, channels,
                        device=device, **({} if events is None else dict(events=events, neighbourhoods_km=neighbourhoods_km)))
    require_gpu(scorer.device, "score_prediction scores with HIP kernels: it needs a GPU", present=True)
    for _, time, state in saved.states(scorer.device):
        scorer.add(time, [state])
    return scorer.result()
