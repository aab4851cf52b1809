"""The lead-time drivers of the single-forecast product routes without a GPU (skyrim_amd/leads.py): ``run_model`` delivers the leads and
leaves the model without a resident state however it ends, ``open_saved`` reads and refuses saved forecasts, the seven saved routes give
their own refusals before "needs a GPU"; with them the two save tails and the command lines' start time and step count."""
from __future__ import annotations

import datetime
import warnings
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from skyrim_amd import aggregate, common, derived, forecast, leads, points, regrid, spectra, tracks, verify
from skyrim_amd import datasource as ds
from skyrim_amd.core.models.base import GlobalPrediction
from skyrim_amd.labeled import DataArray

T0 = datetime.datetime(2024, 5, 13, 18, 0)
H6 = datetime.timedelta(hours=6)
C, H, W = 3, 4, 6


# ---- 1. the model driver ---------------------------------------------------------------------------------------------------------------- #
class _Run:
    """The generator of one ``model(time, x)``: a 4-D output first, then 3-D ones, the second of them non-contiguous; records ``close``."""

    def __init__(self, time, fail_at=None):
        self.time, self.fail_at, self.k, self.closed = time, fail_at, 0, False

    def __next__(self):
        k, self.k = self.k, self.k + 1
        if k == self.fail_at:
            raise FloatingPointError("the loop failed")
        out = torch.full((C, H, W), float(k))
        if k == 0:
            out = out[None]
        elif k == 2:
            out = torch.full((C, W, H), float(k)).transpose(1, 2)
        return self.time + k * H6, out, None

    def close(self):
        self.closed = True


class _Loop:
    def __init__(self, fail_at=None):
        self.fail_at, self.runs = fail_at, []
        self._resident_state, self._state_is_own_output = "stale", True

    def __call__(self, time, x, restart=None):
        assert self._resident_state is None, "the resident state is dropped before the loop opens"
        self.runs.append(_Run(time, self.fail_at))
        return self.runs[-1]


class _Slots:
    __slots__ = ("runs",)

    def __init__(self):
        self.runs = []

    def __call__(self, time, x, restart=None):
        self.runs.append(_Run(time))
        return self.runs[-1]


@pytest.fixture
def ic(monkeypatch):
    monkeypatch.setattr(ds, "get_initial_condition_for_model", lambda model, source, time: torch.zeros(1, 1, C, H, W))


def _left_clean(model):
    return model.runs[-1].closed and model._resident_state is None and "_state_is_own_output" not in model.__dict__


def test_run_model_delivers_every_lead_and_leaves_no_resident_state(ic):
    model, seen = _Loop(), []
    assert leads.run_model(SimpleNamespace(model=model, data_source=None), T0, 3, lambda k, t, s: seen.append((k, t, s))) is None
    assert [k for k, _, _ in seen] == [0, 1, 2, 3] and [t for _, t, _ in seen] == [T0 + k * H6 for k in range(4)]
    for k, _, s in seen:
        assert s.shape == (C, H, W) and s.is_contiguous() and bool((s == k).all())
    assert len(model.runs) == 1 and model.runs[0].k == 4 and _left_clean(model)


def test_run_model_cleans_up_when_each_raises_while_the_exception_is_held(ic):
    model = _Loop()

    def each(k, time, state):
        if k == 1:
            raise ValueError("lead 1")
    with pytest.raises(ValueError, match="lead 1") as caught:
        leads.run_model(SimpleNamespace(model=model, data_source=None), T0, 3, each)
    assert caught.value.__traceback__ is not None          # the traceback, and every frame it names, is still alive here
    assert model.runs[0].k == 2 and _left_clean(model)


def test_run_model_cleans_up_when_the_loop_raises(ic):
    model = _Loop(fail_at=2)
    with pytest.raises(FloatingPointError, match="the loop failed") as caught:
        leads.run_model(SimpleNamespace(model=model, data_source=None), T0, 3, lambda k, t, s: None)
    assert caught.value is not None and _left_clean(model)


def test_run_model_opens_and_clears_nothing_when_the_initial_condition_fails(monkeypatch):
    def refuse(model, source, time):
        raise LookupError("no analysis")
    monkeypatch.setattr(ds, "get_initial_condition_for_model", refuse)
    model = _Loop()
    with pytest.raises(LookupError):
        leads.run_model(SimpleNamespace(model=model, data_source=None), T0, 1, lambda k, t, s: None)
    assert model.runs == [] and model._resident_state == "stale" and model._state_is_own_output is True


def test_run_model_passes_a_model_without_dict_through(ic):
    model, seen = _Slots(), []
    leads.run_model(SimpleNamespace(model=model, data_source=None), T0, 1, lambda k, t, s: seen.append(k))
    assert seen == [0, 1] and model.runs[0].closed


def test_require_gpu():
    with pytest.raises(RuntimeError, match="^my own sentence$"):
        leads.require_gpu("cpu", "my own sentence")
    leads.require_gpu("cuda:0", "unused")                  # a model's device: its type decides
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="^it needs a GPU$"):
            leads.require_gpu("cuda:0", "it needs a GPU", present=True)


# ---- 2. the saved-forecast reader ------------------------------------------------------------------------------------------------------- #
LAT, LON = np.linspace(60, -60, 5), np.arange(8) * 45.0
NAMES = ["u10m", "v10m", "t2m", "msl", "u850", "v850"]


def _forecast(first=0, n=3, names=NAMES, lat=LAT, lon=LON):
    values = np.arange(first, first + n, dtype=np.float32)[:, None, None, None] + np.zeros((n, len(names), len(lat), len(lon)), np.float32)
    return DataArray(values, ["time", "channel", "lat", "lon"],
                     dict(time=[T0 + (first + k) * H6 for k in range(n)], channel=list(names), lat=lat, lon=lon))


def test_open_saved_reads_arrays_predictions_files_and_lists(tmp_path):
    da = _forecast()
    one = leads.open_saved(da, "me")
    assert one.names == NAMES and np.array_equal(one.lat, LAT) and np.array_equal(one.lon, LON) and one.model_name == ""
    assert [e[0] for e in one.entries] == [T0, T0 + H6, T0 + 2 * H6] and [e[2] for e in one.entries] == [0, 1, 2]
    assert all(type(e[0]) is datetime.datetime and e[1] is da for e in one.entries)
    assert leads.open_saved(GlobalPrediction(da, "fuxi"), "me").model_name == "fuxi"
    path = tmp_path / "pangu__gfs__20240513_18:00__20240514_06:00.nc"
    da.to_netcdf(path)
    late = _forecast(first=2)                               # valid times 2, 3, 4: the first repeats the file's last
    both = leads.open_saved([path, late], "me")
    assert both.model_name == "pangu" and both.names == NAMES
    assert [e[0] for e in both.entries] == [T0 + k * H6 for k in range(5)] and [e[2] for e in both.entries] == [0, 1, 2, 1, 2]
    states = list(both.states("cpu"))
    assert [k for k, _, _ in states] == [0, 1, 2, 3, 4] and [t for _, t, _ in states] == [e[0] for e in both.entries]
    assert [float(s[0, 0, 0]) for _, _, s in states] == [0.0, 1.0, 2.0, 3.0, 4.0]
    assert leads.open_saved(str(path), "me").model_name == "pangu" and leads.open_saved((da,), "me").model_name == ""


def test_open_saved_refusals_need_no_gpu():
    da = _forecast()
    with pytest.raises(ValueError, match=r"^me: a forecast is a \(time, channel, lat, lon\) DataArray"):
        leads.open_saved(da.isel(time=0), "me")
    with pytest.raises(ValueError, match="^me: a forecast is a"):
        leads.open_saved(np.zeros((2, 2, 2, 2)), "me")
    for other in (_forecast(first=3, names=NAMES[::-1]), _forecast(first=3, lat=LAT + 1.0), _forecast(first=3, lon=LON + 1.0)):
        with pytest.raises(ValueError, match="^me: the files of one forecast must share channels and grid$"):
            leads.open_saved([da, other], "me")


def test_states_upload_a_copy_of_a_read_only_array():
    da = _forecast()
    da.values.flags.writeable = False
    before = da.values.copy()
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        states = [s for _, _, s in leads.open_saved(da, "me").states("cpu")]
    for k, s in enumerate(states):
        assert s.dtype == torch.float32 and s.shape == da.shape[1:] and s.is_contiguous() and np.array_equal(s.numpy(), before[k])
        s += 1.0                                            # the state is the caller's own
    assert np.array_equal(da.values, before) and not da.values.flags.writeable


POINT = [("a", 10.0, 20.0)]
COARSE = dict(lat_max=10.0, r_msl_km=6000.0)               # a tracker whose windows fit rows 30 degrees apart: the equator row, 3 x 3 points
SAVED_ROUTES = {
    "score": (lambda da: verify.score_prediction(da, da, channels=["nope"]), lambda da: verify.score_prediction(da, da)),
    "track": (lambda da: tracks.track_prediction(da, dict(capacity=0)), lambda da: tracks.track_prediction(da, COARSE)),
    "derive": (lambda da: derived.derive_prediction(da, ["nope"]), lambda da: derived.derive_prediction(da, ["ws10m"])),
    "regrid": (lambda da: regrid.regrid_prediction(da, "bogus"), lambda da: regrid.regrid_prediction(da, "60deg")),
    "aggregate": (lambda da: aggregate.aggregate_prediction(da, ["nope:max:all"]), lambda da: aggregate.aggregate_prediction(da, ["t2m:max:all"])),
    "points": (lambda da: points.extract_prediction(da, POINT, channels=["nope"]), lambda da: points.extract_prediction(da, POINT)),
    "spectra": (lambda da: spectra.spectra_prediction(da, channels=["nope"]), lambda da: spectra.spectra_prediction(da)),
}


@pytest.mark.parametrize("route", list(SAVED_ROUTES))
def test_a_saved_route_refuses_its_request_before_it_asks_for_a_gpu(route):
    bad, good = SAVED_ROUTES[route]
    da = _forecast()
    with pytest.raises(ValueError) as refusal:
        bad(da)
    assert "GPU" not in str(refusal.value) and "must share" not in str(refusal.value)
    with pytest.raises(ValueError, match="must share channels and grid"):          # raised by the reader: before the device, on every route
        good([da, _forecast(first=3, lat=LAT + 1.0)])
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="needs a GPU"):
            good(da)


# ---- 3. the save tails ------------------------------------------------------------------------------------------------------------------ #
def test_save_config_with_id():
    mine = {"output_dir": "somewhere"}
    cfg = common.save_config_with_id(mine)
    assert cfg is not mine and mine == {"output_dir": "somewhere", "forecast_id": cfg["forecast_id"]} and cfg == mine
    assert len(cfg["forecast_id"]) == 10
    given = {"forecast_id": "abc", "file_type": "zarr"}
    assert common.save_config_with_id(given) == given == {"forecast_id": "abc", "file_type": "zarr"}
    assert list(common.save_config_with_id(None)) == ["forecast_id"]
    empty = {}
    assert common.save_config_with_id(empty)["forecast_id"] == empty["forecast_id"]


@pytest.mark.parametrize("make", ["points", "spectra"])
def test_finish_saves_points_and_spectra_under_the_forecast_id(make, tmp_path):
    if make == "points":
        result = points.PointForecast.build(np.zeros((1, 2, 1, 1), np.float32), [T0, T0 + H6], ["t2m"], points.Points(POINT), "bilinear", "pangu", "")
        name = "pangu-points.json"
    else:
        result = spectra.Spectra([T0], ["t2m"], {"globe": None}, [(0, 5)], LAT, 8, 1, np.zeros((1, 1, 1, 3, spectra.n_bins(8))), "pangu", "")
        name = "pangu-spectra.json"
    assert common.finish(result, False, None) is result and not result.forecast_id and getattr(result, "path", None) is None
    cfg = {"output_dir": str(tmp_path)}
    assert common.finish(result, True, cfg) is result
    assert list(cfg) == ["output_dir", "forecast_id"] and result.forecast_id == cfg["forecast_id"]
    assert result.path == str(tmp_path / cfg["forecast_id"] / name) and (tmp_path / cfg["forecast_id"] / name).is_file()


# ---- 4. the command lines --------------------------------------------------------------------------------------------------------------- #
def test_start_time_and_steps_of_the_command_lines():
    assert forecast.start_time_of("20240513", "1800") == T0
    assert forecast.start_time_of("20231231", "0630") == datetime.datetime(2023, 12, 31, 6, 30)
    six, day = (SimpleNamespace(model=SimpleNamespace(time_step=datetime.timedelta(hours=h))) for h in (6, 24))
    assert [forecast.steps_for(six, h) for h in (0, 6, 11, 12, 48)] == [1, 1, 1, 2, 8]        # clipped down to 6 h, at least 6 h
    assert [forecast.steps_for(day, h) for h in (6, 23, 24, 47, 48, 120)] == [0, 0, 1, 1, 2, 5]
    assert all(type(forecast.steps_for(m, 24)) is int for m in (six, day))
