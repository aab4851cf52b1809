"""Event verification without a GPU: the C ABI of include/skyrim_event.h (exports, argument errors, the descriptor's layout), the host's
scores against their per-point definitions, ``windows``, the JSON file, the refusals, the command line's options and the compiler's
resource report of csrc/event_ops.hip."""
from __future__ import annotations

import ctypes
import datetime
import json
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

import _event_reference as R
from skyrim_amd import events as E
from skyrim_amd import native
from skyrim_amd import verify as V

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "skyrim_event.h"
T0 = datetime.datetime(2024, 5, 13, 18, 0)
T = E.MAX_THRESHOLDS


# ---- 1. ABI --------------------------------------------------------------------------------------------------------------------------- #
def test_library_exports_every_declared_symbol():
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    syms = sorted(set(re.findall(r"\b(skevent_[a-z0-9_]+)\s*\(", text)))
    assert len(syms) == 3                                        # (that they are EXPORTS, exported, and the ABI version: tests/test_native.py)
    assert E.SPEC.stem == "skyrim_event" and E.SPEC.prefix == "skevent"
    for name, val in (("MEMBERS", E.MAX_MEMBERS), ("CHANNELS", E.MAX_CHANNELS), ("THRESHOLDS", E.MAX_THRESHOLDS), ("SCALES", E.MAX_SCALES),
                      ("WIDTH", E.MAX_WIDTH)):
        assert int(re.search(rf"SKEVENT_MAX_{name} (\d+)", text).group(1)) == val
    assert "skyrim_event" not in native.__doc__ and "event}" in native.__doc__ and "event}" in (ROOT / "skyrim_amd/csrc/Makefile").read_text()


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not installed")
def test_descriptor_layout_matches_the_header(tmp_path):
    fields = [n for n, _ in E.EventDesc._fields_]
    src = tmp_path / "layout.cpp"
    src.write_text('#include <cstdio>\n#include <cstddef>\n#include "skyrim_event.h"\nint main() {\n  printf("%zu", sizeof(skevent_desc));\n'
                   + "".join(f'  printf(" %zu", offsetof(skevent_desc, {f}));\n' for f in fields) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    r = subprocess.run(["hipcc", "-x", "c++", "-std=c++17", f"-I{ROOT / 'include'}", str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got[0] == ctypes.sizeof(E.EventDesc)
    assert got[1:] == [getattr(E.EventDesc, f).offset for f in fields]


def _desc(M=4, scales=1):
    fake = 4096                                                # never dereferenced: the argument checks come first
    d = E.EventDesc()
    d.members, d.M, d.member_align, d.truth = fake, M, 16, fake
    d.C, d.H, d.W, d.n_events, d.counts = 3, 5, 8, 2, fake
    d.channel[0], d.channel[1], d.n_thr[0], d.n_thr[1] = 2, 0, 1, 4
    d.n_scales, d.hx, d.sums, d.workspace, d.workspace_bytes = scales, fake, fake, fake, 2 * T * 2 * 5 * 8
    d.hy[0] = 1
    return d


def test_argument_errors_need_no_gpu():
    lib = E.load_library()
    run = lambda d: lib.skevent_run(ctypes.byref(d), None)      # noqa: E731
    assert lib.skevent_run(None, None) == -1
    assert lib.skevent_workspace_bytes(2, 5, 8, 1) == 2 * T * 2 * 5 * 8 and lib.skevent_workspace_bytes(2, 5, 8, 0) == 0
    assert lib.skevent_workspace_bytes(17, 5, 8, 1) == 0 and lib.skevent_workspace_bytes(2, 5, 8193, 1) == 0
    assert lib.skevent_workspace_bytes(2, 5, 8, 5) == 0 and lib.skevent_workspace_bytes(2, 0, 8, 1) == 0

    def bad(**kw):
        d = _desc()
        for k, v in kw.items():
            setattr(d, k, v)
        return run(d)
    for M in (0, 65, -1):
        assert run(_desc(M=M)) == -1, M
    for field in ("members", "truth", "counts", "hx", "sums", "workspace"):
        assert bad(**{field: None}) == -1, field
    assert bad(member_align=8) == -1 and bad(truth=4098) == -1 and bad(counts=4098) == -1 and bad(hx=4098) == -1
    assert bad(sums=4100) == -1 and bad(workspace=4104) == -1
    assert bad(n_events=17) == -1 and bad(n_events=-1) == -1 and bad(n_scales=5) == -1 and bad(n_scales=-1) == -1
    assert bad(H=0) == -1 and bad(W=0) == -1 and bad(C=0) == -1
    assert bad(workspace_bytes=2 * T * 2 * 5 * 8 - 1) == -1                                   # a workspace too small
    for ch in (-1, 3):                                                                        # a channel index outside the states
        d = _desc()
        d.channel[1] = ch
        assert run(d) == -1, ch
    for n in (0, 5):                                                                          # thresholds per channel: 1 to 4
        d = _desc()
        d.n_thr[0] = n
        assert run(d) == -1, n
    d = _desc()
    d.thr[1][3] = float("nan")
    assert run(d) == -1
    d = _desc()
    d.hy[0] = -1
    assert run(d) == -1
    d = _desc()
    d.W, d.workspace_bytes = 8193, 1 << 40                                                    # wider than the neighbourhood pass holds
    assert run(d) == -1
    d = _desc()
    d.C, d.H, d.W, d.workspace_bytes = 1 << 10, 1 << 11, 1 << 10, 1 << 40
    d.n_scales = 0
    assert run(d) == -1                                                                       # beyond the 32-bit byte offsets
    d = _desc(M=64)                                                                           # W (M (2 hy + 1) W)^2 >= 2^63
    d.H, d.W, d.hy[0], d.workspace_bytes = 1 << 12, 8192, 1 << 11, 1 << 40
    assert run(d) == -1
    d.hy[0] = 1 << 30
    assert run(d) == -1
    d = _desc()
    d.n_events = 0
    assert run(d) == 0                                                                        # no event channel launches nothing
    d.hx = None                                                                               # ... but is checked all the same
    assert run(d) == -1


def test_op_is_registered_and_has_no_cpu_kernel():
    from skyrim_amd import ops
    assert "event_counts" in ops.OP_NAMES
    with pytest.raises(NotImplementedError):
        torch.ops.skyrim_hip.event_counts([torch.zeros(1, 2, 4)], torch.zeros(1, dtype=torch.int64), torch.zeros(1, 2, 4), [0], [1], [0.5],
                                          torch.zeros(T * 2 * 2 * 2, dtype=torch.int32), [], None, None, None)


# ---- 2. the host's scores ------------------------------------------------------------------------------------------------------------- #
def _event_scores(x, y, thr, w, radii=(), windows=()):
    """EventScores of one time and one channel from the reference's integers: x (M, H, W), y (H, W); windows: (hy, hx) per radius."""
    M, H, W = x.shape
    rows = np.zeros((1, 1, T, H, 2, M + 1), np.int64)
    sums = np.zeros((1, 1, T, len(radii), H, 3), np.int64)
    points = np.ones((len(radii), H), np.int64)
    for t, v in enumerate(thr):
        k, o = R.point_counts(x, y, v)
        rows[0, 0, t] = R.joint_counts(k, o, M)
        for s, (hy, hx) in enumerate(windows):
            sums[0, 0, t, s], points[s] = R.row_sums(k, o, M, hy, hx)
    return E.EventScores.from_rows(M, [T0], ["a"], {"a": list(thr)}, rows, w, W, radii, sums if radii else None, points if radii else None)


@pytest.mark.parametrize("M", [1, 2, 5, 50])
def test_scores_from_the_table_equal_the_definitions(M):
    H, W = 9, 16
    x, y = R.case(M, (1, H, W), seed=M)
    lat = np.linspace(80, -80, H)
    w = V.area_weights(lat)
    thr = [-0.5, 0.25, 1.0]
    hx = np.array([7, 3, 2, 1, 1, 1, 2, 3, 9], np.int32)
    s = _event_scores(x[:, 0], y[0], thr, w, radii=(0.0, 300.0), windows=((0, np.zeros(H, np.int32)), (2, hx)))
    assert s.n_members == M and s.brier.dims == ("time", "channel", "threshold") and s.fss.dims == ("time", "channel", "threshold", "scale")
    for t, v in enumerate(thr):
        k, o = R.point_counts(x[:, 0], y[0], v)
        ref = R.scores(k, o, M, w)
        names = [n for n in s.names if n != "fss"]
        assert set(names) == set(ref) - {"observed_frequency", "weight", "pod_curve", "pofd_curve"}
        for name in names:
            got = getattr(s, name).values[0, 0, t]
            assert abs(got - ref[name]) <= 1e-12 or (np.isnan(got) and np.isnan(ref[name])), (name, v, got, ref[name])
        assert abs(s.brier.values[0, 0, t] - (s.reliability.values[0, 0, t] - s.resolution.values[0, 0, t] + s.uncertainty.values[0, 0, t])) <= 1e-12
        assert np.allclose(s.reliability_curve["observed_frequency"].values[0, 0, t], ref["observed_frequency"], rtol=0, atol=1e-12, equal_nan=True)
        assert np.allclose(s.reliability_curve["weight"].values[0, 0, t], ref["weight"], rtol=0, atol=1e-12)
        assert np.allclose(s.roc.values[0, 0, t, :, 0], ref["pofd_curve"], rtol=0, atol=1e-12, equal_nan=True)
        assert np.allclose(s.roc.values[0, 0, t, :, 1], ref["pod_curve"], rtol=0, atol=1e-12, equal_nan=True)
        assert abs(s.frequency.values[0, 0, t].sum() - 1) <= 1e-12 and s.counts.values[0, 0, t].sum() == H * W
        assert abs(s.fss.values[0, 0, t, 0] - R.fss(k, o, M, 0, np.zeros(H, np.int32), w)) <= 1e-12
        assert abs(s.fss.values[0, 0, t, 1] - R.fss(k, o, M, 2, hx, w)) <= 1e-12
        if M == 1:
            assert np.array_equal(s.table.values[0, 0, t], s.frequency.values[0, 0, t])
    assert np.array_equal(s.reliability_curve["forecast_probability"], np.arange(M + 1) / M)
    assert all(np.isnan(getattr(s, n).values[0, 0, 3:]).all() for n in s.names)               # a threshold the channel does not have


def test_auc_of_a_perfect_and_of_a_constant_forecast():
    H, W, M = 5, 12, 7
    _, y = R.case(M, (1, H, W), seed=3)
    w = V.area_weights(np.linspace(60, -60, H))
    perfect = _event_scores(np.repeat(y, M, axis=0), y[0], [0.0], w)
    assert perfect.auc.values[0, 0, 0] == 1.0 and perfect.brier.values[0, 0, 0] == 0.0 and perfect.resolution.values[0, 0, 0] > 0
    x = np.zeros((M, H, W), np.float32)
    x[:3] = 1.0                                                  # 3 of 7 members above everywhere: no discrimination
    const = _event_scores(x, y[0], [0.0], w)
    assert abs(const.auc.values[0, 0, 0] - 0.5) <= 1e-15 and const.resolution.values[0, 0, 0] <= 1e-30
    never = _event_scores(x, y[0], [1e9], w)                     # an event that is never observed: POD and AUC are undefined
    assert np.isnan(never.auc.values[0, 0, 0]) and never.base_rate.values[0, 0, 0] == 0 and never.brier.values[0, 0, 0] == 0


def test_fss_at_scale_zero_and_of_a_perfect_forecast():
    H, W, M = 6, 10, 5
    x, y = R.case(M, (1, H, W), seed=5)
    k, o = R.point_counts(x[:, 0], y[0], 0.25)
    N = R.joint_counts(k, o, M)
    sums, n = R.row_sums(k, o, M, 0, np.zeros(H, np.int32))
    kk = np.arange(M + 1)
    assert np.all(n == 1)
    assert np.array_equal(sums[:, 0], (N[:, 0] * kk ** 2 + N[:, 1] * (kk - M) ** 2).sum(axis=1))
    assert np.array_equal(sums[:, 1], ((N[:, 0] + N[:, 1]) * kk ** 2).sum(axis=1)) and np.array_equal(sums[:, 2], M * M * N[:, 1].sum(axis=1))
    w = V.area_weights(np.linspace(75, -75, H))
    hx = np.array([4, 2, 1, 1, 2, 4], np.int32)
    s = _event_scores(x[:, 0], y[0], [0.25], w, radii=(0.0, 200.0), windows=((0, np.zeros(H, np.int32)), (1, hx)))
    assert abs((1 - s.fss.values[0, 0, 0, 0]) * (s.fss_terms.values[0, 0, 0, 0, 1] + s.fss_terms.values[0, 0, 0, 0, 2])
               - s.brier.values[0, 0, 0]) <= 1e-12                # at scale 0 the numerator is the Brier score
    same = _event_scores(np.repeat(y, M, axis=0), y[0], [0.25], w, radii=(0.0, 200.0), windows=((0, np.zeros(H, np.int32)), (1, hx)))
    assert np.all(same.fss.values[0, 0, 0] == 1.0)
    assert np.array_equal(E.window_points(1, hx, H, W), R.window_sums(k, o, 1, hx)[2])
    assert np.array_equal(E.window_points(9, [9] * H, H, W), np.full(H, H * 9))               # both clamps


# ---- 3. windows ----------------------------------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize("H,W", [(721, 1440), (720, 1440), (121, 240)])
def test_windows(H, W):
    from skyrim_amd.tracks import EARTH_RADIUS_KM as A
    res = 360.0 / W
    lat = np.linspace(90, -90, 721)[:720] if H == 720 else np.linspace(90, -90, H)
    lon = np.arange(W) * res
    km = A * np.deg2rad(res)                                     # one row, or one column on the equator
    for R_km in (0.0, 0.4 * km, 3.5 * km, 11.2 * km, 1e5):
        hy, hx = E.windows(lat, lon, R_km)
        assert hx.dtype == np.int32 and hx.shape == (H,) and isinstance(hy, int)
        assert hy == min(int(R_km / km), H - 1)
        j = int(np.argmin(np.abs(lat)))
        if R_km < 1e5:
            assert hx[j] == int(R_km / (km * np.cos(np.deg2rad(lat[j]))))
            for jj in (H // 4, H // 3):                           # floor(R / (a cos(phi) dlambda)), away from the clamp
                want = int(np.floor(R_km / (A * np.cos(np.deg2rad(lat[jj])) * np.deg2rad(res))))
                assert hx[jj] == min(want, (W - 1) // 2)
        if R_km == 0:
            assert hy == 0 and np.all(hx == 0)                    # the point itself, the pole rows included
        else:
            assert hx[0] == (W - 1) // 2 and np.all(hx <= (W - 1) // 2) and np.all(hx >= 0)      # the pole row: the whole circle, once
            assert np.all(np.diff(hx[:j + 1]) <= 0)               # never wider towards the equator
        hy2, hx2 = E.windows(lat[::-1].copy(), lon, R_km)         # the other latitude order: the same window for the same latitude
        assert hy2 == hy and np.array_equal(hx2[::-1], hx)
    assert E.windows(lat, lon, 1e5)[0] == H - 1 and np.all(E.windows(lat, lon, 1e5)[1] == (W - 1) // 2)


def test_windows_refuse_a_grid_that_does_not_close_the_circle():
    lat, lon = np.linspace(90, -90, 49), np.arange(192) * 1.875
    E.windows(lat, lon, 100.0)
    for la, lo in ((lat, lon[:100]), (np.linspace(60, 30, 21), np.linspace(-10, 40, 34)), (lat, lon ** 1.01), (np.sort(np.random.default_rng(0).uniform(-80, 80, 20)), lon),
                   (lat[:1], lon), (lat, lon[:1])):
        with pytest.raises(ValueError, match="Point-wise event scores .* are still available"):
            E.windows(la, lo, 100.0)
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="radius"):
            E.windows(lat, lon, bad)
    with pytest.raises(ValueError, match="still available"):       # a regional grid through the driver
        E.LeadEvents(["t2m"], np.linspace(60, 30, 21), np.linspace(-10, 40, 34), 3, {"t2m": [280.0]}, (100.0,))
    assert E.LeadEvents(["t2m"], np.linspace(60, 30, 21), np.linspace(-10, 40, 34), 3, {"t2m": [280.0]}, ()).radii == []


# ---- 4. host logic -------------------------------------------------------------------------------------------------------------------- #
def _scores(M=5):
    rng = np.random.default_rng(2)
    times = [T0, T0 + datetime.timedelta(hours=6)]
    slots = ["bias", "mae", "mse", "var", "crps", "abs", "pair"]
    sums = np.abs(rng.normal(size=(7, 2, 3)))
    sums[2, 1, 2] = np.nan
    counts = rng.integers(0, 100, size=(2, 3, M + 1))
    return V.Scores("pangu", M, times, ["z500", "t850", "t2m"], sums, slots, counts, counts / counts.sum(axis=-1, keepdims=True), "abc"), times


def test_json_round_trip_with_and_without_events(tmp_path):
    s, times = _scores()
    # without events: the document Scores has always written, key for key
    clean = lambda a: [clean(v) for v in a] if isinstance(a, list) else (a if isinstance(a, int) or np.isfinite(a) else None)      # noqa: E731
    doc = dict(model="pangu", n_members=5, forecast_id="abc", times=[t.isoformat() for t in times], channels=s.channels,
               slots=s.sums.slot.values.tolist(), sums=clean(s.sums.values.tolist()), metrics=s.table.metric.values.tolist(),
               table=clean(s.table.values.tolist()), rank_counts=s.rank_counts.values.tolist(), rank_histogram=clean(s.rank_histogram.values.tolist()))
    assert s.events is None and s.to_json() == json.dumps(doc) and "events" not in json.loads(s.to_json())
    assert V.Scores.from_json(s.to_json()).events is None
    M, H, W = 5, 4, 8
    x, y = R.case(M, (2, H, W), seed=9)
    rows = np.zeros((2, 2, T, H, 2, M + 1), np.int64)
    sums = np.zeros((2, 2, T, 1, H, 3), np.int64)
    thr = {"t850": [0.0, 100.0], "t2m": [0.5]}                   # (100: never observed, never forecast -> undefined ratios)
    hx = np.array([3, 1, 1, 3], np.int32)
    for ti in range(2):
        for e, c in enumerate(thr):
            for t, v in enumerate(thr[c]):
                k, o = R.point_counts(np.roll(x[:, e], ti, axis=-1), y[e], v)
                rows[ti, e, t] = R.joint_counts(k, o, M)
                sums[ti, e, t, 0], points = R.row_sums(k, o, M, 1, hx)
    s.events = E.EventScores.from_rows(M, times, list(thr), thr, rows, V.area_weights(np.linspace(60, -60, H)), W, (150.0,), sums, points[None])
    text = s.to_json()
    assert "NaN" not in text and json.loads(text)["events"]["scores"]["auc"][0][0][1] is None      # undefined: null
    back = V.Scores.load(s.save(tmp_path))
    ev = back.events
    assert ev.channels == ["t850", "t2m"] and ev.thresholds == thr and ev.neighbourhoods_km == [150.0] and ev.times == times
    assert np.array_equal(ev.counts.values, s.events.counts.values) and np.array_equal(ev.frequency.values, s.events.frequency.values)
    for name in s.events.names:
        assert np.array_equal(getattr(ev, name).values, getattr(s.events, name).values, equal_nan=True), name
    assert np.array_equal(back.table.values, s.table.values, equal_nan=True) and ev.names == s.events.names and "fss" in ev.names
    assert np.isnan(ev.fss.values[0, 0, 1, 0]) and np.isfinite(ev.fss.values[:, 0, 0, 0]).all()


def _model():
    from test_ens_cpu import _Model
    return _Model()


def test_refusals():
    m = _model()
    names = list(m.model.out_channel_names)
    ens = dict(n_members=3, scores=True)
    with pytest.raises(ValueError, match="not an output channel"):
        m.verify(T0, events={"nope": [1.0]})
    with pytest.raises(ValueError, match="not an output channel"):
        m.ensemble_forecast(T0, events={"nope": [1.0]}, **ens)
    with pytest.raises(ValueError, match="1 to 4 thresholds"):
        m.verify(T0, events={"t2m": [1.0, 2.0, 3.0, 4.0, 5.0]})
    with pytest.raises(ValueError, match="1 to 4 thresholds"):
        m.ensemble_forecast(T0, events={"t2m": []}, **ens)
    with pytest.raises(ValueError, match="at most 16"):
        E.check_request([f"c{i}" for i in range(20)], {f"c{i}": [0.0] for i in range(17)})
    assert len(E.check_request([f"c{i}" for i in range(20)], {f"c{i}": [0.0] for i in range(16)})[0]) == 16
    with pytest.raises(ValueError, match="at most 4"):
        m.verify(T0, events={"t2m": [280.0]}, neighbourhoods_km=(0, 1, 2, 3, 4))
    with pytest.raises(ValueError, match="at most 4"):
        m.ensemble_forecast(T0, events={"t2m": [280.0]}, neighbourhoods_km=(0, 1, 2, 3, 4), **ens)
    with pytest.raises(ValueError, match="not negative"):
        m.verify(T0, events={"t2m": [280.0]}, neighbourhoods_km=(100, -1))
    with pytest.raises(ValueError, match="not negative"):
        m.ensemble_forecast(T0, events={"t2m": [280.0]}, neighbourhoods_km=(-1,), **ens)
    with pytest.raises(ValueError, match="needs scores=True"):
        m.ensemble_forecast(T0, n_members=3, events={"t2m": [280.0]})
    with pytest.raises(ValueError, match="exceed=, which is empty"):
        m.ensemble_forecast(T0, events=True, **ens)
    with pytest.raises(ValueError, match="NaN"):
        m.verify(T0, events={"t2m": [float("nan")]})
    with pytest.raises(ValueError, match="at least one channel"):
        m.verify(T0, events={})
    with pytest.raises(ValueError, match="65"):
        E.check_request(names, {"t2m": [1.0]}, (), 65)
    lat, lon = np.asarray(m.model.grid.lat), np.asarray(m.model.grid.lon)
    from skyrim_amd.labeled import DataArray
    truth = DataArray(np.zeros((1, 1, len(lat), len(lon)), np.float32), ["time", "channel", "lat", "lon"], dict(time=[T0], channel=["t2m"], lat=lat, lon=lon))
    with pytest.raises(ValueError, match="not among the scored channels"):       # the truth does not hold the event channel
        V.LeadScorer("m", names, lat, lon, 1, truth, events={"u1000": [5.0]})
    scorer = V.LeadScorer("m", names, lat, lon, 3, truth, events={"t2m": [280.0, 290.0]}, neighbourhoods_km=(0, 250))
    assert scorer.events.channels == ["t2m"] and scorer.events.radii == [0.0, 250.0] and scorer.events.hy[0] == 0 and scorer.events.hx.shape == (2, len(lat))
    assert V.LeadScorer("m", names, lat, lon, 3, truth).events is None
    assert E.check_request(names, {"t2m": 280.0}) == ({"t2m": [280.0]}, [])
    with pytest.raises(RuntimeError, match="GPU"):
        m.verify(T0, events={"t2m": [280.0]}, neighbourhoods_km=(100,))           # everything valid: counting itself needs the device


def test_events_true_means_the_thresholds_of_exceed():
    from skyrim_amd import ensemble
    ev, radii = ensemble.event_request(True, (0, 100), {"t2m": [280.0, 290.0]}, ["u1000", "t2m"], 5, True)
    assert ev == {"t2m": [280.0, 290.0]} and radii == [0.0, 100.0]
    ev, _ = ensemble.event_request({"ws10m": [15]}, (), None, ["t2m", "ws10m"], 5, True)
    assert ev == {"ws10m": [15.0]}


def test_command_line_options():
    from click.testing import CliRunner
    from skyrim_amd import verify_cli
    res = CliRunner().invoke(verify_cli.verify, ["--help"])
    assert res.exit_code == 0 and "--event" in res.output and "--neighbourhood_km" in res.output
    v = {p.name: p for p in verify_cli.verify.params}
    assert v["event"].multiple and v["neighbourhood_km"].multiple and v["members"].default == 1
    assert E.parse_event("ws10m:15,25") == ("ws10m", [15.0, 25.0]) and E.parse_event("t2m:273.15") == ("t2m", [273.15])
    for bad in ("ws10m", "ws10m:", ":15", "ws10m:a,b"):
        with pytest.raises(ValueError, match="--event"):
            E.parse_event(bad)
    res = CliRunner().invoke(verify_cli.verify, ["-m", "pangu", "--event", "t2m"])
    assert res.exit_code != 0 and "--event" in repr(res.exception)
    res = CliRunner().invoke(verify_cli.verify, ["-m", "pangu", "--neighbourhood_km", "100"])
    assert res.exit_code != 0 and "needs --event" in repr(res.exception)
    assert verify_cli.event_lines(_scores()[0]) == []


# ---- 5. the compiler's resource report ------------------------------------------------------------------------------------------------ #
@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not installed")
def test_kernels_use_no_scratch():
    r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "--cuda-device-only", "-c", "event_ops.hip", "-o", "/dev/null",
                        "-Rpass-analysis=kernel-resource-usage"], cwd=ROOT / "skyrim_amd" / "csrc", capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    out, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and name:
            out[name] = int(m.group(1))
    assert sum("event_count_kernel" in k for k in out) == 2 and sum("event_scale_kernel" in k for k in out) == 1      # vector, scalar; scales
    assert all(v == 0 for v in out.values()), out
