"""Forecast verification without a GPU: the C ABI of include/skyrim_score.h (exports, argument errors), ``area_weights``, the float64
restatement against hand-worked values and identities, the host logic (refusals, the JSON file, the command line) and the compiler's
resource report of csrc/score_ops.hip."""
from __future__ import annotations

import ctypes
import datetime
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

import _score_reference as R
from skyrim_amd import verify as V

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "skyrim_score.h"
T0 = datetime.datetime(2024, 5, 13, 18, 0)


# ---- 1. ABI --------------------------------------------------------------------------------------------------------------------------- #
def test_library_exports_every_declared_symbol():
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    syms = sorted(set(re.findall(r"\b(skscore_[a-z0-9_]+)\s*\(", text)))
    assert len(syms) == 3                                        # (that they are EXPORTS, exported, and the ABI version: tests/test_native.py)
    assert V.SPEC.stem == "skyrim_score" and V.SPEC.prefix == "skscore"
    assert int(re.search(r"SKSCORE_MAX_MEMBERS (\d+)", text).group(1)) == V.MAX_MEMBERS
    assert int(re.search(r"SKSCORE_SLOTS (\d+)", text).group(1)) == len(V.SLOTS)
    assert int(re.search(r"SKSCORE_PARTIALS (\d+)", text).group(1)) == V.PARTIALS
    for k, name in enumerate(("BIAS", "MAE", "MSE", "VARIANCE", "CRPS_FAIR", "ABS", "PAIR", "FA", "FF", "AA")):
        assert int(re.search(rf"SKSCORE_{name} (\d+)", text).group(1)) == k
    for name, val in (("DET", V.DET), ("VAR", V.VAR), ("CRPS", V.CRPS), ("ACC", V.ACC), ("RANK", V.RANK)):
        assert int(re.search(rf"SKSCORE_{name} (\d+)", text).group(1)) == val


def _desc(M=4, flags=V.DET):
    fake = 4096                                                # never dereferenced: the argument checks come first
    d = V.ScoreDesc()
    d.members, d.M, d.member_align, d.truth, d.clim = fake, M, 16, fake, None
    d.C, d.H, d.W, d.c0, d.nc, d.lat_weight, d.flags, d.out, d.counts = 3, 5, 8, 0, 3, fake, flags, fake, None
    d.workspace, d.workspace_bytes = fake, 3 * 5 * V.PARTIALS * 8
    return d


def test_argument_errors_need_no_gpu():
    lib = V.load_library()
    assert lib.skscore_run(None, None) == -1
    assert lib.skscore_workspace_bytes(3, 5, 4, V.DET) == 3 * 5 * V.PARTIALS * 8
    assert lib.skscore_workspace_bytes(3, 5, 0, V.DET) == 0 and lib.skscore_workspace_bytes(3, 5, 4, 0) == 0
    for M in (0, 65, -1):
        assert lib.skscore_run(ctypes.byref(_desc(M=M)), None) == -1, M
    assert lib.skscore_run(ctypes.byref(_desc(flags=0)), None) == -1                          # nothing asked for
    assert lib.skscore_run(ctypes.byref(_desc(flags=64)), None) == -1
    for c0, nc in ((0, 4), (3, 1), (-1, 2), (2, -1)):                                         # a channel range outside C
        d = _desc()
        d.c0, d.nc = c0, nc
        assert lib.skscore_run(ctypes.byref(d), None) == -1, (c0, nc)
    d = _desc()
    d.workspace_bytes -= 1
    assert lib.skscore_run(ctypes.byref(d), None) == -1                                       # a workspace too small
    assert lib.skscore_run(ctypes.byref(_desc(flags=V.RANK)), None) == -1                     # rank counts without a counts pointer
    assert lib.skscore_run(ctypes.byref(_desc(flags=V.ACC)), None) == -1                      # ACC without a climatology
    d = _desc()
    d.member_align = 8
    assert lib.skscore_run(ctypes.byref(d), None) == -1
    d = _desc()
    d.C, d.H, d.W, d.nc, d.workspace_bytes = 1 << 10, 1 << 11, 1 << 10, 1, 1 << 40
    assert lib.skscore_run(ctypes.byref(d), None) == -1                                       # beyond the 32-bit byte offsets
    d = _desc()
    d.nc = 0
    assert lib.skscore_run(ctypes.byref(d), None) == 0                                        # an empty range launches nothing


def test_op_is_registered_and_has_no_cpu_kernel():
    from skyrim_amd import ops
    assert "score_fields" in ops.OP_NAMES
    with pytest.raises(NotImplementedError):
        torch.ops.skyrim_hip.score_fields([torch.zeros(1, 2, 4)], torch.zeros(1, dtype=torch.int64), torch.zeros(1, 2, 4),
                                          torch.ones(2, dtype=torch.float64), torch.zeros(1, 10, dtype=torch.float64),
                                          torch.zeros(18, dtype=torch.float64), V.DET, None, None, 0, 1)


# ---- 2. weights ----------------------------------------------------------------------------------------------------------------------- #
def test_area_weights():
    for n in (721, 49, 73):
        lat = np.linspace(90, -90, n)
        w = V.area_weights(lat)
        assert w.dtype == np.float64 and abs(w.sum() - 2.0) <= 1e-12 and np.all(w > 0)         # pole rows included: a positive cap
        assert np.allclose(w, w[::-1], rtol=0, atol=1e-15)
        assert np.array_equal(V.area_weights(lat[::-1])[::-1], w)                              # the other orientation
        assert np.allclose(w, R.area_weights(lat), rtol=0, atol=1e-15)
    assert abs(V.area_weights(np.linspace(90, -90, 721))[0] - (1 - np.sin(np.deg2rad(89.875)))) <= 1e-15
    # the 720-row grid has no south-pole row: its cells reach to -89.875, so the sphere's 2 is short of exactly the cap beyond that
    lat = np.linspace(90, -90, 721)[:720]
    w = V.area_weights(lat)
    assert abs(w.sum() - (2.0 - (1 - np.sin(np.deg2rad(89.875))))) <= 1e-12 and np.all(w > 0)
    assert np.array_equal(V.area_weights(lat[::-1])[::-1], w) and np.allclose(w, R.area_weights(lat), rtol=0, atol=1e-15)
    assert np.allclose(w[:719], V.area_weights(np.linspace(90, -90, 721))[:719], rtol=0, atol=1e-15)       # the same cells elsewhere
    for bad in ([0.0, 0.0], [10.0, 20.0, 15.0], [100.0, 0.0]):
        with pytest.raises(ValueError):
            V.area_weights(bad)


# ---- 3. the restatement --------------------------------------------------------------------------------------------------------------- #
def test_restatement_against_hand_worked_values():
    """2 x 3 grid, M = 3, one channel; uniform weights so the area mean is the plain mean of the six points."""
    y = np.array([[[0, 0, 0], [1, 1, 1]]], np.float32)
    x = np.array([[[[1, -1, 0], [1, 2, 4]]], [[[2, 0, 0], [1, 3, 0]]], [[[3, 4, 0], [1, 4, 2]]]], np.float32)
    # per point, members (x0, x1, x2) - y:   (1,2,3) (-1,0,4) (0,0,0) | (0,0,0) (1,2,3) (3,-1,1)
    eb = np.array([2, 1, 0, 0, 2, 1.0])
    A = np.array([2, 5 / 3, 0, 0, 2, 5 / 3])
    v = np.array([1, 7, 0, 0, 1, 4.0])                               # sample variances (ddof = 1)
    B = np.array([4 / 6, 10 / 6, 0, 0, 4 / 6, 8 / 6])                # sum_{m<n} |x_m - x_n| / 6
    r = np.array([0, 1, 0, 0, 0, 1])                                 # strictly below the truth
    val, bound, counts = R.scores(x, y, np.ones(2))
    assert np.isclose(val["bias"][0], eb.mean()) and np.isclose(val["mae"][0], np.abs(eb).mean()) and np.isclose(val["mse"][0], (eb ** 2).mean())
    assert np.isclose(val["var"][0], v.mean()) and np.isclose(val["abs"][0], A.mean()) and np.isclose(val["pair"][0], B.mean())
    assert np.isclose(val["crps"][0], A.mean() - B.mean())
    assert counts.shape == (1, 2, 4) and counts[0].tolist() == [[2, 1, 0, 0], [2, 1, 0, 0]] and counts.sum() == 6 and r.sum() == 2
    w = np.array([1.0, 3.0])                                         # weighted: rows count 1 : 3
    val, _, _ = R.scores(x, y, w)
    assert np.isclose(val["bias"][0], (eb[:3].sum() + 3 * eb[3:].sum()) / (3 * 4))
    c = y - 2                                                        # anomaly a = 2 everywhere, f = eb + 2
    val, _, _ = R.scores(x, y, np.ones(2), c)
    assert np.isclose(val["fa"][0], (2 * (eb + 2)).mean()) and np.isclose(val["ff"][0], ((eb + 2) ** 2).mean()) and np.isclose(val["aa"][0], 4.0)
    t = R.table(val, 3)
    assert np.isclose(t["ssr"][0], np.sqrt(4 / 3) * np.sqrt(v.mean()) / np.sqrt((eb ** 2).mean()))


def test_restatement_identities():
    rng = np.random.default_rng(0)
    y = rng.normal(size=(2, 5, 7)).astype(np.float32)
    w = R.area_weights(np.linspace(90, -90, 5))
    x = (y + rng.normal(size=(1, 2, 5, 7))).astype(np.float32)
    val, _, counts = R.scores(x, y, w)
    assert np.array_equal(val["crps"], val["mae"]) and np.all(val["var"] == 0) and np.all(val["pair"] == 0)      # M = 1
    x = np.repeat(y[None], 6, axis=0)
    val, _, counts = R.scores(x, y, w)
    assert np.all(val["crps"] == 0) and np.all(counts[..., 0] == 7) and np.all(counts[..., 1:] == 0)             # members equal to the truth
    # pairwise and sorted forms of B agree
    x = rng.normal(size=(9, 1, 1, 50))
    t = R.point_terms(x.astype(np.float32), np.zeros((1, 1, 50), np.float32))
    x32 = x.astype(np.float32).astype(np.float64)
    pair = sum(np.abs(x32[m] - x32[n]) for m in range(9) for n in range(m + 1, 9)) / (9 * 8)
    assert np.allclose(t["B"], pair, rtol=1e-12, atol=0)


@pytest.mark.parametrize("M", [2, 7, 8, 9, 33, 50, 64])
def test_restatement_equals_the_literal_definitions(M):
    """The restatement forms v from d_m = x_m - x_0 and B from the gaps of the sorted members, as the header does.  Here both are held
    to the definitions as first written -- v = sum (e_m - e_bar)^2 / (M - 1) with e_m = x_m - y, B = sum_{m<n} |x_m - x_n| / (M (M - 1)) --
    at every member count the GPU tests use, on a z-like field (2e5, members 1e-3 sigma apart) with the truth 30 sigma away: the case
    in which the two forms of v differ most.  Tolerance: in float64 e_m - e_bar carries an error of (M + 2) 2^-53 |e|, relative to
    |d| ~ 1e-3 sigma that is (M + 2) 2^-53 3e4 <= 2.2e-10 at M = 64, twice that in the square; 1e-8 of the value leaves room and is a
    sixth of one float32 rounding.  The pairwise sum has M (M - 1) / 2 non-negative addends: 2016 * 2^-53 relative."""
    rng = np.random.default_rng(M)
    sigma = 3.0e3
    x0 = (2.0e5 + sigma * rng.normal(size=(1, 2, 3, 11))).astype(np.float32)
    x = (x0 + 1e-3 * sigma * rng.normal(size=(M, 2, 3, 11))).astype(np.float32)
    x[-1, :, :, 0] = x[0, :, :, 0]                                   # ties among the members
    y = (x0[0] + 30 * sigma).astype(np.float32)
    t = R.point_terms(x, y)
    x64, y64 = x.astype(np.float64), y.astype(np.float64)
    e = x64 - y64
    v = ((e - e.sum(axis=0) / M) ** 2).sum(axis=0) / (M - 1)
    B = sum(np.abs(x64[m] - x64[n]) for m in range(M) for n in range(m + 1, M)) / (M * (M - 1))
    assert np.all(np.abs(t["v"] - v) <= 1e-8 * v), np.max(np.abs(t["v"] - v) / v)
    assert np.all(np.abs(t["B"] - B) <= 1e-12 * B), np.max(np.abs(t["B"] - B) / B)
    assert np.array_equal(t["r"], (x64 < y64).sum(axis=0))


def test_fair_crps_is_unbiased():
    """Members and truth from the same distribution N(0, 1): the fair CRPS of an M-member ensemble estimates the CRPS of the
    distribution itself, 1 / sqrt(pi), without bias, for every M -- over 2^16 draws, within 5 standard errors."""
    rng = np.random.default_rng(1)
    n = 1 << 16
    for M in (2, 5, 20):
        x = rng.normal(size=(M, 1, 1, n)).astype(np.float32)
        y = rng.normal(size=(1, 1, n)).astype(np.float32)
        t = R.point_terms(x, y)
        per_point = t["A"] - t["B"]
        se = per_point.std() / np.sqrt(n)
        assert abs(per_point.mean() - 1 / np.sqrt(np.pi)) <= 5 * se, (M, per_point.mean(), se)
        val, _, _ = R.scores(x, y, np.ones(1))
        assert np.isclose(val["crps"][0], per_point.mean())


# ---- 4. host logic -------------------------------------------------------------------------------------------------------------------- #
def _model():
    from test_ens_cpu import _Model
    return _Model()


def test_refusals():
    from skyrim_amd.core.models.ensemble import GlobalEnsemble
    from skyrim_amd.core.models.graphcast import GraphcastModel
    from skyrim_amd.labeled import DataArray
    m = _model()
    with pytest.raises(ValueError, match="multi-model"):
        GlobalEnsemble(["pangu", "fuxi"], ic_source="synthetic").verify(T0)
    with pytest.raises(NotImplementedError, match="score_prediction"):
        GraphcastModel.verify(object.__new__(GraphcastModel), T0)
    with pytest.raises(ValueError, match="not output channels"):
        m.verify(T0, channels=["nope"])
    with pytest.raises(ValueError, match="64"):
        m.ensemble_forecast(T0, n_members=65, scores=True)
    with pytest.raises(ValueError, match="64"):
        V.check_request(0, ["t2m"])
    lat, lon = np.asarray(m.model.grid.lat), np.asarray(m.model.grid.lon)
    other = DataArray(np.zeros((1, 1, len(lat), len(lon)), np.float32), ["time", "channel", "lat", "lon"],
                      dict(time=[T0], channel=["q50"], lat=lat, lon=lon))
    with pytest.raises(ValueError, match="share no channel"):
        m.verify(T0, truth=other)
    with pytest.raises(ValueError, match="share no channel"):
        m.ensemble_forecast(T0, n_members=3, scores=True, truth=other)
    wrong = DataArray(np.zeros((1, 1, len(lat), len(lon)), np.float32), ["time", "channel", "lat", "lon"],
                      dict(time=[T0], channel=["t2m"], lat=lat * 0.5, lon=lon))
    with pytest.raises(ValueError, match="different lat"):
        m.verify(T0, truth=wrong)
    with pytest.raises(ValueError, match="expected a data source"):
        m.verify(T0, truth=object())
    with pytest.raises(ValueError, match="need a truth"):
        V.LeadScorer("m", ["t2m"], lat, lon, 3, None)
    with pytest.raises(RuntimeError, match="GPU"):
        m.verify(T0)                                             # everything valid: scoring itself needs the device
    flipped = DataArray(np.zeros((1, 1, len(lat), len(lon)), np.float32), ["time", "channel", "lat", "lon"],
                        dict(time=[T0], channel=["t2m"], lat=lat[::-1].copy(), lon=lon))
    assert V.LeadScorer("m", ["u1000", "t2m"], lat, lon, 1, flipped).truth.flip is True          # a reversed latitude axis is turned round


def test_more_than_one_rank_is_refused(monkeypatch):
    monkeypatch.setattr(V, "_world_size", lambda: 2)
    with pytest.raises(NotImplementedError, match="one GPU"):
        _model().verify(T0)
    with pytest.raises(NotImplementedError, match="one GPU"):
        V.check_request(3, ["t2m"])


def test_scores_table_and_json_round_trip(tmp_path):
    rng = np.random.default_rng(2)
    times = [T0, T0 + datetime.timedelta(hours=6)]
    slots = ["bias", "mae", "mse", "var", "crps", "abs", "pair"]
    sums = np.abs(rng.normal(size=(7, 2, 3)))
    sums[2, 1, 2] = np.nan
    counts = rng.integers(0, 100, size=(2, 3, 6))
    s = V.Scores("pangu", 5, times, ["z500", "t850", "t2m"], sums, slots, counts, counts / counts.sum(axis=-1, keepdims=True), "abc")
    assert s.table.dims == ("metric", "time", "channel") and s.table.metric.values.tolist() == ["bias", "mae", "rmse", "crps", "spread", "ssr"]
    assert np.allclose(s.metric("ssr")[0], np.sqrt(6 / 5) * np.sqrt(sums[3, 0]) / np.sqrt(sums[2, 0]))
    assert s.rank_histogram.dims == ("time", "channel", "rank") and s.file_name() == "pangu-ens5-scores.json"
    path = s.save(tmp_path)
    assert Path(path) == tmp_path / "abc" / "pangu-ens5-scores.json"
    back = V.Scores.load(path)
    assert np.array_equal(back.table.values, s.table.values, equal_nan=True) and np.array_equal(back.rank_counts.values, s.rank_counts.values)
    assert back.times == times and back.channels == s.channels and back.n_members == 5 and back.forecast_id == "abc"
    det = V.Scores("fuxi", 1, times, ["t2m"], sums[[0, 1, 2, 4], :, :1], ["bias", "mae", "mse", "crps"])
    assert det.table.metric.values.tolist() == ["bias", "mae", "rmse", "crps"] and det.rank_histogram is None       # absent, not NaN-filled
    assert det.file_name() == "fuxi-scores.json"


def test_command_line_help():
    from click.testing import CliRunner
    from skyrim_amd import forecast, verify_cli
    res = CliRunner().invoke(verify_cli.verify, ["--help"])
    assert res.exit_code == 0
    for opt in ("--model_name", "--date", "--time", "--lead_time", "--initial_conditions", "--output_dir", "--members", "--climatology",
                "--channels", "--perturb_scale", "--seed"):
        assert opt in res.output, opt
    f = {p.name: p for p in forecast.main.params}
    v = {p.name: p for p in verify_cli.verify.params}
    assert verify_cli.verify.name == "verify"
    for name, p in f.items():
        assert name in v and v[name].opts == p.opts and v[name].default == p.default and v[name].is_flag == p.is_flag, name
    assert v["members"].opts == ["--members", "-n"] and v["members"].default == 1 and v["climatology"].default is None


# ---- 5. the compiler's resource report ------------------------------------------------------------------------------------------------ #
@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not installed")
def test_kernels_use_no_scratch_and_keep_their_occupancy():
    keys = {"VGPRs": "vgprs", "ScratchSize [bytes/lane]": "scratch", "Occupancy [waves/SIMD]": "occupancy"}
    r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "--cuda-device-only", "-c", "score_ops.hip", "-o", "/dev/null",
                        "-Rpass-analysis=kernel-resource-usage"], cwd=ROOT / "skyrim_amd" / "csrc", capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    out, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            out[name] = {}
        for key, short in keys.items():
            m = re.search(re.escape(key) + r": (\d+)", line)
            if m and name:
                out[name][short] = int(m.group(1))
    rows = {k: v for k, v in out.items() if "score_rows_kernel" in k}
    assert len(rows) == 14 and any("score_reduce_kernel" in k for k in out)      # buckets 1 | 8, 16, 32, 64 x sort x (vector, scalar)
    for k, v in sorted(out.items()):
        print(f"{k}: {v['vgprs']} VGPRs, scratch {v['scratch']}, {v['occupancy']} waves / SIMD")
        assert v["scratch"] == 0, k
    for k, v in rows.items():
        if "ILi64E" in k:
            assert v["occupancy"] >= 2, (k, v)
        if "ILi1E" in k:
            assert v["occupancy"] >= 4, (k, v)
