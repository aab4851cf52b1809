"""Perturbed-IC ensembles without a GPU: the C ABI of include/skyrim_ens.h (exports, argument errors), the generator's restatement
against the Philox4x32-10 known answers, and the host logic of ``ensemble_forecast`` (naming, refusals, the command line)."""
from __future__ import annotations

import ctypes
import datetime
import inspect
import os
import re
import socket
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import _ens_reference as R
from skyrim_amd import ensemble as E
from skyrim_amd.core.models.base import GlobalModel
from skyrim_amd.pangu.spec import PanguGeometry

HEADER = Path(__file__).resolve().parent.parent / "include" / "skyrim_ens.h"
T0 = datetime.datetime(2024, 5, 13, 18, 0)
GEOM = PanguGeometry(9, 96)


# ---- 1. ABI --------------------------------------------------------------------------------------------------------------------------- #
def test_library_exports_every_declared_symbol():
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    syms = sorted(set(re.findall(r"\b(skens_[a-z0-9_]+)\s*\(", text)))
    lib = E.load_library()
    assert syms == sorted(E.EXPORTS) and len(syms) == 3
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in skyrim_ens.h but not exported"
    assert lib.skens_abi_version() == E.ABI_VERSION == int(re.search(r"SKENS_ABI_VERSION (\d+)", text).group(1))
    for name, val in (("MAX_MEMBERS", E.MAX_MEMBERS), ("MAX_THRESHOLDS", E.MAX_THRESHOLDS), ("MAX_QUANTILES", E.MAX_QUANTILES)):
        assert int(re.search(rf"SKENS_{name} (\d+)", text).group(1)) == val


def test_argument_errors_need_no_gpu():
    lib = E.load_library()
    assert lib.skens_stats(None, None) == -1
    assert lib.skens_perturb(None, None, None, 16, 4, 4, 1.0, 0, 0, 1, None) == -1
    fake = 4096                                                # never dereferenced: the argument checks come first
    assert lib.skens_perturb(fake, fake, fake, 0, 4, 4, 1.0, 0, 0, 1, None) == -1
    assert lib.skens_perturb(fake, fake, fake, 18, 4, 4, 1.0, 0, 0, 1, None) == -1           # n is not L * C * chan_stride
    d = E.StatsDesc()
    d.members, d.member_align, d.offset, d.n, d.mean = fake, 16, 0, 8, fake
    for M in (0, 65, -1):
        d.M = M
        assert lib.skens_stats(ctypes.byref(d), None) == -1, M
    d.M = 4
    d.mean = None
    assert lib.skens_stats(ctypes.byref(d), None) == -1                                       # nothing asked for
    d.mean, d.n_thr = fake, 5
    assert lib.skens_stats(ctypes.byref(d), None) == -1
    d.n_thr, d.n_quant, d.quant = 0, 1, fake
    d.q_index[0] = 4
    assert lib.skens_stats(ctypes.byref(d), None) == -1                                       # index outside the members
    d.q_index[0], d.n_quant, d.quant, d.n = 0, 0, None, 0
    assert lib.skens_stats(ctypes.byref(d), None) == 0                                        # an empty range launches nothing


def test_ops_are_registered_and_have_no_cpu_kernel():
    from skyrim_amd import ops
    assert {"ens_perturb", "ens_stats"} <= set(ops.OP_NAMES)
    with pytest.raises(NotImplementedError):
        torch.ops.skyrim_hip.ens_perturb(torch.zeros(4), torch.ones(1), torch.zeros(4), 4, 1.0, 0, 1)
    with pytest.raises(NotImplementedError):
        torch.ops.skyrim_hip.ens_stats([torch.zeros(4)], torch.zeros(1, dtype=torch.int64), 0, 4, torch.zeros(4), None, None, None, None, [],
                                       None, [])


# ---- 2. the generator's restatement --------------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize("ctr,key,want", [
    ("00000000 00000000 00000000 00000000", "00000000 00000000", "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ("ffffffff ffffffff ffffffff ffffffff", "ffffffff ffffffff", "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ("243f6a88 85a308d3 13198a2e 03707344", "a4093822 299f31d0", "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox_known_answers(ctr, key, want):
    h = lambda s: np.array([int(w, 16) for w in s.split()], np.uint32)    # noqa: E731
    assert R.philox4x32_10(h(ctr), h(key)).tolist() == h(want).tolist()


def test_restated_normals_are_standard_and_member_keyed():
    n = 1 << 20
    z = R.normals(3, 1, n)
    assert abs(z.mean()) <= 5 / np.sqrt(n) and abs(z.var() - 1) <= 5 * np.sqrt(2 / n)
    assert np.array_equal(R.normals(3, 1, 1001), z[:1001])                 # a function of (seed, member, i) only
    assert not np.array_equal(R.normals(3, 2, 64), z[:64]) and not np.array_equal(R.normals(4, 1, 64), z[:64])
    u = R.uniform(np.array([0, 0xFFFFFFFF], np.uint32))
    assert 0 < u[0] and u[1] < 1          # (25 significant bits in the upper half: the kernel never rounds U itself, include/skyrim_ens.h)


def test_quantile_position_is_numpys_linear_method():
    rng = np.random.default_rng(0)
    for M in (1, 2, 3, 9, 50, 64):
        x = np.sort(rng.normal(size=M))
        for q in (0.0, 0.1, 0.5, 0.9, 1.0, 1 / 3):
            k, f = E.quantile_position(q, M)
            assert 0 <= k < M and 0 <= f < 1
            assert np.isclose(x[k] + f * (x[min(k + 1, M - 1)] - x[k]), np.quantile(x, q), rtol=0, atol=1e-6)
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError):
            E.quantile_position(bad, 5)


# ---- 3. host logic -------------------------------------------------------------------------------------------------------------------- #
class _Loop:
    n_history_levels = 1
    time_step = datetime.timedelta(hours=6)
    device = torch.device("cpu")
    in_channel_names = out_channel_names = ["u1000", "v1000", "t2m"]
    geom = grid = GEOM
    channel_std = torch.ones(3)

    def __call__(self, time, x, restart=None):
        raise AssertionError("a refused ensemble must not start a loop")


class _Model(GlobalModel):
    def __init__(self):
        super().__init__("boring", ic_source="synthetic")

    def build_model(self):
        return _Loop()


def test_product_and_file_naming():
    from skyrim_amd.common import generate_filename
    name = E.product_model_name("pangu", 50, "spread")
    assert name == "pangu-ens50-spread" and "__" not in name
    fn = generate_filename(name, T0, T0 + datetime.timedelta(hours=6), "gfs")
    assert fn == "pangu-ens50-spread__gfs__20240513_18:00__20240514_00:00.nc" and len(Path(fn).stem.split("__")) == 4
    assert E.PRODUCTS == ("mean", "spread", "min", "max")


def test_refusals():
    from skyrim_amd.core.models.ensemble import GlobalEnsemble
    from skyrim_amd.core.models.graphcast import GraphcastModel
    m = _Model()
    with pytest.raises(ValueError, match="64"):
        m.ensemble_forecast(T0, n_members=65)
    with pytest.raises(ValueError, match="64"):
        m.ensemble_forecast(T0, n_members=0)
    with pytest.raises(ValueError, match="not an output channel"):
        m.ensemble_forecast(T0, exceed={"nope": [1.0]})
    with pytest.raises(ValueError, match="1 to 4"):
        m.ensemble_forecast(T0, exceed={"t2m": [1.0, 2.0, 3.0, 4.0, 5.0]})
    with pytest.raises(ValueError, match="1 to 4"):
        m.ensemble_forecast(T0, quantiles={"t2m": [0.1, 0.2, 0.3, 0.4, 0.5]})
    with pytest.raises(ValueError, match=r"outside \[0, 1\]"):
        m.ensemble_forecast(T0, quantiles={"t2m": [1.2]})
    with pytest.raises(ValueError, match="unknown products"):
        m.ensemble_forecast(T0, products=("mean", "median"))
    with pytest.raises(ValueError, match="keep_members"):
        m.ensemble_forecast(T0, n_steps=200000, n_members=64, keep_members=True)
    with pytest.raises(RuntimeError, match="GPU"):
        m.ensemble_forecast(T0, n_members=3)                     # everything valid: the members themselves need the device
    with pytest.raises(ValueError, match="multi-model"):
        GlobalEnsemble(["pangu", "fuxi"], ic_source="synthetic").ensemble_forecast(T0)
    with pytest.raises(NotImplementedError, match="stepper"):
        GraphcastModel.ensemble_forecast(object.__new__(GraphcastModel), T0)


# ---- 4. the product set: the host half of every family of products, on torch-CPU tensors ---------------------------------------------- #
FIELDS, GRID_LAT, GRID_LON = ["a", "b"], np.linspace(30.0, -30.0, 4), np.arange(8) * 45.0
TIMES = [T0 + k * datetime.timedelta(hours=6) for k in range(3)]
EXCEED, QUANT = {"b": [0.0, 0.5]}, {"a": [0.5]}


@pytest.fixture
def launches(monkeypatch):
    """``ensemble.stats`` restated on torch-CPU tensors with tests/_ens_reference.stats; the list of (offset, n, outputs) it was asked for."""
    calls = []

    def stats(members, table, offset, n, mean=None, spread=None, min=None, max=None, exceed=None, thresholds=(), quant=None, levels=()):
        r = R.stats(np.stack([m.reshape(-1)[offset:offset + n].numpy() for m in members]), thresholds, levels)
        r["quant"] = np.stack([q for q, _ in r["quant"]]) if levels else None
        out = dict(mean=mean, spread=spread, min=min, max=max, exceed=exceed, quant=quant)
        given = sorted(k for k, t in out.items() if t is not None)
        assert given, "a stats call with zero outputs"
        for k in given:
            out[k].reshape(-1).copy_(torch.from_numpy(np.asarray(r[k], np.float32).reshape(-1)))
        calls.append((offset, n, given))
    monkeypatch.setattr(E, "stats", stats)
    return calls


def _states(entry):
    return list(torch.from_numpy(np.random.default_rng(entry).normal(size=(3, 2, 4, 8)).astype(np.float32)))


def _set(products=("mean", "max"), exceed=EXCEED, quantiles=QUANT, keep_members=True, prefix="", always=()):
    ps = E.ProductSet("toy", 3, products, "cpu", FIELDS, GRID_LAT, GRID_LON, 3, exceed, quantiles, keep_members, prefix, always)
    for arr in (*ps.host.values(), *ps.host_ex.values(), *ps.host_q.values(), *([] if ps.members is None else [ps.members])):
        arr[:] = -7.0                                          # a sentinel: what no reduce has written
    return ps


def _filled(**kw):
    ps = _set(**kw)
    for k in (2, 0, 1):
        ps.reduce(_states(k), None, k)
    return ps


def _when(values):
    return [np.datetime64(t, "s") for t in values]


def test_product_set_reduces_into_its_slot(launches):
    ps = _set(always=("mean",))
    ps.reduce(_states(5), None, None)                          # the every-step launch: the always-outputs, nothing stored
    assert launches == [(0, 64, ["mean"])]
    assert all(np.all(a == -7.0) for a in (*ps.host.values(), *ps.host_ex.values(), *ps.host_q.values(), ps.members))
    assert np.array_equal(ps.dev["mean"].numpy().reshape(-1), R.stats(torch.stack(_states(5)).reshape(3, -1).numpy())["mean"].astype(np.float32))
    del launches[:]
    for k in (2, 0, 1):                                        # any order: an entry goes where ``slot`` says
        ps.reduce(_states(k), None, k)
    assert launches == [(0, 64, ["max", "mean"]), (32, 32, ["exceed"]), (0, 32, ["quant"])] * 3
    for k in range(3):
        x = torch.stack(_states(k)).numpy()
        ref = R.stats(x.reshape(3, -1))
        assert np.array_equal(ps.host["mean"][k].reshape(-1), ref["mean"].astype(np.float32))
        assert np.array_equal(ps.host["max"][k].reshape(-1), ref["max"])
        assert np.array_equal(ps.host_ex["b"][k].reshape(2, -1), R.stats(x[:, 1].reshape(3, -1), thresholds=EXCEED["b"])["exceed"])
        assert np.array_equal(ps.host_q["a"][k].reshape(-1), R.stats(x[:, 0].reshape(3, -1), levels=QUANT["a"])["quant"][0][0].astype(np.float32))
        assert np.array_equal(ps.members[:, k], x)
    assert ps.host["mean"].shape == (3, 2, 4, 8) and ps.host_ex["b"].shape == (3, 2, 4, 8) and ps.host_q["a"].shape == (3, 1, 4, 8)
    assert ps.members.shape == (3, 3, 2, 4, 8) and sorted(ps.dev) == ["max", "mean"]


def test_product_set_without_products_launches_no_empty_call(launches):
    ps = _set(products=(), quantiles={}, keep_members=False)
    ps.reduce(_states(0), None, None)
    assert launches == [] and ps.members is None and ps.host == {} and ps.dev == {}
    ps.reduce(_states(0), None, 1)
    assert launches == [(32, 32, ["exceed"])] and np.all(ps.host_ex["b"][0] == -7.0) and not np.any(ps.host_ex["b"][1] == -7.0)


def test_product_set_fills_a_result_with_labelled_arrays(launches):
    from skyrim_amd.aggregate import AggregatedProducts
    ps = _filled()
    for channels, picked in ((None, [0, 1]), (["b"], [1])):    # raw and regridded select ``channels``; derived and aggregated pass none
        ens = E.EnsembleForecast("toy", 3, 0, 1e-3)
        ps.fill(ens, TIMES, channels)
        assert ens.spread is None and ens.min is None
        for p in ("mean", "max"):
            da = getattr(ens, p)
            assert da.dims == ("time", "channel", "lat", "lon") and list(da._coords) == ["time", "channel", "lat", "lon"]
            assert da.channel.values.tolist() == [FIELDS[i] for i in picked] and np.array_equal(da.values, ps.host[p][:, picked])
            assert _when(da.time.values) == _when(TIMES) and np.array_equal(da.lat.values, GRID_LAT) and np.array_equal(da.lon.values, GRID_LON)
        ex, qu = ens.exceedance["b"], ens.quantile["a"]
        assert list(ens.exceedance) == ["b"] and ex.dims == ("time", "threshold", "lat", "lon") and np.array_equal(ex.values, ps.host_ex["b"])
        assert ex.threshold.values.dtype == np.float32 and ex.threshold.values.tolist() == [0.0, 0.5] and _when(ex.time.values) == _when(TIMES)
        assert list(ens.quantile) == ["a"] and qu.dims == ("time", "quantile", "lat", "lon") and np.array_equal(qu.values, ps.host_q["a"])
        assert qu._coords["quantile"].dtype == np.float64 and qu._coords["quantile"].tolist() == [0.5]
        mem = ens.members
        assert mem.dims == ("member", "time", "channel", "lat", "lon") and list(mem._coords) == ["member", "time", "channel", "lat", "lon"]
        assert mem.member.values.tolist() == [0, 1, 2] and mem.channel.values.tolist() == [FIELDS[i] for i in picked]
        assert np.array_equal(mem.values, ps.members[:, :, picked]) and _when(mem.time.values) == _when(TIMES)
    # a window group: the time axis holds the window ends, ``window_start`` goes with it on every array
    ends, starts = TIMES, [t - datetime.timedelta(hours=12) for t in TIMES]
    prod = AggregatedProducts("12h", list(FIELDS))
    ps.fill(prod, ends, window_start=starts)
    for da in (prod.mean, prod.max, prod.exceedance["b"], prod.quantile["a"], prod.members):
        assert _when(da.time.values) == _when(ends) and _when(da._coords["window_start"]) == _when(starts)
        assert list(da._coords)[-3:] == ["window_start", "lat", "lon"]
    assert prod.mean.channel.values.tolist() == FIELDS and np.array_equal(prod.members.values, ps.members)
    # members only when they were kept
    ens = E.EnsembleForecast("toy", 3, 0, 1e-3)
    _filled(keep_members=False).fill(ens, TIMES)
    assert ens.members is None and ens.mean is not None


def test_product_set_saves_one_file_per_product(launches, monkeypatch):
    import skyrim_amd.common as common
    saved = []

    def save_forecast(da, name, start, end, source, config=None):
        saved.append((da, name, start, end, source, config))
        return f"{config['forecast_id']}:{name}"
    monkeypatch.setattr(common, "save_forecast", save_forecast)
    nc, zarr = {"forecast_id": "F", "output_dir": "out"}, {"forecast_id": "F", "output_dir": "out", "file_type": "zarr"}
    # the families of saved leads: two entries per file, the source handed in
    for prefix in ("", "derived-", "regrid-"):
        ps = _filled(prefix=prefix)
        del saved[:]
        assert ps.save(1, TIMES[1:3], TIMES[1], "gfs", nc) == [f"F:toy-ens3-{prefix}mean", f"F:toy-ens3-{prefix}max"]
        assert ps.save(1, TIMES[1:3], TIMES[1], "file", zarr) == [f"F/toy-ens3-{prefix}{p}:toy-ens3-{prefix}{p}" for p in ("mean", "max")]
        for n, (da, name, start, end, source, config) in enumerate(saved):
            p = ("mean", "max")[n % 2]
            assert name == f"toy-ens3-{prefix}{p}" and (start, end) == (TIMES[1], TIMES[2]) and source == ("gfs", "file")[n // 2]
            assert da.dims == ("time", "channel", "lat", "lon") and list(da._coords) == ["time", "channel", "lat", "lon"]
            assert _when(da.time.values) == _when(TIMES[1:3]) and da.channel.values.tolist() == FIELDS
            assert np.array_equal(da.values, ps.host[p][1:3]) and np.array_equal(da.lat.values, GRID_LAT)
            assert config is nc if n < 2 else config == dict(zarr, forecast_id=f"F/{name}")      # zarr: one store per product
    # a window group: one entry per file, from the window's start to its end, no ``window_start`` coordinate
    ps = _filled(prefix="agg12h-")
    del saved[:]
    start = TIMES[2] - datetime.timedelta(hours=12)
    assert ps.save(2, [TIMES[2]], start, "gfs", nc) == ["F:toy-ens3-agg12h-mean", "F:toy-ens3-agg12h-max"]
    for (da, name, *when, config), p in zip(saved, ("mean", "max")):
        assert when == [start, TIMES[2], "gfs"] and list(da._coords) == ["time", "channel", "lat", "lon"]
        assert da.shape == (1, 2, 4, 8) and np.array_equal(da.values, ps.host[p][2:3]) and _when(da.time.values) == _when([TIMES[2]])
    assert _filled(products=()).save(1, TIMES[1:3], TIMES[1], "gfs", nc) == [] and len(saved) == 2


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _rank(rank, world, port, q):
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    os.environ["SKYRIM_SYNTHETIC_IC"] = "1"
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        try:
            _Model().ensemble_forecast(T0, n_members=4)
            q.put((rank, "no error"))
        except NotImplementedError as e:
            q.put((rank, str(e)))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(120)
def test_more_than_one_rank_is_refused():
    ctx = mp.get_context("spawn")
    q, port = ctx.Queue(), _free_port()
    procs = [ctx.Process(target=_rank, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = dict(q.get(timeout=100) for _ in range(2))
    for p in procs:
        p.join(30)
        assert p.exitcode == 0
    assert all("MemberParallelEnsemble" in got[r] for r in range(2)), got


def test_command_lines():
    """``forecast`` keeps its options and ``run_forecast`` its signature; ``ensemble`` carries every one of them with the same defaults."""
    from skyrim_amd import ensemble_cli, forecast
    f = {p.name: p for p in forecast.main.params}
    assert sorted(f) == sorted(["model_name", "date", "time", "lead_time", "list_models", "initial_conditions", "output_dir", "filter_vars", "modal"])
    assert list(inspect.signature(forecast.run_forecast).parameters) == ["model_name", "date", "time", "lead_time", "list_models",
                                                                         "initial_conditions", "output_dir", "filter_vars"]
    e = {p.name: p for p in ensemble_cli.ensemble.params}
    assert ensemble_cli.ensemble.name == "ensemble"
    for name, p in f.items():
        assert name in e and e[name].opts == p.opts and e[name].default == p.default and e[name].is_flag == p.is_flag, name
    assert set(e) - set(f) == {"members", "perturb_scale", "seed"}
    assert e["members"].opts == ["--members", "-n"] and e["members"].default == 10
    assert e["perturb_scale"].default == 1e-3 and e["seed"].default == 0


# ---- 5. the member source: one generator per member behind ``advance`` / ``close`` ------------------------------------------------------ #
class _Fake:
    """A CPU "model": ``model(time, x)`` is a generator of (time, out, None) whose state at lead k is ``x + k``; ``fail`` = (the first
    element of the seed that fails, the lead it fails at); ``on_close``: what the generator of the seed ``on_close[0]`` raises when closed."""
    time_step = datetime.timedelta(hours=6)

    def __init__(self, fail=None, on_close=None):
        self.fail, self.on_close, self.closed = fail, on_close, []

    def __call__(self, time, x):
        who = int(x.flatten()[0])
        try:
            for k in range(100):
                if self.fail == (who, k):
                    raise FloatingPointError("non-finite values after the step")
                yield time + k * self.time_step, (x + k).reshape(1, 2, 3, 4), None
        finally:
            self.closed.append(who)
            if self.on_close is not None and self.on_close[0] == who:
                raise self.on_close[1]


def _seeds(M=3):
    return [torch.full((1, 1, 2, 3, 4), float(10 * m)) for m in range(M)]


def test_member_source_advances_all_members_in_order():
    model = _Fake()
    members = E.Members(model, T0, _seeds())
    for k in range(3):
        time, states = members.advance(k)
        assert time == T0 + k * model.time_step and len(states) == 3
        for m, st in enumerate(states):
            assert st.shape == (2, 3, 4) and st.is_contiguous() and torch.equal(st, torch.full((2, 3, 4), 10.0 * m + k))
    members.close()
    assert model.closed == [0, 10, 20]


def test_member_source_names_the_member_and_step_that_failed():
    members = E.Members(_Fake(fail=(20, 1)), T0, _seeds())
    members.advance(0)
    with pytest.raises(FloatingPointError, match=r"^ensemble member 2, step 1: non-finite values after the step$"):
        members.advance(1)
    members.close()


@pytest.mark.parametrize("error", [FloatingPointError("a pending check"), RuntimeError("a loop that will not close")])
def test_member_source_closes_every_loop_when_one_raises(error):
    """The second generator raises when it is closed: the third is closed all the same.  A loop's own pending non-finite check is
    dropped (every delivered step was checked by member); anything else comes out once every loop is closed."""
    model = _Fake(on_close=(10, error))
    members = E.Members(model, T0, _seeds())
    members.advance(0)
    if isinstance(error, FloatingPointError):
        members.close()
    else:
        with pytest.raises(RuntimeError, match="will not close"):
            members.close()
    assert model.closed == [0, 10, 20]
