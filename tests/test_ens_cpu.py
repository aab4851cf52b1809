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
