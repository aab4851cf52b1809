"""Bred perturbations without a GPU: the C ABI of include/skyrim_breed.h (exports, every argument error), ``breeding.factors`` against its
numpy restatement, every refusal of ``breeding.plan`` and of ``ensemble_forecast(breeding=...)``, the ``verify`` command's options, and
the compiler's resource report of the kernels."""
from __future__ import annotations

import ctypes
import datetime
import re
import shutil
import subprocess
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import _breed_reference as BR
from skyrim_amd import breeding as B
from skyrim_amd.core.models.base import GlobalModel
from skyrim_amd.pangu.spec import PanguGeometry

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "skyrim_breed.h"
T0 = datetime.datetime(2024, 5, 13, 18, 0)
FAKE = 4096                                                    # never dereferenced: the argument checks come first


# ---- 1. ABI --------------------------------------------------------------------------------------------------------------------------- #
def test_library_exports_every_declared_symbol():
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    syms = sorted(set(re.findall(r"\b(skbreed_[a-z0-9_]+)\s*\(", text)))
    lib = B.load_library()
    assert syms == sorted(B.EXPORTS) and len(syms) == 5
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in skyrim_breed.h but not exported"
    assert lib.skbreed_abi_version() == B.ABI_VERSION == 1 == int(re.search(r"SKBREED_ABI_VERSION (\d+)", text).group(1))
    for name, val in (("MAX_MEMBERS", B.MAX_MEMBERS), ("MAX_CHANNELS", B.MAX_CHANNELS), ("TILE", B.TILE), ("MAX_GROUPS", B.MAX_GROUPS)):
        assert int(re.search(rf"SKBREED_{name} (\d+)", text).group(1)) == val


def _table(ptrs):
    return None if ptrs is None else (ctypes.c_void_p * len(ptrs))(*ptrs)


def _addr(table):
    return None if table is None else ctypes.addressof(table)


def _norms_desc(M=3, C=2, H=5, W=8, **kw):
    host = _table(kw.pop("members_host", [FAKE * (2 + m) for m in range(max(M, 1))]))
    d = B.NormsDesc()
    d.y0, d.members, d.members_host, d.M, d.C, d.H, d.W = FAKE, FAKE, _addr(host), M, C, H, W
    d.lat_weight, d.S, d.workspace, d.workspace_bytes = FAKE, FAKE, FAKE, 1 << 30
    for k, v in kw.items():
        setattr(d, k, v)
    return d, host


def _apply_desc(M=3, C=2, H=5, W=8, **kw):
    n = 1 << 20                                                # the fake states lie 1 MiB apart: no overlap at these sizes
    members = _table(kw.pop("members_host", [n * (4 + m) for m in range(max(M, 1))]))
    out = _table(kw.pop("out_host", [n * (100 + m) for m in range(max(M, 1))]))
    d = B.ApplyDesc()
    d.x0, d.y0, d.members, d.members_host, d.out, d.out_host = n, 2 * n, FAKE, _addr(members), FAKE, _addr(out)
    d.M, d.C, d.H, d.W, d.f = M, C, H, W, FAKE
    for k, v in kw.items():
        setattr(d, k, v)
    return d, (members, out)


def test_argument_errors_need_no_gpu():
    lib = B.load_library()
    assert lib.skbreed_norms(None, None) == -1 and lib.skbreed_apply(None, None) == -1
    bad_norms = [dict(y0=None), dict(members=None), dict(members_host=None), dict(lat_weight=None), dict(S=None), dict(workspace=None),
                 dict(y0=FAKE + 2), dict(members=FAKE + 4), dict(members_host=[FAKE, FAKE + 1, FAKE]), dict(members_host=[FAKE, 0, FAKE]),
                 dict(lat_weight=FAKE + 4), dict(S=FAKE + 4), dict(workspace=FAKE + 4),
                 dict(M=0), dict(M=65), dict(C=0), dict(C=257), dict(H=0), dict(W=0), dict(C=256, H=1 << 12, W=1 << 12),
                 dict(workspace_bytes=B.workspace_bytes(3, 2, 5, 8) - 1)]
    for kw in bad_norms:
        d, keep = _norms_desc(**kw)
        assert lib.skbreed_norms(ctypes.byref(d), None) == -1, kw
    bad_apply = [dict(x0=None), dict(y0=None), dict(members=None), dict(members_host=None), dict(out=None), dict(out_host=None), dict(f=None),
                 dict(x0=(1 << 20) + 2), dict(y0=(2 << 20) + 1), dict(f=FAKE + 2), dict(members_host=[4 << 20, (5 << 20) + 2, 6 << 20]),
                 dict(out_host=[100 << 20, 0, 102 << 20]), dict(out_host=[100 << 20, (101 << 20) + 1, 102 << 20]),
                 dict(M=0), dict(M=65), dict(C=0), dict(C=257), dict(H=0), dict(W=0),
                 dict(out_host=[1 << 20, 101 << 20, 102 << 20]),              # out_0 is x_0
                 dict(out_host=[100 << 20, 2 << 20, 102 << 20]),              # out_1 is y_0
                 dict(out_host=[5 << 20, 101 << 20, 102 << 20]),              # out_0 is the y of member 1
                 dict(out_host=[100 << 20, 100 << 20, 102 << 20]),            # two outputs are one buffer
                 dict(out_host=[(4 << 20) + 16, 101 << 20, 102 << 20]),       # a partial overlap with its own y
                 dict(out_host=[(1 << 20) + 64, 101 << 20, 102 << 20])]       # ... and with x_0
    for kw in bad_apply:
        d, keep = _apply_desc(**kw)
        assert lib.skbreed_apply(ctypes.byref(d), None) == -1, kw
    # the workspace query
    assert B.workspace_bytes(3, 2, 5, 8) == 5 * 2 * 3 * 8                    # five tiles, one workgroup each
    assert B.workspace_bytes(50, 69, 721, 1440) == 60 * 69 * 50 * 8
    for bad in ((0, 2, 5, 8), (65, 2, 5, 8), (3, 0, 5, 8), (3, 257, 5, 8), (3, 2, 0, 8), (3, 2, 5, 0), (3, 256, 1 << 12, 1 << 12)):
        assert B.workspace_bytes(*bad) == 0, bad
    for C, H, W in ((1, 1, 1), (2, 5, 67), (69, 721, 1440), (256, 3, 300), (1, 721, 1440), (17, 1, 100000)):
        assert lib.skbreed_groups(C, H, W) == B.groups(C, H, W) >= 1
        assert 1 <= B.bound_k(C, H, W) <= H * W + H + 2
    assert lib.skbreed_groups(0, 5, 8) == 0


def test_ops_are_registered_and_have_no_cpu_kernel():
    from skyrim_amd import ops
    assert {"breed_norms", "breed_apply"} <= set(ops.OP_NAMES)
    z = torch.zeros(1, 2, 4)
    tab = torch.zeros(1, dtype=torch.int64)
    with pytest.raises(NotImplementedError):
        torch.ops.skyrim_hip.breed_norms(z, [z.clone()], tab, torch.ones(2, dtype=torch.float64), torch.zeros(1, 1, dtype=torch.float64),
                                         torch.zeros(8, dtype=torch.float64))
    with pytest.raises(NotImplementedError):
        torch.ops.skyrim_hip.breed_apply(z, z.clone(), [z.clone()], tab, torch.ones(1, 1), [z.clone()], tab)


# ---- 2. factors ------------------------------------------------------------------------------------------------------------------------- #
def _ulp_equal(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.all((a == b) | (np.abs(a.astype(np.float64) - b.astype(np.float64)) <= np.spacing(np.abs(b)).astype(np.float64)))


@pytest.mark.parametrize("norm", ["total", "channel"])
def test_factors_against_the_restatement(norm):
    rng = np.random.default_rng(5)
    M, C, n_lon, wsum = 6, 7, 192, 1.9
    S = rng.uniform(1e-9, 1e-3, (M, C))
    S[2, 3] = 0.0                                             # a channel without a difference
    S[4] = 0.0                                                # a member without any
    std = rng.uniform(0.1, 50.0, C)
    for mask in (None, np.array([True, False, True, True, False, True, True]), np.eye(C, dtype=bool)[5]):
        f = B.factors(torch.from_numpy(S), torch.from_numpy(std).float(), 1e-3, norm, mask, wsum, n_lon)
        assert f.dtype == torch.float32 and tuple(f.shape) == (M, C)
        ref = BR.factors(S, std.astype(np.float32), 1e-3, norm, mask, wsum, n_lon)
        assert _ulp_equal(f.numpy(), ref), (norm, mask)
        on = np.ones(C, bool) if mask is None else mask
        assert np.all(f.numpy()[:, ~on] == 0) and np.all(f.numpy()[4] == 0)
        if norm == "channel":
            assert f.numpy()[2, 3] == 0 and np.all(f.numpy()[[0, 1, 3, 5]][:, on] > 0)
        else:
            rows = f.numpy()[[0, 1, 2, 3, 5]][:, on]
            assert np.all(rows > 0) and np.all(rows == rows[:, :1])          # one factor per member
    # the definition itself, on numbers one can follow: A = S / (2 * 4)
    S = torch.tensor([[8.0, 0.0, 72.0]], dtype=torch.float64)
    std = torch.tensor([1.0, 2.0, 3.0])
    assert np.array_equal(B.factors(S, std, 0.5, "channel", None, 2.0, 4).numpy(), np.array([[0.5, 0.0, 0.5]], np.float32))
    assert np.array_equal(B.factors(S, std, 0.5, "total", [True, False, True], 2.0, 4).numpy(),
                          np.array([[0.5, 0.0, 0.5]], np.float32))           # mean of (1 / 1, 9 / 9) = 1
    one = B.factors(S, std, 0.5, "total", [False, False, True], 2.0, 4).numpy()
    assert np.array_equal(one, np.array([[0.0, 0.0, 0.5]], np.float32))      # a single perturbed channel: both norms agree
    assert np.array_equal(one, B.factors(S, std, 0.5, "channel", [False, False, True], 2.0, 4).numpy())
    assert np.all(B.factors(S, torch.zeros(3), 0.5, "total", None, 2.0, 4).numpy() == 0)       # no sigma: nothing is perturbed
    with pytest.raises(ValueError, match="choose from"):
        B.factors(S, std, 0.5, "energy", None, 2.0, 4)


def test_restated_norms_and_apply_on_numbers_one_can_follow():
    y0 = np.zeros((1, 2, 2), np.float32)
    mem = np.array([[[[1.0, 2.0], [3.0, 4.0]]]], np.float32)
    S, T = BR.norms(y0, mem, np.array([1.0, -0.5]))
    assert S[0, 0] == 5.0 - 12.5 and T[0, 0] == 5.0 + 12.5
    x0 = np.array([[[-0.0, 1.0], [np.inf, 2.0]]], np.float32)
    out = BR.apply(x0, y0, mem, np.array([[0.0]], np.float32))
    assert out.tobytes() == x0[None].tobytes()                               # f = 0: bits of x_0, the sign of the zero included
    out = BR.apply(x0, y0, mem, np.array([[-2.0]], np.float32))
    assert np.array_equal(out[0, 0], np.array([[-2.0, -3.0], [np.inf, -6.0]], np.float32))


# ---- 3. the request ------------------------------------------------------------------------------------------------------------------------ #
class _Loop:
    n_history_levels = 1
    time_step = datetime.timedelta(hours=6)
    device = torch.device("cpu")
    in_channel_names = out_channel_names = ["u1000", "v1000", "t2m"]
    geom = grid = PanguGeometry(9, 96)
    channel_std = torch.ones(3)

    def __call__(self, time, x, restart=None):
        raise AssertionError("a refused ensemble must not start a loop")


class _TwoLevels(_Loop):
    n_history_levels = 2


class _Forced(_Loop):
    in_channel_names = ["u1000", "v1000", "t2m", "tisr"]
    channel_std = torch.ones(4)


class _Model(GlobalModel):
    def __init__(self, loop=_Loop):
        self._loop = loop
        super().__init__("boring", ic_source="synthetic")

    def build_model(self):
        return self._loop()


def test_plan():
    m = _Loop()
    assert B.plan(m, None) is None
    p = B.plan(m, {"cycles": 3})
    assert (p.cycles, p.norm, p.paired) == (3, "total", False) and p.as_dict() == dict(cycles=3, norm="total", paired=False)
    assert B.plan(m, dict(cycles=50, norm="channel", paired=True)).as_dict() == dict(cycles=50, norm="channel", paired=True)
    for bad in (0, 51, -1, 2.0, "3", None, True):
        with pytest.raises(ValueError, match="cycles"):
            B.plan(m, {"cycles": bad})
    with pytest.raises(ValueError, match="cycles"):
        B.plan(m, {})
    with pytest.raises(ValueError, match="norm"):
        B.plan(m, {"cycles": 2, "norm": "energy"})
    with pytest.raises(ValueError, match="paired"):
        B.plan(m, {"cycles": 2, "paired": 1})
    with pytest.raises(ValueError, match=r"unknown keys \['cycle', 'orthogonal'\]"):
        B.plan(m, {"cycle": 2, "cycles": 2, "orthogonal": True})
    with pytest.raises(ValueError, match="dict"):
        B.plan(m, 3)
    with pytest.raises(ValueError, match="2 history levels"):
        B.plan(_TwoLevels(), {"cycles": 2})
    with pytest.raises(ValueError, match="forcing"):
        B.plan(_Forced(), {"cycles": 2})


def test_the_models_that_are_bred_and_those_that_are_not():
    """The history levels of the real TimeLoop classes, read without building an engine."""
    from skyrim_amd.dlwp.timeloop import DlwpTimeLoop
    from skyrim_amd.fcn.timeloop import FcnTimeLoop
    from skyrim_amd.fengwu.timeloop import FengwuTimeLoop
    from skyrim_amd.fuxi.timeloop import FuxiTimeLoop
    from skyrim_amd.pangu.timeloop import PanguTimeLoop
    names = ["a", "b"]
    for cls in (PanguTimeLoop, FcnTimeLoop):
        loop = SimpleNamespace(n_history_levels=cls.n_history_levels, in_channel_names=names, out_channel_names=names)
        assert B.plan(loop, {"cycles": 1}).cycles == 1
    for cls in (DlwpTimeLoop, FuxiTimeLoop, FengwuTimeLoop):
        with pytest.raises(ValueError, match="2 history levels"):
            B.plan(SimpleNamespace(n_history_levels=cls.n_history_levels, in_channel_names=names, out_channel_names=names), {"cycles": 1})


def test_refusals_through_ensemble_forecast():
    from skyrim_amd.core.models.ensemble import GlobalEnsemble
    from skyrim_amd.core.models.graphcast import GraphcastModel
    m = _Model()
    with pytest.raises(ValueError, match="2 history levels"):
        _Model(_TwoLevels).ensemble_forecast(T0, breeding={"cycles": 2})
    with pytest.raises(ValueError, match="forcing"):
        _Model(_Forced).ensemble_forecast(T0, breeding={"cycles": 2})
    for bad, what in (({"cycles": 0}, "cycles"), ({"cycles": 51}, "cycles"), ({"cycles": 2, "norm": "rms"}, "norm"),
                      ({"cycles": 2, "rescale": 1}, "unknown keys"), ({"norm": "total"}, "cycles")):
        with pytest.raises(ValueError, match=what):
            m.ensemble_forecast(T0, breeding=bad)
    with pytest.raises(ValueError, match="choose from"):
        m.ensemble_forecast(T0, perturbation="bred", breeding={"cycles": 2})   # the kind names the seed; "bred" is not one
    with pytest.raises(ValueError, match="multi-model"):
        GlobalEnsemble(["pangu", "fuxi"], ic_source="synthetic").ensemble_forecast(T0, breeding={"cycles": 2})
    with pytest.raises(NotImplementedError, match="stepper"):
        GraphcastModel.ensemble_forecast(object.__new__(GraphcastModel), T0, breeding={"cycles": 2})
    for kw in (dict(breeding={"cycles": 2}), dict(breeding=dict(cycles=1, norm="channel", paired=True), perturbation="spherical", lmax=9),
               dict(breeding={"cycles": 3}, perturb_channels=["t2m"])):
        with pytest.raises(RuntimeError, match="the model must be on a GPU"):
            m.ensemble_forecast(T0, n_members=3, **kw)                        # everything valid: the members themselves need the device


def test_signatures_dataclass_and_the_verify_command():
    import inspect
    from click.testing import CliRunner
    from skyrim_amd import ensemble as E
    from skyrim_amd import ensemble_cli, verify_cli
    from skyrim_amd.core import Skyrim
    ens = E.EnsembleForecast("pangu", 3, 0, 1e-3)
    assert ens.breeding is None and ens.breeding_growth is None
    for fn in (E.run, GlobalModel.ensemble_forecast, E.validate):
        assert inspect.signature(fn).parameters["breeding"].default is None
    assert any(p.kind is inspect.Parameter.VAR_KEYWORD for p in inspect.signature(Skyrim.ensemble_forecast).parameters.values())
    res = CliRunner().invoke(verify_cli.verify, ["--help"])
    assert res.exit_code == 0
    for opt in ("--breed_cycles", "--breed_norm", "[total|channel]", "--breed_paired"):
        assert opt in res.output, opt
    v = {p.name: p for p in verify_cli.verify.params}
    assert v["breed_cycles"].default == 0 and v["breed_norm"].default == "total" and v["breed_paired"].is_flag
    assert not {"breed_cycles", "breed_norm", "breed_paired"} & {p.name for p in ensemble_cli.ensemble.params}
    d = inspect.signature(verify_cli.run_verify).parameters
    assert d["breed_cycles"].default == 0 and d["breed_norm"].default == "total" and d["breed_paired"].default is False


# ---- 4. the compiler's resource report ------------------------------------------------------------------------------------------------ #
@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not installed")
def test_kernels_use_no_scratch():
    r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "--cuda-device-only", "-c",
                        "breed_ops.hip", "-o", "/dev/null", "-Rpass-analysis=kernel-resource-usage"], cwd=ROOT / "skyrim_amd" / "csrc",
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    out, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            out[name] = {}
        for key, short in (("ScratchSize [bytes/lane]", "scratch"), ("Occupancy [waves/SIMD]", "occupancy"), ("VGPRs", "vgprs")):
            m = re.search(r"\s" + re.escape(key) + r": (\d+)", line)
            if m and name:
                out[name][short] = int(m.group(1))
    for kernel, n in (("norms_kernel", 2), ("apply_kernel", 2), ("fold_kernel", 1)):
        rows = [v for k, v in out.items() if kernel in k]
        assert len(rows) == n and all(v["scratch"] == 0 and v["occupancy"] >= 8 and v["vgprs"] <= 64 for v in rows), (kernel, out)
