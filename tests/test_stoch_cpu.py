"""Per-step stochastic perturbations without a GPU: the C ABI of include/skyrim_stoch.h (exports, every argument error), the restatements
of tests/_stoch_reference.py, every refusal of ``ensemble_forecast(stochastic=...)``, the autoregressive factors, ``validate`` without the
new keyword, the ``verify`` command's flags, and the compiler's resource report of the kernels."""
from __future__ import annotations

import datetime
import inspect
import math
import re
import shutil
import subprocess
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import _noise_reference as NR
import _stoch_reference as SR
from skyrim_amd import noise as N
from skyrim_amd import stochastic as S
from skyrim_amd.core.models.base import GlobalModel
from skyrim_amd.pangu.spec import PanguGeometry

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "skyrim_stoch.h"
T0 = datetime.datetime(2024, 5, 13, 18, 0)
E_ARG = -1


# ---- 1. ABI --------------------------------------------------------------------------------------------------------------------------- #
def test_library_exports_every_declared_symbol():
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    syms = sorted(set(re.findall(r"\b(skstoch_[a-z0-9_]+)\s*\(", text)))
    lib = S.load_library()
    assert syms == sorted(S.EXPORTS) and len(syms) == 4
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in skyrim_stoch.h but not exported"
    assert lib.skstoch_abi_version() == S.ABI_VERSION == int(re.search(r"SKSTOCH_ABI_VERSION (\d+)", text).group(1))
    assert int(re.search(r"SKSTOCH_E_ARG \((-\d+)\)", text).group(1)) == E_ARG
    assert int(re.search(r"SKSTOCH_MAX_LMAX (\d+)", text).group(1)) == N.MAX_LMAX
    assert int(re.search(r"SKSTOCH_MAX_DRAW (0x[0-9A-Fa-f]+)u", text).group(1), 16) == S.MAX_DRAW == 2 ** 32 - 2
    noise_h = (ROOT / "include" / "skyrim_noise.h").read_text()
    assert "SKNOISE_ABI_VERSION 1" in noise_h and N.ABI_VERSION == 1                 # the header this one builds on is where it was


def test_argument_errors_need_no_gpu():
    lib = S.load_library()
    a, b, c, d, e, f, g = (4096 * k for k in range(1, 8))      # never dereferenced: the argument checks come first
    for call, tail in ((lib.skstoch_coeffs, ()), (lib.skstoch_evolve, (0.5, 0.5))):
        assert call(None, b, 8, 1, 0, 0, 1, 1, 1, *tail, None) == E_ARG
        assert call(a, None, 8, 1, 0, 0, 1, 1, 1, *tail, None) == E_ARG
        assert call(a + 2, b, 8, 1, 0, 0, 1, 1, 1, *tail, None) == E_ARG                     # a misaligned state
        assert call(a, b + 1, 8, 1, 0, 0, 1, 1, 1, *tail, None) == E_ARG                     # a misaligned table
        assert call(a, b, 0, 1, 0, 0, 1, 1, 1, *tail, None) == E_ARG                         # lmax < 1
        assert call(a, b, N.MAX_LMAX + 1, 1, 0, 0, 1, 1, 1, *tail, None) == E_ARG
        assert call(a, b, 8, 0, 0, 0, 1, 1, 1, *tail, None) == E_ARG                         # F < 1
        assert call(a, b, 8, 1, 0, 0, 1, 0, 1, *tail, None) == E_ARG                         # no member
        assert call(a, b, 8, 1, 0, 0, 1, 65536, 1, *tail, None) == E_ARG                     # more members than a grid's y extent
        assert call(a, b, 8, 2, 2 ** 32 - 1, 0, 1, 1, 1, *tail, None) == E_ARG               # the field index leaves 32 bits
        assert call(a, b, 4096, 2 ** 31 - 1, 0, 0, 1, 1, 1, *tail, None) == E_ARG            # the item index leaves 32 bits
        assert call(a, b, 8, 1, 0, 0, 1, 1, 2 ** 32 - 1, *tail, None) == E_ARG               # 1 + draw would wrap to white noise's word
    for phi, psi in ((float("nan"), 0.5), (0.5, float("inf"))):
        assert lib.skstoch_evolve(a, b, 8, 1, 0, 0, 1, 1, 1, phi, psi, None) == E_ARG
    ok = (a, b, c, d, e, f, 0.9, g, 16, 4, 4, None)            # xp, xn, r, y, gs, ga, lim, out, n, chan_stride, C, stream

    def apply(**kw):
        names = ("xp", "xn", "r", "y", "gs", "ga", "lim", "out", "n", "chan_stride", "C", "stream")
        return lib.skstoch_apply(*[kw.get(k, v) for k, v in zip(names, ok)])
    assert apply(xn=None) == E_ARG and apply(out=None) == E_ARG and apply(xp=None) == E_ARG      # (xp is read by the SPPT term)
    assert apply(r=None, y=None, gs=None, ga=None) == E_ARG                                       # both terms NULL
    assert apply(r=None) == E_ARG and apply(gs=None) == E_ARG and apply(y=None) == E_ARG and apply(ga=None) == E_ARG      # half a pair
    for name in ("xp", "xn", "r", "y", "gs", "ga", "out"):
        assert apply(**{name: dict(zip(("xp", "xn", "r", "y", "gs", "ga"), ok)).get(name, g) + 2}) == E_ARG, name          # misaligned
    for lim in (0.0, 1.5, -0.5, float("nan")):
        assert apply(lim=lim) == E_ARG, lim
    assert apply(out=a) == E_ARG                                                                  # out == xp
    assert apply(n=18) == E_ARG and apply(n=24) == E_ARG                                         # n is not L * C * chan_stride
    assert apply(n=0) == E_ARG and apply(chan_stride=0) == E_ARG and apply(C=0) == E_ARG and apply(n=2 ** 32) == E_ARG


def test_ops_are_registered_and_have_no_cpu_kernel():
    from skyrim_amd import ops
    assert {"stoch_coeffs", "stoch_evolve", "stoch_apply"} <= set(ops.OP_NAMES)
    with pytest.raises(NotImplementedError):
        torch.ops.skyrim_hip.stoch_coeffs(torch.zeros(8 * 8 * 2), torch.ones(8), 1, 0, 0, 1, 1)
    with pytest.raises(NotImplementedError):
        torch.ops.skyrim_hip.stoch_evolve(torch.zeros(8 * 8 * 2), torch.ones(8), 1, 0, 0, 1, 2, 0.5, 0.5)
    with pytest.raises(NotImplementedError):
        torch.ops.skyrim_hip.stoch_apply(torch.zeros(4), torch.zeros(4), torch.zeros(4), None, torch.ones(1), None, 0.9, torch.zeros(4), 4)


# ---- 2. the restatements ---------------------------------------------------------------------------------------------------------------- #
def test_restated_draws():
    t = N.spectrum(16)
    a0, b0 = SR.coefficients(5, 3, np.arange(3), 16, t, 0)
    ref, bref = NR.coefficients(5, 3, np.arange(3), 16, t)
    assert np.array_equal(a0, ref) and np.array_equal(b0, bref)                  # draw 0 is the initial-condition draw
    draws = [SR.coefficients(5, 3, np.arange(3), 16, t, d)[0] for d in SR.DRAWS]
    live = SR.live_mask(16)
    for i, a in enumerate(draws):
        assert np.all(a[~live] == 0) and np.all(a[live] != 0)
        assert all(not np.any(a[live] == o[live]) for o in [a0] + draws[:i])    # another counter word: no value repeats


def test_fma_emulation():
    for L, C, hw in SR.APPLY_SHAPES:
        xp, xn, r, y, gs, ga = SR.apply_inputs(L, C, hw)
        g = np.repeat(np.tile(gs, L), hw)
        w = np.fmin(np.fmax(g * np.tile(r, L * C), -np.float32(SR.LIM)), np.float32(SR.LIM))
        assert SR.fma32_is_exact(w, xn - xp, xn)
        t = SR.apply(xp, xn, r, None, gs, None, SR.LIM, C, hw)
        assert SR.fma32_is_exact(np.repeat(np.tile(ga, L), hw), y, t)
    # the fused operation, not mul-then-add
    g, y, x = np.float32(1 + 2.0 ** -12), np.float32(1 + 2.0 ** -12), np.float32(-1.0)
    assert SR.fma32(g, y, x) != np.float32(g * y) + x
    # a case the float64 route rounds twice: a b = 2^-24 - 2^-70, so 1 + 2^-23 + a b lies just BELOW a float32 tie and the float64 sum ON it
    a, b, c = np.float32(2.0 ** -12 + 2.0 ** -35), np.float32(2.0 ** -12 - 2.0 ** -35), np.float32(1 + 2.0 ** -23)
    assert not SR.fma32_is_exact(a, b, c) and NR.fma32(a, b, c) == np.float32(1 + 2.0 ** -22)      # (tie to even: up)
    assert SR.fma32(a, b, c) == np.float32(1 + 2.0 ** -23)                       # the correctly rounded fma: down
    assert SR.evolve(np.float32(3.0), np.float32(0.0), 0.5, 0.7) == np.float32(1.5) and SR.evolve(0.0, 0.0, 0.5, 0.7).view(np.uint32) == 0


def test_apply_restatement_clips_and_copies():
    xp, xn, r, y, gs, ga = SR.apply_inputs(1, 3, 1000)
    out = SR.apply(xp, xn, r, y, gs, ga, SR.LIM, 3, 1000).reshape(3, 1000)
    x = xn.reshape(3, 1000)
    assert np.array_equal(out[1].view(np.uint32), x[1].view(np.uint32))          # both amplitudes 0: a bit copy
    only_add = SR.apply(None, xn, None, y, None, ga, SR.LIM, 3, 1000).reshape(3, 1000)
    assert np.array_equal(out[2], only_add[2]) and not np.array_equal(out[0], only_add[0])
    w = (out[0].astype(np.float64) - only_add[0]) / (x[0].astype(np.float64) - xp.reshape(3, 1000)[0])
    assert np.nanmax(np.abs(w)) <= SR.LIM * (1 + 1e-3)                           # the multiplier never leaves +-lim


# ---- 3. host logic -------------------------------------------------------------------------------------------------------------------- #
class _Loop:
    n_history_levels = 1
    time_step = datetime.timedelta(hours=6)
    device = torch.device("cpu")
    in_channel_names = out_channel_names = ["u1000", "v1000", "t2m"]
    geom = grid = PanguGeometry(9, 96)
    channel_std = torch.ones(3)

    def __call__(self, time, x, restart=None):
        raise AssertionError("a refused ensemble must not start a loop")


class _Model(GlobalModel):
    def __init__(self):
        super().__init__("boring", ic_source="synthetic")

    def build_model(self):
        return _Loop()


def _loop(**kw):
    loop = _Loop()
    for k, v in kw.items():
        setattr(loop, k, v)
    return loop


def test_plan_defaults_and_record():
    assert S.plan(_Loop(), None) is None
    p = S.plan(_Loop(), dict(kind="sppt"), 1e-3)
    assert (p.kind, p.amplitude, p.clip, p.tau_h, p.sppt, p.additive) == ("sppt", 0.3, 0.9, 6.0, True, False)
    assert (p.spectrum.lmax, p.spectrum.length_scale_km, p.spectrum.alpha) == (9, 500.0, 2.0) and p.channel_mask is None
    assert p.spectrum.e == N.scale_exponent(N.spectrum(9)) and (p.phi, p.psi) == S.ar1(6.0, 6.0)
    assert p.as_dict() == dict(kind="sppt", amplitude=0.3, clip=0.9, additive_scale=1e-3, tau_h=6.0, length_scale_km=500.0, alpha=2.0,
                               lmax=9, channels=None)
    q = S.plan(_Loop(), dict(kind="both", amplitude=0.5, clip=1.0, additive_scale=2e-3, tau_h=0, length_scale_km=800.0, alpha=1.5, lmax=7,
                             channels=["t2m"]))
    assert (q.sppt, q.additive, q.phi, q.psi, q.additive_scale) == (True, True, 0.0, 1.0, 2e-3) and q.channel_mask.tolist() == [False, False, True]
    assert S.plan(_Loop(), dict(kind="sppt"), 0.0).kind == "sppt"               # perturb_scale = 0: the SPPT term needs no additive scale


def test_refusals_of_plan():
    ok = dict(kind="both")
    for bad, match in (("sppt", "None or a dict"), (dict(kind="sppt", tau=3.0), "unknown keys"), (dict(), "kind"), (dict(kind="skeb"), "kind"),
                       (dict(ok, amplitude=0.0), "amplitude"), (dict(ok, amplitude=float("nan")), "amplitude"), (dict(ok, amplitude="big"), "amplitude"),
                       (dict(ok, clip=0.0), "clip"), (dict(ok, clip=1.5), "clip"), (dict(ok, additive_scale=0.0), "additive_scale"),
                       (dict(ok, additive_scale=-1e-3), "additive_scale"), (dict(ok, tau_h=-1.0), "tau_h"), (dict(ok, tau_h=float("inf")), "tau_h"),
                       (dict(ok, length_scale_km=0.0), "length_scale_km"), (dict(ok, lmax=1), "lmax"), (dict(ok, lmax=10), "lmax"),
                       (dict(ok, lmax=2.5), "lmax"), (dict(ok, channels=["t2m", "nope"]), "not input channels"), (dict(ok, channels=[]), "channels"),
                       (dict(ok, length_scale_km=20000.0, alpha=12.0), "dynamic range")):
        with pytest.raises(ValueError, match=match):
            S.plan(_Loop(), bad, 1e-3)
    with pytest.raises(ValueError, match="perturb_scale"):
        S.plan(_Loop(), dict(kind="additive"), 0.0)                            # the additive term's default scale would be 0
    with pytest.raises(ValueError, match="stochastic.*history levels"):
        S.plan(_loop(n_history_levels=2), ok)
    with pytest.raises(ValueError, match="stochastic.*not its output channels"):
        S.plan(_loop(in_channel_names=["u1000", "v1000", "t2m", "zenith"]), ok)
    with pytest.raises(ValueError, match="24-h network"):
        S.plan(_loop(engine24=object()), ok)
    gauss = np.degrees(np.arcsin(np.polynomial.legendre.leggauss(32)[0][::-1]))
    with pytest.raises(ValueError, match="32 x 64 grid"):
        S.plan(_loop(grid=SimpleNamespace(lat=gauss, lon=360.0 / 64 * np.arange(64))), ok)


def test_refusals_through_the_interface():
    from skyrim_amd.core.models.ensemble import GlobalEnsemble
    from skyrim_amd.core.models.graphcast import GraphcastModel
    m = _Model()
    with pytest.raises(ValueError, match="unknown keys"):
        m.ensemble_forecast(T0, stochastic=dict(kind="sppt", scale=1.0))
    with pytest.raises(ValueError, match="clip"):
        m.ensemble_forecast(T0, stochastic=dict(kind="sppt", clip=2.0), breeding=dict(cycles=1))
    with pytest.raises(ValueError, match="cycles"):
        m.ensemble_forecast(T0, stochastic=dict(kind="sppt"), breeding=dict(cycles=0))
    for kw in (dict(stochastic=dict(kind="sppt")), dict(stochastic=dict(kind="both", tau_h=0.0, channels=["t2m"]), perturbation="spherical"),
               dict(stochastic=dict(kind="additive"), breeding=dict(cycles=1), perturb_scale=0.01)):
        with pytest.raises(RuntimeError, match="GPU"):
            m.ensemble_forecast(T0, n_members=3, **kw)                         # everything valid: the members themselves need the device
    with pytest.raises(ValueError, match="multi-model"):
        GlobalEnsemble(["pangu", "fuxi"], ic_source="synthetic").ensemble_forecast(T0, stochastic=dict(kind="sppt"))
    with pytest.raises(NotImplementedError, match="stepper"):
        GraphcastModel.ensemble_forecast(object.__new__(GraphcastModel), T0, stochastic=dict(kind="sppt"))


def test_autoregressive_factors():
    assert S.ar1(6.0, 0.0) == (0.0, 1.0)                                        # white in time
    phi, psi = S.ar1(6.0, 6.0)                                                  # tau = dt
    assert phi == float(np.float32(math.exp(-1.0))) and psi == float(np.float32(math.sqrt(1.0 - math.exp(-2.0))))
    for dt, tau in ((6.0, 6.0), (6.0, 1.0), (6.0, 72.0), (1.0, 6.0), (24.0, 3.0), (6.0, 1e-3), (6.0, 1e6)):
        phi, psi = S.ar1(dt, tau)
        assert phi == float(np.float32(phi)) and psi == float(np.float32(psi)) and 0 <= phi <= 1 and 0 <= psi <= 1
        assert abs(phi * phi + psi * psi - 1.0) <= 2.0 ** -23, (dt, tau)
        assert abs(phi - math.exp(-dt / tau)) <= 2.0 ** -24 * math.exp(-dt / tau)
    assert S.plan(_loop(time_step=datetime.timedelta(hours=1)), dict(kind="sppt", tau_h=3.0)).phi == S.ar1(1.0, 3.0)[0]


def test_validate_and_signatures_without_the_keyword():
    from skyrim_amd import ensemble as E
    m = _Model()
    args = (m.model, 2, 3, 0, ("mean",), {"t2m": [280.0]}, {"t2m": [0.5]}, None, 1, False)
    plain = E.validate(*args)
    assert plain == E.validate(*args, stochastic=None) == E.validate(*args, stochastic=dict(kind="both"))
    assert plain == (("mean",), {"t2m": [280.0]}, {"t2m": [0.5]}, [0, 1, 2])
    with pytest.raises(ValueError, match="kind"):
        E.validate(*args, stochastic=dict(kind="spp"))
    for fn in (E.run, GlobalModel.ensemble_forecast, E.validate):
        names = list(inspect.signature(fn).parameters)
        assert inspect.signature(fn).parameters["stochastic"].default is None
        assert names[names.index("stochastic") - 1] == "breeding"              # next to the other way of making members
        assert names[-5:] == ["perturbation", "length_scale_km", "alpha", "lmax", "perturb_channels"]
    assert E.EnsembleForecast("pangu", 3, 0, 1e-3).stochastic is None


def test_verify_command_lists_the_new_options():
    from click.testing import CliRunner
    from skyrim_amd import ensemble_cli, verify_cli
    res = CliRunner().invoke(verify_cli.verify, ["--help"])
    assert res.exit_code == 0
    for opt in ("--stochastic", "[sppt|additive|both]", "--stoch_amplitude", "--stoch_tau_h", "--stoch_length_scale_km"):
        assert opt in res.output, opt
    v = {p.name: p for p in verify_cli.verify.params}
    assert all(v[k].default is None for k in ("stochastic", "stoch_amplitude", "stoch_tau_h", "stoch_length_scale_km"))
    assert not {"stochastic", "stoch_amplitude", "stoch_tau_h", "stoch_length_scale_km"} & {p.name for p in ensemble_cli.ensemble.params}
    d = inspect.signature(verify_cli.run_verify).parameters
    assert all(d[k].default is None for k in ("stochastic", "stoch_amplitude", "stoch_tau_h", "stoch_length_scale_km"))


def test_verify_command_passes_the_request_through(monkeypatch):
    from skyrim_amd import verify_cli
    from skyrim_amd.core import Skyrim
    seen = {}

    class _Done(Exception):
        pass

    class _Fake:
        model = SimpleNamespace(time_step=datetime.timedelta(hours=6))

        def __init__(self, *a, **kw):
            pass

        def ensemble_forecast(self, *a, **kw):
            seen.update(kw)
            raise _Done

    monkeypatch.setattr("skyrim_amd.core.Skyrim", _Fake)
    base = ("pangu", "20240513", "1800", 6, False, "gfs", "", "")
    with pytest.raises(_Done):
        verify_cli.run_verify(*base, members=4, stochastic="both", stoch_amplitude=0.4, stoch_tau_h=12.0, stoch_length_scale_km=800.0)
    assert seen["stochastic"] == dict(kind="both", amplitude=0.4, tau_h=12.0, length_scale_km=800.0)
    seen.clear()
    with pytest.raises(_Done):
        verify_cli.run_verify(*base, members=4, stochastic="sppt")
    assert seen["stochastic"] == dict(kind="sppt")
    seen.clear()
    with pytest.raises(_Done):
        verify_cli.run_verify(*base, members=4)
    assert "stochastic" not in seen                                              # without the flag the call is what it was
    with pytest.raises(ValueError, match="--stochastic"):
        verify_cli.run_verify(*base, members=4, stoch_tau_h=3.0)
    assert Skyrim is not _Fake


# ---- 4. the compiler's resource report ------------------------------------------------------------------------------------------------ #
@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not installed")
def test_kernels_use_no_scratch():
    make = (ROOT / "skyrim_amd" / "csrc" / "Makefile").read_text()
    assert "$(HIPCC) $(CXXFLAGS) -shared -o $@ stoch_ops.hip" in make            # the flags of noise_ops.hip: draw 0 shares its bits
    r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "--cuda-device-only", "-c",
                        "stoch_ops.hip", "-o", "/dev/null", "-Rpass-analysis=kernel-resource-usage"], cwd=ROOT / "skyrim_amd" / "csrc",
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    out, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            out[name] = {}
        for key, short in (("ScratchSize [bytes/lane]", "scratch"), ("Occupancy [waves/SIMD]", "occupancy"), ("LDS Size [bytes/block]", "lds")):
            m = re.search(re.escape(key) + r": (\d+)", line)
            if m and name:
                out[name][short] = int(m.group(1))
    for kernel, count in (("coeffs_kernel", 2), ("apply_kernel", 3)):
        rows = [v for k, v in out.items() if kernel in k]
        assert len(rows) == count and all(v["scratch"] == 0 and v["lds"] == 0 and v["occupancy"] >= 4 for v in rows), (kernel, out)
