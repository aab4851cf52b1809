"""Spherical perturbations without a GPU: the C ABI of include/skyrim_noise.h (exports, argument errors), the host-side definitions in
float64 (spectrum, unit variance on the real transform matrices, the power-of-two rule), the restated coefficients, every refusal of
``ensemble_forecast``'s new keywords, the ``verify`` command's options, and the compiler's resource report of the two kernels."""
from __future__ import annotations

import datetime
import re
import shutil
import subprocess
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import _noise_reference as NR
from skyrim_amd import noise as N
from skyrim_amd.core.models.base import GlobalModel
from skyrim_amd.pangu.spec import PanguGeometry

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "skyrim_noise.h"
T0 = datetime.datetime(2024, 5, 13, 18, 0)


# ---- 1. ABI --------------------------------------------------------------------------------------------------------------------------- #
def test_library_exports_every_declared_symbol():
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    syms = sorted(set(re.findall(r"\b(sknoise_[a-z0-9_]+)\s*\(", text)))
    lib = N.load_library()
    assert syms == sorted(N.EXPORTS) and len(syms) == 3
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in skyrim_noise.h but not exported"
    assert lib.sknoise_abi_version() == N.ABI_VERSION == int(re.search(r"SKNOISE_ABI_VERSION (\d+)", text).group(1))
    assert int(re.search(r"SKNOISE_MAX_LMAX (\d+)", text).group(1)) == N.MAX_LMAX


def test_argument_errors_need_no_gpu():
    lib = N.load_library()
    fake = 4096                                                # never dereferenced: the argument checks come first
    assert lib.sknoise_coeffs(None, None, 8, 1, 0, 0, 1, 1, None) == -1
    assert lib.sknoise_coeffs(fake, None, 8, 1, 0, 0, 1, 1, None) == -1
    assert lib.sknoise_coeffs(fake, fake, 0, 1, 0, 0, 1, 1, None) == -1                       # lmax < 1
    assert lib.sknoise_coeffs(fake, fake, N.MAX_LMAX + 1, 1, 0, 0, 1, 1, None) == -1
    assert lib.sknoise_coeffs(fake, fake, 8, 0, 0, 0, 1, 1, None) == -1                       # F < 1
    assert lib.sknoise_coeffs(fake, fake, 8, 1, 0, 0, 1, 0, None) == -1                       # no member
    assert lib.sknoise_coeffs(fake + 2, fake, 8, 1, 0, 0, 1, 1, None) == -1                   # a misaligned out
    assert lib.sknoise_coeffs(fake, fake, 8, 2, 2 ** 32 - 1, 0, 1, 1, None) == -1             # the field index leaves 32 bits
    assert lib.sknoise_apply(None, None, None, None, 16, 4, 4, None) == -1
    assert lib.sknoise_apply(fake, fake, fake, fake + 1, 16, 4, 4, None) == -1                # a misaligned out
    assert lib.sknoise_apply(fake, fake, fake, fake, 0, 4, 4, None) == -1
    assert lib.sknoise_apply(fake, fake, fake, fake, 18, 4, 4, None) == -1                    # n is not L * C * chan_stride
    assert lib.sknoise_apply(fake, fake, fake, fake, 16, 4, 0, None) == -1


def test_ops_are_registered_and_have_no_cpu_kernel():
    from skyrim_amd import ops
    assert {"noise_coeffs", "noise_apply"} <= set(ops.OP_NAMES)
    with pytest.raises(NotImplementedError):
        torch.ops.skyrim_hip.noise_coeffs(torch.zeros(8 * 8 * 2), torch.ones(8), 1, 0, 0, 1)
    with pytest.raises(NotImplementedError):
        torch.ops.skyrim_hip.noise_apply(torch.zeros(4), torch.zeros(4), torch.ones(1), torch.zeros(4), 4)


# ---- 2. spectrum, variance, the power of two -------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize("lmax,scale,alpha", [(2, 500.0, 2.0), (32, 500.0, 2.0), (256, 500.0, 2.0), (720, 250.0, 2.0), (49, 2000.0, 3.0)])
def test_spectrum_is_normalised(lmax, scale, alpha):
    s = N.spectrum(lmax, scale, alpha)
    l = np.arange(lmax)
    assert s.dtype == np.float64 and s[0] == 0.0 and np.all(s[1:] > 0)
    assert abs(np.sum((2 * l + 1) * s * s) / (4 * np.pi) - 1.0) <= 1e-14
    assert np.allclose(s, NR.spectrum(lmax, scale, alpha), rtol=1e-15, atol=0)
    kappa2 = (6371.0 / scale) ** 2
    assert np.allclose(s[1:-1] / s[2:], ((kappa2 + l[2:] * (l[2:] + 1)) / (kappa2 + l[1:-1] * (l[1:-1] + 1))) ** (alpha / 2), rtol=1e-13)


@pytest.mark.parametrize("n_lat,n_lon,lmax", [(33, 64, 32), (49, 192, 49)])
def test_unit_variance_at_every_latitude_on_the_real_matrices(n_lat, n_lon, lmax):
    """The addition theorem on the matrices the device multiplies with (fp32-rounded, hence 1e-5): with every order present
    sum_l sigma_l^2 (Pbar_l0^2 + 2 sum_{m >= 1} Pbar_lm^2) = 1 at every row, the poles (only m = 0 survives) included."""
    from skyrim_amd.sfno.sht import ShtMatrices
    p = ShtMatrices(n_lat, n_lon, lmax, lmax, "equiangular").synthesis.astype(np.float64)      # [m][lat][l]
    s = N.spectrum(lmax)
    cm = np.where(np.arange(lmax) == 0, 1.0, 2.0)
    var = np.einsum("m,mkl,l->k", cm, p * p, s * s)
    print(f"{n_lat} x {n_lon}, lmax {lmax}: |variance - 1| <= {np.abs(var - 1).max():.2e}")
    assert np.abs(var - 1).max() <= 1e-5
    assert np.all(p[1:, 0, :] == 0) and np.abs(p[1:, -1, :]).max() < 1e-12             # the poles hold the zonal order alone


def test_scale_exponent_rule_and_refusal():
    for lmax in (7, 32, 49, 128, 256, 720):
        s = N.spectrum(lmax)
        e = N.scale_exponent(s)
        nz = s[s > 0]
        assert 0.25 <= nz.min() * 2.0 ** e < 0.5 and 6.5 * nz.max() * 2.0 ** e <= 2.0 ** 14, lmax
    assert N.scale_exponent(np.array([0.0, 1.0, 0.25])) == 0 and N.scale_exponent(np.array([0.0, 0.2499, 3.0])) == 1
    assert N.scale_exponent(np.array([0.0, 2.0 ** -40])) == 38
    assert N.scale_exponent(np.array([0.0, 1.0, 5041.0 / 2])) == -2                    # the range that always fits (header)
    with pytest.raises(ValueError, match="dynamic range"):
        N.scale_exponent(np.array([0.0, 1.0, 1.1e4]))
    with pytest.raises(ValueError, match="dynamic range"):
        N.scale_exponent(N.spectrum(256, 500.0, 4.0))
    with pytest.raises(ValueError):
        N.scale_exponent(np.zeros(4))


# ---- 3. the restated coefficients ------------------------------------------------------------------------------------------------------- #
def test_restated_coefficients_do_not_depend_on_lmax_or_the_field_set():
    t32 = N.spectrum(32)
    a8, _ = NR.coefficients(5, 3, np.arange(4), 8, t32[:8])
    a32, b32 = NR.coefficients(5, 3, np.arange(4), 32, t32)
    assert np.array_equal(a8, a32[:8, :8])                                     # the common coefficients, bit for bit
    one, _ = NR.coefficients(5, 3, np.array([2]), 32, t32)
    assert np.array_equal(one[..., 0], a32[..., 2])
    l, m = np.arange(32)[:, None], np.arange(32)[None, :]
    dead = (m > l) | (l == 0)
    assert np.all(a32[dead] == 0) and np.all(a32[:, 0, 1, :] == 0) and np.all(b32[dead] == 0)
    assert np.all(a32[~dead][:, 0, :] != 0)
    other, _ = NR.coefficients(5, 4, np.arange(4), 32, t32)
    assert not np.array_equal(other, a32)
    # disjoint from the white-noise stream: counter word 3 is 1 there, 0 here
    import _ens_reference as R
    z_white = R.normals(5, 3, 4)
    assert not np.array_equal(NR.normals4(5, 3, 0, 0, 0), z_white)


def test_restated_coefficients_have_the_spectrum():
    """Per degree, sum over m, fields and members of |a_lm|^2 with the Hermitian weight (1 for m = 0, 2 above) is
    sigma_l^2 chi^2 with (2 l + 1) F M degrees of freedom: held at the 1e-6 quantiles."""
    lmax, F, members = 24, 16, 8
    s = N.spectrum(lmax)
    tot = np.zeros(lmax)
    for mem in range(1, members + 1):
        a, _ = NR.coefficients(11, mem, np.arange(F), lmax, s)
        p = (a ** 2).sum(axis=2)                                               # [l][m][F]
        tot += p[:, 0].sum(axis=-1) + 2.0 * p[:, 1:].sum(axis=(1, 2))
    for l in range(1, lmax):
        nu = (2 * l + 1) * F * members
        lo, hi = NR.chi2_quantiles(nu)
        assert lo <= tot[l] / (nu * s[l] ** 2) <= hi, l
    assert tot[0] == 0


def test_restated_fields_pass_the_statistics_the_device_is_held_to():
    """The float64 restatement with the seed of tests/test_noise_kernels_gpu.py passes that test's bars (the bars were fixed before the
    device was asked)."""
    worst = NR.statistics_check(NR.statistics_fields_float64())
    print("restatement: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


def test_fma_emulation_is_exact_on_the_values_of_the_apply_test():
    for L, C, hw in NR.APPLY_SHAPES:
        x0, y, g = NR.apply_inputs(L, C, hw)
        assert NR.fma32_is_exact(np.repeat(np.tile(g, L), hw), y, x0)
    # and it is the fused operation, not mul-then-add: a case where the two differ
    g, y, x = np.float32(1 + 2.0 ** -12), np.float32(1 + 2.0 ** -12), np.float32(-1.0)
    assert NR.fma32(g, y, x) != np.float32(g * y) + x


# ---- 4. host logic -------------------------------------------------------------------------------------------------------------------- #
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


def test_refusals():
    from skyrim_amd.core.models.ensemble import GlobalEnsemble
    from skyrim_amd.core.models.graphcast import GraphcastModel
    m = _Model()
    with pytest.raises(ValueError, match="choose from"):
        m.ensemble_forecast(T0, perturbation="bred")
    for bad in (0.0, -5.0, float("nan")):
        with pytest.raises(ValueError, match="length_scale_km"):
            m.ensemble_forecast(T0, perturbation="spherical", length_scale_km=bad)
    with pytest.raises(ValueError, match="length_scale_km"):
        m.ensemble_forecast(T0, length_scale_km=0.0)                           # refused for either kind
    for bad in (1, 0, -3, 10, 2.5):
        with pytest.raises(ValueError, match="lmax"):                         # 9 x 96: 2 .. min(9, 48)
            m.ensemble_forecast(T0, perturbation="spherical", lmax=bad)
    with pytest.raises(ValueError, match="not input channels"):
        m.ensemble_forecast(T0, perturbation="spherical", perturb_channels=["t2m", "nope"])
    with pytest.raises(ValueError, match="not input channels"):
        m.ensemble_forecast(T0, perturb_channels=["nope"])
    with pytest.raises(ValueError, match="dynamic range"):
        m.ensemble_forecast(T0, perturbation="spherical", length_scale_km=20000.0, alpha=12.0)
    with pytest.raises(ValueError, match="64"):
        m.ensemble_forecast(T0, n_members=65, perturbation="spherical")
    for kw in (dict(perturbation="spherical"), dict(perturbation="spherical", lmax=9, length_scale_km=800.0, alpha=1.5,
                                                    perturb_channels=["t2m"]), dict(perturb_channels=["u1000"])):
        with pytest.raises(RuntimeError, match="GPU"):
            m.ensemble_forecast(T0, n_members=3, **kw)                         # everything valid: the members themselves need the device
    with pytest.raises(ValueError, match="multi-model"):
        GlobalEnsemble(["pangu", "fuxi"], ic_source="synthetic").ensemble_forecast(T0, perturbation="spherical", length_scale_km=300.0)
    with pytest.raises(NotImplementedError, match="stepper"):
        GraphcastModel.ensemble_forecast(object.__new__(GraphcastModel), T0, perturbation="spherical", lmax=64)


def test_grids():
    lon = 360.0 / 1440 * np.arange(1440)
    assert N.full_grid(90.0 - 0.25 * np.arange(721), lon) == 721
    assert N.full_grid(90.0 - 0.25 * np.arange(720), lon) == 721               # FourCastNet: rows 0 .. 719 of the 721-row grid
    assert N.full_grid(PanguGeometry(49, 192).lat, PanguGeometry(49, 192).lon) == 49
    gauss = np.degrees(np.arcsin(np.polynomial.legendre.leggauss(32)[0][::-1]))
    for lat, ln in ((gauss, 360.0 / 64 * np.arange(64)), (89.875 - 0.25 * np.arange(720), lon), (-90.0 + 0.25 * np.arange(721), lon),
                    (90.0 - 0.25 * np.arange(721), np.linspace(0, 359, 1440) ** 1.0001)):
        with pytest.raises(ValueError, match=r"\d+ x \d+ grid"):
            N.full_grid(lat, ln)
    model = SimpleNamespace(grid=SimpleNamespace(lat=gauss, lon=360.0 / 64 * np.arange(64)), in_channel_names=["a"])
    with pytest.raises(ValueError, match="32 x 64 grid"):
        N.plan(model, "spherical")
    N.plan(model, "white")                                                     # white noise asks nothing of the grid
    p = N.plan(SimpleNamespace(grid=PanguGeometry(721, 1440), in_channel_names=["a", "b"]), "spherical", perturb_channels=["b"])
    assert (p.lmax, p.n_lat_full, p.e) == (256, 721, N.scale_exponent(N.spectrum(256))) and p.channel_mask.tolist() == [False, True]
    assert N.default_lmax(721, 1440) == 256 and N.default_lmax(33, 64) == 32 and N.default_lmax(49, 192) == 49


def test_ensemble_forecast_dataclass_and_signatures():
    import inspect
    from skyrim_amd import ensemble as E
    ens = E.EnsembleForecast("pangu", 3, 0, 1e-3)
    assert (ens.perturbation, ens.length_scale_km, ens.alpha, ens.lmax) == ("white", 500.0, 2.0, None)
    new = ["perturbation", "length_scale_km", "alpha", "lmax", "perturb_channels"]
    for fn in (E.run, GlobalModel.ensemble_forecast, E.validate):
        assert list(inspect.signature(fn).parameters)[-5:] == new
    d = {k: v.default for k, v in inspect.signature(E.run).parameters.items()}
    assert [d[k] for k in new] == ["white", 500.0, 2.0, None, None]


def test_verify_command_lists_the_new_options():
    from click.testing import CliRunner
    from skyrim_amd import ensemble_cli, verify_cli
    res = CliRunner().invoke(verify_cli.verify, ["--help"])
    assert res.exit_code == 0
    for opt in ("--perturbation", "[white|spherical]", "--length_scale_km", "--lmax"):
        assert opt in res.output, opt
    v = {p.name: p for p in verify_cli.verify.params}
    assert v["perturbation"].default == "white" and v["length_scale_km"].default == 500.0 and v["lmax"].default is None
    assert not {"perturbation", "length_scale_km", "lmax"} & {p.name for p in ensemble_cli.ensemble.params}


# ---- 5. the compiler's resource report ------------------------------------------------------------------------------------------------ #
@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not installed")
def test_kernels_use_no_scratch():
    r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "--cuda-device-only", "-c", "noise_ops.hip", "-o", "/dev/null",
                        "-Rpass-analysis=kernel-resource-usage"], cwd=ROOT / "skyrim_amd" / "csrc", capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    out, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            out[name] = {}
        for key, short in (("ScratchSize [bytes/lane]", "scratch"), ("Occupancy [waves/SIMD]", "occupancy")):
            m = re.search(re.escape(key) + r": (\d+)", line)
            if m and name:
                out[name][short] = int(m.group(1))
    for kernel in ("coeffs_kernel", "apply_kernel"):
        rows = [v for k, v in out.items() if kernel in k]
        assert len(rows) == 1 and rows[0]["scratch"] == 0 and rows[0]["occupancy"] >= 4, (kernel, out)
