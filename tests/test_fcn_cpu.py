"""FourCastNet v1 (AFNO) without a GPU: C ABI surface and argument checks, op registration, the model registry and wrapper, the
checkpoint mapping, the restatement's filter against an explicit DFT sum, and the 721 -> 720 initial-condition crop."""
from __future__ import annotations

import ctypes
import datetime
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import _fcn_reference as R

ROOT = Path(__file__).resolve().parent.parent


def _lib():
    from skyrim_amd.fcn import engine
    return engine.load_library()


def test_header_symbols_equal_exports_and_library_has_them():
    from skyrim_amd.fcn import engine
    hdr = (ROOT / "include" / "skyrim_fcn.h").read_text()
    names = set(re.findall(r"^(?:int|const char\*) (skfcn_\w+)\(", hdr, re.M))
    assert names == set(engine.EXPORTS)
    lib = _lib()
    for n in engine.EXPORTS:
        assert hasattr(lib, n)


def test_abi_version_and_error_strings():
    lib = _lib()
    assert lib.skfcn_abi_version() == 1
    assert lib.skfcn_error_string(-1) == b"invalid argument" and lib.skfcn_error_string(-2) == b"HIP runtime error"


def test_argument_errors_without_gpu():
    from skyrim_amd.fcn import engine
    lib = _lib()
    assert lib.skfcn_prepare_weight(None, 1, 1, 4, 4, None, 16, 8, None) == -1
    assert lib.skfcn_prepare_mlp_weights(1, 1, 30, 32, 32, 1, 1, 1, None) == -1             # K not a multiple of 32
    assert lib.skfcn_layer_norm(1, 1, 1, 1, 10, 770, 1e-6, None) == -1                        # C not a multiple of 4
    assert lib.skfcn_patch_embed(None, None) == -1
    assert lib.skfcn_spectral_mlp(None, None) == -1
    assert lib.skfcn_spectral_run(None, None) == -1
    assert lib.skfcn_mlp_run(None, None) == -1
    assert lib.skfcn_head_run(None, None) == -1
    d = engine.MlpDesc(1, 1, 100, 512, 2048, 1, 1, 1e-6, 1, 1, 1, 1)                           # C not compiled
    assert lib.skfcn_mlp_run(ctypes.byref(d), None) == -1
    d = engine.MlpDesc(1, 1, 100, 768, 3072, 1, 1, 1e-6, 1, 1, 1, 1)                           # out aliases x
    assert lib.skfcn_mlp_run(ctypes.byref(d), None) == -1
    s = engine.SpectralDesc()
    s.t = s.u = s.s0 = s.s1 = s.gamma = s.beta = s.fw = s.fl = s.il = s.iw = s.w1f = s.w2f = s.b1e = s.b2e = 1
    s.h, s.w, s.C, s.km, s.nblocks = 90, 180, 768, 92, 8                                       # km > w/2 + 1
    assert lib.skfcn_spectral_run(ctypes.byref(s), None) == -1
    h = engine.HeadDesc(1, 1, 10 ** 9, 768, 1, 1, 26, 720, 1444, 8, 768)                      # grid not a multiple of the patch
    assert lib.skfcn_head_run(ctypes.byref(h), None) == -1


def test_fcn_ops_have_no_cpu_kernel():
    from skyrim_amd import ops
    names = [n for n in ops.OP_NAMES if n.startswith("fcn_")]
    assert set(names) == {"fcn_layer_norm", "fcn_mlp", "fcn_spectral_mlp"}
    x = torch.zeros(4, 192)
    with pytest.raises(NotImplementedError):
        ops.hip.fcn_layer_norm(x, torch.ones(192), torch.zeros(192), x.clone(), 4, 192, 1e-6)


def test_fourcastnet_is_a_registered_model_and_cli_choice():
    from skyrim_amd import common, forecast
    from skyrim_amd.core import Skyrim
    from skyrim_amd.core import models
    assert "fourcastnet" in Skyrim.list_available_models()
    assert "fourcastnet" in common.AVAILABLE_MODELS and "fourcastnet" in models.MODELS
    opt = next(p for p in forecast.main.params if p.name == "model_name")
    assert "fourcastnet" in opt.type.choices


def test_wrapper_channels_grid_and_time_step():
    from skyrim_amd.core.models.fourcastnet import CHANNELS, FourcastnetModel
    from skyrim_amd.fcn.timeloop import FcnTimeLoop
    assert CHANNELS[:5] == ["u10m", "v10m", "t2m", "sp", "msl"] and CHANNELS[-1] == "t250" and len(CHANNELS) == 26
    loop = FcnTimeLoop.__new__(FcnTimeLoop)
    assert FcnTimeLoop.time_step == datetime.timedelta(hours=6) and FcnTimeLoop.n_history_levels == 1
    from skyrim_amd.fcn.spec import FcnConfig
    cfg = FcnConfig()
    assert (cfg.h, cfg.w, cfg.tokens, cfg.km, cfg.hidden) == (90, 180, 16200, 46, 3072)
    step = 180.0 / cfg.n_lat
    lat = 90.0 - step * np.arange(cfg.n_lat)
    assert lat[0] == 90.0 and lat[-1] == -89.75 and len(lat) == 720
    assert FourcastnetModel.model_name == "fourcastnet"
    del loop


def _archive(cfg, prefix="module.", wrap=True):
    from skyrim_amd.fcn.spec import init_synthetic
    p = init_synthetic(cfg, 4)
    sd = {prefix + k: v.clone() for k, v in p.items() if not k.startswith("norm.")}
    sd[prefix + "blocks.0.filter.scale"] = torch.tensor(0.02)            # read by nobody: tolerated
    return p, ({"model_state": sd} if wrap else sd)


def test_checkpoint_round_trip_and_renamed_key(tmp_path):
    from skyrim_amd.fcn import checkpoint
    from skyrim_amd.fcn.spec import FcnConfig
    cfg = FcnConfig(n_lat=16, n_lon=48, patch=4, embed_dim=192, depth=2, num_blocks=2)
    for prefix, wrap in (("module.", True), ("", False)):
        p, arc = _archive(cfg, prefix, wrap)
        torch.save(arc, tmp_path / "weights.tar")
        np.save(tmp_path / "global_means.npy", p["norm.mean"].numpy().reshape(1, -1, 1, 1))
        np.save(tmp_path / "global_stds.npy", p["norm.std"].numpy().reshape(1, -1, 1, 1))
        got = checkpoint.load_package(str(tmp_path), cfg)
        assert set(got) == set(p) and all(torch.equal(got[k], p[k]) for k in p)
    sd = arc["model_state"] if wrap else arc
    sd["blocks.1.mlp.fc3.weight"] = sd.pop("blocks.1.mlp.fc2.weight")
    with pytest.raises(ValueError, match=r"blocks\.1\.mlp\.fc3\.weight"):
        checkpoint.convert(sd, cfg, p["norm.mean"].numpy(), p["norm.std"].numpy())


def _dft_filter(u, w1, b1, w2, b2, km, lam):
    """The filter as explicit float64 DFT sums (notes 1 and 2 of DESIGN.md 13): all latitude frequencies, longitude modes m < km, the
    C2R of the inverse taking Re of m = 0 and 2 Re(X e^{+i}) for 0 < m < km."""
    h, w, C = u.shape
    nb = w1.shape[1]
    ys, xs = np.arange(h), np.arange(w)
    U = np.zeros((h, km, C), complex)
    for k in range(h):
        for m in range(km):
            ph = np.exp(-2j * np.pi * (k * ys[:, None] / h + m * xs[None, :] / w)) / np.sqrt(h * w)
            U[k, m] = np.einsum("yx,yxc->c", ph, u)
    Ut = torch.from_numpy(U).reshape(h, km, nb, C // nb)
    S = R.spectral_mlp(Ut, w1, b1, w2, b2, lam).reshape(h, km, C).numpy()
    X = np.zeros((h, km, C), complex)                   # latitude inverse
    for y in range(h):
        X[y] = np.einsum("k,kmc->mc", np.exp(2j * np.pi * np.arange(h) * y / h), S) / np.sqrt(h)
    f = np.zeros((h, w, C))
    for x in range(w):
        f[:, x] = X[:, 0].real
        for m in range(1, km):
            f[:, x] += 2 * (X[:, m].real * np.cos(2 * np.pi * m * x / w) - X[:, m].imag * np.sin(2 * np.pi * m * x / w))
    return torch.from_numpy(f / np.sqrt(w))


def test_restatement_filter_equals_explicit_dft_sum():
    from skyrim_amd.fcn.spec import FcnConfig
    cfg = FcnConfig(n_lat=48, n_lon=80, patch=8, embed_dim=192, depth=1, num_blocks=2)    # 6 x 10 tokens, km = 4
    g = torch.Generator().manual_seed(0)
    u = torch.randn(cfg.h, cfg.w, 192, generator=g, dtype=torch.float64)
    w1, w2 = 0.2 * torch.randn(2, 2, 96, 96, generator=g, dtype=torch.float64), 0.2 * torch.randn(2, 2, 96, 96, generator=g, dtype=torch.float64)
    b1, b2 = 0.1 * torch.randn(2, 2, 96, generator=g, dtype=torch.float64), 0.1 * torch.randn(2, 2, 96, generator=g, dtype=torch.float64)
    assert R.kept_lon_modes(cfg) == cfg.km == 4
    got = R.afno_filter(u, w1, b1, w2, b2, cfg)
    ref = _dft_filter(u.numpy(), w1, b1, w2, b2, cfg.km, cfg.sparsity_threshold)
    assert (got - ref).abs().max().item() < 1e-12 * max(1.0, ref.abs().max().item())


def test_engine_dft_matrices_equal_torch_fft():
    """The four DFT matrices against torch.fft in float64: even and odd h and w, the longitude Nyquist column kept (km = w // 2 + 1, w
    even) or absent (w odd), km = 1.  The inverse gets a spectrum that is not Hermitian where the C2R has to drop something: random
    imaginary parts in the m = 0 and the Nyquist column."""
    from skyrim_amd.fcn.engine import dft_matrices
    gen = torch.Generator().manual_seed(0)
    for h, w, km in [(6, 12, 4), (9, 16, 5), (8, 25, 13), (8, 24, 13), (5, 10, 6), (9, 9, 5), (7, 12, 1)]:
        m = {k: torch.from_numpy(v) for k, v in dft_matrices(h, w, km).items()}
        assert m["fw"].shape == (2 * km, w) and m["fl"].shape == m["il"].shape == (2 * h, 2 * h) and m["iw"].shape == (w, 2 * km)
        x = torch.randn(h, w, dtype=torch.float64, generator=gen)
        U = torch.fft.rfft2(x, norm="ortho")[:, :km]
        Y = (m["fw"] @ x.T).T.reshape(h, 2, km).reshape(2 * h, km)        # [2 h + ri][m]
        Z = m["fl"] @ Y
        assert torch.allclose(torch.complex(Z[0::2], Z[1::2]), U, atol=1e-12), (h, w, km)
        S = torch.complex(torch.randn(h, km, dtype=torch.float64, generator=gen), torch.randn(h, km, dtype=torch.float64, generator=gen))
        assert (S[:, 0].imag.abs() > 0).all() and (w % 2 or km < w // 2 + 1 or (S[:, w // 2].imag.abs() > 0).all())
        Zs = torch.stack([S.real, S.imag], 1).reshape(2 * h, km)
        f = (m["iw"] @ (m["il"] @ Zs).reshape(h, 2 * km).T).T
        full = torch.zeros(h, w // 2 + 1, dtype=torch.complex128)
        full[:, :km] = S
        assert torch.allclose(f, torch.fft.irfft2(full, s=(h, w), norm="ortho"), atol=1e-12), (h, w, km)


class _Loop:
    n_history_levels = 1
    time_step = datetime.timedelta(hours=6)
    device = "cpu"

    def __init__(self, n_lat):
        self.grid = type("G", (), {"lat": list(range(n_lat))})()


class _Src:
    def __init__(self, rows):
        self.rows = rows

    def __getitem__(self, t):
        return np.arange(2 * self.rows * 4, dtype=np.float32).reshape(2, self.rows, 4)


def test_initial_condition_crop_721_to_720():
    from skyrim_amd.datasource import get_initial_condition_for_model
    t = datetime.datetime(2024, 1, 1)
    x = get_initial_condition_for_model(_Loop(720), _Src(721), t)
    assert tuple(x.shape) == (1, 1, 2, 720, 4) and np.array_equal(x[0, 0].numpy(), _Src(721)[t][:, :720])
    assert tuple(get_initial_condition_for_model(_Loop(721), _Src(721), t).shape) == (1, 1, 2, 721, 4)   # unchanged
    assert tuple(get_initial_condition_for_model(_Loop(720), _Src(720), t).shape) == (1, 1, 2, 720, 4)


def test_mixed_ensemble_with_a_720_row_member_is_refused():
    from skyrim_amd.core.models.ensemble import _on_grid_of
    from skyrim_amd.labeled import DataArray
    a = DataArray(np.zeros((1, 721, 4), np.float32), dims=("channel", "lat", "lon"),
                  coords={"channel": ["t2m"], "lat": 90.0 - 0.25 * np.arange(721), "lon": np.arange(4.0)})
    b = DataArray(np.zeros((1, 720, 4), np.float32), dims=("channel", "lat", "lon"),
                  coords={"channel": ["t2m"], "lat": 90.0 - 0.25 * np.arange(720), "lon": np.arange(4.0)})
    with pytest.raises(ValueError, match="different lat axes"):
        _on_grid_of(a, b)
