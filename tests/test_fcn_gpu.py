"""FourCastNet v1 (AFNO) on the MI355X: each kernel of include/skyrim_fcn.h against float64, full steps against the CPU restatement
(tests/_fcn_reference.py, torch.fft), the golden fixture, determinism, longitude equivariance, the full 720 x 1440 grid and the
Skyrim("fourcastnet") API."""
from __future__ import annotations

import datetime
from dataclasses import replace
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _fcn_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = Path(__file__).resolve().parent / "golden" / "fcn_toy_16x48.npz"


def _cfgs():
    from skyrim_amd.fcn.spec import FcnConfig
    return {
        "A": FcnConfig(n_lat=64, n_lon=128, patch=8, embed_dim=768, depth=2, num_blocks=8),
        "B": FcnConfig(n_lat=40, n_lon=120, patch=4, embed_dim=192, depth=3, num_blocks=2),     # 10 x 30 = 300 tokens
        "C": FcnConfig(n_lat=36, n_lon=100, patch=4, embed_dim=192, depth=2, num_blocks=2, kept_lon_modes=13),    # odd h 9, odd w 25, every mode
        "D": FcnConfig(n_lat=32, n_lon=96, patch=4, embed_dim=192, depth=2, num_blocks=2, kept_lon_modes=13),     # w 24, Nyquist column kept
    }


def _engine(cfg, params):
    from skyrim_amd.fcn.engine import FcnEngine
    eng = FcnEngine(cfg, DEV)
    eng.load_params(params)
    return eng


def _rel(a, b):
    return ((a.double() - b.double()).abs().max() / b.double().abs().max()).item()


@pytest.fixture(scope="module")
def toy_b():
    from skyrim_amd.fcn.spec import init_synthetic
    cfg = _cfgs()["B"]
    p = init_synthetic(cfg, 1)
    return cfg, p, _engine(cfg, p)


# ---- kernels against float64 ---------------------------------------------------------------------------------------------------- #
def test_patch_embed_kernel(toy_b):
    from skyrim_amd.fcn.spec import synthetic_state
    cfg, p, eng = toy_b
    x = synthetic_state(cfg, 2)
    out = torch.empty(cfg.tokens * cfg.embed_dim, device=DEV)
    eng.patch_embed(x.to(DEV), out)
    q = {k: v.double() for k, v in p.items()}
    xn = (x.double() - q["norm.mean"][:, None, None]) / q["norm.std"][:, None, None]
    ref = F.conv2d(xn[None], q["patch_embed.proj.weight"], q["patch_embed.proj.bias"], stride=cfg.patch)[0].permute(1, 2, 0).reshape(cfg.tokens, -1)
    ref = ref + q["pos_embed"].reshape(cfg.tokens, -1)
    assert _rel(out.cpu().reshape(cfg.tokens, -1), ref) < 1e-5


@pytest.mark.parametrize("C", [192, 768])
def test_token_mlp_kernel(C):
    from skyrim_amd import ops
    from skyrim_amd.fcn.engine import _Pairs, FcnEngine
    from skyrim_amd.fcn.spec import FcnConfig
    g = torch.Generator().manual_seed(C)
    rows, hid = 16 * 37 + 5, 4 * C                              # ragged tail: not a multiple of 16
    x = torch.randn(rows, C, generator=g) * 3 + 1
    w1, w2 = torch.randn(hid, C, generator=g) * C ** -0.5, torch.randn(C, hid, generator=g) * hid ** -0.5
    b1, b2 = torch.randn(hid, generator=g) * 0.1, torch.randn(C, generator=g) * 0.1
    gm, bt = 1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    eng = FcnEngine(FcnConfig(n_lat=16, n_lon=48, patch=4, embed_dim=C, num_blocks=C // 96), DEV)
    pr = _Pairs(eng, w1, w2)
    out = torch.full((rows, C), float("nan"), device=DEV)
    ops.hip.fcn_mlp(x.to(DEV), pr.w1f, pr.w2f, b1.to(DEV), b2.to(DEV), gm.to(DEV), bt.to(DEV), out, rows, C, hid, 1e-6)
    xd = x.double()
    v = F.layer_norm(xd, (C,), gm.double(), bt.double(), 1e-6)
    ref = xd + F.linear(F.gelu(F.linear(v, w1.double(), b1.double())), w2.double(), b2.double())
    assert _rel(out.cpu(), ref) < 1e-5


def test_spectral_mlp_kernel():
    from skyrim_amd import ops
    from skyrim_amd.fcn.engine import _Pairs, FcnEngine, complex_block_matrices
    from skyrim_amd.fcn.spec import FcnConfig
    g = torch.Generator().manual_seed(5)
    nb, bs, nf, km = 2, 96, 10, 6
    C = nb * bs
    w1, w2 = 0.1 * torch.randn(2, nb, bs, bs, generator=g), 0.1 * torch.randn(2, nb, bs, bs, generator=g)
    b1, b2 = 0.05 * torch.randn(2, nb, bs, generator=g), 0.05 * torch.randn(2, nb, bs, generator=g)
    z = torch.randn(nf, 2, km, C, generator=g)                    # [freq][re, im][m][C]
    eng = FcnEngine(FcnConfig(n_lat=40, n_lon=120, patch=4, embed_dim=C, num_blocks=nb), DEV)
    w1e, b1e = complex_block_matrices(w1, b1)
    w2e, b2e = complex_block_matrices(w2, b2)
    pr = _Pairs(eng, w1e, w2e)
    zd = z.to(DEV).contiguous()
    ops.hip.fcn_spectral_mlp(zd.view(-1), pr.w1f, pr.w2f, b1e.float().to(DEV), b2e.float().to(DEV), [nf * km, km, C, 2 * km * C, km * C, nb], 0.01)
    U = torch.complex(z[:, 0].double(), z[:, 1].double()).reshape(nf, km, nb, bs)
    S = R.spectral_mlp(U, w1.double(), b1.double(), w2.double(), b2.double(), 0.01).reshape(nf, km, C)
    got = zd.cpu()
    assert _rel(got[:, 0], S.real) < 1e-5 and _rel(got[:, 1], S.imag) < 1e-5


def test_head_kernel(toy_b):
    cfg, p, eng = toy_b
    g = torch.Generator().manual_seed(7)
    t = torch.randn(cfg.tokens, cfg.embed_dim, generator=g)
    y = torch.empty(cfg.out_chans, cfg.n_lat, cfg.n_lon, device=DEV)
    eng.head(t.to(DEV).contiguous(), y)
    q = {k: v.double() for k, v in p.items()}
    P, co = cfg.patch, cfg.out_chans
    r = F.linear(t.double(), q["head.weight"]).reshape(cfg.h, cfg.w, P, P, co).permute(4, 0, 2, 1, 3).reshape(co, cfg.n_lat, cfg.n_lon)
    ref = r * q["norm.std"][:, None, None] + q["norm.mean"][:, None, None]
    assert R.per_channel_rel_err(y.cpu(), ref).max().item() < 1e-5


# ---- whole steps ------------------------------------------------------------------------------------------------------------------ #
@pytest.mark.parametrize("name", ["A", "B", "C", "D"])
def test_step_matches_restatement(name):
    from skyrim_amd.fcn.spec import init_synthetic, synthetic_state
    cfg = _cfgs()[name]
    p, x = init_synthetic(cfg, 11), synthetic_state(cfg, 12)
    y = _engine(cfg, p).step(x.to(DEV)).cpu()
    ref = R.forward(p, x.double(), cfg)
    err = R.per_channel_rel_err(y, ref).max().item()
    assert torch.isfinite(y).all() and err < 1e-4, f"config {name}: per-channel rel err {err:.3e}"


def test_golden_fixture():
    from skyrim_amd.fcn.spec import FcnConfig, init_synthetic
    z = np.load(GOLDEN)
    n_lat, n_lon, patch, e, depth, nb = (int(v) for v in z["grid"])
    cfg = FcnConfig(n_lat=n_lat, n_lon=n_lon, patch=patch, embed_dim=e, depth=depth, num_blocks=nb)
    eng = _engine(cfg, init_synthetic(cfg, int(z["seed"])))
    y1 = eng.step(torch.from_numpy(z["x"]).to(DEV))
    y2 = eng.step(y1)
    assert R.per_channel_rel_err(y1.cpu(), torch.from_numpy(z["y1"])).max().item() < 1e-4
    assert R.per_channel_rel_err(y2.cpu(), torch.from_numpy(z["y2"])).max().item() < 1e-4


def test_deterministic(toy_b):
    from skyrim_amd.fcn.spec import synthetic_state
    cfg, _, eng = toy_b
    x = synthetic_state(cfg, 4).to(DEV)
    a = eng.step(x).cpu()
    b = eng.step(x).cpu()
    assert torch.equal(a, b)


def test_longitude_roll():
    """AFNO is not shift-equivariant: a longitude shift turns into a phase of the spectrum, and ReLU / softshrink act on the real and
    imaginary parts separately.  So: with pos_embed = 0 and the spectral MLP zeroed the network is circular in longitude (rolling the input
    by 8 s columns rolls the output); with the filter on, the engine follows the restatement on the rolled input."""
    from skyrim_amd.fcn.spec import init_synthetic, synthetic_state
    cfg = _cfgs()["B"]
    p = init_synthetic(cfg, 9)
    p["pos_embed"] = torch.zeros_like(p["pos_embed"])
    x = synthetic_state(cfg, 10)
    s = 3 * cfg.patch
    xr = torch.roll(x, s, dims=2).contiguous()
    eng = _engine(cfg, p)
    got = eng.step(xr.to(DEV)).cpu()
    assert R.per_channel_rel_err(got, R.forward(p, xr.double(), cfg)).max().item() < 1e-4
    q = dict(p)
    for i in range(cfg.depth):
        for k in ("w1", "b1", "w2", "b2"):
            q[f"blocks.{i}.filter.{k}"] = torch.zeros_like(p[f"blocks.{i}.filter.{k}"])
    eng = _engine(cfg, q)
    y = eng.step(x.to(DEV)).cpu()
    yr = eng.step(xr.to(DEV)).cpu()
    assert R.per_channel_rel_err(yr, torch.roll(y, s, dims=2)).max().item() < 1e-5


# ---- full size ------------------------------------------------------------------------------------------------------------------- #
@pytest.fixture(scope="module")
def full():
    from skyrim_amd.fcn.spec import FcnConfig, init_synthetic, synthetic_state
    cfg = FcnConfig()
    p = init_synthetic(cfg, 0)
    return cfg, p, synthetic_state(cfg, 0), _engine(cfg, p)


def test_full_size_step_and_rollout(full):
    cfg, p, x, eng = full
    ref, y = x, x.to(DEV)
    for k in range(4):
        y = eng.step(y)
        ref = R.forward(p, ref, cfg, dtype=torch.float32)
        err = R.per_channel_rel_err(y.cpu(), ref).max().item()
        assert torch.isfinite(y).all()
        assert err < (1e-4 if k == 0 else 1e-3), f"step {k + 1}: per-channel rel err {err:.3e}"


def test_skyrim_predict_and_restart(tmp_path, full):
    from skyrim_amd.core import Skyrim
    from skyrim_amd.core.models.utils import run_basic_inference
    from skyrim_amd.labeled import open_dataarray
    s = Skyrim("fourcastnet")
    pred, paths = s.predict("20240513", "1800", lead_time=24, save=True, save_config={"output_dir": str(tmp_path), "file_type": "netcdf"})
    assert len(paths) == 4
    for q in paths:
        da = open_dataarray(q)
        assert da.shape[-3:] == (26, 720, 1440) and da.lat.values[0] == 90.0 and da.lat.values[-1] == -89.75
    m = s.model
    again = run_basic_inference(m.model, 1, m.data_source, datetime.datetime(2024, 5, 14, 18), x=paths[-1])
    last = open_dataarray(paths[-1]).values[-1]
    assert np.array_equal(again.values[0], last)
    # one more step from the restart equals one more step of an uninterrupted rollout
    full5 = run_basic_inference(m.model, 5, m.data_source, datetime.datetime(2024, 5, 13, 18))
    assert np.allclose(again.values[-1], full5.values[-1], rtol=0, atol=1e-4 * np.abs(full5.values[-1]).max())
