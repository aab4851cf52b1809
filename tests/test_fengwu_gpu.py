"""FengWu on the MI355X: each stage of include/skyrim_fengwu.h against the float64 restatement (tests/_fengwu_reference.py) on toy shapes
(<= 1e-5), the batched launch against one launch per modality (bit-identical), whole calls on a toy grid, at full width on a small grid
and at 721 x 1440 with reduced width and depth (<= 1e-4), determinism, rollout == forecast, the non-finite report, release() and
Skyrim("fengwu").predict at full size.  Bar: per-channel max error over the channel's max magnitude.

Parity is against the restatement of the assumed architecture, not against the released FengWu graph."""
from __future__ import annotations

import datetime

import numpy as np
import pytest
import torch

import _fengwu_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T0 = datetime.datetime(2024, 6, 21, 6)
TOY = dict(n_lat=33, n_lon=64, modalities=(("surface", 2), ("z", 3), ("q", 3), ("u", 3), ("v", 3), ("t", 3)), dims=(64, 128),
           heads=(2, 4), enc_depths=(2, 2), dec_depths=(2, 2), fuser_depth=2, window2d=(4, 4), window3d=(2, 4, 4))


def _cfg(**kw):
    from skyrim_amd.fengwu.spec import FengwuConfig
    return FengwuConfig(**{**TOY, **kw})


def _engine(cfg, p):
    from skyrim_amd.fengwu.engine import FengwuEngine
    eng = FengwuEngine(cfg, DEV)
    eng.load_params(p)
    return eng


def _states(cfg, seed=0):
    from skyrim_amd.fengwu.spec import synthetic_state
    return synthetic_state(cfg, seed), synthetic_state(cfg, seed + 1)


def _dev(t):
    return t.float().contiguous().to(DEV)


def _rand(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, dtype=torch.float64, generator=torch.Generator().manual_seed(seed)) * scale


@pytest.fixture(scope="module")
def toy():
    from skyrim_amd.fengwu.spec import init_synthetic
    cfg = _cfg()
    p = init_synthetic(cfg, 3)
    return cfg, p, _engine(cfg, p), _states(cfg)


def _names(cfg):
    return [n for n, _ in cfg.modalities]


def test_embed_and_layer_norm_all_modalities(toy):
    cfg, p, eng, (x0, x1) = toy
    ref = torch.cat(R.embed(p, cfg, x0, x1))                                  # [mods][h1][w1][D1]
    eng.embed_stage(_dev(x0), _dev(x1))
    assert R.token_err(eng.buf["xe"][:ref.numel()], ref).max().item() <= 1e-5


@pytest.mark.parametrize("block", [0, 1])
def test_2d_swin_block(toy, block):
    """An encoder block at 181 x 360's stand-in, unshifted (0) and shifted (1): the lat padding (9 -> 12 rows, one in front), the mask."""
    cfg, p, eng, _ = toy
    h1, w1 = cfg.grid1
    x = _rand(cfg.n_mod, h1, w1, cfg.dims[0], seed=block)
    ref = torch.cat([R.swin_block(p, cfg, f"enc.{n}.s0.{block}", x[z:z + 1], "s0", block) for z, n in enumerate(_names(cfg))])
    xd = _dev(x)
    eng.swin_block(eng.w["enc0"][block], xd, "s0")
    assert R.token_err(xd, ref).max().item() <= 1e-5


def test_patch_merge(toy):
    cfg, p, eng, _ = toy
    h1, w1 = cfg.grid1
    x = _rand(cfg.n_mod, h1, w1, cfg.dims[0], seed=5)
    ref = torch.cat([R.merge(p, cfg, n, x[z:z + 1]) for z, n in enumerate(_names(cfg))])
    out = torch.zeros(ref.numel(), device=DEV)
    eng.merge(_dev(x), out)
    assert R.token_err(out, ref).max().item() <= 1e-5


@pytest.mark.parametrize("block", [0, 1])
def test_3d_fuser_block(toy, block):
    """A fuser block over (modality, lat, lon): 3 x 2 x 2 windows of 2 x 4 x 4; shifted, the modality axis and latitude are masked."""
    cfg, p, eng, _ = toy
    h2, w2 = cfg.grid2
    x = _rand(cfg.n_mod, h2, w2, cfg.dims[1], seed=10 + block)
    ref = R.swin_block(p, cfg, f"fuser.{block}", x, "fuser", block)
    xd = _dev(x)
    eng.swin_block(eng.w["fuser"][block], xd, "fuser")
    assert R.token_err(xd, ref).max().item() <= 1e-5


def test_expand_and_skip(toy):
    cfg, p, eng, _ = toy
    (h1, w1), (h2, w2) = cfg.grid1, cfg.grid2
    x2 = _rand(cfg.n_mod, h2, w2, cfg.dims[1], seed=20)
    skip = _rand(cfg.n_mod, h1, w1, cfg.dims[0], seed=21)
    ref = torch.cat([R.expand_skip(p, cfg, n, x2[z:z + 1], skip[z:z + 1]) for z, n in enumerate(_names(cfg))])
    out = torch.zeros(ref.numel(), device=DEV)
    eng.expand_skip(_dev(x2), _dev(skip), out)
    assert R.token_err(out, ref).max().item() <= 1e-5


def test_recovery_crop_and_denormalisation(toy):
    cfg, p, eng, _ = toy
    h1, w1 = cfg.grid1
    x = _rand(cfg.n_mod, h1, w1, cfg.dims[0], seed=30)
    y = torch.cat([R.recover(p, cfg, n, x[z:z + 1]) for z, n in enumerate(_names(cfg))])
    ref = y * R.P(p, "norm.std")[:, None, None] + R.P(p, "norm.mean")[:, None, None]
    out = torch.full(eng.state_shape, float("nan"), device=DEV)
    eng.recover(_dev(x), out)
    assert R.per_channel_err(out, ref).max().item() <= 1e-5


def test_batched_launch_equals_single_modality_launches(toy):
    """fc1 + GELU and the shifted window attention: one launch over six modalities == six launches of one, bit for bit."""
    cfg, p, eng, _ = toy
    h1, w1 = cfg.grid1
    D, rows = cfg.dims[0], h1 * w1
    B = eng.w["enc0"][1]
    x = _dev(_rand(cfg.n_mod, rows, D, seed=40))
    whole = torch.zeros(cfg.n_mod * rows * 4 * D, device=DEV)
    eng.linear(x, B["fc1"], B["fc1_b"], whole, rows, act=1)
    one = torch.zeros_like(whole)
    for z in range(cfg.n_mod):
        eng.linear(x[z], B["fc1"], B["fc1_b"], one[z * rows * 4 * D:], rows, act=1, mod=z)
    assert torch.equal(whole, one)
    qkv = _dev(_rand(cfg.n_mod, rows, 3 * D, seed=41))
    att = torch.zeros(cfg.n_mod * rows * D, device=DEV)
    eng.attention(qkv, B["qkv_b"], B["table"], att, "s0", B["shift"], B["types"])
    att1 = torch.zeros_like(att)
    for z in range(cfg.n_mod):
        eng.attention(qkv[z], B["qkv_b"], B["table"], att1[z * rows * D:], "s0", B["shift"], B["types"], mod=z)
    assert torch.equal(att, att1)


def test_toy_call_determinism_and_ops(toy):
    from skyrim_amd import ops
    cfg, p, eng, (x0, x1) = toy
    a = eng.call(_dev(x0), _dev(x1))
    b = eng.call(_dev(x0), _dev(x1))
    assert torch.equal(a, b)
    assert R.per_channel_err(a, R.call(p, cfg, x0, x1)).max().item() <= 1e-4
    h1, w1 = cfg.grid1
    x = _dev(_rand(cfg.n_mod, h1 * w1, cfg.dims[0], seed=50))
    o1, o2 = torch.zeros_like(x), torch.zeros_like(x)
    eng.layer_norm(x, eng.w["en_g"], eng.w["en_b"], o1, h1 * w1, cfg.n_mod, cfg.dims[0])
    ops.hip.fengwu_layer_norm(x, eng.w["en_g"], eng.w["en_b"], o2, h1 * w1, cfg.n_mod, cfg.dims[0], cfg.ln_eps)
    assert torch.equal(o1, o2)


def test_full_width_small_grid_call():
    """The default widths, heads, windows (72 and 144 tokens: several query chunks and key tiles) and the six real modalities on 49 x 192
    (13 x 48 tokens padded to 18 rows, 7 x 24 padded to 12)."""
    from skyrim_amd.fengwu.spec import FengwuConfig, init_synthetic
    cfg = FengwuConfig(n_lat=49, n_lon=192, enc_depths=(2, 2), dec_depths=(2, 2), fuser_depth=2)
    p = init_synthetic(cfg, 7)
    eng = _engine(cfg, p)
    x0, x1 = _states(cfg)
    y = eng.call(_dev(x0), _dev(x1))
    assert R.per_channel_err(y, R.call(p, cfg, x0, x1)).max().item() <= 1e-4


def test_721x1440_reduced_call():
    """The full grid (721 -> 724 rows, 181 -> 186 and 91 -> 96 window rows, the 182-row merge and its crop) at reduced width and depth,
    earth-specific bias tables (one per window row)."""
    from skyrim_amd.fengwu.spec import FengwuConfig, init_synthetic
    cfg = FengwuConfig(dims=(64, 128), heads=(2, 4), enc_depths=(1, 1), dec_depths=(1, 1), fuser_depth=2, bias="earth_specific")
    p = init_synthetic(cfg, 9)
    eng = _engine(cfg, p)
    x0, x1 = _states(cfg, 4)
    y = eng.call(_dev(x0), _dev(x1))
    assert R.per_channel_err(y, R.call(p, cfg, x0, x1)).max().item() <= 1e-4


def _model(cfg, p):
    from skyrim_amd.core.models.fengwu import FengwuModel
    return FengwuModel(ic_source="synthetic", cfg=cfg, params=p, device=DEV)


def test_rollout_equals_forecast(tmp_path):
    from skyrim_amd.fengwu.spec import init_synthetic
    cfg = _cfg()
    p = init_synthetic(cfg, 11)
    m = _model(cfg, p)
    fc = m.forecast(T0, n_steps=3)
    pred, paths = m.rollout(T0, n_steps=3, save=True, save_config={"output_dir": str(tmp_path), "file_type": "netcdf"})
    assert len(paths) == 3
    assert np.array_equal(np.asarray(pred.values)[-1], np.asarray(fc.values)[-1])
    vals = np.asarray(fc.values)
    x0 = m.data_source[T0 - datetime.timedelta(hours=6)]
    ref = R.call(p, cfg, torch.tensor(np.asarray(x0), dtype=torch.float32), torch.tensor(vals[0]))
    assert R.per_channel_err(torch.tensor(vals[1]), ref).max().item() <= 1e-4
    m.release_model()


def test_non_finite_state_is_reported():
    from skyrim_amd.fengwu.spec import init_synthetic
    cfg = _cfg()
    p = dict(init_synthetic(cfg, 3))
    b = p["dec.t.recovery.bias"].clone()
    b[0] = float("inf")
    p["dec.t.recovery.bias"] = b
    m = _model(cfg, p)
    with pytest.raises(FloatingPointError, match="after step 1"):
        m.forecast(T0, n_steps=2).values


def test_release_frees_engine_memory():
    from skyrim_amd.fengwu.engine import FengwuEngine
    from skyrim_amd.fengwu.spec import init_synthetic
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated(DEV)
    cfg = _cfg()
    eng = FengwuEngine(cfg, DEV)
    eng.load_params(init_synthetic(cfg, 0))
    assert torch.cuda.memory_allocated(DEV) > before
    eng.release()
    assert torch.cuda.memory_allocated(DEV) == before and not eng.prepared
    with pytest.raises(RuntimeError, match="not prepared"):
        eng.call(torch.zeros(eng.state_shape, device=DEV), torch.zeros(eng.state_shape, device=DEV))


def test_skyrim_predict_full_size():
    from skyrim_amd.core import Skyrim
    from skyrim_amd.fengwu.spec import CHANNELS
    s = Skyrim("fengwu", ic_source="synthetic")
    pred, _ = s.predict("20240513", "1800", lead_time=12)
    da = pred.prediction
    assert da.dims[-3:] == ("channel", "lat", "lon") and "time" in da.coords
    assert list(np.asarray(da.coords["channel"].values)) == CHANNELS
    assert da.shape[-3:] == (69, 721, 1440) and np.isfinite(np.asarray(da.values)).all()
    s.model.release_model()
