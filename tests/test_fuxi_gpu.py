"""FuXi on the MI355X: each stage of include/skyrim_fuxi.h against the float64 restatement (tests/_fuxi_reference.py) on toy shapes
(<= 1e-5), whole calls at full width on a small grid and at 721 x 1440 with reduced width and depth (<= 1e-4), determinism, the cascade
(each stage's parameters, rollout == forecast), the non-finite report, release() and Skyrim("fuxi").predict at full size.
Bar: per-channel max error over the channel's max magnitude."""
from __future__ import annotations

import datetime

import numpy as np
import pytest
import torch

import _fuxi_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T0 = datetime.datetime(2024, 6, 21, 6)
TOY = dict(n_lat=73, n_lon=144, channels=6, embed=128, heads=2, depth=2, window=(3, 6))


def _cfg(**kw):
    from skyrim_amd.fuxi.spec import FuxiConfig
    return FuxiConfig(**{**TOY, **kw})


def _engine(cfg, p):
    from skyrim_amd.fuxi.engine import FuxiEngine
    eng = FuxiEngine(cfg, DEV)
    eng.load_params(p)
    return eng


def _states(cfg, seed=0):
    from skyrim_amd.fuxi.spec import synthetic_state
    return synthetic_state(cfg, seed), synthetic_state(cfg, seed + 1)


def _dev(t):
    return t.float().contiguous().to(DEV)


@pytest.fixture(scope="module")
def toy():
    from skyrim_amd.fuxi.spec import init_synthetic
    cfg = _cfg()
    p = init_synthetic(cfg, 3)
    return cfg, p, _engine(cfg, p), _states(cfg)


def test_embed_and_layer_norm(toy):
    from skyrim_amd.fuxi.spec import time_encoding
    cfg, p, eng, (x0, x1) = toy
    ref = R.embed(p, cfg, x0, x1, T0, "medium")
    eng.embed(_dev(x0), _dev(x1), time_encoding(T0), "medium")
    h0, w0 = cfg.grid0
    eng.layer_norm(eng.buf["emb"], eng.stages["medium"]["en_g"], eng.stages["medium"]["en_b"], eng.buf["h0"], h0 * w0)
    assert R.token_err(eng.buf["h0"], ref).max().item() <= 1e-5


def test_stride2_conv_and_residual_block(toy):
    """The down block: stride-2 conv, then GN statistics and GroupNorm + SiLU applied on load (4 channels per group: chunks of 8
    channels straddle groups)."""
    cfg, p, eng, _ = toy
    g0, g1 = cfg.grid0, cfg.grid1
    h = torch.randn(g0[0], g0[1], cfg.embed, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    d0_ref, d_ref = R.down(p, cfg, h, "short")
    S, b = eng.stages["short"], eng.buf
    eng.conv(_dev(h), S["down"], S["down_b"], b["d0"], g0, g1, stride=2)
    assert R.token_err(b["d0"], d0_ref).max().item() <= 1e-5
    eng.res_block(_dev(d0_ref), S["down_res"], b["d"], g1, b["ra1"], b["rb1"])
    assert R.token_err(b["d"], d_ref).max().item() <= 1e-5


def test_gn_stats_against_float64(toy):
    cfg, p, eng, _ = toy
    x = torch.randn(200, cfg.embed, dtype=torch.float64, generator=torch.Generator().manual_seed(2)) * 3 + 5
    st = eng.gn_stats(_dev(x), 200).cpu().double().reshape(-1, 2)
    g = x.reshape(200, cfg.groups, -1).permute(1, 0, 2).reshape(cfg.groups, -1)
    assert torch.allclose(st[:, 0], g.mean(1), rtol=1e-6, atol=1e-6)
    assert torch.allclose(st[:, 1], 1 / torch.sqrt(g.var(1, unbiased=False) + cfg.gn_eps), rtol=1e-5)


def test_transposed_conv_over_concat_and_residual_block(toy):
    cfg, p, eng, _ = toy
    g0, g1 = cfg.grid0, cfg.grid1
    gen = torch.Generator().manual_seed(3)
    d = torch.randn(g1[0], g1[1], cfg.embed, dtype=torch.float64, generator=gen)
    x = torch.randn(g1[0], g1[1], cfg.embed, dtype=torch.float64, generator=gen) * 2
    u0_ref, u_ref = R.up(p, cfg, d, x, "long")
    S, b = eng.stages["long"], eng.buf
    eng.conv(_dev(d), S["up"], S["up_b"], b["u0"], g1, g1, taps=1, src1=_dev(x), shuffle=1)
    assert R.token_err(b["u0"], u0_ref).max().item() <= 1e-5
    eng.res_block(_dev(u0_ref), S["up_res"], b["u"], g0, b["ra0"], b["rb0"])
    assert R.token_err(b["u"], u_ref).max().item() <= 1e-5


@pytest.mark.parametrize("window", [(3, 6), (9, 9)])
@pytest.mark.parametrize("block", [0, 1])
def test_swin_block(window, block):
    """One block unshifted (0) and shifted (1) at two window shapes: 18 keys (one partial key tile) and 81 (two queries' chunks of
    64, three key tiles, the last partial)."""
    from skyrim_amd.fuxi.spec import init_synthetic
    cfg = _cfg(window=window)
    p = init_synthetic(cfg, 5)
    eng = _engine(cfg, p)
    g1 = cfg.grid1
    x = torch.randn(g1[0], g1[1], cfg.embed, dtype=torch.float64, generator=torch.Generator().manual_seed(4))
    ref = R.swin_block(p, cfg, x, "short", block)
    xd = _dev(x)
    eng.swin_block(block, "short", x=xd)
    assert R.token_err(xd, ref).max().item() <= 1e-5


def test_head_and_bilinear(toy):
    cfg, p, eng, _ = toy
    g0 = cfg.grid0
    u = torch.randn(g0[0], g0[1], cfg.embed, dtype=torch.float64, generator=torch.Generator().manual_seed(6))
    ref = R.head(p, cfg, u, "short")
    S, b = eng.stages["short"], eng.buf
    y = torch.empty(eng.state_shape, device=DEV)
    eng.linear(_dev(u), S["head"], S["head_b"], b["head"], g0[0] * g0[1], head=True)
    eng.resample(b["head"], y)
    assert R.per_channel_err(y, ref).max().item() <= 1e-5


def test_window_must_tile_the_grid(toy):
    cfg, p, eng, _ = toy
    with pytest.raises(RuntimeError, match="does not tile"):
        eng.attention(eng.buf["qkv"], eng.buf["att"], eng.stages["short"]["blocks"][0]["cpb"], eng.stages["short"]["blocks"][0]["scale"],
                      cfg.grid1, 0, 0, window=(4, 6))


def test_toy_calls_each_stage_and_ops(toy):
    cfg, p, eng, (x0, x1) = toy
    for st in ("short", "medium", "long"):
        y = eng.call(_dev(x0), _dev(x1), T0, st)
        assert R.per_channel_err(y, R.call(p, cfg, x0, x1, T0, st)).max().item() <= 1e-4
    from skyrim_amd import ops
    g0 = cfg.grid0
    y2 = torch.empty_like(y)
    ops.hip.fuxi_resample(eng.buf["head"], eng.mean, eng.std, y2, 4 * g0[0], 4 * g0[1], cfg.n_lat, cfg.n_lon, False)
    assert torch.equal(y2, y)


def test_full_width_toy_call():
    from skyrim_amd.fuxi.spec import init_synthetic
    cfg = _cfg(embed=1536, heads=24, window=(9, 18), channels=70)
    p = init_synthetic(cfg, 7)
    eng = _engine(cfg, p)
    x0, x1 = _states(cfg)
    y = eng.call(_dev(x0), _dev(x1), T0, "short")
    assert R.per_channel_err(y, R.call(p, cfg, x0, x1, T0, "short")).max().item() <= 1e-4


def test_721x1440_reduced_call_and_determinism():
    """The full grid (the cropped 721st row, 10 x 10 windows of 9 x 18 on 90 x 180, the bilinear edge) at C = 192, 2 blocks; two runs
    are bit-identical."""
    from skyrim_amd.fuxi.spec import FuxiConfig, init_synthetic
    cfg = FuxiConfig(embed=192, heads=3, depth=2)
    p = init_synthetic(cfg, 9)
    eng = _engine(cfg, p)
    x0, x1 = _states(cfg, 4)
    a = eng.call(_dev(x0), _dev(x1), T0, "long")
    b = eng.call(_dev(x0), _dev(x1), T0, "long")
    assert torch.equal(a, b)
    assert R.per_channel_err(a, R.call(p, cfg, x0, x1, T0, "long")).max().item() <= 1e-4


def _model(cfg, p):
    from skyrim_amd.core.models.fuxi import FuxiModel
    return FuxiModel(ic_source="synthetic", cfg=cfg, params=p, device=DEV)


def test_cascade_rollout_equals_forecast_and_stages(tmp_path):
    from skyrim_amd.fuxi.spec import init_synthetic
    cfg = _cfg(cascade_steps=(2, 4))
    p = init_synthetic(cfg, 11)
    m = _model(cfg, p)
    assert [m.model.stage_for(k) for k in range(1, 6)] == ["short", "short", "medium", "medium", "long"]
    fc = m.forecast(T0, n_steps=5)
    pred, paths = m.rollout(T0, n_steps=5, save=True, save_config={"output_dir": str(tmp_path), "file_type": "netcdf"})
    assert len(paths) == 5
    assert np.array_equal(np.asarray(pred.values)[-1], np.asarray(fc.values)[-1])
    # each step against the restatement run with that step's parameters, from the engine's own previous two states
    vals = np.asarray(fc.values)
    x0 = m.data_source[T0 - datetime.timedelta(hours=6)]
    states = [torch.tensor(np.asarray(x0), dtype=torch.float32), torch.tensor(vals[0])]
    for k in range(1, 6):
        ref = R.call(p, cfg, states[k - 1], states[k], T0 + datetime.timedelta(hours=6 * (k - 1)), m.model.stage_for(k))
        assert R.per_channel_err(torch.tensor(vals[k]), ref).max().item() <= 1e-4, k
        states.append(torch.tensor(vals[k]))
    m.release_model()


def test_non_finite_state_names_its_step():
    from skyrim_amd.fuxi.spec import init_synthetic
    cfg = _cfg(cascade_steps=(1, 4))
    p = dict(init_synthetic(cfg, 3))
    b = p["medium.head.bias"].clone()
    b[0] = float("inf")                              # the medium network runs from step 2
    p["medium.head.bias"] = b
    m = _model(cfg, p)
    with pytest.raises(FloatingPointError, match="after step 2"):
        m.forecast(T0, n_steps=3).values


def test_release_frees_engine_memory():
    from skyrim_amd.fuxi.engine import FuxiEngine
    from skyrim_amd.fuxi.spec import init_synthetic
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated(DEV)
    cfg = _cfg()
    eng = FuxiEngine(cfg, DEV)
    eng.load_params(init_synthetic(cfg, 0))
    assert torch.cuda.memory_allocated(DEV) > before
    eng.release()
    assert torch.cuda.memory_allocated(DEV) == before and not eng.prepared
    with pytest.raises(RuntimeError, match="not prepared"):
        eng.call(torch.zeros(eng.state_shape, device=DEV), torch.zeros(eng.state_shape, device=DEV), T0)


def test_skyrim_predict_full_size_writes_files(tmp_path):
    from skyrim_amd.core import Skyrim
    from skyrim_amd.labeled import open_dataarray
    s = Skyrim("fuxi", ic_source="synthetic")
    pred, paths = s.predict("20240513", "1800", lead_time=12, save=True, save_config={"output_dir": str(tmp_path), "file_type": "netcdf"})
    assert len(paths) == 2
    for q in paths:
        da = open_dataarray(q)
        assert da.shape[-3:] == (70, 721, 1440) and np.isfinite(da.values).all()
    s.model.release_model()
