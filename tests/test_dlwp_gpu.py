"""DLWP on the MI355X: each stage of include/skyrim_dlwp.h against the float64 restatement (tests/_dlwp_reference.py) on a toy cube
with maps of varying non-zeros per row, whole calls at toy and full size, the rollout / forecast contract of Skyrim("dlwp"), the
non-finite report and release().  Bar: per-channel max error over the channel's max magnitude."""
from __future__ import annotations

import datetime
from dataclasses import replace

import numpy as np
import pytest
import torch

import _dlwp_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T0 = datetime.datetime(2024, 6, 21, 6)


def _toy():
    from skyrim_amd.dlwp.spec import DlwpConfig, init_synthetic
    cfg = DlwpConfig(n_lat=33, n_lon=64, face=8)
    p = init_synthetic(cfg, 3)
    for name, (rows, cols) in (("ll_to_cs", (cfg.cells, cfg.points)), ("cs_to_ll", (cfg.points, cfg.cells))):
        r, c, s = R.random_csr(rows, cols, seed=rows)
        p[name + ".row"], p[name + ".col"], p[name + ".S"] = torch.from_numpy(r), torch.from_numpy(c), torch.from_numpy(s)
    return cfg, p


def _engine(cfg, p):
    from skyrim_amd.dlwp.engine import DlwpEngine
    eng = DlwpEngine(cfg, DEV)
    eng.load_params(p)
    return eng


def _states(cfg, seed=0):
    from skyrim_amd.dlwp.spec import synthetic_state
    return synthetic_state(cfg, seed), synthetic_state(cfg, seed + 1)


@pytest.fixture(scope="module")
def toy():
    cfg, p = _toy()
    x0, x1 = _states(cfg)
    xin = R.ingest(p, cfg, x0, x1, T0)
    outs, h = [], xin
    for i in range(11):
        h = R.unet(p, cfg, xin, upto=i + 1)
        outs.append(h)
    return cfg, p, _engine(cfg, p), x0, x1, xin, outs


def test_ingest_stage(toy):
    cfg, p, eng, x0, x1, xin, _ = toy
    from skyrim_amd.dlwp.engine import IN_LD
    out = torch.full((cfg.cells * IN_LD,), float("nan"), device=DEV)
    eng.ingest(x0.to(DEV), x1.to(DEV), *eng.tisr_days(T0), out=out)
    got = out.view(cfg.cells, IN_LD).cpu()
    ref = R.channels_last(xin)
    assert R.rel_err(got[:, :cfg.in_ch], ref, dim=1).max().item() <= 1e-5
    assert torch.equal(got[:, cfg.in_ch:], torch.zeros(cfg.cells, IN_LD - cfg.in_ch))


@pytest.mark.parametrize("i", range(11))
def test_conv_stage(toy, i):
    """Conv i alone, fed the restatement's own input (pooled / upsampled / concatenated inside the loader), on every face."""
    from skyrim_amd.dlwp.engine import IN_LD, OUT_LD
    from skyrim_amd.dlwp.spec import SKIP_OF, convs
    cfg, p, eng, _, _, xin, outs = toy
    names = [c[0] for c in convs(cfg)]
    if i == 0:
        src = torch.zeros(cfg.cells, IN_LD, dtype=torch.float64)
        src[:, :cfg.in_ch] = R.channels_last(xin)
    else:
        src = R.channels_last(outs[i - 1])
    skip = SKIP_OF.get(names[i])
    skip_t = R.channels_last(outs[names.index(skip)]).float().contiguous().to(DEV) if skip else None
    L = eng.layers[i]
    out = torch.full((L["out"].numel(),), float("nan"), device=DEV)
    eng.conv(i, src=src.float().contiguous().to(DEV), skip=skip_t, out=out)
    got = out.view(-1, L["ld"]).cpu()[:, :L["cout"]]
    ref = R.channels_last(outs[i])
    err = R.rel_err(got, ref, dim=1)
    assert err.max().item() <= 1e-5, f"conv {names[i]}: per-channel rel err {err.max().item():.3e}"
    assert L["ld"] == (OUT_LD if names[i] == "last" else L["cout"])


def test_egress_stage(toy):
    from skyrim_amd.dlwp.engine import OUT_LD
    cfg, p, eng, _, _, _, outs = toy
    y = torch.zeros(cfg.cells, OUT_LD, dtype=torch.float64)
    y[:, :cfg.out_ch] = R.channels_last(outs[-1])
    y6 = torch.empty((cfg.channels, cfg.n_lat, cfg.n_lon), device=DEV)
    y12 = torch.empty_like(y6)
    eng.egress(y6, y12, y=y.float().contiguous().to(DEV))
    r6, r12 = R.egress(p, cfg, outs[-1])
    assert R.rel_err(y6.cpu(), r6).max().item() <= 1e-5
    assert R.rel_err(y12.cpu(), r12).max().item() <= 1e-5


def test_toy_call_and_ops(toy):
    cfg, p, eng, x0, x1, _, _ = toy
    y6, y12 = eng.call(x0.to(DEV), x1.to(DEV), T0)
    r6, r12 = R.call(p, cfg, x0, x1, T0)
    assert R.rel_err(y6.cpu(), r6).max().item() <= 1e-5
    assert R.rel_err(y12.cpu(), r12).max().item() <= 1e-5
    # the torch.ops entry points run the same kernels
    from skyrim_amd import ops
    from skyrim_amd.dlwp.engine import IN_LD, OUT_LD
    m = eng.ll_to_cs
    xin = torch.empty(cfg.cells * IN_LD, device=DEV)
    ops.hip.dlwp_ingest(x0.to(DEV), x1.to(DEV), eng.center, eng.inv_scale, m.ptr, m.col, m.S, eng.lat, eng.lon, eng.statics,
                        *eng.tisr_days(T0), xin, cfg.channels, IN_LD)
    assert torch.equal(xin, eng.x)
    L = eng.layers[-1]
    last = torch.empty_like(L["out"])
    ops.hip.dlwp_conv(eng.layers[-2]["out"], None, eng.pad, L["w"].buf, L["w"].plane, L["w"].w_sb, L["w"].ldw, L["bias"], last,
                      [L["n"], 64, 0, 0, 1, cfg.out_ch, OUT_LD, 0, cfg.polar_flip_face], cfg.leaky_slope, cfg.clamp_max)
    assert torch.equal(last.view(-1, OUT_LD)[:, :cfg.out_ch], L["out"].view(-1, OUT_LD)[:, :cfg.out_ch])
    o6, o12 = torch.empty_like(y6), torch.empty_like(y12)
    c = eng.cs_to_ll
    ops.hip.dlwp_egress(last, c.ptr, c.col, c.S, eng.center, eng.scale, o6, o12, cfg.channels, OUT_LD)
    assert torch.equal(o6, y6) and torch.equal(o12, y12)


def test_deterministic(toy):
    cfg, p, eng, x0, x1, _, _ = toy
    a = eng.call(x0.to(DEV), x1.to(DEV), T0)
    b = eng.call(x0.to(DEV), x1.to(DEV), T0)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.fixture(scope="module")
def full():
    from skyrim_amd.dlwp.spec import DlwpConfig, init_synthetic
    cfg = DlwpConfig()
    p = init_synthetic(cfg, 0)
    return cfg, p, _engine(cfg, p), _states(cfg)


def test_full_size_call_and_four_steps(full):
    cfg, p, eng, (x0, x1) = full
    torch.set_num_threads(min(16, torch.get_num_threads()))
    refs = R.rollout(p, cfg, x0, x1, T0, 4)
    a, b, t = x0.to(DEV), x1.to(DEV), T0
    for k in range(4):
        a, b = eng.call(a, b, t)
        t += datetime.timedelta(hours=12)
        assert torch.isfinite(b).all()
        err = R.rel_err(b.cpu(), refs[k]).max().item()
        assert err <= (1e-5 if k == 0 else 1e-4), f"call {k + 1}: per-channel rel err {err:.3e}"


def _model(cfg, p):
    from skyrim_amd.core.models.dlwp import DLWPModel
    return DLWPModel(ic_source="synthetic", cfg=cfg, params=p)


@pytest.mark.parametrize("save", [False, True])
def test_rollout_equals_forecast(tmp_path, save):
    cfg, p = _toy()
    m = _model(cfg, p)
    fc = m.forecast(T0, n_steps=4)
    want = np.array([T0 + datetime.timedelta(hours=12 * k) for k in range(5)]).astype("datetime64[s]")
    assert np.array_equal(np.asarray(fc.time.values).astype("datetime64[s]"), want)
    pred, paths = m.rollout(T0, n_steps=4, save=save, save_config={"output_dir": str(tmp_path), "file_type": "netcdf"})
    assert np.array_equal(pred.values[-1], fc.values[-1])
    if save:
        from skyrim_amd.labeled import open_dataarray
        assert len(paths) == 4
        ends = [open_dataarray(q).time.values[-1] for q in paths]
        gaps = np.diff(np.asarray(ends).astype("datetime64[s]")).astype("timedelta64[h]").astype(int)
        assert gaps.tolist() == [12, 12, 12]
        # a saved step holds (t, t + 12 h): not a restart point
        with pytest.raises(ValueError, match="apart"):
            m.predict_one_step(T0 + datetime.timedelta(hours=48), initial_condition=paths[-1])
    else:
        assert paths == []


def test_non_finite_state_names_its_step():
    cfg, p = _toy()
    p = dict(p)
    b = p["polar_last.bias"].clone()
    b[cfg.channels + 2] = float("inf")              # z700 of the t + 12 h half: the state yielded by call 1
    p["polar_last.bias"] = b
    m = _model(cfg, p)
    with pytest.raises(FloatingPointError, match="after step 1"):
        m.forecast(T0, n_steps=2).values


def test_release_frees_engine_memory():
    cfg, p = _toy()
    from skyrim_amd.dlwp.engine import DlwpEngine
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated(DEV)
    eng = DlwpEngine(replace(cfg, face=16), DEV)
    from skyrim_amd.dlwp.spec import init_synthetic
    eng.load_params(init_synthetic(eng.cfg, 0))
    held = torch.cuda.memory_allocated(DEV)
    assert held > before
    eng.release()
    assert torch.cuda.memory_allocated(DEV) == before and not eng.prepared
    with pytest.raises(RuntimeError, match="not prepared"):
        eng.call(torch.zeros(eng.state_shape, device=DEV), torch.zeros(eng.state_shape, device=DEV), T0)


def test_skyrim_predict_writes_12h_files(tmp_path):
    from skyrim_amd.core import Skyrim
    from skyrim_amd.labeled import open_dataarray
    s = Skyrim("dlwp", ic_source="synthetic")
    pred, paths = s.predict("20240513", "1800", lead_time=24, save=True, save_config={"output_dir": str(tmp_path), "file_type": "netcdf"})
    assert len(paths) == 2
    for q in paths:
        da = open_dataarray(q)
        assert da.shape[-3:] == (7, 721, 1440) and np.isfinite(da.values).all()
    assert np.asarray(pred.prediction.time.values).astype("datetime64[s]")[-1] == np.datetime64("2024-05-14T18:00:00")
    with pytest.raises(ValueError, match="shorter than one 12-h step"):
        s.predict("20240513", "1800", lead_time=6)
    s.model.release_model()
