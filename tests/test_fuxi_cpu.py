"""FuXi without a GPU: spec sizes and parameter layout, the Swin V2 tables against direct loops, the time encoding, the cascade's stage
choice, the model registry, the C ABI surface and its argument checks, op registration, the ONNX reader's external-data opt-in with the
directory loader, and the refusals (grids that windows do not tile, external data without the opt-in)."""
from __future__ import annotations

import ctypes
import datetime
import json
import math
import re
from dataclasses import replace
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent


def _toy(**kw):
    from skyrim_amd.fuxi.spec import FuxiConfig
    return FuxiConfig(**{**dict(n_lat=73, n_lon=144, channels=6, embed=128, heads=2, depth=2, window=(3, 6)), **kw})


# ---- spec ------------------------------------------------------------------------------------------------------------------------------ #
def test_spec_sizes_and_param_spec():
    from skyrim_amd.fuxi.spec import CHANNELS, FuxiConfig, flops_per_call, full_param_spec, n_parameters, param_spec
    cfg = FuxiConfig()
    assert len(CHANNELS) == 70 and CHANNELS[:2] == ["z50", "z100"] and CHANNELS[13] == "t50" and CHANNELS[-5:] == ["t2m", "u10m", "v10m", "msl", "tp"]
    assert cfg.grid0 == (180, 360) and cfg.grid1 == (90, 180) and cfg.head_dim == 64 and cfg.k_embed == 2240 and cfg.n_out == 1120
    spec = dict(param_spec(cfg))
    assert spec["embed.weight"] == (1536, 70, 2, 4, 4) and spec["time_embed.weight"] == (1536, 12)
    assert spec["blocks.47.attn.qkv.weight"] == (4608, 1536) and spec["blocks.47.attn.logit_scale"] == (24, 1, 1)
    assert spec["blocks.0.attn.cpb_mlp.2.weight"] == (24, 512) and spec["blocks.0.mlp.fc1.weight"] == (6144, 1536)
    assert spec["up.conv.weight"] == (3072, 1536, 2, 2) and spec["head.weight"] == (1120, 1536)
    assert "blocks.48.norm1.weight" not in spec and len(spec) == 8 + 8 + 48 * 17 + 2 + 8 + 2
    full = [n for n, _ in full_param_spec(cfg)]
    assert full[:2] == ["norm.mean", "norm.std"] and len(full) == 2 + 3 * len(spec) and "long.head.bias" in full
    assert 1.4e9 < n_parameters(cfg) < 1.6e9
    assert 50e12 < flops_per_call(cfg) < 56e12                 # the ~53 TFLOP of one call


def test_cpb_table_and_shift_mask_against_direct_loops():
    from skyrim_amd.fuxi.spec import cpb_table, shift_mask
    cfg = _toy(window=(3, 4))
    wh, ww = cfg.window
    g = torch.Generator().manual_seed(0)
    w0, b0, w2 = torch.randn(16, 2, generator=g), torch.randn(16, generator=g), torch.randn(2, 16, generator=g)
    tab = cpb_table(cfg.window, w0, b0, w2)
    for dy in range(-(wh - 1), wh):
        for dx in range(-(ww - 1), ww):
            c = [dy / (wh - 1) * 8, dx / (ww - 1) * 8]
            c = [math.copysign(math.log2(abs(v) + 1) / 3.0, v) if v else 0.0 for v in c]
            h = [max(0.0, sum(float(w0[j, i]) * c[i] for i in range(2)) + float(b0[j])) for j in range(16)]
            for head in range(2):
                want = 16 / (1 + math.exp(-sum(float(w2[head, j]) * h[j] for j in range(16))))
                assert abs(tab[head, (dy + wh - 1) * (2 * ww - 1) + dx + ww - 1].item() - want) < 1e-12
    H, W, sh, sw = 6, 8, 1, 2
    for lon in (True, False):
        c = replace(cfg, shift_mask_lon=lon)
        m = shift_mask(c, (H, W), sh, sw)
        # Swin's img_mask construction, directly
        img = torch.zeros(H, W)
        cnt = 0
        wsl = (slice(0, -ww), slice(-ww, -sw), slice(-sw, None)) if lon else (slice(None),)
        for hs in (slice(0, -wh), slice(-wh, -sh), slice(-sh, None)):
            for ws in wsl:
                img[hs, ws] = cnt
                cnt += 1
        win = img.reshape(H // wh, wh, W // ww, ww).permute(0, 2, 1, 3).reshape(-1, wh * ww)
        assert torch.equal(m, (win[:, None, :] - win[:, :, None]) != 0)


def test_time_encoding_hand_computed():
    from skyrim_amd.fuxi.spec import time_encoding
    te = time_encoding(datetime.datetime(2024, 3, 1, 6))          # 2024 is a leap year: March 1 is day 61
    days, hours = [61, 61, 61], [0, 6, 12]
    want = []
    for d, h in zip(days, hours):
        want += [math.sin(d / 366), math.sin(h / 24), math.cos(d / 366), math.cos(h / 24)]
    assert te.dtype == np.float64 and np.array_equal(te, np.asarray(want))
    te = time_encoding(datetime.datetime(2023, 1, 1, 3))          # t - 6 h falls on Dec 31 (day 365), hour 21
    assert te[0] == math.sin(365 / 366) and te[1] == math.sin(21 / 24) and te[4] == math.sin(1 / 366)


def test_stage_for():
    from skyrim_amd.fuxi.spec import FuxiConfig, stage_for
    got = {k: stage_for(k, FuxiConfig().cascade_steps) for k in (1, 20, 21, 40, 41, 60)}
    assert got == {1: "short", 20: "short", 21: "medium", 40: "medium", 41: "long", 60: "long"}
    with pytest.raises(ValueError):
        stage_for(0)


def test_fuxi_is_registered_but_not_a_cli_choice():
    from skyrim_amd import common
    from skyrim_amd.core import Skyrim
    from skyrim_amd.core.models import MODELS
    assert "fuxi" in MODELS and MODELS["fuxi"].model_name == "fuxi"
    assert "fuxi" in Skyrim.list_available_models()
    assert "fuxi" not in common.AVAILABLE_MODELS


def test_window_that_does_not_tile_is_refused():
    from skyrim_amd.fuxi import engine
    from skyrim_amd.fuxi.spec import check_config
    with pytest.raises(ValueError, match="does not tile"):
        check_config(_toy(window=(4, 6)))
    with pytest.raises(ValueError, match="does not tile"):
        check_config(_toy(window=(3, 5)))
    lib = engine.load_library()
    d = engine.AttnDesc(16, 16, 16, 16, 9, 18, 128, 2, 4, 6, 0, 0, 1, -100.0, 4.6, 1e-12)
    assert lib.skfuxi_window_attention(ctypes.byref(d), None) == -3
    assert b"does not tile" in lib.skfuxi_error_string(-3)


# ---- C ABI ----------------------------------------------------------------------------------------------------------------------------- #
def test_header_symbols_equal_exports_and_library_has_them():
    from skyrim_amd.fuxi import engine
    hdr = (ROOT / "include" / "skyrim_fuxi.h").read_text()
    names = set(re.findall(r"^(?:int|const char\*) (skfuxi_\w+)\(", hdr, re.M))
    assert names == set(engine.EXPORTS)
    lib = engine.load_library()
    assert lib.skfuxi_abi_version() == 1
    assert lib.skfuxi_error_string(-1) == b"invalid argument" and lib.skfuxi_error_string(-2) == b"HIP runtime error"


def test_argument_errors_without_gpu():
    from skyrim_amd.fuxi import engine
    lib = engine.load_library()
    assert lib.skfuxi_prepare_weight(None, 1, 1, 4, 4, None, 16, 8, None) == -1
    for fn in (lib.skfuxi_embed, lib.skfuxi_conv, lib.skfuxi_linear, lib.skfuxi_window_attention, lib.skfuxi_resample):
        assert fn(None, None) == -1
    assert lib.skfuxi_layer_norm(16, None, 16, 16, 16, 4, 2048, 1e-5, None) == -1             # C above 1536
    assert lib.skfuxi_gn_stats(16, 4, 100, 32, 1e-5, 16, None) == -1                         # C not divisible into groups
    assert lib.skfuxi_gn_residual(16, 16, 16, 16, 16, 16, 4, 130, 32, None) == -1
    c = engine.ConvDesc(16, None, None, None, None, 16, 9 * 12 * 16, 9 * 12, 16, 16, 8, 8, 4, 4, 12, 0, 9, 2, 32, 16, 0)   # c0 % 8
    assert lib.skfuxi_conv(ctypes.byref(c), None) == -1
    c = engine.ConvDesc(16, None, None, None, None, 16, 16 * 16, 16, 16, 16, 8, 8, 4, 4, 16, 0, 1, 2, 32, 16, 0)           # 1 x 1, stride 2
    assert lib.skfuxi_conv(ctypes.byref(c), None) == -1
    li = engine.LinearDesc(16, 16, 64 * 16, 16, 16, 16, 10, 64, 12, 0, 0, 0, 0)                                           # K % 8
    assert lib.skfuxi_linear(ctypes.byref(li), None) == -1
    li = engine.LinearDesc(16, 16, 64 * 16, 16, 16, 16, 10, 40, 16, 0, 1, 3, 4)                                            # M % w_tok
    assert lib.skfuxi_linear(ctypes.byref(li), None) == -1
    a = engine.AttnDesc(16, 16, 16, 16, 9, 18, 96, 2, 3, 6, 0, 0, 1, -100.0, 4.6, 1e-12)                                   # head dim 48
    assert lib.skfuxi_window_attention(ctypes.byref(a), None) == -1
    a = engine.AttnDesc(16, 16, 16, 16, 9, 18, 128, 2, 3, 6, 3, 0, 1, -100.0, 4.6, 1e-12)                                  # shift = window
    assert lib.skfuxi_window_attention(ctypes.byref(a), None) == -1


def test_fuxi_ops_have_no_cpu_kernel():
    from skyrim_amd import ops
    assert {n for n in ops.OP_NAMES if n.startswith("fuxi_")} == {"fuxi_layer_norm", "fuxi_window_attention", "fuxi_resample"}
    with pytest.raises(NotImplementedError):
        ops.hip.fuxi_layer_norm(torch.zeros(8), None, torch.ones(4), torch.zeros(4), torch.zeros(8), 2, 4, 1e-5)
    with pytest.raises(NotImplementedError):
        ops.hip.fuxi_resample(torch.zeros(16), torch.zeros(1), torch.ones(1), torch.zeros(25), 4, 4, 5, 5, False)


# ---- ONNX ------------------------------------------------------------------------------------------------------------------------------ #
def _vi(n):
    out = bytearray()
    while True:
        b = n & 0x7F
        n >>= 7
        out.append(b | (0x80 if n else 0))
        if not n:
            return bytes(out)


def _ld(fno, payload):
    return _vi(fno << 3 | 2) + _vi(len(payload)) + payload


def _ext_tensor(name, arr, location, offset):
    """A float32 TensorProto whose bytes live in ``location`` at ``offset`` (data_location = EXTERNAL)."""
    msg = b"".join(_vi(1 << 3 | 0) + _vi(d) for d in arr.shape) + _vi(2 << 3 | 0) + _vi(1) + _ld(8, name.encode())
    for k, v in (("location", location), ("offset", str(offset)), ("length", str(arr.nbytes))):
        msg += _ld(13, _ld(1, k.encode()) + _ld(2, v.encode()))
    return msg + _vi(14 << 3 | 0) + _vi(1)


def _write_stage(path: Path, cfg, params, stage: str, drop=()):
    """``<stage>.onnx`` + ``<stage>.bin``: the stage's parameters under opaque names, used in forward order by one node each (Linear
    weights transposed for MatMul, as torch.onnx exports them)."""
    from skyrim_amd.fuxi.spec import param_spec
    blob, inits, nodes = bytearray(), b"", b""
    for i, (slot, shape) in enumerate(param_spec(cfg)):
        if slot in drop:
            continue
        a = np.ascontiguousarray(params[f"{stage}.{slot}"].numpy().astype("<f4"))
        op = "Add"
        if len(shape) == 2:
            a, op = np.ascontiguousarray(a.T), "MatMul"
        elif len(shape) >= 4:
            op = "Conv"
        name = f"onnx::{op}_{1000 + i}"
        inits += _ld(5, _ext_tensor(name, a, f"{stage}.bin", len(blob)))
        blob += a.tobytes()
        nodes += _ld(1, _ld(1, b"h") + _ld(1, name.encode()) + _ld(2, b"h") + _ld(4, op.encode()))
    (path / f"{stage}.bin").write_bytes(bytes(blob))
    (path / f"{stage}.onnx").write_bytes(_vi(1 << 3 | 0) + _vi(8) + _ld(7, nodes + _ld(2, b"g") + inits))


def _onnx_dir(path: Path, cfg, params, drop=()):
    for st in ("short", "medium", "long"):
        _write_stage(path, cfg, params, st, drop)
    (path / "norm.json").write_text(json.dumps({"mean": params["norm.mean"].tolist(), "std": params["norm.std"].tolist()}))


def test_onnx_directory_round_trip_with_external_data(tmp_path):
    from skyrim_amd.fuxi import checkpoint
    from skyrim_amd.fuxi.spec import full_param_spec, init_synthetic
    cfg = _toy(depth=1, embed=256, heads=4, groups=8)
    params = dict(init_synthetic(cfg, 2))
    _onnx_dir(tmp_path, cfg, params)
    got = checkpoint.load(str(tmp_path), cfg)
    assert set(got) == {n for n, _ in full_param_spec(cfg)}
    for k, v in params.items():
        assert torch.equal(got[k], v.float()), k
    # an explicit mapping takes precedence over the automatic one
    from skyrim_amd.pangu.onnx_weights import read_model
    mapping, unresolved = checkpoint.stage_mapping(read_model(tmp_path / "short.onnx", base_dir=tmp_path), cfg)
    assert not unresolved
    swapped = dict(mapping, **{"embed.bias": mapping["time_embed.bias"], "time_embed.bias": mapping["embed.bias"]})
    (tmp_path / "short.map.json").write_text(json.dumps(swapped))
    got = checkpoint.load(str(tmp_path), cfg)
    assert torch.equal(got["short.embed.bias"], params["short.time_embed.bias"]) and torch.equal(got["medium.embed.bias"], params["medium.embed.bias"])


def test_onnx_unresolved_slots_are_reported(tmp_path):
    from skyrim_amd.fuxi import checkpoint
    from skyrim_amd.fuxi.spec import init_synthetic
    cfg = _toy(depth=1, embed=256, heads=4, groups=8)
    params = dict(init_synthetic(cfg, 2))
    _onnx_dir(tmp_path, cfg, params, drop=("head.weight", "head.bias"))
    with pytest.raises(ValueError, match=r"2 parameter slots unresolved: \['head.weight', 'head.bias'\]"):
        checkpoint.load(str(tmp_path), cfg)


def test_a_stage_is_one_graph_of_the_shared_reader(tmp_path):
    from skyrim_amd.fuxi import checkpoint
    from skyrim_amd.fuxi.spec import init_synthetic, param_spec
    from skyrim_amd.pangu.onnx_weights import load_graph_slots, read_norm_json
    cfg = _toy(depth=1, embed=256, heads=4, groups=8)
    params = dict(init_synthetic(cfg, 2))
    _onnx_dir(tmp_path, cfg, params)
    stage = load_graph_slots(str(tmp_path / "long.onnx"), param_spec(cfg), str(tmp_path / "long.map.json"))
    got = checkpoint.load(str(tmp_path), cfg)
    assert list(stage) == [s for s, _ in param_spec(cfg)]
    for slot, t in stage.items():
        assert t.dtype == torch.float32 and torch.equal(t, got[f"long.{slot}"]) and torch.equal(t, params[f"long.{slot}"].float()), slot
    mean, std = read_norm_json(str(tmp_path))
    assert torch.equal(mean, got["norm.mean"]) and torch.equal(std, got["norm.std"]) and read_norm_json(str(tmp_path / "nowhere")) is None
    (tmp_path / "norm.json").unlink()
    with pytest.raises(ValueError, match=r'norm\.json missing -- the input affine \(\{"mean": \[6\], "std": \[6\]\}\) of the graphs'):
        checkpoint.load(str(tmp_path), cfg)


def test_onnx_map_with_an_unknown_slot_or_a_failed_transform_is_refused_by_name(tmp_path):
    """The refusals of the directory reader FuXi shares with FengWu (pangu/onnx_weights.load_graph_slots): a mapped name that is no slot
    of the config, and a transform that does not give the slot's shape -- reported with the graph, the slot and the initializer."""
    from skyrim_amd.fuxi import checkpoint
    from skyrim_amd.fuxi.spec import init_synthetic
    from skyrim_amd.pangu.onnx_weights import read_model
    cfg = _toy(depth=1, embed=256, heads=4, groups=8)
    _onnx_dir(tmp_path, cfg, dict(init_synthetic(cfg, 2)))
    mapping, _ = checkpoint.stage_mapping(read_model(tmp_path / "medium.onnx", base_dir=tmp_path), cfg)
    (tmp_path / "medium.map.json").write_text(json.dumps(dict(mapping, **{"blocks.9.norm1.weight": mapping["embed.bias"]})))
    with pytest.raises(KeyError, match=r"medium\.map\.json: 'blocks\.9\.norm1\.weight' is not a parameter slot of this config"):
        checkpoint.load(str(tmp_path), cfg)
    (tmp_path / "medium.map.json").write_text(json.dumps(dict(mapping, **{"embed.bias": mapping["head.weight"]})))
    with pytest.raises(ValueError, match=r"medium\.onnx: slot embed\.bias: initializer 'onnx::MatMul_\d+': shape \(\d+, 256\) after 'T', slot wants \(256,\)"):
        checkpoint.load(str(tmp_path), cfg)
    (tmp_path / "medium.map.json").write_text(json.dumps(dict(mapping, **{"embed.bias": "no_such_tensor"})))
    with pytest.raises(KeyError, match=r"embed\.bias: initializer 'no_such_tensor' not in .*medium\.onnx"):
        checkpoint.load(str(tmp_path), cfg)


def test_external_data_without_the_opt_in_is_refused_as_before(tmp_path):
    from skyrim_amd.fuxi.spec import init_synthetic
    from skyrim_amd.pangu.onnx_weights import read_model
    cfg = _toy(depth=1, embed=256, heads=4, groups=8)
    _write_stage(tmp_path, cfg, dict(init_synthetic(cfg, 2)), "short")
    m = read_model(tmp_path / "short.onnx")
    t = next(iter(m.initializers.values()))
    with pytest.raises(ValueError, match="external_data initializers are not supported \\(re-export with raw data\\)"):
        t.array()
    # with the opt-in, a location outside the base directory is refused
    m = read_model(tmp_path / "short.onnx", base_dir=tmp_path / "elsewhere")
    with pytest.raises(ValueError, match="not a file inside"):
        next(iter(m.initializers.values())).array()
