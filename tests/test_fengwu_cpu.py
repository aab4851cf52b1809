"""FengWu without a GPU: the channel list and modality slices, spec sizes and parameter layout, the dense bias tables and the shift masks
against direct loops, the model registry, the C ABI surface and its argument checks, op registration, and the checkpoint reader (an ONNX
directory with external data against the torch file, unresolved slots, the explicit map, shape refusals)."""
from __future__ import annotations

import ctypes
import json
import re
from dataclasses import replace
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
# the reference's skyrim/core/models/fengwu.py CHANNELS, as data
REFERENCE_CHANNELS = (["u10m", "v10m", "t2m", "msl"] + [f"z{p}" for p in (50, 100, 150, 200, 250, 300, 400, 500, 600, 700, 850, 925, 1000)]
                      + [f"q{p}" for p in (50, 100, 150, 200, 250, 300, 400, 500, 600, 700, 850, 925, 1000)]
                      + [f"u{p}" for p in (50, 100, 150, 200, 250, 300, 400, 500, 600, 700, 850, 925, 1000)]
                      + [f"v{p}" for p in (50, 100, 150, 200, 250, 300, 400, 500, 600, 700, 850, 925, 1000)]
                      + [f"t{p}" for p in (50, 100, 150, 200, 250, 300, 400, 500, 600, 700, 850, 925, 1000)])
TOY = dict(n_lat=33, n_lon=64, modalities=(("surface", 4), ("z", 5), ("q", 5), ("u", 5), ("v", 5), ("t", 5)), dims=(64, 128),
           heads=(2, 4), enc_depths=(1, 1), dec_depths=(1, 1), fuser_depth=2, window2d=(4, 4), window3d=(2, 4, 4))


def _toy(**kw):
    from skyrim_amd.fengwu.spec import FengwuConfig
    return FengwuConfig(**{**TOY, **kw})


# ---- spec ------------------------------------------------------------------------------------------------------------------------------ #
def test_channels_and_modality_slices():
    from skyrim_amd.fengwu.spec import CHANNELS, FengwuConfig
    assert CHANNELS == REFERENCE_CHANNELS and len(CHANNELS) == 69
    cfg = FengwuConfig()
    covered = []
    for name, off, c in cfg.mod_slices():
        names = CHANNELS[off:off + c]
        covered += names
        assert all(n.startswith(name) for n in names) if name != "surface" else names == ["u10m", "v10m", "t2m", "msl"]
    assert covered == CHANNELS


def test_grid_sizes_param_spec_and_flops():
    from skyrim_amd.fengwu.spec import FengwuConfig, block_geometry, flops_per_call, full_param_spec, n_launches, n_parameters, param_spec
    cfg = FengwuConfig()
    assert cfg.lat_pad == (724, 1) and cfg.grid1 == (181, 360) and cfg.merge_pad == (182, 0) and cfg.grid2 == (91, 180)
    assert block_geometry(cfg, "s0") == ((1, 186, 360), (1, 6, 12), 192, 6)
    assert block_geometry(cfg, "s1") == ((1, 96, 180), (1, 6, 12), 384, 12)
    assert block_geometry(cfg, "fuser") == ((6, 96, 180), (2, 6, 12), 384, 12)
    assert cfg.k_embed == 416 and cfg.n_recover == 208 and n_launches(cfg) == 161
    spec = dict(param_spec(cfg))
    per_block = 13
    blocks = 6 * (2 + 6 + 6 + 2) + 6
    assert len(spec) == blocks * per_block + 6 * (4 + 3) + 6 * (3 + 2)
    assert spec["enc.surface.embed.weight"] == (192, 8, 4, 4) and spec["enc.t.embed.weight"] == (192, 26, 4, 4)
    assert spec["enc.z.s0.1.attn.qkv.weight"] == (576, 192) and spec["enc.z.s0.1.attn.bias_table"] == (11 * 23, 6)
    assert spec["enc.q.merge.reduction.weight"] == (384, 768) and spec["enc.q.s1.5.mlp.fc1.weight"] == (1536, 384)
    assert spec["fuser.5.attn.bias_table"] == (3 * 11 * 23, 12) and "fuser.6.norm1.weight" not in spec
    assert spec["dec.u.expand.weight"] == (768, 384) and spec["dec.u.skip.weight"] == (192, 384)
    assert spec["dec.surface.recovery.weight"] == (192, 4, 4, 4) and spec["dec.v.recovery.bias"] == (13,)
    assert next(iter(spec)) == "enc.surface.embed.weight" and list(spec)[-1] == "dec.t.recovery.bias"
    full = [n for n, _ in full_param_spec(cfg)]
    assert full[:2] == ["norm.mean", "norm.std"] and len(full) == 2 + len(spec)
    assert 140e6 < n_parameters(cfg) < 170e6
    assert 7.5e12 < flops_per_call(cfg) < 9.5e12              # the ~8.3 TFLOP of one call
    es = dict(param_spec(replace(cfg, bias="earth_specific")))
    assert es["enc.z.s0.0.attn.bias_table"] == (31, 36 * 23, 6) and es["fuser.0.attn.bias_table"] == (3 * 16, 4 * 36 * 23, 12)


def test_check_config_refusals():
    from skyrim_amd.fengwu.spec import FengwuConfig, check_config
    check_config(FengwuConfig())
    with pytest.raises(ValueError, match="does not tile"):
        check_config(FengwuConfig(window2d=(6, 7)))
    with pytest.raises(ValueError, match="does not tile"):
        check_config(FengwuConfig(window3d=(4, 6, 12)))
    with pytest.raises(ValueError, match="head dim"):
        check_config(FengwuConfig(heads=(3, 12)))
    for k, v in (("predicts", "increment"), ("skip", "add"), ("shift_mask", "all"), ("out_select", "both")):
        with pytest.raises(ValueError, match=k):
            check_config(replace(FengwuConfig(), **{k: v}))


def _swin_img_regions(Z, H, W, win, shift):
    """Region id of every padded-grid token, Swin's img_mask construction extended to (modality, lat); longitude never split."""
    img = torch.zeros(Z, H, W)
    cnt = 0
    zs = (slice(0, -win[0]), slice(-win[0], -shift[0]), slice(-shift[0], None)) if shift[0] else (slice(None),)
    hs = (slice(0, -win[1]), slice(-win[1], -shift[1]), slice(-shift[1], None)) if shift[1] else (slice(None),)
    for a in zs:
        for b in hs:
            img[a, b, :] = cnt
            cnt += 1
    return img


@pytest.mark.parametrize("grid,win,shift", [((1, 12, 8), (1, 4, 4), (0, 2, 2)), ((6, 8, 8), (2, 4, 4), (1, 2, 2)), ((6, 8, 8), (2, 4, 4), (0, 0, 0))])
def test_shift_mask_against_direct_loops(grid, win, shift):
    from skyrim_amd.fengwu.spec import shift_mask
    Z, H, W = grid
    m = shift_mask(grid, win, shift)
    img = _swin_img_regions(Z, H, W, win, shift)
    wz, wh, ww = win
    for a in range(Z // wz):
        for b in range(H // wh):
            for c in range(W // ww):
                reg = [float(img[a * wz + iz, b * wh + iy, c * ww + ix]) for iz in range(wz) for iy in range(wh) for ix in range(ww)]
                want = torch.tensor([[ri != rj for rj in reg] for ri in reg])
                assert torch.equal(m[a, b], want), (a, b, c)


@pytest.mark.parametrize("bias", ["relative", "earth_specific"])
@pytest.mark.parametrize("shifted", [False, True])
def test_bias_table_against_direct_loops(bias, shifted):
    """The dense table the kernel reads, entry by entry: the position bias of the convention + mask_value where the mask separates
    query and key, for every window (through the kernel's type rule)."""
    from skyrim_amd.fengwu.spec import bias_param_shape, bias_table, block_shift, shift_mask, type_of, window_types
    cfg = _toy(bias=bias)
    grid, win, heads = (6, 8, 8), (2, 4, 4), 3
    wz, wh, ww = win
    sh = block_shift(win, 1 if shifted else 0)
    param = torch.randn(bias_param_shape(cfg, grid, win, heads), generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    tab = bias_table(cfg, param, grid, win, sh)
    tz, ty = window_types(cfg, grid, win, sh)
    assert tab.shape == (tz * ty, heads, wz * wh * ww, wz * wh * ww)
    mask = shift_mask(grid, win, sh)
    nz, ny = grid[0] // wz, grid[1] // wh
    for a in range(nz):
        for b in range(ny):
            t = type_of(tz, nz, a) * ty + type_of(ty, ny, b)
            for i in range(wz * wh * ww):
                zi, yi, xi = i // (wh * ww), (i // ww) % wh, i % ww
                for j in range(wz * wh * ww):
                    zj, yj, xj = j // (wh * ww), (j // ww) % wh, j % ww
                    if bias == "relative":
                        row = ((zi - zj + wz - 1) * (2 * wh - 1) + yi - yj + wh - 1) * (2 * ww - 1) + xi - xj + ww - 1
                        want = param[row]
                    else:
                        row = ((zi * wz + zj) * wh * wh + yi * wh + yj) * (2 * ww - 1) + xi - xj + ww - 1
                        want = param[a * ny + b, row]
                    want = want + (cfg.mask_value if mask[a, b, i, j] else 0.0)
                    assert torch.equal(tab[t, :, i, j], want), (a, b, i, j)


def test_fengwu_is_registered_but_not_a_cli_choice():
    from skyrim_amd import common
    from skyrim_amd.core import Skyrim
    from skyrim_amd.core.models import MODELS
    assert "fengwu" in MODELS and MODELS["fengwu"].model_name == "fengwu"
    assert "fengwu" in Skyrim.list_available_models()
    assert "fengwu" not in common.AVAILABLE_MODELS


# ---- C ABI ----------------------------------------------------------------------------------------------------------------------------- #
def test_header_symbols_equal_exports_and_library_has_them():
    from skyrim_amd.fengwu import engine
    hdr = (ROOT / "include" / "skyrim_fengwu.h").read_text()
    names = set(re.findall(r"^(?:int|const char\*) (skfw_\w+)\(", hdr, re.M))
    assert names == set(engine.EXPORTS)
    lib = engine.load_library()
    for n in names:
        assert hasattr(lib, n)
    assert lib.skfw_abi_version() == 1 == engine.ABI_VERSION
    assert "#define SKFW_ABI_VERSION 1" in hdr
    assert lib.skfw_error_string(-1) == b"invalid argument" and lib.skfw_error_string(-2) == b"HIP runtime error"
    assert b"does not tile" in lib.skfw_error_string(-3)


def _attn(**kw):
    from skyrim_amd.fengwu import engine
    f = dict(qkv=16, qkv_bias=16, table=16, out=16, table_sb=0, batch=1, Z=1, H=9, W=16, Zp=1, Hp=12, Wp=16, fz=0, fh=1, fw=0, wz=1, wh=4, ww=4,
             sz=0, sh=0, sw=0, types_z=1, types_y=1, C=64, heads=2, scale=0.17)
    f.update(kw)
    return engine.AttnDesc(**f)


def test_argument_errors_without_gpu():
    from skyrim_amd.fengwu import engine
    lib = engine.load_library()
    assert lib.skfw_prepare_weight(None, 1, 1, 4, 4, None, 16, 8, None) == -1
    for fn in (lib.skfw_embed, lib.skfw_layer_norm, lib.skfw_linear, lib.skfw_window_attention, lib.skfw_recover):
        assert fn(None, None) == -1
    # a window that does not tile its padded grid, in latitude, longitude or the modality axis
    for kw in (dict(Hp=10), dict(Wp=18, W=18), dict(Z=3, Zp=3, wz=2)):
        assert lib.skfw_window_attention(ctypes.byref(_attn(**kw)), None) == -3, kw
    for kw in (dict(C=96, heads=2), dict(sh=4), dict(types_y=4), dict(Hp=8), dict(fh=4), dict(qkv=8)):        # head dim 48, shift = window,
        assert lib.skfw_window_attention(ctypes.byref(_attn(**kw)), None) == -1, kw                           # 4 types of 3 rows, grid too small,
    ln = engine.LnDesc(16, 16, 16, 16, 10, 1, 2048, 0, 0, 0, 0, 1e-5)                                         # unaligned
    assert lib.skfw_layer_norm(ctypes.byref(ln), None) == -1                                                   # C above 1536
    ln = engine.LnDesc(16, 16, 16, 16, 10, 1, 136, 1, 9, 16, 0, 1e-5)                                          # merge: C % 16
    assert lib.skfw_layer_norm(ctypes.byref(ln), None) == -1
    li = engine.LinearDesc(16, None, 16, 64 * 16, 64 * 16, 16, None, None, 16, 0, 0, 0, 0, 1, 10, 64, 12, 12, 0, 0, 0, 0, 0, 0, 0)   # K % 8
    assert lib.skfw_linear(ctypes.byref(li), None) == -1
    li = engine.LinearDesc(16, None, 16, 5 * 64 * 16, 64 * 16, 16, None, None, 16, 0, 0, 0, 0, 6, 10, 64, 16, 16, 0, 0, 0, 0, 0, 0, 0)  # W planes
    assert lib.skfw_linear(ctypes.byref(li), None) == -1                                                                                    # of 6 overlap
    off, cnt = (ctypes.c_int * 8)(0, 2), (ctypes.c_int * 8)(2, 0)
    e = engine.EmbedDesc(16, 16, 16, 16, 16, 10 ** 6, 10 ** 5, 64, 16, 16, 2, 33, 64, 1, 9, 64, 64, off, cnt)   # a modality of 0 channels
    assert lib.skfw_embed(ctypes.byref(e), None) == -1
    r = engine.RecoverDesc(16, 16, 10 ** 6, 10 ** 5, 64, 16, 16, 16, 16, 2, 9, 16, 64, 1, 33, 1, (ctypes.c_int * 8)(0, 2),
                           (ctypes.c_int * 8)(2, 3))                                                         # 3 channels > c_max 1
    assert lib.skfw_recover(ctypes.byref(r), None) == -1


def test_fengwu_ops_have_no_cpu_kernel():
    from skyrim_amd import ops
    assert {n for n in ops.OP_NAMES if n.startswith("fengwu_")} == {"fengwu_layer_norm", "fengwu_window_attention"}
    with pytest.raises(NotImplementedError):
        ops.hip.fengwu_layer_norm(torch.zeros(8), torch.ones(4), torch.zeros(4), torch.zeros(8), 2, 1, 4, 1e-5)


# ---- checkpoint ------------------------------------------------------------------------------------------------------------------------ #
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


def _onnx_dir(path: Path, cfg, params, drop=(), reshape=None):
    """``fengwu.onnx`` + ``fengwu.bin``: the parameters under opaque names, used in order of use by one node each (Linear weights
    transposed for MatMul, as torch.onnx exports them; bias tables read by Gather), plus global_means.npy / global_stds.npy."""
    from skyrim_amd.fengwu.spec import param_spec
    blob, inits, nodes = bytearray(), b"", b""
    for i, (slot, shape) in enumerate(param_spec(cfg)):
        if slot in drop:
            continue
        a = np.ascontiguousarray(params[slot].numpy().astype("<f4"))
        if reshape and slot in reshape:
            a = np.ascontiguousarray(a.reshape(reshape[slot]))
        op = "Add"
        if slot.endswith("bias_table"):
            op = "Gather"
        elif len(shape) == 2:
            a, op = np.ascontiguousarray(a.T), "MatMul"
        elif len(shape) >= 4:
            op = "Conv"
        name = f"onnx::{op}_{1000 + i}"
        inits += _ld(5, _ext_tensor(name, a, "fengwu.bin", len(blob)))
        blob += a.tobytes()
        nodes += _ld(1, _ld(1, b"h") + _ld(1, name.encode()) + _ld(2, b"h") + _ld(4, op.encode()))
    (path / "fengwu.bin").write_bytes(bytes(blob))
    (path / "fengwu.onnx").write_bytes(_vi(1 << 3 | 0) + _vi(8) + _ld(7, nodes + _ld(2, b"g") + inits))
    np.save(path / "global_means.npy", params["norm.mean"].numpy().reshape(1, -1, 1, 1))
    np.save(path / "global_stds.npy", params["norm.std"].numpy().reshape(1, -1, 1, 1))


def test_onnx_directory_loads_into_the_torch_file_dict(tmp_path):
    from skyrim_amd.fengwu import checkpoint
    from skyrim_amd.fengwu.spec import full_param_spec, init_synthetic
    cfg = _toy()
    params = {k: v.float() for k, v in init_synthetic(cfg, 2).items()}
    torch.save(params, tmp_path / "fengwu.pt")
    d = tmp_path / "graph"
    d.mkdir()
    _onnx_dir(d, cfg, params)
    from_torch = checkpoint.load(str(tmp_path / "fengwu.pt"), cfg)
    from_onnx = checkpoint.load(str(d), cfg)
    assert set(from_onnx) == set(from_torch) == {n for n, _ in full_param_spec(cfg)}
    for k, v in from_torch.items():
        assert torch.equal(from_onnx[k], v), k
    # the explicit map takes precedence over the automatic one
    from skyrim_amd.pangu.onnx_weights import read_model
    mapping, unresolved = checkpoint.graph_mapping(read_model(d / "fengwu.onnx", base_dir=d), cfg)
    assert not unresolved
    swapped = dict(mapping, **{"enc.z.embed.bias": mapping["enc.q.embed.bias"], "enc.q.embed.bias": mapping["enc.z.embed.bias"]})
    (d / checkpoint.MAP_FILE).write_text(json.dumps(swapped))
    got = checkpoint.load(str(d), cfg)
    assert torch.equal(got["enc.z.embed.bias"], params["enc.q.embed.bias"]) and torch.equal(got["enc.u.embed.bias"], params["enc.u.embed.bias"])


def test_onnx_unresolved_slots_are_reported(tmp_path):
    from skyrim_amd.fengwu import checkpoint
    from skyrim_amd.fengwu.spec import init_synthetic
    cfg = _toy()
    _onnx_dir(tmp_path, cfg, {k: v.float() for k, v in init_synthetic(cfg, 2).items()}, drop=("dec.t.recovery.weight", "dec.t.recovery.bias"))
    with pytest.raises(ValueError, match=r"2 parameter slots unresolved: \['dec.t.recovery.weight', 'dec.t.recovery.bias'\]"):
        checkpoint.load(str(tmp_path), cfg)


def test_the_graph_is_one_graph_of_the_shared_reader(tmp_path):
    from skyrim_amd.fengwu import checkpoint
    from skyrim_amd.fengwu.spec import init_synthetic, param_spec
    from skyrim_amd.pangu.onnx_weights import load_graph_slots, read_model
    cfg = _toy()
    params = {k: v.float() for k, v in init_synthetic(cfg, 2).items()}
    _onnx_dir(tmp_path, cfg, params)
    graph = load_graph_slots(str(tmp_path / "fengwu.onnx"), param_spec(cfg), str(tmp_path / checkpoint.MAP_FILE))
    assert list(graph) == [s for s, _ in param_spec(cfg)] and all(torch.equal(t, params[s]) for s, t in graph.items())
    # norm.json stands in for the two .npy files, with the same size check
    (tmp_path / "global_means.npy").unlink()
    with pytest.raises(ValueError, match=r"the input affine is missing \(global_means\.npy \+ global_stds\.npy, or norm\.json\)"):
        checkpoint.load(str(tmp_path), cfg)
    (tmp_path / "norm.json").write_text(json.dumps({"mean": params["norm.mean"].tolist(), "std": params["norm.std"].tolist()}))
    got = checkpoint.load(str(tmp_path), cfg)
    assert torch.equal(got["norm.mean"], params["norm.mean"]) and torch.equal(got["norm.std"], params["norm.std"])
    # a mapped name that is no slot of this config
    mapping, _ = checkpoint.graph_mapping(read_model(tmp_path / "fengwu.onnx", base_dir=tmp_path), cfg)
    (tmp_path / checkpoint.MAP_FILE).write_text(json.dumps(dict(mapping, **{"enc.w.embed.bias": mapping["enc.z.embed.bias"]})))
    with pytest.raises(KeyError, match=r"fengwu\.map\.json: 'enc\.w\.embed\.bias' is not a parameter slot of this config"):
        checkpoint.load(str(tmp_path), cfg)


def test_shape_mismatch_names_the_slot_and_the_field(tmp_path):
    from skyrim_amd.fengwu import checkpoint
    from skyrim_amd.fengwu.engine import FengwuEngine
    from skyrim_amd.fengwu.spec import init_synthetic
    cfg = _toy()
    params = {k: v.float() for k, v in init_synthetic(cfg, 2).items()}
    _onnx_dir(tmp_path, cfg, params)
    from skyrim_amd.pangu.onnx_weights import read_model
    mapping, _ = checkpoint.graph_mapping(read_model(tmp_path / "fengwu.onnx", base_dir=tmp_path), cfg)
    # a map that points a slot at an initializer of another shape
    (tmp_path / checkpoint.MAP_FILE).write_text(json.dumps(dict(mapping, **{"enc.z.s0.0.attn.bias_table": mapping["enc.z.s0.0.norm1.weight"]})))
    with pytest.raises(ValueError, match=r"slot enc\.z\.s0\.0\.attn\.bias_table \(shape from FengwuConfig\.bias"):
        checkpoint.load(str(tmp_path), cfg)
    # a parameter dict of another config: refused before anything touches a GPU
    other = _toy(dims=(96, 128), heads=(3, 4))
    bad = {k: v.float() for k, v in init_synthetic(other, 2).items()}
    eng = FengwuEngine.__new__(FengwuEngine)
    eng.cfg, eng.device = cfg, torch.device("cpu")
    with pytest.raises(ValueError, match=r"parameter enc\.surface\.embed\.weight: expected shape \(64, 8, 4, 4\) \(from FengwuConfig\.dims"):
        eng.load_params(bad)
    with pytest.raises(ValueError, match="the input affine holds 29 / 29 values, the config's modalities 69 channels"):
        checkpoint.load(str(tmp_path), replace(cfg, modalities=(("surface", 4), ("z", 13), ("q", 13), ("u", 13), ("v", 13), ("t", 13))))
