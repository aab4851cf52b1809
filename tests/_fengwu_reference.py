"""Float64 restatement of one FengWu call, written from skyrim_amd/fengwu/spec.py's fields with plain torch ops (conv2d with zero-padded
rows, torch.roll + window partition / reverse, a dense bias gathered per window by relative coordinates, layer_norm, conv_transpose2d).
It shares nothing with the engine or the HIP side: it reads the configuration, spec.py's geometry helpers (padding, shifts, the bias
index and the shift mask -- each tested against direct loops in test_fengwu_cpu.py) and a parameter mapping.

Token grids are [Z][H][W][C] float64 tensors (Z = 1 in the encoders and decoders, the modalities in the fuser); states
[C][n_lat][n_lon]."""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

from skyrim_amd.fengwu.spec import bias_index, block_geometry, block_shift, pad_to, shift_mask


def P(params, name):
    return torch.as_tensor(params[name]).double().cpu()


def _ln(x, params, prefix, eps):
    return F.layer_norm(x, (x.shape[-1],), P(params, prefix + ".weight"), P(params, prefix + ".bias"), eps)


def _norm(params, x):
    m = P(params, "norm.mean")[:, None, None]
    s = P(params, "norm.std")[:, None, None]
    return (x.double().cpu() - m) / s


def embed(params, cfg, x0, x1):
    """Per modality: Conv2d(2 c_m -> D1, 4, stride 4) over [x0 ; x1] normalised and zero-padded in latitude, + bias, then LayerNorm
    -> list of [1][h1][w1][D1]."""
    n0, n1 = _norm(params, x0), _norm(params, x1)
    padded, front = cfg.lat_pad
    out = []
    for name, off, c in cfg.mod_slices():
        x = torch.cat([n0[off:off + c], n1[off:off + c]])
        x = F.pad(x, (0, 0, front, padded - cfg.n_lat - front))
        y = F.conv2d(x[None], P(params, f"enc.{name}.embed.weight"), P(params, f"enc.{name}.embed.bias"), stride=tuple(cfg.patch))[0]
        out.append(_ln(y.permute(1, 2, 0), params, f"enc.{name}.embed_norm", cfg.ln_eps)[None])
    return out


def attention(params, cfg, prefix, x, where, i):
    """Shifted-window attention of block ``prefix`` on h = x (already LayerNorm-ed) [Z][H][W][C]: zero-pad to the window multiple, roll,
    partition, qkv, scores + position bias (+ shift mask), softmax, reverse, roll back, crop."""
    grid, win, D, heads = block_geometry(cfg, where)
    Z, H, W, C = x.shape
    Zp, Hp, Wp = grid
    wz, wh, ww = win
    N, hd = wz * wh * ww, D // heads
    fh = pad_to(H, wh, cfg.pad)[1]
    s = block_shift(win, i)
    xp = F.pad(x, (0, 0, 0, Wp - W, fh, Hp - H - fh, 0, Zp - Z))
    xp = torch.roll(xp, tuple(-v for v in s), (0, 1, 2))
    nz, ny, nx = Zp // wz, Hp // wh, Wp // ww
    win_x = xp.reshape(nz, wz, ny, wh, nx, ww, C).permute(0, 2, 4, 1, 3, 5, 6).reshape(nz, ny, nx, N, C)
    qkv = win_x @ P(params, f"{prefix}.attn.qkv.weight").T + P(params, f"{prefix}.attn.qkv.bias")
    qkv = qkv.reshape(nz, ny, nx, N, 3, heads, hd).permute(4, 0, 1, 2, 5, 3, 6)          # [3][nz][ny][nx][heads][N][hd]
    q, k, v = qkv[0] / math.sqrt(hd), qkv[1], qkv[2]
    a = q @ k.transpose(-2, -1)                                                          # [nz][ny][nx][heads][N][N]
    tab = P(params, f"{prefix}.attn.bias_table")
    idx = bias_index(cfg, win)
    mask = shift_mask(grid, win, s).double() * cfg.mask_value
    bias = torch.empty(nz, ny, heads, N, N, dtype=torch.float64)
    for za in range(nz):
        for yb in range(ny):
            t = tab[idx] if cfg.bias == "relative" else tab[za * ny + yb][idx]
            bias[za, yb] = t.permute(2, 0, 1) + mask[za, yb][None]
    a = a + bias[:, :, None]
    o = a.softmax(-1) @ v                                                                # [nz][ny][nx][heads][N][hd]
    o = o.permute(0, 1, 2, 4, 3, 5).reshape(nz, ny, nx, wz, wh, ww, C).permute(0, 3, 1, 4, 2, 5, 6).reshape(Zp, Hp, Wp, C)
    o = torch.roll(o, s, (0, 1, 2))
    return o[:Z, fh:fh + H, :W]


def swin_block(params, cfg, prefix, x, where, i):
    """Pre-norm Swin block: x + proj(attn(LN1 x)), then x + fc2(GELU(fc1(LN2 x)))."""
    o = attention(params, cfg, prefix, _ln(x, params, f"{prefix}.norm1", cfg.ln_eps), where, i)
    x = x + o @ P(params, f"{prefix}.attn.proj.weight").T + P(params, f"{prefix}.attn.proj.bias")
    h = F.gelu(_ln(x, params, f"{prefix}.norm2", cfg.ln_eps) @ P(params, f"{prefix}.mlp.fc1.weight").T + P(params, f"{prefix}.mlp.fc1.bias"))
    return x + h @ P(params, f"{prefix}.mlp.fc2.weight").T + P(params, f"{prefix}.mlp.fc2.bias")


def merge(params, cfg, name, x):
    """Swin patch merge of [1][h1][w1][D1]: zero-pad rows to even, [x00 ; x10 ; x01 ; x11], LayerNorm, Linear(4 D1 -> D2, no bias)."""
    x = x[0]
    padded, front = cfg.merge_pad
    x = F.pad(x, (0, 0, 0, 0, front, padded - x.shape[0] - front))
    x = torch.cat([x[0::2, 0::2], x[1::2, 0::2], x[0::2, 1::2], x[1::2, 1::2]], -1)
    x = _ln(x, params, f"enc.{name}.merge.norm", cfg.ln_eps)
    return (x @ P(params, f"enc.{name}.merge.reduction.weight").T)[None]


def expand_skip(params, cfg, name, x, skip):
    """Linear(D2 -> 4 D1, no bias), 2 x 2 pixel shuffle, crop to h1 rows; then Linear([up ; skip]) -> D1."""
    h2, w2, _ = x[0].shape
    D1 = cfg.dims[0]
    y = (x[0] @ P(params, f"dec.{name}.expand.weight").T).reshape(h2, w2, 2, 2, D1).permute(0, 2, 1, 3, 4).reshape(2 * h2, 2 * w2, D1)
    front = cfg.merge_pad[1]
    up = y[front:front + cfg.grid1[0]]
    return (torch.cat([up, skip[0]], -1) @ P(params, f"dec.{name}.skip.weight").T + P(params, f"dec.{name}.skip.bias"))[None]


def recover(params, cfg, name, x):
    """ConvTranspose2d(D1 -> c_m, 4, stride 4), crop to n_lat rows, de-normalise its channels -> [c_m][n_lat][n_lon]."""
    y = F.conv_transpose2d(x[0].permute(2, 0, 1)[None], P(params, f"dec.{name}.recovery.weight"), P(params, f"dec.{name}.recovery.bias"),
                           stride=tuple(cfg.patch))[0]
    front = cfg.lat_pad[1]
    return y[:, front:front + cfg.n_lat]


def call(params, cfg, x0, x1):
    names = [n for n, _ in cfg.modalities]
    xs = embed(params, cfg, x0, x1)
    skips, x2 = [], []
    for name, x in zip(names, xs):
        for i in range(cfg.enc_depths[0]):
            x = swin_block(params, cfg, f"enc.{name}.s0.{i}", x, "s0", i)
        skips.append(x)
        y = merge(params, cfg, name, x)
        for i in range(cfg.enc_depths[1]):
            y = swin_block(params, cfg, f"enc.{name}.s1.{i}", y, "s1", i)
        x2.append(y)
    f = torch.cat(x2)                                                                    # [mods][h2][w2][D2]
    for i in range(cfg.fuser_depth):
        f = swin_block(params, cfg, f"fuser.{i}", f, "fuser", i)
    out = []
    for z, name in enumerate(names):
        y = f[z:z + 1]
        for i in range(cfg.dec_depths[0]):
            y = swin_block(params, cfg, f"dec.{name}.s1.{i}", y, "s1", i)
        x = expand_skip(params, cfg, name, y, skips[z])
        for i in range(cfg.dec_depths[1]):
            x = swin_block(params, cfg, f"dec.{name}.s0.{i}", x, "s0", i)
        out.append(recover(params, cfg, name, x))
    y = torch.cat(out)
    return y * P(params, "norm.std")[:, None, None] + P(params, "norm.mean")[:, None, None]


def per_channel_err(got, ref):
    """max |got - ref| / max |ref| per channel of [C][...] states."""
    got, ref = got.double().cpu().reshape(ref.shape), ref.double().cpu()
    return ((got - ref).abs().amax(dim=tuple(range(1, ref.dim()))) / ref.abs().amax(dim=tuple(range(1, ref.dim()))).clamp_min(1e-30))


def token_err(got, ref):
    """Per-channel error of token grids (channel = last axis)."""
    got, ref = got.double().cpu().reshape(-1, ref.shape[-1]), ref.double().cpu().reshape(-1, ref.shape[-1])
    return (got - ref).abs().amax(0) / ref.abs().amax(0).clamp_min(1e-30)
