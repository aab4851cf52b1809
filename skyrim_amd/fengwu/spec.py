"""Shapes, constants, parameter layout, tables and synthetic inputs of the FengWu call (cross-modal Swin transformer).

The network is FengWu (arXiv 2304.02948) as earth2studio's ``FengWu`` wraps it (the reference's skyrim/core/models/fengwu.py): two
69-channel levels (t - 6 h, t) on 721 x 1440 -> one encoder per modality (surface, z, q, u, v, t: patch embedding, Swin blocks at
181 x 360, patch merge, Swin blocks at 91 x 180) -> a fuser of 3-D Swin blocks over the six encoded fields stacked as a (modality, lat,
lon) grid -> one decoder per modality (Swin blocks, patch expand, skip from the encoder, Swin blocks, transposed-conv recovery) -> the
state at t + 6 h.

Every constant the kernels (csrc/fengwu_ops.hip), the engine and the float64 restatement (tests/_fengwu_reference.py) must agree on is a
field of ``FengwuConfig`` or a function here.  The released ONNX graph could not be inspected offline; the fields marked UNVERIFIED are
the points DESIGN.md 16 lists, each with where its default came from.
"""
from __future__ import annotations

import math
import zlib
from collections.abc import Mapping
from dataclasses import dataclass

import numpy as np
import torch

LEVELS = [50, 100, 150, 200, 250, 300, 400, 500, 600, 700, 850, 925, 1000]
# the reference's order (skyrim/core/models/fengwu.py CHANNELS): the four surface fields, then z, q, u, v, t at 13 levels
CHANNELS = ["u10m", "v10m", "t2m", "msl"] + [f"{v}{p}" for v in ("z", "q", "u", "v", "t") for p in LEVELS]
# (center, scale) of the synthetic data: ERA5-like magnitudes (geopotential in m^2 s^-2, specific humidity in kg / kg)
_Z_M = [20600, 16200, 13600, 11800, 10400, 9200, 7200, 5600, 4200, 3000, 1460, 770, 110]
_Q = [2.6e-6, 2.6e-6, 2.8e-6, 4e-6, 1e-5, 3e-5, 1.2e-4, 4e-4, 9e-4, 1.7e-3, 4e-3, 6e-3, 8e-3]
_T_K = [212, 208, 210, 216, 222, 229, 243, 253, 261, 267, 274, 278, 283]
_STATS = ([(0.0, 5.0), (0.0, 4.5), (278.0, 21.0), (101100.0, 1100.0)]
          + [(9.80665 * z, 9.80665 * (40 + 0.02 * z)) for z in _Z_M] + [(q, 0.8 * q) for q in _Q]
          + [(6.0, 12.0)] * 13 + [(0.0, 7.0)] * 13 + [(t, 6.0 + 0.02 * (t - 200)) for t in _T_K])
MAX_MODALITIES = 8                          # the kernels' per-modality argument arrays
HEAD_DIM = 32                               # the only head dim compiled


def pad_to(n: int, mult: int, pad: str = "centre") -> tuple[int, int]:
    """(padded, front): n zero-padded up to a multiple of ``mult``; "centre" puts (padded - n) // 2 in front, "back" none
    (PanguGeometry.pad's meaning)."""
    padded = (n + mult - 1) // mult * mult
    return padded, ((padded - n) // 2 if pad == "centre" else 0)


@dataclass(frozen=True)
class FengwuConfig:
    n_lat: int = 721                        # 90 .. -90
    n_lon: int = 1440                       # 0 .. 359.75
    # UNVERIFIED (the split; the order is the reference's): contiguous slices of CHANNELS, one encoder / decoder each
    modalities: tuple = (("surface", 4), ("z", 13), ("q", 13), ("u", 13), ("v", 13), ("t", 13))
    io_layout: str = "concat_levels"        # UNVERIFIED: input [x(t-6h) ; x(t)] normalised; modality m reads its 2 c_m planes
    out_select: str = "first"               # UNVERIFIED: output planes 0..68 = the state; the uncertainty planes are not computed
    predicts: str = "state"                 # UNVERIFIED: the output is the state, not an increment
    affine_from: str = "params"             # UNVERIFIED: norm.mean / norm.std applied outside the graph
    patch: tuple = (4, 4)                   # UNVERIFIED: stride-4 patch embedding; 721 rows zero-padded to 724 -> 181 x 360 tokens
    pad: str = "centre"                     # UNVERIFIED: where zero rows go ("centre" | "back"); also pads token grids to the window
    dims: tuple = (192, 384)                # UNVERIFIED: token width at 181 x 360 and at 91 x 180
    heads: tuple = (6, 12)                  # UNVERIFIED: head dim 32 at both widths
    enc_depths: tuple = (2, 6)              # UNVERIFIED: Swin blocks per encoder stage
    dec_depths: tuple = (6, 2)              # UNVERIFIED: Swin blocks per decoder stage (91 x 180 first)
    fuser_depth: int = 6                    # UNVERIFIED: 3-D blocks over the (modalities, 91, 180) stack at width dims[1]
    window2d: tuple = (6, 12)               # UNVERIFIED: (lat, lon) windows of the encoders and decoders
    window3d: tuple = (2, 6, 12)            # UNVERIFIED: (modality, lat, lon) windows of the fuser
    shift_mask: str = "lat+mod"             # UNVERIFIED: odd blocks shift by half a window; lat and modality masked, lon periodic
    bias: str = "relative"                  # UNVERIFIED: "relative" (Swin) | "earth_specific" (Pangu-style, one table per window type)
    skip: str = "concat_linear"             # UNVERIFIED: decoder 181 x 360 input = Linear([expand ; encoder stage 1]) -> dims[0]
    recovery: str = "tconv4"                # UNVERIFIED: ConvTranspose2d(dims[0] -> c_m, 4, stride 4), cropped, then y std + mean
    mlp_ratio: int = 4                      # exact-erf GELU between fc1 and fc2
    ln_eps: float = 1e-5
    mask_value: float = -100.0              # Swin's additive shifted-window mask

    @property
    def n_mod(self):
        return len(self.modalities)

    @property
    def channels(self):
        return sum(c for _, c in self.modalities)

    @property
    def offsets(self):                      # first channel of each modality
        return tuple(int(v) for v in np.cumsum([0] + [c for _, c in self.modalities])[:-1])

    @property
    def c_max(self):
        return max(c for _, c in self.modalities)

    @property
    def lat_pad(self):                      # (padded rows, front rows) of the input
        return pad_to(self.n_lat, self.patch[0], self.pad)

    @property
    def grid1(self):                        # 181 x 360
        return (self.lat_pad[0] // self.patch[0], self.n_lon // self.patch[1])

    @property
    def merge_pad(self):                    # (padded rows, front rows) of grid1 before the 2 x 2 merge
        return pad_to(self.grid1[0], 2, self.pad)

    @property
    def grid2(self):                        # 91 x 180
        return (self.merge_pad[0] // 2, self.grid1[1] // 2)

    @property
    def k_embed(self):                      # 2 c_max 16: every modality's K (smaller ones zero-padded)
        return 2 * self.c_max * self.patch[0] * self.patch[1]

    @property
    def n_recover(self):                    # c_max 16: every modality's recovery columns
        return self.c_max * self.patch[0] * self.patch[1]

    def mod_slices(self):
        return [(name, off, c) for (name, c), off in zip(self.modalities, self.offsets)]


def check_config(cfg: FengwuConfig):
    """The shapes and choices this build runs; ValueError otherwise (the kernels refuse the same shapes with an argument error)."""
    fixed = dict(io_layout="concat_levels", out_select="first", predicts="state", affine_from="params", skip="concat_linear",
                 recovery="tconv4", shift_mask="lat+mod", patch=(4, 4))
    for k, v in fixed.items():
        if getattr(cfg, k) != v:
            raise ValueError(f"{k} = {getattr(cfg, k)!r}: this build runs {v!r} only")
    if cfg.pad not in ("centre", "back"):
        raise ValueError(f"pad = {cfg.pad!r}: 'centre' or 'back'")
    if cfg.bias not in ("relative", "earth_specific"):
        raise ValueError(f"bias = {cfg.bias!r}: 'relative' or 'earth_specific'")
    if not 1 <= cfg.n_mod <= MAX_MODALITIES:
        raise ValueError(f"{cfg.n_mod} modalities: 1 .. {MAX_MODALITIES}")
    for d, h in zip(cfg.dims, cfg.heads):
        if d != HEAD_DIM * h:
            raise ValueError(f"dims {cfg.dims} / heads {cfg.heads}: head dim must be {HEAD_DIM} (the only one compiled)")
    if len(cfg.dims) != 2 or 4 * cfg.dims[0] > 1536 or cfg.dims[1] > 1536 or cfg.dims[0] % 8 or cfg.dims[1] % 8:
        raise ValueError(f"dims {cfg.dims}: two widths, multiples of 8, 4 dims[0] and dims[1] at most 1536 (the LayerNorm row)")
    if cfg.n_lon % (2 * cfg.patch[1]):
        raise ValueError(f"n_lon {cfg.n_lon} must be a multiple of {2 * cfg.patch[1]} (patch, then the 2 x 2 merge)")
    for name, grid, win in (("window2d", padded_grid(cfg, cfg.grid1, cfg.window2d), cfg.window2d),
                            ("window2d", padded_grid(cfg, cfg.grid2, cfg.window2d), cfg.window2d)):
        if grid[1] % win[1] or win[0] < 1 or win[1] < 1:
            raise ValueError(f"{name} {win} does not tile the padded token grid {grid}")
    wz, wh, ww = cfg.window3d
    if cfg.n_mod % wz or cfg.grid2[1] % ww or wz < 1:
        raise ValueError(f"window3d {cfg.window3d} does not tile the ({cfg.n_mod}, {cfg.grid2[0]}, {cfg.grid2[1]}) stack "
                         "(modality and longitude are not padded)")
    if (cfg.window2d[0] * cfg.window2d[1] > 1024) or (wz * wh * ww > 1024):
        raise ValueError("windows of at most 1024 tokens")


def padded_grid(cfg: FengwuConfig, grid, window) -> tuple:
    """A (lat, lon) token grid padded in latitude to a multiple of the window's rows (longitude must tile: periodic)."""
    return (pad_to(grid[0], window[0], cfg.pad)[0], grid[1])


def block_shift(window, block: int) -> tuple:
    """The cyclic shift of Swin block ``block`` (one entry per window axis): half a window on odd blocks."""
    return tuple(w // 2 for w in window) if block % 2 else tuple(0 for _ in window)


# ---- windows, masks and the dense bias table ------------------------------------------------------------------------------------- #
def window_region(i: int, n: int, win: int, s: int) -> int:
    """Swin's mask region of shifted-grid coordinate i (0: [0, n - win), 1: [n - win, n - s), 2: [n - s, n)); 0 without a shift."""
    if s == 0:
        return 0
    return 0 if i < n - win else (1 if i < n - s else 2)


def shift_mask(grid, window, shift) -> torch.Tensor:
    """[nWz][nWy][N][N] bool over a padded (Z, H, W) grid and (wz, wh, ww) windows of the shifted grid: True where query and key sit
    in different mask regions.  Modality (z) and latitude (h) are masked; longitude is periodic and never masked.  The mask does not
    depend on the longitude window, so one entry per (z, y) window row."""
    Z, H, W = grid
    wz, wh, ww = window
    sz, sh, _ = shift
    nz, ny = Z // wz, H // wh
    r = torch.arange(wz * wh * ww)
    rz, ry = r // (wh * ww), (r // ww) % wh
    out = torch.zeros(nz, ny, r.numel(), r.numel(), dtype=torch.bool)
    for a in range(nz):
        for b in range(ny):
            reg = torch.tensor([3 * window_region(a * wz + int(z), Z, wz, sz) + window_region(b * wh + int(y), H, wh, sh)
                                for z, y in zip(rz, ry)])
            out[a, b] = reg[:, None] != reg[None, :]
    return out


def window_types(cfg: FengwuConfig, grid, window, shift) -> tuple:
    """(types_z, types_y) of one block's dense table.  Window (a, b) of the nWz x nWy rows of windows uses type (tz, ty) with
    t = a / b itself when types == nW, (last row of windows ? 1 : 0) when types == 2, 0 when types == 1 (the kernel's rule)."""
    Z, H, _ = grid
    wz, wh, _ = window
    nz, ny = Z // wz, H // wh
    if cfg.bias == "earth_specific":
        return nz, ny
    tz = 2 if shift[0] and nz > 1 else 1
    ty = 2 if shift[1] and ny > 1 else 1
    return tz, ty


def type_of(n_types: int, n_win: int, i: int) -> int:
    return i if n_types == n_win else (int(i == n_win - 1) if n_types == 2 else 0)


def bias_param_shape(cfg: FengwuConfig, grid, window, heads: int) -> tuple:
    """The shape of one block's bias parameter.  relative: [(2 wz - 1)(2 wh - 1)(2 ww - 1)][heads] (Swin); earth_specific:
    [nWz nWy][wz^2 wh^2 (2 ww - 1)][heads] (Pangu's convention: absolute positions in modality and latitude, relative in longitude,
    one table per window row)."""
    wz, wh, ww = window
    if cfg.bias == "relative":
        return ((2 * wz - 1) * (2 * wh - 1) * (2 * ww - 1), heads)
    Z, H, _ = grid
    return ((Z // wz) * (H // wh), wz * wz * wh * wh * (2 * ww - 1), heads)


def bias_index(cfg: FengwuConfig, window) -> torch.Tensor:
    """[N][N] long: the row of the bias parameter that query i, key j of a window read (the second axis for earth_specific)."""
    wz, wh, ww = window
    r = torch.arange(wz * wh * ww)
    z, y, x = r // (wh * ww), (r // ww) % wh, r % ww
    dx = x[:, None] - x[None, :] + ww - 1
    if cfg.bias == "relative":
        dz = z[:, None] - z[None, :] + wz - 1
        dy = y[:, None] - y[None, :] + wh - 1
        return (dz * (2 * wh - 1) + dy) * (2 * ww - 1) + dx
    zz = z[:, None] * wz + z[None, :]
    yy = y[:, None] * wh + y[None, :]
    return (zz * (wh * wh) + yy) * (2 * ww - 1) + dx


def bias_table(cfg: FengwuConfig, param: torch.Tensor, grid, window, shift) -> torch.Tensor:
    """The dense float64 table [types_z types_y][heads][N][N] the attention kernel reads: the position bias of either convention,
    gathered per query / key pair, plus ``mask_value`` where the shift mask separates them.  Built once at load time."""
    Z, H, _ = grid
    wz, wh, _ = window
    nz, ny = Z // wz, H // wh
    tz, ty = window_types(cfg, grid, window, shift)
    idx = bias_index(cfg, window)
    p = param.double().cpu()
    mask = shift_mask(grid, window, shift)
    out = []
    for a in range(tz):
        for b in range(ty):
            # a representative window of this type: type t of n types is window t (n == nW), the last row (t == 1) or the first (t == 0)
            wa = a if tz == nz else (nz - 1 if a == 1 else 0)
            wb = b if ty == ny else (ny - 1 if b == 1 else 0)
            tab = p[idx] if cfg.bias == "relative" else p[wa * ny + wb][idx]        # [N][N][heads]
            out.append(tab.permute(2, 0, 1) + cfg.mask_value * mask[wa, wb].double()[None])
    return torch.stack(out).contiguous()


# ---- parameters ------------------------------------------------------------------------------------------------------------------ #
def _block(prefix: str, D: int, heads: int, hidden: int, bias_shape: tuple) -> list:
    return [(f"{prefix}.norm1.weight", (D,)), (f"{prefix}.norm1.bias", (D,)), (f"{prefix}.attn.qkv.weight", (3 * D, D)),
            (f"{prefix}.attn.qkv.bias", (3 * D,)), (f"{prefix}.attn.bias_table", bias_shape), (f"{prefix}.attn.proj.weight", (D, D)),
            (f"{prefix}.attn.proj.bias", (D,)), (f"{prefix}.norm2.weight", (D,)), (f"{prefix}.norm2.bias", (D,)),
            (f"{prefix}.mlp.fc1.weight", (hidden, D)), (f"{prefix}.mlp.fc1.bias", (hidden,)), (f"{prefix}.mlp.fc2.weight", (D, hidden)),
            (f"{prefix}.mlp.fc2.bias", (D,))]


def block_geometry(cfg: FengwuConfig, where: str):
    """(padded (Z, H, W) grid, window (wz, wh, ww), width, heads) of the blocks at ``where``: "s0" (181 x 360), "s1" (91 x 180) or
    "fuser" (modalities x 91 x 180)."""
    if where == "fuser":
        wz, wh, ww = cfg.window3d
        return (cfg.n_mod, pad_to(cfg.grid2[0], wh, cfg.pad)[0], cfg.grid2[1]), cfg.window3d, cfg.dims[1], cfg.heads[1]
    g = cfg.grid1 if where == "s0" else cfg.grid2
    lvl = 0 if where == "s0" else 1
    return (1,) + padded_grid(cfg, g, cfg.window2d), (1,) + tuple(cfg.window2d), cfg.dims[lvl], cfg.heads[lvl]


def param_spec(cfg: FengwuConfig) -> list[tuple]:
    """(name, shape) of the network's parameters in the graph's assumed order of use: each encoder in modality order (surface, z, q,
    u, v, t), the fuser, then each decoder in modality order.  Torch shapes (Linear [out, in], Conv2d [out, in, kh, kw],
    ConvTranspose2d [in, out, kh, kw]).  The z, q, u, v and t stacks have identical shapes: a checkpoint reader that maps by shape
    (checkpoint.py) tells them apart by this order alone.  The full dict adds ``norm.mean`` / ``norm.std`` in front."""
    D1, D2 = cfg.dims
    ph, pw = cfg.patch
    out = []
    geo = {w: block_geometry(cfg, w) for w in ("s0", "s1", "fuser")}

    def blocks(prefix, where, n):
        g, win, D, h = geo[where]
        return sum((_block(f"{prefix}.{i}", D, h, cfg.mlp_ratio * D, bias_param_shape(cfg, g, win, h)) for i in range(n)), [])

    for name, c in cfg.modalities:
        e = f"enc.{name}"
        out += [(f"{e}.embed.weight", (D1, 2 * c, ph, pw)), (f"{e}.embed.bias", (D1,)), (f"{e}.embed_norm.weight", (D1,)),
                (f"{e}.embed_norm.bias", (D1,))]
        out += blocks(f"{e}.s0", "s0", cfg.enc_depths[0])
        out += [(f"{e}.merge.norm.weight", (4 * D1,)), (f"{e}.merge.norm.bias", (4 * D1,)), (f"{e}.merge.reduction.weight", (D2, 4 * D1))]
        out += blocks(f"{e}.s1", "s1", cfg.enc_depths[1])
    out += blocks("fuser", "fuser", cfg.fuser_depth)
    for name, c in cfg.modalities:
        d = f"dec.{name}"
        out += blocks(f"{d}.s1", "s1", cfg.dec_depths[0])
        out += [(f"{d}.expand.weight", (4 * D1, D2)), (f"{d}.skip.weight", (D1, 2 * D1)), (f"{d}.skip.bias", (D1,))]
        out += blocks(f"{d}.s0", "s0", cfg.dec_depths[1])
        out += [(f"{d}.recovery.weight", (D1, c, ph, pw)), (f"{d}.recovery.bias", (c,))]
    return out


def shape_source(name: str) -> str:
    """The FengwuConfig fields a slot's shape follows from (named in shape errors)."""
    if name.startswith("norm."):
        return "modalities"
    if name.endswith("bias_table"):
        return "bias / window2d / window3d / heads / pad"
    if "embed.weight" in name or "recovery" in name:
        return "dims / modalities / patch"
    if "mlp" in name:
        return "dims / mlp_ratio"
    return "dims"


def full_param_spec(cfg: FengwuConfig) -> list[tuple]:
    return [("norm.mean", (cfg.channels,)), ("norm.std", (cfg.channels,))] + param_spec(cfg)


def n_parameters(cfg: FengwuConfig) -> int:
    return sum(int(np.prod(s)) for _, s in param_spec(cfg))


def n_launches(cfg: FengwuConfig) -> int:
    """Kernel launches of one call: embed, its LayerNorm, 7 per Swin block (LN, QKV, attention, proj + residual, LN, fc1 + GELU,
    fc2 + residual), merge gather + LN and its linear, expand and the skip linear, recovery."""
    return 7 + 7 * (sum(cfg.enc_depths) + cfg.fuser_depth + sum(cfg.dec_depths))


def flops_per_call(cfg: FengwuConfig) -> float:
    """Multiply-adds x 2 of one call: every GEMM at its true K / N (no zero padding) and the attention products over the padded
    windows."""
    D1, D2 = cfg.dims
    (h1, w1), (h2, w2) = cfg.grid1, cfg.grid2
    t1, t2 = h1 * w1, h2 * w2
    pp = cfg.patch[0] * cfg.patch[1]

    def blocks(where, n, batch):
        g, win, D, _ = block_geometry(cfg, where)
        tp, N = g[0] * g[1] * g[2], win[0] * win[1] * win[2]
        t = t1 if where == "s0" else t2
        if where == "fuser":
            t = cfg.n_mod * t2
        return n * batch * (t * D * (4 * D + 2 * cfg.mlp_ratio * D) + 2 * tp * N * D)

    f = sum(t1 * D1 * 2 * c * pp + t1 * D1 * c * pp for _, c in cfg.modalities)            # embeddings, recoveries
    f += cfg.n_mod * (t2 * 4 * D1 * D2 + t2 * D2 * 4 * D1 + t1 * 2 * D1 * D1)              # merge, expand, skip
    f += blocks("s0", sum(cfg.enc_depths[:1]) + cfg.dec_depths[1], cfg.n_mod) + blocks("s1", cfg.enc_depths[1] + cfg.dec_depths[0], cfg.n_mod)
    f += blocks("fuser", cfg.fuser_depth, 1)
    return 2.0 * f


def channel_stats(cfg: FengwuConfig):
    if cfg.channels == len(CHANNELS):
        st = _STATS
    else:
        st = [_STATS[(13 * c) % len(_STATS)] for c in range(cfg.channels)]
    return torch.tensor([s[0] for s in st], dtype=torch.float64), torch.tensor([s[1] for s in st], dtype=torch.float64)


def _init(name: str, shape: tuple, gen: torch.Generator, device) -> torch.Tensor:
    """Seeded stand-in values of magnitudes a trained network has (weights ~ 1 / sqrt(fan_in), pre-norm gains ~ 1, bias tables ~ 0.5)."""
    rnd = lambda s=1.0: torch.randn(shape, generator=gen, device=device, dtype=torch.float32) * s     # noqa: E731
    if name.endswith("bias_table"):
        return rnd(0.5)
    if "norm" in name and name.endswith(".weight"):
        return 1.0 + rnd(0.1)
    if name.endswith("bias"):
        return rnd(0.02)
    fan_in = int(np.prod(shape[1:]))
    if name.endswith("recovery.weight"):
        fan_in = shape[0]
    if name.endswith("fc2.weight") or name.endswith("proj.weight"):
        return rnd(0.5 / math.sqrt(fan_in))                 # residual branches a little smaller: a deep stack stays O(1)
    return rnd(1.0 / math.sqrt(fan_in))


class SyntheticParams(Mapping):
    """The full parameter dict of ``full_param_spec`` as seeded random values, generated when a key is read (each from its own seed,
    so the order of reads does not matter) on ``device``."""

    def __init__(self, cfg: FengwuConfig, seed: int = 0, device="cpu"):
        self.cfg, self.seed, self.device = cfg, seed, torch.device(device)
        self._shapes = dict(full_param_spec(cfg))

    def __getitem__(self, key):
        shape = self._shapes[key]
        if key in ("norm.mean", "norm.std"):
            m, s = channel_stats(self.cfg)
            return (m if key == "norm.mean" else s).float().to(self.device)
        gen = torch.Generator(device=self.device).manual_seed((self.seed * 1000003 + zlib.crc32(key.encode())) & 0x7FFFFFFFFFFF)
        return _init(key, shape, gen, self.device)

    def __iter__(self):
        return iter(self._shapes)

    def __len__(self):
        return len(self._shapes)


def init_synthetic(cfg: FengwuConfig, seed: int = 0, device="cpu") -> SyntheticParams:
    return SyntheticParams(cfg, seed, device)


def latlon_axes(cfg: FengwuConfig):
    lat = 90.0 - (180.0 / (cfg.n_lat - 1)) * np.arange(cfg.n_lat)
    lon = (360.0 / cfg.n_lon) * np.arange(cfg.n_lon)
    return lat, lon


def synthetic_state(cfg: FengwuConfig, seed: int = 0) -> torch.Tensor:
    """(channels, n_lat, n_lon) fp32 state of ERA5 magnitudes per channel: center + scale * smooth noise (q kept non-negative)."""
    gen = torch.Generator().manual_seed(seed + 7919)
    lat, lon = latlon_axes(cfg)
    la = torch.from_numpy(np.radians(lat))[:, None]
    lo = torch.from_numpy(np.radians(lon))[None, :]
    center, scale = channel_stats(cfg)
    out = torch.empty(cfg.channels, cfg.n_lat, cfg.n_lon, dtype=torch.float32)
    for c in range(cfg.channels):
        a = torch.randn(4, generator=gen, dtype=torch.float64)
        k = torch.randint(1, 5, (2,), generator=gen)
        f = (a[0] * torch.cos(la) * torch.sin(k[0] * lo + a[1]) + a[2] * torch.sin(2 * la + a[3]) * torch.cos(k[1] * lo)) * 0.6
        v = center[c] + scale[c] * f
        if cfg.channels == len(CHANNELS) and CHANNELS[c].startswith("q"):
            v = v.abs()
        out[c] = v.float()
    return out.contiguous()
