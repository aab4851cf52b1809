"""Shapes, constants, parameter layout, tables and synthetic inputs of the FuXi call (Swin V2 U-Transformer cascade).

The network is FuXi (arXiv 2306.12873) as earth2studio's ``FuXi`` wraps it (the reference's skyrim/core/models/fuxi.py:53-54): two
70-channel levels (t - 6 h, t) on 721 x 1440 -> cube embedding (Conv3d 2 x 4 x 4) -> down block -> 48 Swin V2 blocks -> up block -> head
-> the state at t + 6 h.  Three parameter sets of identical shapes (short, medium, long) take over at fixed step counts.

Every constant the kernels (csrc/fuxi_ops.hip), the engine and the float64 restatement (tests/_fuxi_reference.py) must agree on is a
field of ``FuxiConfig`` or a function here.  The real ONNX graphs could not be inspected offline; the fields marked UNVERIFIED are the
points DESIGN.md 15 lists, each with where its default came from.
"""
from __future__ import annotations

import datetime
import math
import zlib
from collections.abc import Mapping
from dataclasses import dataclass

import numpy as np
import torch

LEVELS = [50, 100, 150, 200, 250, 300, 400, 500, 600, 700, 850, 925, 1000]
# the reference's order (skyrim/core/models/fuxi.py:14-22): z, t, u, v, r at 13 levels, then the five surface fields
CHANNELS = [f"{v}{p}" for v in ("z", "t", "u", "v", "r") for p in LEVELS] + ["t2m", "u10m", "v10m", "msl", "tp"]
STAGES = ("short", "medium", "long")
# (center, scale) of the synthetic data: ERA5-like magnitudes (geopotential in m^2 s^-2, as FuXi reads it: the reference's fuxi.py:41)
_Z_M = [20600, 16200, 13600, 11800, 10400, 9200, 7200, 5600, 4200, 3000, 1460, 770, 110]
_T_K = [212, 208, 210, 216, 222, 229, 243, 253, 261, 267, 274, 278, 283]
_STATS = ([(9.80665 * z, 9.80665 * (40 + 0.02 * z)) for z in _Z_M] + [(t, 6.0 + 0.02 * (t - 200)) for t in _T_K]
          + [(6.0, 12.0)] * 13 + [(0.0, 7.0)] * 13 + [(55.0, 28.0)] * 13
          + [(278.0, 21.0), (0.0, 5.0), (0.0, 4.5), (101100.0, 1100.0), (0.0, 1e-3)])


@dataclass(frozen=True)
class FuxiConfig:
    n_lat: int = 721                        # 90 .. -90
    n_lon: int = 1440                       # 0 .. 359.75
    channels: int = 70
    embed: int = 1536                       # C
    heads: int = 24                         # head dim C / heads = 64 (the only one compiled)
    depth: int = 48                         # Swin V2 blocks
    patch: tuple = (2, 4, 4)                # cube embedding kernel = stride (levels, lat, lon); the 721st row falls outside the last patch
    # UNVERIFIED: the window (lat, lon) of the Swin blocks.  No source available offline states it; (9, 18) is the shape that tiles the
    # 90 x 180 grid into 10 x 10 windows, an assumption.  The kernel takes the window at run time (any shape that tiles the grid).
    window: tuple = (9, 18)
    # UNVERIFIED: odd blocks shift by half a window and mask as standard Swin does (in latitude AND longitude: True).  False: longitude
    # treated as periodic (no mask across the seam).  Default: Swin V2's reference implementation, which masks both axes.
    shift_mask_lon: bool = True
    mask_value: float = -100.0              # Swin's additive shifted-window mask
    mlp_ratio: int = 4                      # exact-erf GELU between fc1 and fc2
    groups: int = 32                        # GroupNorm groups of the residual blocks
    cpb_hidden: int = 512                   # Swin V2 continuous position bias MLP: Linear(2, 512) -> ReLU -> Linear(512, heads, no bias)
    logit_max: float = math.log(100.0)      # cosine attention scale = exp(min(logit_scale, ln 100)) (Swin V2)
    ln_eps: float = 1e-5
    gn_eps: float = 1e-5
    norm_eps: float = 1e-12                 # F.normalize of q and k
    # UNVERIFIED: the points below are each one named choice; the engine refuses any value it was not built for
    time_embed_at: str = "embed_epilogue"   # Linear(12, C)(time encoding) added with the embedding bias, BEFORE its LayerNorm
    affine_from: str = "params"             # the input affine (norm.mean, norm.std) is a parameter; ONNX graphs that normalise inside
                                            # their graph load as mean 0, std 1 (checkpoint.py)
    conv_padding: str = "zeros"             # 3 x 3 convs of the down / up blocks pad with zeros (torch Conv2d's default)
    skip_from: str = "down_block"           # the up block concatenates [down block output, last Swin block output] (in this order)
    res_order: str = "conv_gn_silu"         # residual block: x + SiLU(GN(conv(SiLU(GN(conv(x))))))
    align_corners: bool = False             # head resample 720 -> 721 rows: F.interpolate(bilinear) with torch's default
    cascade_steps: tuple = (20, 40)         # short for steps 1..20, medium 21..40, long 41.. (earth2studio FuXi wrapper)

    @property
    def head_dim(self):
        return self.embed // self.heads

    @property
    def grid0(self):                        # embedded tokens (lat, lon): 180 x 360
        return (self.n_lat // self.patch[1], self.n_lon // self.patch[2])

    @property
    def grid1(self):                        # Swin tokens after the stride-2 conv: 90 x 180
        h, w = self.grid0
        return ((h - 1) // 2 + 1, (w - 1) // 2 + 1)

    @property
    def k_embed(self):                      # 70 * 2 * 4 * 4 = 2240
        return self.channels * self.patch[0] * self.patch[1] * self.patch[2]

    @property
    def n_out(self):                        # head outputs per token: 70 * 4 * 4
        return self.channels * self.patch[1] * self.patch[2]

    @property
    def hidden(self):
        return self.mlp_ratio * self.embed


def check_config(cfg: FuxiConfig):
    """The shapes this build runs; ValueError otherwise (the kernels refuse the same shapes with an argument error)."""
    wh, ww = cfg.window
    h1, w1 = cfg.grid1
    h0, w0 = cfg.grid0
    if cfg.embed % cfg.heads or cfg.head_dim != 64:
        raise ValueError(f"head dim {cfg.embed} / {cfg.heads} is not 64 (the only one compiled)")
    if cfg.embed % 8 or cfg.embed > 1536 or cfg.embed % cfg.groups or cfg.patch[0] != 2:
        raise ValueError(f"embed {cfg.embed} must be a multiple of 8 and of {cfg.groups} groups, at most 1536; two levels")
    if h0 % 2 or w0 % 2:
        raise ValueError(f"embedded grid {h0} x {w0} must be even (the 2 x 2 transposed conv restores it)")
    if wh < 2 or ww < 2 or h1 % wh or w1 % ww:
        raise ValueError(f"window {cfg.window} does not tile the {h1} x {w1} token grid")
    fixed = dict(time_embed_at="embed_epilogue", affine_from="params", conv_padding="zeros", skip_from="down_block", res_order="conv_gn_silu")
    for k, v in fixed.items():
        if getattr(cfg, k) != v:
            raise ValueError(f"{k} = {getattr(cfg, k)!r}: this build runs {v!r} only")


def shift(cfg: FuxiConfig, block: int) -> tuple:
    """The cyclic shift (lat, lon) of Swin block ``block``: half a window on odd blocks."""
    return (cfg.window[0] // 2, cfg.window[1] // 2) if block % 2 else (0, 0)


def stage_for(step: int, cascade_steps=(20, 40)) -> str:
    """The parameter set that computes step ``step`` (1 = the first call from the initial condition)."""
    if step < 1:
        raise ValueError(f"step {step}: steps count from 1")
    return STAGES[0] if step <= cascade_steps[0] else (STAGES[1] if step <= cascade_steps[1] else STAGES[2])


def time_encoding(time: datetime.datetime) -> np.ndarray:
    """The 12 values of a call whose newest input level is at ``time``: for t - 6 h, t, t + 6 h the pair (day_of_year / 366, hour / 24),
    then [sin d, sin h, cos d, cos h] per time (the FuXi release's ``time_encoding``: sin / cos of the fractions themselves), float64."""
    out = []
    for h in (-6, 0, 6):
        t = time + datetime.timedelta(hours=h)
        d, hr = t.timetuple().tm_yday / 366.0, t.hour / 24.0
        out += [math.sin(d), math.sin(hr), math.cos(d), math.cos(hr)]
    return np.asarray(out, dtype=np.float64)


# ---- Swin V2 tables ------------------------------------------------------------------------------------------------------------- #
def relative_coords(window) -> torch.Tensor:
    """[(2 wh - 1)(2 ww - 1)][2] float64: Swin V2's log-spaced relative coordinates (pretrained window = window)."""
    wh, ww = window
    dy = torch.arange(-(wh - 1), wh, dtype=torch.float64) / (wh - 1) * 8
    dx = torch.arange(-(ww - 1), ww, dtype=torch.float64) / (ww - 1) * 8
    t = torch.stack(torch.meshgrid(dy, dx, indexing="ij"), -1).reshape(-1, 2)
    return torch.sign(t) * torch.log2(t.abs() + 1.0) / math.log2(8)


def cpb_table(window, w0, b0, w2) -> torch.Tensor:
    """[heads][(2 wh - 1)(2 ww - 1)] float64: 16 sigmoid(cpb_mlp(relative coords)); entry (dy + wh - 1)(2 ww - 1) + dx + ww - 1 is the
    bias of a query dy rows and dx columns from its key.  Independent of the input: computed once at load time."""
    t = relative_coords(window)
    h = torch.relu(t @ w0.double().T + b0.double())
    return (16.0 * torch.sigmoid(h @ w2.double().T)).T.contiguous()


def window_region(i: int, n: int, win: int, sh: int) -> int:
    """Swin's mask region of shifted-grid coordinate i (0: [0, n - win), 1: [n - win, n - sh), 2: [n - sh, n)); 0 without a shift."""
    if sh == 0:
        return 0
    return 0 if i < n - win else (1 if i < n - sh else 2)


def shift_mask(cfg: FuxiConfig, grid, sh: int, sw: int) -> torch.Tensor:
    """[nW][N][N] bool: True where the query and key of a shifted window sit in different regions (their score gets ``mask_value``)."""
    H, W = grid
    wh, ww = cfg.window
    ys = torch.arange(H)
    xs = torch.arange(W)
    ry = torch.tensor([window_region(int(i), H, wh, sh) for i in ys])
    rx = torch.tensor([window_region(int(i), W, ww, sw if cfg.shift_mask_lon else 0) for i in xs])
    reg = (3 * ry[:, None] + rx[None, :])                                   # [H][W]
    reg = reg.reshape(H // wh, wh, W // ww, ww).permute(0, 2, 1, 3).reshape(-1, wh * ww)
    return reg[:, :, None] != reg[:, None, :]


# ---- parameters ------------------------------------------------------------------------------------------------------------------ #
def param_spec(cfg: FuxiConfig) -> list[tuple]:
    """(name, shape) of one stage's parameters in order of use, torch shapes (Linear [out, in], Conv [out, in, ...], ConvTranspose2d
    [in, out, kh, kw]).  A full parameter dict keys them as ``<stage>.<name>`` and adds the shared ``norm.mean`` / ``norm.std``."""
    C, H, G = cfg.embed, cfg.heads, cfg.n_out
    out = [("embed.weight", (C, cfg.channels) + tuple(cfg.patch)), ("embed.bias", (C,)), ("time_embed.weight", (C, 12)), ("time_embed.bias", (C,)),
           ("embed_norm.weight", (C,)), ("embed_norm.bias", (C,)), ("down.conv.weight", (C, C, 3, 3)), ("down.conv.bias", (C,))]

    def res(prefix):
        r = []
        for j in range(2):
            r += [(f"{prefix}.res.{j}.conv.weight", (C, C, 3, 3)), (f"{prefix}.res.{j}.conv.bias", (C,)),
                  (f"{prefix}.res.{j}.norm.weight", (C,)), (f"{prefix}.res.{j}.norm.bias", (C,))]
        return r

    out += res("down")
    for i in range(cfg.depth):
        b = f"blocks.{i}"
        out += [(f"{b}.attn.logit_scale", (H, 1, 1)), (f"{b}.attn.cpb_mlp.0.weight", (cfg.cpb_hidden, 2)), (f"{b}.attn.cpb_mlp.0.bias", (cfg.cpb_hidden,)),
                (f"{b}.attn.cpb_mlp.2.weight", (H, cfg.cpb_hidden)), (f"{b}.attn.qkv.weight", (3 * C, C)), (f"{b}.attn.q_bias", (C,)),
                (f"{b}.attn.v_bias", (C,)), (f"{b}.attn.proj.weight", (C, C)), (f"{b}.attn.proj.bias", (C,)), (f"{b}.norm1.weight", (C,)),
                (f"{b}.norm1.bias", (C,)), (f"{b}.mlp.fc1.weight", (cfg.hidden, C)), (f"{b}.mlp.fc1.bias", (cfg.hidden,)),
                (f"{b}.mlp.fc2.weight", (C, cfg.hidden)), (f"{b}.mlp.fc2.bias", (C,)), (f"{b}.norm2.weight", (C,)), (f"{b}.norm2.bias", (C,))]
    out += [("up.conv.weight", (2 * C, C, 2, 2)), ("up.conv.bias", (C,))]
    out += res("up")
    out += [("head.weight", (G, C)), ("head.bias", (G,))]
    return out


def full_param_spec(cfg: FuxiConfig) -> list[tuple]:
    return [("norm.mean", (cfg.channels,)), ("norm.std", (cfg.channels,))] + [(f"{s}.{n}", sh) for s in STAGES for n, sh in param_spec(cfg)]


def n_parameters(cfg: FuxiConfig) -> int:
    return sum(int(np.prod(s)) for _, s in param_spec(cfg))


def flops_per_call(cfg: FuxiConfig) -> float:
    """Multiply-adds x 2 of one call (every GEMM and the attention products)."""
    C = cfg.embed
    h0, w0 = cfg.grid0
    h1, w1 = cfg.grid1
    t0, t1 = h0 * w0, h1 * w1
    n = cfg.window[0] * cfg.window[1]
    f = t0 * C * cfg.k_embed + t1 * C * 9 * C * 3                                   # embedding; down conv + 2 residual convs
    f += cfg.depth * (t1 * C * (3 * C + C + 2 * cfg.hidden) + 2 * t1 * n * C)       # Swin linears + QK^T, PV
    f += t1 * 2 * C * 4 * C + 2 * t0 * 9 * C * C + t0 * C * cfg.n_out               # transposed conv, 2 residual convs, head
    return 2.0 * f


def channel_stats(cfg: FuxiConfig):
    if cfg.channels == len(CHANNELS):
        st = _STATS
    else:
        st = [_STATS[(13 * c) % len(_STATS)] for c in range(cfg.channels)]
    return torch.tensor([s[0] for s in st], dtype=torch.float64), torch.tensor([s[1] for s in st], dtype=torch.float64)


def _init(name: str, shape: tuple, gen: torch.Generator, device) -> torch.Tensor:
    """Seeded stand-in values of magnitudes a trained network has (weights ~ 1 / sqrt(fan_in); res-post-norm gains small)."""
    rnd = lambda s=1.0: torch.randn(shape, generator=gen, device=device, dtype=torch.float32) * s     # noqa: E731
    if name.endswith("logit_scale"):
        return math.log(10.0) + rnd(0.3)
    if "cpb_mlp.0.weight" in name:
        return rnd(0.5)
    if "cpb_mlp.0.bias" in name:
        return rnd(0.1)
    if "cpb_mlp.2" in name:
        return rnd(0.05)
    if name.endswith("norm1.weight") or name.endswith("norm2.weight"):
        return 0.2 + rnd(0.02)
    if "norm" in name and name.endswith(".weight"):
        return 1.0 + rnd(0.1)
    if name.endswith("bias"):
        return rnd(0.02)
    fan_in = int(np.prod(shape[1:]))
    if name == "up.conv.weight" or name.endswith(".up.conv.weight"):
        fan_in = shape[0]
    return rnd(1.0 / math.sqrt(fan_in))


class SyntheticParams(Mapping):
    """The full parameter dict of ``full_param_spec`` as seeded random values, generated when a key is read (each from its own
    seed, so the order of reads does not matter) on ``device``: a full-size cascade (3 x 1.4 G values) is never held twice."""

    def __init__(self, cfg: FuxiConfig, seed: int = 0, device="cpu"):
        self.cfg, self.seed, self.device = cfg, seed, torch.device(device)
        self._shapes = dict(full_param_spec(cfg))

    def __getitem__(self, key):
        shape = self._shapes[key]
        if key in ("norm.mean", "norm.std"):
            m, s = channel_stats(self.cfg)
            return (m if key == "norm.mean" else s).float().to(self.device)
        gen = torch.Generator(device=self.device).manual_seed((self.seed * 1000003 + zlib.crc32(key.encode())) & 0x7FFFFFFFFFFF)
        return _init(key.split(".", 1)[1], shape, gen, self.device)

    def __iter__(self):
        return iter(self._shapes)

    def __len__(self):
        return len(self._shapes)


def init_synthetic(cfg: FuxiConfig, seed: int = 0, device="cpu") -> SyntheticParams:
    return SyntheticParams(cfg, seed, device)


def latlon_axes(cfg: FuxiConfig):
    lat = 90.0 - (180.0 / (cfg.n_lat - 1)) * np.arange(cfg.n_lat)
    lon = (360.0 / cfg.n_lon) * np.arange(cfg.n_lon)
    return lat, lon


def synthetic_state(cfg: FuxiConfig, seed: int = 0) -> torch.Tensor:
    """(channels, n_lat, n_lon) fp32 state of ERA5 magnitudes per channel: center + scale * smooth noise (tp kept non-negative)."""
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
        if cfg.channels == len(CHANNELS) and CHANNELS[c] == "tp":
            v = v.abs()
        out[c] = v.float()
    return out.contiguous()
