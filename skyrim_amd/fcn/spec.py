"""Shapes, parameter layout and synthetic inputs of the FourCastNet v1 (AFNO) step.

The network is the published ``AFNONet`` as earth2mip's ``fcn.load`` wraps it (the reference's skyrim/core/models/fourcastnet.py:24-25):
patch embedding (8 x 8, stride 8) + position embedding, ``depth`` AFNO blocks (LayerNorm -> 2-D Fourier filter with a block-diagonal
complex MLP -> double skip -> LayerNorm -> MLP), a linear head and the (p1 p2 c) -> (c, h p1, w p2) rearrangement.  Parameter slots
are keyed by the published module names (checkpoint.py maps an archive onto them).
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import torch

from ..sfno import spec as sfno_spec

# channel order of the reference wrapper (fourcastnet.py:8-10)
CHANNELS = ["u10m", "v10m", "t2m", "sp", "msl", "t850", "u1000", "v1000", "z1000", "u850",
            "v850", "z850", "u500", "v500", "z500", "t500", "z50", "r500", "r850", "tcwv",
            "u100m", "v100m", "u250", "v250", "z250", "t250"]


@dataclass(frozen=True)
class FcnConfig:
    n_lat: int = 720                        # 90 .. -89.75: no south-pole row
    n_lon: int = 1440
    in_chans: int = 26
    out_chans: int = 26
    patch: int = 8
    embed_dim: int = 768
    depth: int = 12
    num_blocks: int = 8
    mlp_ratio: float = 4.0
    sparsity_threshold: float = 0.01        # softshrink lambda
    hard_thresholding_fraction: float = 1.0
    kept_lon_modes: int | None = None       # default int((h // 2 + 1) * hard_thresholding_fraction); see DESIGN.md 13, note 1
    eps: float = 1e-6                       # both LayerNorms

    @property
    def h(self):                            # token grid
        return self.n_lat // self.patch

    @property
    def w(self):
        return self.n_lon // self.patch

    @property
    def tokens(self):
        return self.h * self.w

    @property
    def km(self):
        if self.kept_lon_modes is not None:
            return self.kept_lon_modes
        return int((self.h // 2 + 1) * self.hard_thresholding_fraction)

    @property
    def block_size(self):
        return self.embed_dim // self.num_blocks

    @property
    def hidden(self):
        return int(self.embed_dim * self.mlp_ratio)


def param_spec(cfg: FcnConfig) -> list[tuple[str, tuple]]:
    e, p, nb, bs, hid = cfg.embed_dim, cfg.patch, cfg.num_blocks, cfg.block_size, cfg.hidden
    spec = [("norm.mean", (cfg.in_chans,)), ("norm.std", (cfg.in_chans,)),
            ("patch_embed.proj.weight", (e, cfg.in_chans, p, p)), ("patch_embed.proj.bias", (e,)),
            ("pos_embed", (1, cfg.tokens, e))]
    for i in range(cfg.depth):
        b = f"blocks.{i}."
        spec += [(b + "norm1.weight", (e,)), (b + "norm1.bias", (e,)),
                 (b + "filter.w1", (2, nb, bs, bs)), (b + "filter.b1", (2, nb, bs)),
                 (b + "filter.w2", (2, nb, bs, bs)), (b + "filter.b2", (2, nb, bs)),
                 (b + "norm2.weight", (e,)), (b + "norm2.bias", (e,)),
                 (b + "mlp.fc1.weight", (hid, e)), (b + "mlp.fc1.bias", (hid,)),
                 (b + "mlp.fc2.weight", (e, hid)), (b + "mlp.fc2.bias", (e,))]
    spec += [("head.weight", (cfg.out_chans * p * p, e))]
    return spec


def channel_stats(cfg: FcnConfig):
    """Per-channel (mean, std) of the synthetic data: SFNO's magnitudes for the same channel names (all 26 are in its list)."""
    mean, std = sfno_spec.channel_stats(sfno_spec.SfnoConfig())
    if cfg.in_chans == len(CHANNELS):
        idx = torch.tensor([sfno_spec.CHANNELS.index(c) for c in CHANNELS])
    else:
        idx = torch.linspace(0, len(sfno_spec.CHANNELS) - 1, cfg.in_chans).long()
    return mean[idx].clone(), std[idx].clone()


def init_synthetic(cfg: FcnConfig, seed: int = 0) -> dict:
    """Seeded random parameters at the published init scales (trunc-normal 0.02 for linear maps and pos_embed, 0.02 * randn for the
    spectral weights); LayerNorm gamma / beta away from 1 / 0 and small non-zero biases so that every term is exercised."""
    gen = torch.Generator().manual_seed(seed)
    mean, std = channel_stats(cfg)
    out = {}
    for name, shape in param_spec(cfg):
        if name == "norm.mean":
            t = mean
        elif name == "norm.std":
            t = std
        elif name.endswith("norm1.weight") or name.endswith("norm2.weight"):
            t = 1.0 + 0.1 * torch.randn(shape, generator=gen)
        elif name.endswith("norm1.bias") or name.endswith("norm2.bias"):
            t = 0.1 * torch.randn(shape, generator=gen)
        elif name.endswith("filter.w1") or name.endswith("filter.w2"):
            t = 0.02 * torch.randn(shape, generator=gen)
        elif name.endswith("filter.b1") or name.endswith("filter.b2"):
            t = 0.02 * torch.randn(shape, generator=gen)
        elif name == "patch_embed.proj.weight":
            fan_in = shape[1] * shape[2] * shape[3]
            t = torch.randn(shape, generator=gen) * math.sqrt(1.0 / fan_in)
        elif name.endswith(".bias"):
            t = 0.02 * torch.randn(shape, generator=gen)
        else:                                            # pos_embed, fc1, fc2, head
            t = (0.02 * torch.randn(shape, generator=gen)).clamp(-0.04, 0.04)
        out[name] = t.float().contiguous()
    return out


def synthetic_state(cfg: FcnConfig, seed: int = 0) -> torch.Tensor:
    """(in_chans, n_lat, n_lon) fp32 state of ERA5 magnitudes: per-channel mean + std * smooth noise (sfno.spec.synthetic_state)."""
    c = sfno_spec.SfnoConfig(n_lat=cfg.n_lat, n_lon=cfg.n_lon, in_chans=cfg.in_chans, out_chans=cfg.in_chans)
    z = (sfno_spec.synthetic_state(c, seed) - sfno_spec.channel_stats(c)[0][:, None, None]) / sfno_spec.channel_stats(c)[1][:, None, None]
    mean, std = channel_stats(cfg)
    return (mean[:, None, None] + std[:, None, None] * z).float().contiguous()


def flops_per_step(cfg: FcnConfig) -> float:
    """Algorithmic FLOPs of one step as the engine computes it (DFTs as the GEMMs they are)."""
    e, t, p, hid, km = cfg.embed_dim, cfg.tokens, cfg.patch, cfg.hidden, cfg.km
    total = 2.0 * t * e * cfg.in_chans * p * p + 2.0 * t * e * cfg.out_chans * p * p
    dft = 2.0 * e * (cfg.h * cfg.w * 2 * km * 2 + km * (2 * cfg.h) ** 2 * 2)
    spec = 2.0 * cfg.h * km * cfg.num_blocks * 2 * (2 * cfg.block_size) ** 2
    mlp = 2.0 * t * 2 * e * hid
    return total + cfg.depth * (dft + spec + mlp)
