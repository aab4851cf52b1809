"""The object ``FourcastnetModel.build_model()`` returns: earth2mip's TimeLoop protocol (the reference's
skyrim/core/models/fourcastnet.py:24-25, consumed by models/utils.py) on the HIP AFNO engine.

    loop(time, x) -> iterator of (time, state (B=1, 26, 720, 1440) on .device, restart);  first yield = the input state.
"""
from __future__ import annotations

import datetime
import os
from dataclasses import dataclass

import numpy as np
import torch

from .. import weights
from .engine import FcnEngine
from .spec import CHANNELS, FcnConfig, init_synthetic, synthetic_state


@dataclass
class Grid:
    lat: list
    lon: list

    @property
    def shape(self):
        return (len(self.lat), len(self.lon))


class FcnTimeLoop:
    n_history_levels = 1
    time_step = datetime.timedelta(hours=6)

    def __init__(self, params: dict | None = None, cfg: FcnConfig | None = None, device: str | torch.device = "cuda:0", seed: int = 0):
        """``params``: state dict keyed by ``spec.param_spec``; default: ``SKYRIM_FCN_WEIGHTS`` (a torch file of that dict, or earth2mip's
        package directory), or seeded random parameters only with ``SKYRIM_SYNTHETIC_WEIGHTS=1`` (weights.resolve)."""
        self.cfg = cfg or FcnConfig()
        self.engine = FcnEngine(self.cfg, device)
        if params is None:
            params = weights.resolve("SKYRIM_FCN_WEIGHTS", self._load, lambda: init_synthetic(self.cfg, seed), "fourcastnet")
        self.engine.load_params(params)
        names = CHANNELS if self.cfg.in_chans == len(CHANNELS) else [f"c{i}" for i in range(self.cfg.in_chans)]
        self.in_channel_names = list(names)
        self.out_channel_names = list(names[: self.cfg.out_chans])
        step = 180.0 / (self.cfg.n_lat if self.cfg.n_lat % 2 == 0 else self.cfg.n_lat - 1)
        # 90, 89.75, ..., -89.75 at full size: no south-pole row
        self.grid = Grid(list(90.0 - step * np.arange(self.cfg.n_lat)), list(np.arange(self.cfg.n_lon) * (360.0 / self.cfg.n_lon)))

    def _load(self, path: str) -> dict:
        if os.path.isdir(path):
            from . import checkpoint
            return checkpoint.load_package(path, self.cfg)
        return torch.load(path, map_location="cpu")

    @property
    def device(self):
        return self.engine.device

    def to(self, device):
        if torch.device(device) != self.engine.device:
            raise NotImplementedError("the engine's buffers are bound to one GPU; build a new FcnTimeLoop for another device")
        return self

    def synthetic_state(self, seed: int) -> torch.Tensor:
        """Initial-condition hook of the synthetic DataSource."""
        return synthetic_state(self.cfg, seed)

    def release(self):
        self.engine.release()

    def __call__(self, time: datetime.datetime, x: torch.Tensor, restart=None):
        if x.dim() != 5 or x.shape[0] != 1 or x.shape[1] != 1 or tuple(x.shape[2:]) != self.engine.state_shape:
            raise ValueError(f"expected x of shape (1, 1, {', '.join(map(str, self.engine.state_shape))}), got {tuple(x.shape)}")
        state = x[0, 0].to(self.device, torch.float32).contiguous()
        yield time, state.unsqueeze(0).clone(), restart
        while True:
            state = self.engine.step(state)
            time = time + self.time_step
            yield time, state.unsqueeze(0), restart
