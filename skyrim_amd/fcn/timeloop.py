"""The object ``FourcastnetModel.build_model()`` returns: earth2mip's TimeLoop protocol (the reference's
skyrim/core/models/fourcastnet.py:24-25, consumed by models/utils.py) on the HIP AFNO engine.

    loop(time, x) -> iterator of (time, state (B=1, 26, 720, 1440) on .device, restart);  first yield = the input state.
"""
from __future__ import annotations

import os

import numpy as np
import torch

from .. import weights
from ..timeloop import EngineTimeLoop, Grid
from .engine import FcnEngine
from .spec import CHANNELS, FcnConfig, init_synthetic, synthetic_state


class FcnTimeLoop(EngineTimeLoop):
    def __init__(self, params: dict | None = None, cfg: FcnConfig | None = None, device: str | torch.device = "cuda:0", seed: int = 0):
        """``params``: state dict keyed by ``spec.param_spec``; default: ``SKYRIM_FCN_WEIGHTS`` (a torch file of that dict, or earth2mip's
        package directory), or seeded random parameters only with ``SKYRIM_SYNTHETIC_WEIGHTS=1`` (weights.resolve)."""
        self.cfg = cfg or FcnConfig()
        self.engine = FcnEngine(self.cfg, device)
        if params is None:
            params = weights.resolve("SKYRIM_FCN_WEIGHTS", self._load, lambda: init_synthetic(self.cfg, seed), "fourcastnet")
        self.engine.load_params(params)
        self.channel_std = torch.as_tensor(params["norm.std"]).float().reshape(-1)    # the scale of a perturbed ensemble member (skyrim_amd/ensemble.py)
        self._channels(CHANNELS, self.cfg.in_chans, self.cfg.out_chans)
        step = 180.0 / (self.cfg.n_lat if self.cfg.n_lat % 2 == 0 else self.cfg.n_lat - 1)
        # 90, 89.75, ..., -89.75 at full size: no south-pole row
        self.grid = Grid(list(90.0 - step * np.arange(self.cfg.n_lat)), list(np.arange(self.cfg.n_lon) * (360.0 / self.cfg.n_lon)))

    def _load(self, path: str) -> dict:
        if os.path.isdir(path):
            from . import checkpoint
            return checkpoint.load_package(path, self.cfg)
        return torch.load(path, map_location="cpu")

    def synthetic_state(self, seed: int) -> torch.Tensor:
        """Initial-condition hook of the synthetic DataSource."""
        return synthetic_state(self.cfg, seed)
