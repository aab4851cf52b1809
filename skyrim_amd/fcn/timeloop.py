"""The object ``FourcastnetModel.build_model()`` returns: earth2mip's TimeLoop protocol (the reference's
skyrim/core/models/fourcastnet.py:24-25, consumed by models/utils.py) on the HIP AFNO engine.

    loop(time, x) -> iterator of (time, state (B=1, 26, 720, 1440) on .device, restart);  first yield = the input state.

``params``: state dict keyed by ``spec.param_spec``; default: ``SKYRIM_FCN_WEIGHTS`` (a torch file of that dict, or earth2mip's package
directory), or seeded random parameters only with ``SKYRIM_SYNTHETIC_WEIGHTS=1`` (weights.resolve).
"""
from __future__ import annotations

import numpy as np

from ..timeloop import SpecTimeLoop
from . import spec as _spec
from .engine import FcnEngine


class FcnTimeLoop(SpecTimeLoop):
    engine_class, config_class, spec = FcnEngine, _spec.FcnConfig, _spec
    weights_env, label = "SKYRIM_FCN_WEIGHTS", "fourcastnet"

    def widths(self, cfg):
        return cfg.in_chans, cfg.out_chans

    def axes(self, cfg):
        step = 180.0 / (cfg.n_lat if cfg.n_lat % 2 == 0 else cfg.n_lat - 1)
        # 90, 89.75, ..., -89.75 at full size: no south-pole row
        return 90.0 - step * np.arange(cfg.n_lat), np.arange(cfg.n_lon) * (360.0 / cfg.n_lon)
