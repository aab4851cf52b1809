"""The object ``FourcastnetV2Model.build_model()`` returns: earth2mip's TimeLoop protocol
(/root/reference/skyrim/core/models/fourcastnet_v2.py:24-28, consumed by models/utils.py:10-49) on the HIP SFNO engine.

    loop(time, x) -> iterator of (time, state (B=1, 73, 721, 1440) on .device, restart);  first yield = the input state.

``params``: state dict keyed by ``spec.param_spec``; default: ``SKYRIM_SFNO_WEIGHTS`` = a torch file of that dict or the reference's own
package directory (``checkpoint.load``), or seeded random parameters only with ``SKYRIM_SYNTHETIC_WEIGHTS=1`` -- the e2mip://fcnv2_sm
checkpoint is not obtainable in this environment.
"""
from __future__ import annotations

import numpy as np

from ..timeloop import SpecTimeLoop
from . import spec as _spec
from .engine import SfnoEngine


class SfnoTimeLoop(SpecTimeLoop):
    engine_class, config_class, spec = SfnoEngine, _spec.SfnoConfig, _spec
    weights_env, label = "SKYRIM_SFNO_WEIGHTS", "fourcastnet_v2"

    def widths(self, cfg):
        return cfg.in_chans, cfg.out_chans

    def axes(self, cfg):
        return np.linspace(90.0, -90.0, cfg.n_lat), np.arange(cfg.n_lon) * (360.0 / cfg.n_lon)
