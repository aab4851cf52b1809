"""FengwuModel wrapper -- the reference's skyrim/core/models/fengwu.py, with ``build_model`` returning the HIP FengWu TimeLoop instead of
earth2studio's ``FengWu.load_model(...)``; ``predict``, ``rollout``, saving and ensembles come from the shared GlobalModel (the reference's
FengwuModel runs ``forecast`` only: its rollout raises NotImplementedError)."""
from __future__ import annotations

import datetime

from ...fengwu.spec import CHANNELS  # noqa: F401  (the reference's fengwu.py channel list)
from .base import GlobalModel


class FengwuModel(GlobalModel):
    """
    From:
    https://github.com/NVIDIA/earth2studio/blob/68dd00bd76be8abc90badd39d0f51f26294ce526/earth2studio/models/px/fengwu.py#L113-L125

        FengWu (operational) weather model consists of single auto-regressive model with
        a time-step size of 6 hours. FengWu operates on 0.25 degree lat-lon grid (south-pole
        including) equirectangular grid with 69 atmospheric/surface variables. This model
        uses two time-steps as an input.

    - https://arxiv.org/abs/2304.02948
    - https://github.com/OpenEarthLab/FengWu

    n_history_levels: int = 2  (states at t - 6 h and t; one step = 6 h)
    grid.lat: list of length 721, [90, 89.75, 89.50, ..., -89.75, -90]
    grid.lon: list of length 1440, [0.0, 0.25, ..., 359.75]
    in_channel_names / out_channel_names: list of length 69, u10m v10m t2m msl, then z, q, u, v, t at 13 levels
    """

    model_name = "fengwu"

    def __init__(self, *args, cfg=None, device="cuda:0", params=None, **kwargs):
        # extras beyond the reference's signature (all optional): network configuration, device, parameter dict
        self._engine_kw = dict(cfg=cfg, device=device, params=params)
        super().__init__(self.model_name, *args, **kwargs)

    def build_model(self):
        from ...fengwu.timeloop import FengwuTimeLoop
        return FengwuTimeLoop(**self._engine_kw)

    @property
    def device(self):
        return self.model.device

    @property
    def time_step(self):
        return datetime.timedelta(hours=6)

    @property
    def in_channel_names(self):
        return self.model.in_channel_names

    @property
    def out_channel_names(self):
        return self.model.out_channel_names
