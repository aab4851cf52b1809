"""FuxiModel wrapper -- the reference's skyrim/core/models/fuxi.py, with ``build_model`` returning the HIP FuXi TimeLoop instead of
earth2studio's ``FuXi.load_model(...)``; ``predict``, ``rollout``, saving and ensembles come from the shared GlobalModel (the reference's
FuxiModel runs ``forecast`` only: its rollout raises NotImplementedError, fuxi.py:120-124)."""
from __future__ import annotations

import datetime

from ...fuxi.spec import CHANNELS  # noqa: F401  (the reference's fuxi.py:14-22 channel list)
from .base import GlobalModel


class FuxiModel(GlobalModel):
    """
    n_history_levels: int = 2  (states at t - 6 h and t; one step = 6 h)
    grid.lat: list of length 721, [90, 89.75, 89.50, ..., -89.75, -90]
    grid.lon: list of length 1440, [0.0, 0.25, ..., 359.75]
    in_channel_names / out_channel_names: list of length 70, z, t, u, v, r at 13 levels, then t2m u10m v10m msl tp
    cascade: the short / medium / long networks run steps 1-20 / 21-40 / 41- (FuxiConfig.cascade_steps)
    """

    model_name = "fuxi"

    def __init__(self, *args, cfg=None, device="cuda:0", params=None, **kwargs):
        # extras beyond the reference's signature (all optional): network configuration, device, parameter dict
        self._engine_kw = dict(cfg=cfg, device=device, params=params)
        super().__init__(self.model_name, *args, **kwargs)

    def build_model(self):
        from ...fuxi.timeloop import FuxiTimeLoop
        return FuxiTimeLoop(**self._engine_kw)

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
