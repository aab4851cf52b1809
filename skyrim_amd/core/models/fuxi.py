"""FuxiModel wrapper -- the reference's skyrim/core/models/fuxi.py, with ``build_model`` returning the HIP FuXi TimeLoop instead of
earth2studio's ``FuXi.load_model(...)``; ``predict``, ``rollout``, saving and ensembles come from the shared GlobalModel (the reference's
FuxiModel runs ``forecast`` only: its rollout raises NotImplementedError, fuxi.py:120-124)."""
from __future__ import annotations

from ...fuxi.spec import CHANNELS  # noqa: F401  (the reference's fuxi.py:14-22 channel list)
from .base import EngineModel


class FuxiModel(EngineModel):
    """
    n_history_levels: int = 2  (states at t - 6 h and t; one step = 6 h)
    grid.lat: list of length 721, [90, 89.75, 89.50, ..., -89.75, -90]
    grid.lon: list of length 1440, [0.0, 0.25, ..., 359.75]
    in_channel_names / out_channel_names: list of length 70, z, t, u, v, r at 13 levels, then t2m u10m v10m msl tp
    cascade: the short / medium / long networks run steps 1-20 / 21-40 / 41- (FuxiConfig.cascade_steps)
    """

    model_name = "fuxi"
    timeloop = "fuxi.timeloop:FuxiTimeLoop"
