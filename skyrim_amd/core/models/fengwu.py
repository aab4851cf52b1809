"""FengwuModel wrapper -- the reference's skyrim/core/models/fengwu.py, with ``build_model`` returning the HIP FengWu TimeLoop instead of
earth2studio's ``FengWu.load_model(...)``; ``predict``, ``rollout``, saving and ensembles come from the shared GlobalModel (the reference's
FengwuModel runs ``forecast`` only: its rollout raises NotImplementedError)."""
from __future__ import annotations

from ...fengwu.spec import CHANNELS  # noqa: F401  (the reference's fengwu.py channel list)
from .base import EngineModel


class FengwuModel(EngineModel):
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
    timeloop = "fengwu.timeloop:FengwuTimeLoop"
