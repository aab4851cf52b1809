"""DLWPModel wrapper -- the reference's skyrim/core/models/dlwp.py, with ``build_model`` returning the HIP DLWP TimeLoop instead of
``dlwp.load(registry.get_model("e2mip://dlwp"))``."""
from __future__ import annotations

import datetime

from ...dlwp.spec import CHANNELS  # noqa: F401  (the reference's dlwp.py:16-17 channel list)
from .base import EngineModel


class DLWPModel(EngineModel):
    """
    n_history_levels: int = 2  (states at t - 6 h and t; one step = 12 h)
    grid.lat: list of length 721, [90, 89.75, 89.50, ..., -89.75, -90]
    grid.lon: list of length 1440, [0.0, 0.25, ..., 359.75]
    in_channel_names / out_channel_names: list of length 7, ['t850', 'z1000', 'z700', 'z500', 'z300', 'tcwv', 't2m']
    """

    model_name = "dlwp"
    model_time_step = datetime.timedelta(hours=12)      # known before the model is built (GlobalEnsemble compares its members')
    timeloop = "dlwp.timeloop:DlwpTimeLoop"
