"""DLWPModel wrapper -- the reference's skyrim/core/models/dlwp.py, with ``build_model`` returning the HIP DLWP TimeLoop instead of
``dlwp.load(registry.get_model("e2mip://dlwp"))``."""
from __future__ import annotations

import datetime

from ...dlwp.spec import CHANNELS  # noqa: F401  (the reference's dlwp.py:16-17 channel list)
from .base import GlobalModel


class DLWPModel(GlobalModel):
    """
    n_history_levels: int = 2  (states at t - 6 h and t; one step = 12 h)
    grid.lat: list of length 721, [90, 89.75, 89.50, ..., -89.75, -90]
    grid.lon: list of length 1440, [0.0, 0.25, ..., 359.75]
    in_channel_names / out_channel_names: list of length 7, ['t850', 'z1000', 'z700', 'z500', 'z300', 'tcwv', 't2m']
    """

    model_name = "dlwp"
    model_time_step = datetime.timedelta(hours=12)      # known before the model is built (GlobalEnsemble compares its members')

    def __init__(self, *args, cfg=None, device="cuda:0", params=None, **kwargs):
        # extras beyond the reference's signature (all optional): network configuration, device, parameter dict
        self._engine_kw = dict(cfg=cfg, device=device, params=params)
        super().__init__(self.model_name, *args, **kwargs)

    def build_model(self):
        from ...dlwp.timeloop import DlwpTimeLoop
        return DlwpTimeLoop(**self._engine_kw)

    @property
    def device(self):
        return self.model.device

    @property
    def time_step(self):
        return self.model.time_step

    @property
    def in_channel_names(self):
        return self.model.in_channel_names

    @property
    def out_channel_names(self):
        return self.model.out_channel_names
