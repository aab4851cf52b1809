"""FourcastnetModel wrapper -- the reference's skyrim/core/models/fourcastnet.py, with ``build_model`` returning the HIP AFNO TimeLoop
instead of ``fcn.load(registry.get_model("e2mip://fcn"))``."""
from __future__ import annotations

from ...fcn.spec import CHANNELS  # noqa: F401  (same list as the reference's fourcastnet.py:8-10)
from .base import GlobalModel


class FourcastnetModel(GlobalModel):
    """
    NOTE: its grid does not include the south pole
    n_history_levels: int = 1
    grid.lat: list of length 720, [90, 89.75, 89.50, ..., -89.75]
    grid.lon: list of length 1440, [0.0, 0.25, ..., 359.75]
    in_channel_names / out_channel_names: list of length 26, ['u10m', 'v10m', 't2m', 'sp', ..., 't250']
    """

    model_name = "fourcastnet"

    def __init__(self, *args, cfg=None, device="cuda:0", params=None, **kwargs):
        # extras beyond the reference's signature (all optional): network configuration, device, parameter dict
        self._engine_kw = dict(cfg=cfg, device=device, params=params)
        super().__init__(self.model_name, *args, **kwargs)

    def build_model(self):
        from ...fcn.timeloop import FcnTimeLoop
        return FcnTimeLoop(**self._engine_kw)

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
