"""FourcastnetV2Model wrapper -- /root/reference/skyrim/core/models/fourcastnet_v2.py, with ``build_model`` returning
the HIP SFNO TimeLoop instead of ``fcnv2_sm.load(registry.get_model("e2mip://fcnv2_sm"))``."""
from __future__ import annotations

from ...sfno.spec import CHANNELS  # noqa: F401  (same list as the reference's fourcastnet_v2.py:12-21)
from .base import EngineModel


class FourcastnetV2Model(EngineModel):
    """
    n_history_levels: int = 1
    grid.lat: list of length 721, [90, 89.75, 89.50, ..., -89.75, -90]
    grid.lon: list of length 1440, [0.0, 0.25, ..., 359.75]
    in_channel_names / out_channel_names: list of length 73, ['u10m', 'v10m', 'u100m', 'v100m', ..., 'r1000']
    """

    model_name = "fourcastnet_v2"
    timeloop = "sfno.timeloop:SfnoTimeLoop"
