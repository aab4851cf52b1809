"""FourcastnetModel wrapper -- the reference's skyrim/core/models/fourcastnet.py, with ``build_model`` returning the HIP AFNO TimeLoop
instead of ``fcn.load(registry.get_model("e2mip://fcn"))``."""
from __future__ import annotations

from ...fcn.spec import CHANNELS  # noqa: F401  (same list as the reference's fourcastnet.py:8-10)
from .base import EngineModel


class FourcastnetModel(EngineModel):
    """
    NOTE: its grid does not include the south pole
    n_history_levels: int = 1
    grid.lat: list of length 720, [90, 89.75, 89.50, ..., -89.75]
    grid.lon: list of length 1440, [0.0, 0.25, ..., 359.75]
    in_channel_names / out_channel_names: list of length 26, ['u10m', 'v10m', 't2m', 'sp', ..., 't250']
    """

    model_name = "fourcastnet"
    timeloop = "fcn.timeloop:FcnTimeLoop"
