"""The object ``DLWPModel.build_model()`` returns: earth2mip's TimeLoop protocol (the reference's skyrim/core/models/dlwp.py:25,
consumed by models/utils.py) on the HIP DLWP engine.

    loop(time, x) -> iterator of (time, state (B=1, 7, 721, 1440) on .device, restart);  x: (1, 2, 7, 721, 1440) = states at
    time - 6 h and time.  First yield = the input's newest level; each later yield is the t + 12 h output of one network call, whose
    t + 6 h output stays on the GPU as the next call's older level.
"""
from __future__ import annotations

import datetime
import os

import torch

from .. import weights
from ..timeloop import EngineTimeLoop, Grid
from .engine import DlwpEngine
from .spec import CHANNELS, DlwpConfig, init_synthetic, latlon_axes, synthetic_state


class DlwpTimeLoop(EngineTimeLoop):
    n_history_levels = 2
    history_time_step = datetime.timedelta(hours=6)
    time_step = datetime.timedelta(hours=12)

    def __init__(self, params: dict | None = None, cfg: DlwpConfig | None = None, device: str | torch.device = "cuda:0", seed: int = 0):
        """``params``: dict keyed by ``spec.param_spec`` plus the two maps; default: ``SKYRIM_DLWP_WEIGHTS`` (a torch file of that dict,
        or earth2mip's package directory), or seeded random parameters only with ``SKYRIM_SYNTHETIC_WEIGHTS=1`` (weights.resolve)."""
        self.cfg = cfg or DlwpConfig()
        self.engine = DlwpEngine(self.cfg, device)
        if params is None:
            params = weights.resolve("SKYRIM_DLWP_WEIGHTS", self._load, lambda: init_synthetic(self.cfg, seed), "dlwp")
        self.engine.load_params(params)
        self.channel_std = torch.as_tensor(params["scale"]).float().reshape(-1)       # DLWP's own scaling constants: the scale of a perturbed ensemble member
        self._channels(CHANNELS, self.cfg.channels)
        lat, lon = latlon_axes(self.cfg)
        self.grid = Grid(list(lat), list(lon))
        self.guard = weights.FiniteGuard("the DLWP network produced non-finite values")
        self._history = None                    # (yielded tensor, [older level, newer level]) of the last yield

    def _load(self, path: str) -> dict:
        if os.path.isdir(path):
            from . import checkpoint
            return checkpoint.load_package(path, self.cfg)
        return torch.load(path, map_location="cpu")

    def synthetic_state(self, seed: int) -> torch.Tensor:
        """Initial-condition hook of the synthetic DataSource."""
        return synthetic_state(self.cfg, seed)

    def history_for(self, state):
        """The two levels (t - 6 h, t), each (1, C, lat, lon), that continue the loop from ``state`` -- the object this loop yielded last --
        or None.  The yielded states are 12 h apart, so the last two of them are not a valid input (models/utils.py ResidentState)."""
        if self._history is not None and self._history[0] is state:
            return list(self._history[1])
        return None

    def take_pending_check(self):
        """(flag, step, hint) of the last yielded state's deferred finite check, handed to the caller (models/utils.py)."""
        p = self.guard.take()
        return None if p is None else (p[0], p[1], self.guard.hint)

    def _yield(self, time, older, newer, step, restart, guard):
        out = newer.unsqueeze(0)
        self._history = (out, [older.unsqueeze(0), out])
        if step > 0:
            guard.push(newer, step)
        return time, out, restart

    def __call__(self, time: datetime.datetime, x: torch.Tensor, restart=None):
        shape = (1, 2) + self.engine.state_shape
        if x.dim() != 5 or tuple(x.shape) != shape:
            raise ValueError(f"expected x of shape {shape} (states at time - 6 h and time), got {tuple(x.shape)}")
        x = x.to(self.device, torch.float32)
        older, newer = x[0, 0].contiguous().clone(), x[0, 1].contiguous().clone()
        # the deferred check belongs to THIS generator (several may be open at once: skyrim_amd/ensemble.py interleaves one per member);
        # ``self.guard`` names the one opened last, which is the one take_pending_check's caller is draining
        guard = self.guard = weights.FiniteGuard(self.guard.hint)
        step = 0
        try:
            yield self._yield(time, older, newer, step, restart, guard)
            while True:
                older, newer = self.engine.call(older, newer, time)
                time = time + self.time_step
                step += 1
                yield self._yield(time, older, newer, step, restart, guard)
        finally:
            guard.check()
