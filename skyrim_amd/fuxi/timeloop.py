"""The object ``FuxiModel.build_model()`` returns: earth2mip's TimeLoop protocol (consumed by models/utils.py) on the HIP FuXi engine.

    loop(time, x) -> iterator of (time, state (B=1, 70, 721, 1440) on .device, restart);  x: (1, 2, 70, 721, 1440) = states at
    time - 6 h and time.  First yield = the input's newest level; each later yield is one network call's t + 6 h state.

The cascade: call k (k = 1 for the first call from the initial condition) runs the parameter set ``stage_for(k)``.  A loop continued
from its own last output (run_basic_inference's resident state: ``rollout``) keeps counting; any other input starts again at step 1.
"""
from __future__ import annotations

import datetime
import os

import torch

from .. import weights
from ..timeloop import EngineTimeLoop, Grid
from .engine import FuxiEngine
from .spec import CHANNELS, FuxiConfig, init_synthetic, latlon_axes, stage_for, synthetic_state


class FuxiTimeLoop(EngineTimeLoop):
    n_history_levels = 2
    time_step = datetime.timedelta(hours=6)

    def __init__(self, params=None, cfg: FuxiConfig | None = None, device: str | torch.device = "cuda:0", seed: int = 0):
        """``params``: mapping keyed by ``spec.full_param_spec``; default: ``SKYRIM_FUXI_WEIGHTS`` (a directory of short / medium /
        long.onnx, or a torch file of that dict), or seeded random parameters only with ``SKYRIM_SYNTHETIC_WEIGHTS=1`` (weights.resolve)."""
        self.cfg = cfg or FuxiConfig()
        self.engine = FuxiEngine(self.cfg, device)
        if params is None:
            params = weights.resolve("SKYRIM_FUXI_WEIGHTS", self._load, lambda: init_synthetic(self.cfg, seed, self.engine.device), "fuxi")
        self.engine.load_params(params)
        self.channel_std = torch.as_tensor(params["norm.std"]).float().reshape(-1)    # the scale of a perturbed ensemble member (skyrim_amd/ensemble.py)
        self._channels(CHANNELS, self.cfg.channels)
        lat, lon = latlon_axes(self.cfg)
        self.grid = Grid(list(lat), list(lon))
        self.guard = weights.FiniteGuard("the FuXi network produced non-finite values")
        self._last = (None, 0)                  # (yielded tensor, its step) of the last yield

    def _load(self, path: str):
        from . import checkpoint
        return checkpoint.load(path, self.cfg)

    def stage_for(self, step: int) -> str:
        """The parameter set of call ``step`` (1-based, counted from the loop's initial condition)."""
        return stage_for(step, self.cfg.cascade_steps)

    def synthetic_state(self, seed: int) -> torch.Tensor:
        """Initial-condition hook of the synthetic DataSource."""
        return synthetic_state(self.cfg, seed)

    def take_pending_check(self):
        """(flag, step, hint) of the last yielded state's deferred finite check, handed to the caller (models/utils.py)."""
        p = self.guard.take()
        return None if p is None else (p[0], p[1], self.guard.hint)

    def _yield(self, time, state, step, restart, guard):
        out = state.unsqueeze(0)
        self._last = (out, step)
        if step > 0:
            guard.push(state, step)
        return time, out, restart

    def __call__(self, time: datetime.datetime, x: torch.Tensor, restart=None):
        shape = (1, 2) + self.engine.state_shape
        if x.dim() != 5 or tuple(x.shape) != shape:
            raise ValueError(f"expected x of shape {shape} (states at time - 6 h and time), got {tuple(x.shape)}")
        own = self.__dict__.pop("_state_is_own_output", False)      # run_basic_inference: x holds this loop's last outputs, still in HBM
        step = self._last[1] if own else 0
        x = x.to(self.device, torch.float32)
        older, newer = x[0, 0].contiguous().clone(), x[0, 1].contiguous().clone()
        # the deferred check belongs to THIS generator (several may be open at once: skyrim_amd/ensemble.py interleaves one per member);
        # ``self.guard`` names the one opened last, which is the one take_pending_check's caller is draining
        guard = self.guard = weights.FiniteGuard(self.guard.hint)
        try:
            yield self._yield(time, newer, step, restart, guard)
            while True:
                step += 1
                older, newer = newer, self.engine.call(older, newer, time, self.stage_for(step))
                time = time + self.time_step
                yield self._yield(time, newer, step, restart, guard)
        finally:
            guard.check()
