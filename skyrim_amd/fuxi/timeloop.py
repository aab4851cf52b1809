"""The object ``FuxiModel.build_model()`` returns: earth2mip's TimeLoop protocol (consumed by models/utils.py) on the HIP FuXi engine.

    loop(time, x) -> iterator of (time, state (B=1, 70, 721, 1440) on .device, restart);  x: (1, 2, 70, 721, 1440) = states at
    time - 6 h and time.  First yield = the input's newest level; each later yield is one network call's t + 6 h state.

The cascade: call k (k = 1 for the first call from the initial condition) runs the parameter set ``stage_for(k)``.  A loop continued
from its own last output (run_basic_inference's resident state: ``rollout``) keeps counting; any other input starts again at step 1.

``params``: mapping keyed by ``spec.full_param_spec``; default: ``SKYRIM_FUXI_WEIGHTS`` (a directory of short / medium / long.onnx, or a
torch file of that dict), or seeded random parameters only with ``SKYRIM_SYNTHETIC_WEIGHTS=1`` (weights.resolve).
"""
from __future__ import annotations

from ..timeloop import HistoryTimeLoop
from . import spec as _spec
from .engine import FuxiEngine


class FuxiTimeLoop(HistoryTimeLoop):
    engine_class, config_class, spec = FuxiEngine, _spec.FuxiConfig, _spec
    weights_env, label = "SKYRIM_FUXI_WEIGHTS", "fuxi"
    guard_hint = "the FuXi network produced non-finite values"
    synthetic_on_device = True

    def stage_for(self, step: int) -> str:
        """The parameter set of call ``step`` (1-based, counted from the loop's initial condition)."""
        return _spec.stage_for(step, self.cfg.cascade_steps)

    def advance(self, older, newer, time, step):
        return newer, self.engine.call(older, newer, time, self.stage_for(step))
