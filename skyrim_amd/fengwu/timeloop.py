"""The object ``FengwuModel.build_model()`` returns: earth2mip's TimeLoop protocol (consumed by models/utils.py) on the HIP FengWu engine.

    loop(time, x) -> iterator of (time, state (B=1, 69, 721, 1440) on .device, restart);  x: (1, 2, 69, 721, 1440) = states at
    time - 6 h and time.  First yield = the input's newest level; each later yield is one network call's t + 6 h state.

A loop continued from its own last output (run_basic_inference's resident state: ``rollout``) keeps counting its steps, so a non-finite
state is reported with the step of the whole rollout; there is no cascade, every step runs the same network.

``params``: mapping keyed by ``spec.full_param_spec``; default: ``SKYRIM_FENGWU_WEIGHTS`` (a directory with one *.onnx graph and the input
affine, or a torch file of that dict), or seeded random parameters only with ``SKYRIM_SYNTHETIC_WEIGHTS=1`` (weights.resolve).
"""
from __future__ import annotations

from ..timeloop import HistoryTimeLoop
from . import spec as _spec
from .engine import FengwuEngine


class FengwuTimeLoop(HistoryTimeLoop):
    engine_class, config_class, spec = FengwuEngine, _spec.FengwuConfig, _spec
    weights_env, label = "SKYRIM_FENGWU_WEIGHTS", "fengwu"
    guard_hint = "the FengWu network produced non-finite values"
    synthetic_on_device = True

    def advance(self, older, newer, time, step):
        return newer, self.engine.call(older, newer)
