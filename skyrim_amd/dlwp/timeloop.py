"""The object ``DLWPModel.build_model()`` returns: earth2mip's TimeLoop protocol (the reference's skyrim/core/models/dlwp.py:25,
consumed by models/utils.py) on the HIP DLWP engine.

    loop(time, x) -> iterator of (time, state (B=1, 7, 721, 1440) on .device, restart);  x: (1, 2, 7, 721, 1440) = states at
    time - 6 h and time.  First yield = the input's newest level; each later yield is the t + 12 h output of one network call, whose
    t + 6 h output stays on the GPU as the next call's older level.

``params``: dict keyed by ``spec.param_spec`` plus the two maps; default: ``SKYRIM_DLWP_WEIGHTS`` (a torch file of that dict, or
earth2mip's package directory), or seeded random parameters only with ``SKYRIM_SYNTHETIC_WEIGHTS=1`` (weights.resolve).
"""
from __future__ import annotations

import datetime

from ..timeloop import HistoryTimeLoop
from . import spec as _spec
from .engine import DlwpEngine


class DlwpTimeLoop(HistoryTimeLoop):
    history_time_step = datetime.timedelta(hours=6)
    time_step = datetime.timedelta(hours=12)
    engine_class, config_class, spec = DlwpEngine, _spec.DlwpConfig, _spec
    weights_env, label = "SKYRIM_DLWP_WEIGHTS", "dlwp"
    std_key = "scale"                       # DLWP's own scaling constants
    guard_hint = "the DLWP network produced non-finite values"
    resumes_step_count = False              # every call counts from 0; the mark is leads.forget_resident's to clear
    _history = None                         # (yielded tensor, [older level, newer level]) of the last yield

    def history_for(self, state):
        """The two levels (t - 6 h, t), each (1, C, lat, lon), that continue the loop from ``state`` -- the object this loop yielded last --
        or None.  The yielded states are 12 h apart, so the last two of them are not a valid input (models/utils.py ResidentState)."""
        if self._history is not None and self._history[0] is state:
            return list(self._history[1])
        return None

    def _yield(self, time, older, newer, step, restart, guard):
        item = super()._yield(time, older, newer, step, restart, guard)
        self._history = (item[1], [older.unsqueeze(0), item[1]])
        return item

    def advance(self, older, newer, time, step):
        return self.engine.call(older, newer, time)
