"""What the engine-backed TimeLoops share (earth2mip's TimeLoop protocol; the reference's skyrim/core/models/*.py build them): the
grid, the device an engine is bound to, the construction around an engine, and the two loops

    EngineTimeLoop    loop(time, x) -> iterator of (time, state (B=1, C, n_lat, n_lon) on .device, restart);  x: (1, 1, C, n_lat, n_lon);
                      first yield = the input state.
    SpecTimeLoop      the same, built from declarations: a model's loop states what differs (the class attributes below).
    HistoryTimeLoop   a SpecTimeLoop over x: (1, 2, C, n_lat, n_lon) = states at time - 6 h and time; first yield = the input's newest
                      level, each later yield one network call's output, with a deferred non-finite check per generator; a model's loop
                      also states how one call advances the pair.
"""
from __future__ import annotations

import datetime
import importlib
from dataclasses import dataclass

import torch

from . import weights


@dataclass
class Grid:
    lat: list
    lon: list

    @property
    def shape(self):
        return (len(self.lat), len(self.lon))


class EngineTimeLoop:
    """A TimeLoop over ``self.engine`` (a HIP engine whose buffers live on one GPU), one history level, 6-h steps."""
    n_history_levels = 1
    time_step = datetime.timedelta(hours=6)

    def _channels(self, names: list, n_in: int, n_out: int | None = None):
        """The model's channel names when its width is theirs, ``c{i}`` otherwise (toy configurations)."""
        names = names if n_in == len(names) else [f"c{i}" for i in range(n_in)]
        self.in_channel_names = list(names)
        self.out_channel_names = list(names[:n_in if n_out is None else n_out])

    @property
    def device(self):
        return self.engine.device

    def to(self, device):
        if torch.device(device) != self.engine.device:
            raise NotImplementedError(f"the engine's buffers are bound to one GPU; build a new {type(self).__name__} for another device")
        return self

    def release(self):
        """Drop every prepared matrix and work buffer of the engine (GlobalModel.release_model)."""
        self.engine.release()

    def __call__(self, time: datetime.datetime, x: torch.Tensor, restart=None):
        if x.dim() != 5 or x.shape[0] != 1 or x.shape[1] != 1 or tuple(x.shape[2:]) != self.engine.state_shape:
            raise ValueError(f"expected x of shape (1, 1, {', '.join(map(str, self.engine.state_shape))}), got {tuple(x.shape)}")
        state = x[0, 0].to(self.device, torch.float32).contiguous()
        yield time, state.unsqueeze(0).clone(), restart
        while True:
            state = self.engine.step(state)                  # new buffer each step: the caller keeps the yielded one
            time = time + self.time_step
            yield time, state.unsqueeze(0), restart


class SpecTimeLoop(EngineTimeLoop):
    """An EngineTimeLoop built from declarations: the one construction sequence of the SFNO, FourCastNet v1, DLWP, FuXi and FengWu loops,
    their weight reader and their synthetic initial condition.  (Pangu's loop and GraphCast's stepper build themselves: calibration and
    conventions, forcings and a stepper state; they stay on EngineTimeLoop.)"""
    engine_class = config_class = None
    spec = None                         # the model's spec module: CHANNELS, init_synthetic, synthetic_state (and latlon_axes for ``axes``)
    weights_env = ""                    # the variable that names a weight file
    label = ""                          # the model's name in weights.resolve's messages
    std_key = "norm.std"                # the parameter that is ``channel_std``
    guard_hint = None                   # the hint of the deferred finite check; None: the loop has none
    synthetic_on_device = False         # ``init_synthetic`` takes the engine's device (lazy parameter sets made where they are used)

    def __init__(self, params=None, cfg=None, device: str | torch.device = "cuda:0", seed: int = 0):
        """``params``: mapping keyed by the model's parameter spec; default: the file or directory ``weights_env`` names (``_load``), or
        seeded random parameters only with ``SKYRIM_SYNTHETIC_WEIGHTS=1`` (weights.resolve)."""
        self.cfg = cfg or self.config_class()
        self.engine = self.engine_class(self.cfg, device)
        if params is None:
            where = (self.engine.device,) if self.synthetic_on_device else ()
            params = weights.resolve(self.weights_env, self._load, lambda: self.spec.init_synthetic(self.cfg, seed, *where), self.label)
        self.engine.load_params(params)
        self.channel_std = torch.as_tensor(params[self.std_key]).float().reshape(-1)  # the scale of a perturbed ensemble member (skyrim_amd/ensemble.py)
        self._channels(self.spec.CHANNELS, *self.widths(self.cfg))
        lat, lon = self.axes(self.cfg)
        self.grid = Grid(list(lat), list(lon))
        if self.guard_hint is not None:
            self.guard = weights.FiniteGuard(self.guard_hint)

    def widths(self, cfg) -> tuple:
        """(input channels,) or (input channels, output channels) of ``cfg``."""
        return (cfg.channels,)

    def axes(self, cfg):
        return self.spec.latlon_axes(cfg)

    def _load(self, path: str):
        """A torch file of the slot dict, or the model's package directory: ``checkpoint.load`` of the model's package (imported on use)."""
        checkpoint = importlib.import_module(".checkpoint", type(self).__module__.rpartition(".")[0])
        return checkpoint.load(path, self.cfg)

    def synthetic_state(self, seed: int) -> torch.Tensor:
        """Initial-condition hook of the synthetic DataSource."""
        return self.spec.synthetic_state(self.cfg, seed)


class HistoryTimeLoop(SpecTimeLoop):
    """Two history levels.  A model supplies ``advance``; ``time_step`` is the spacing of the yields (the levels are 6 h apart)."""
    n_history_levels = 2
    # A loop continued from its own last output (run_basic_inference's resident state marks it ``_state_is_own_output``) goes on counting
    # its steps from the last yield, and takes the mark off.  False: every call counts from 0 and leaves the mark alone.
    resumes_step_count = True
    _last = (None, 0)                   # (yielded tensor, its step) of the last yield

    def advance(self, older, newer, time, step: int):
        """Call ``step`` (1-based) of the network on the levels at ``time`` - 6 h and ``time`` -> the next (older, newer); newer is yielded."""
        raise NotImplementedError

    def take_pending_check(self):
        """(flag, step, hint) of the last yielded state's deferred finite check, handed to the caller (models/utils.py)."""
        p = self.guard.take()
        return None if p is None else (p[0], p[1], self.guard.hint)

    def _yield(self, time, older, newer, step, restart, guard):
        out = newer.unsqueeze(0)
        self._last = (out, step)
        if step > 0:
            guard.push(newer, step)
        return time, out, restart

    def __call__(self, time: datetime.datetime, x: torch.Tensor, restart=None):
        shape = (1, 2) + self.engine.state_shape
        if x.dim() != 5 or tuple(x.shape) != shape:
            raise ValueError(f"expected x of shape {shape} (states at time - 6 h and time), got {tuple(x.shape)}")
        own = self.resumes_step_count and self.__dict__.pop("_state_is_own_output", False)   # x holds this loop's last outputs, still in HBM
        step = self._last[1] if own else 0
        x = x.to(self.device, torch.float32)
        older, newer = x[0, 0].contiguous().clone(), x[0, 1].contiguous().clone()
        # the deferred check belongs to THIS generator (several may be open at once: skyrim_amd/ensemble.py interleaves one per member);
        # ``self.guard`` names the one opened last, which is the one take_pending_check's caller is draining
        guard = self.guard = weights.FiniteGuard(self.guard.hint)
        try:
            yield self._yield(time, older, newer, step, restart, guard)
            while True:
                step += 1
                older, newer = self.advance(older, newer, time, step)
                time = time + self.time_step
                yield self._yield(time, older, newer, step, restart, guard)
        finally:
            guard.check()
