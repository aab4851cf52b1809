"""What the engine-backed TimeLoops share (earth2mip's TimeLoop protocol; the reference's skyrim/core/models/*.py build them): the
grid, the device an engine is bound to, and the single-history loop

    loop(time, x) -> iterator of (time, state (B=1, C, n_lat, n_lon) on .device, restart);  first yield = the input state.
"""
from __future__ import annotations

import datetime
from dataclasses import dataclass

import torch


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
