"""What the ctypes-bound engines share (FuXi, FengWu, FourCastNet v1, DLWP, SFNO, GraphCast): the binding of library, device and state shape,
``release()``, the refusals of an unprepared engine and of a wrong state tensor, the fp16 hi/lo weight upload, the input affine and the
shape-checking view of a parameter mapping.  Config validation, ``load_params``, descriptors and launches are each model's own."""
from __future__ import annotations

import torch

from . import native


class Engine:
    keep = ()                   # attributes besides cfg / lib / device / state_shape that ``release()`` leaves in place
    prepare_symbol = ""         # the library's export that splits a matrix into fp16 hi/lo planes (native.HiLoWeight)

    def _bind(self, lib, device, state_shape):
        self.lib, self.device, self.state_shape, self.prepared = lib, torch.device(device), tuple(state_shape), False

    def release(self):
        """Drop every prepared matrix, table and work buffer.  The C ABI holds no state of its own -- all device memory is torch tensors
        owned here -- so this IS the teardown; the engine is unusable until ``load_params`` runs again."""
        kept = {k: v for k, v in vars(self).items() if k in ("cfg", "lib", "device", "state_shape") + self.keep}
        self.__dict__.clear()
        self.__dict__.update(kept)
        self.prepared = False

    def require_prepared(self, method: str):
        if not self.prepared:
            raise RuntimeError(f"{type(self).__name__}.{method} before load_params: not prepared")

    def check_state(self, x: torch.Tensor, what: str | None = None):
        if x.device != self.device or x.dtype != torch.float32 or tuple(x.shape) != self.state_shape or not x.is_contiguous():
            raise ValueError(f"{what + ': ' if what else ''}expected a contiguous float32 tensor of shape {self.state_shape} on {self.device}")

    def _weight(self, w: torch.Tensor) -> native.HiLoWeight:
        """A constant matrix (or a stack of them) as the fp16 hi/lo planes the library's GEMMs read."""
        return native.HiLoWeight(self.device, getattr(self.lib, self.prepare_symbol), w)

    def upload_affine(self, mean, std, n: int):
        """``norm.mean`` / ``norm.std`` -> ``self.mean``, ``self.std``, ``self.inv_std`` on the device (1 / std formed in float64)."""
        std = torch.as_tensor(std).double()
        if tuple(std.shape) != (n,) or not bool((std != 0).all()):
            raise ValueError(f"norm.std must hold {n} non-zero values")
        self.mean = torch.as_tensor(mean).float().contiguous().to(self.device)
        self.std, self.inv_std = std.float().to(self.device), (1.0 / std).float().to(self.device)


class CheckedParams:
    """``params`` read one key at a time, shape-checked against ``shapes``.  ``prefix`` is put in front of every key (FuXi's stage);
    ``source(name)`` says where a slot's shape comes from, for the message (FengWu's config fields)."""

    def __init__(self, params, shapes: dict, prefix: str = "", source=None):
        self.params, self.shapes, self.prefix, self.source = params, shapes, prefix, source

    def __getitem__(self, name):
        t = torch.as_tensor(self.params[self.prefix + name])
        if tuple(t.shape) != tuple(self.shapes[name]):
            origin = f" (from {self.source(name)})" if self.source else ""
            raise ValueError(f"parameter {self.prefix}{name}: expected shape {self.shapes[name]}{origin}, got {tuple(t.shape)}")
        return t
