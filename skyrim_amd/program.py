"""The host prelude of the program-driven product bindings (derived, thermo, vertical, aggregate, neighbourhood): each
``run`` takes M members, their device table, a small program of ops and a float32 (M, D, H, W) output, and makes the same refusals in
the same order before it fills the same head of its descriptor and launches.  Those steps live here once; what a binding checks of its
own ops and extra planes stays in the binding, in the place it had.  The C++ side of the same layer is csrc/program.h.
"""
from __future__ import annotations

import ctypes

import torch

from . import native
from .members import member_count, member_set


def counts(what: str, members, ops, max_members: int, max_ops: int) -> None:
    """The two refusals that need no member: the number of members, then the number of ops.  ``bind`` begins with them; a binding whose
    next refusal needs no member either (neighbourhood: the number of radii) calls this first and ``bind`` with ``counted=True``, so that
    its refusals keep their order."""
    member_count(members, what, max_members)
    if not 1 <= len(ops) <= max_ops:
        raise ValueError(f"{what}: {len(ops)} ops; 1 to {max_ops} are supported")


def bind(what: str, members, table, ops, out, out_what: str, max_members: int, max_ops: int, counted: bool = False) -> tuple:
    """Every refusal the bindings share, in their order: ``counts`` (unless the caller has made them: ``counted``), the member set
    (``members.member_set``), then ``out`` -- a contiguous float32 tensor on the members' device, (M, D, H, W) for members of (C, H, W);
    ``out_what`` is its name in the messages ("derive_fields: out").  Returns (M, device, align, C, H, W, D, the address of ``out``).
    This runs per lead time and product, so it builds no string that only a refusal needs, reads ``out.shape`` once and returns a
    plain tuple."""
    if not counted:
        counts(what, members, ops, max_members, max_ops)
    M, dev, align = member_set(members, table, what, max_members)
    C, H, W = members[0].shape
    po = native.tensor_ptr(out, out_what, torch.float32, dev)
    shape = out.shape
    if len(shape) != 4 or shape[0] != M or shape[2:] != (H, W):
        raise ValueError(f"{out_what} must be ({M}, D, {H}, {W})")
    return M, dev, align, C, H, W, shape[1], po


def fill_head(d, M, C, H, W, D, member_stride, member_align) -> None:
    """The seven fields every descriptor begins with (after its ``members`` pointer)."""
    d.M, d.member_align, d.C, d.H, d.W, d.D, d.member_stride = M, member_align, C, H, W, D, member_stride


def plane(what: str, t, name: str, shape: tuple, dtype, dev) -> int:
    """The address of an extra plane of a call (a surface geopotential): of ``shape``, then contiguous, of ``dtype`` and on ``dev``."""
    if tuple(t.shape) != shape:
        raise ValueError(f"{what}: {name} must be {shape}")
    return native.tensor_ptr(t, f"{what}: {name}", dtype, dev)


def launch(lib: ctypes.CDLL, fn, d, dev) -> None:
    """``fn(&d, stream)`` -- ``fn`` an entry point of ``lib`` -- on torch's current stream of ``dev``; a non-zero return code is a
    RuntimeError."""
    with torch.cuda.device(dev):
        native.check(fn(ctypes.byref(d), native.stream(dev)), fn.__name__, lib)
