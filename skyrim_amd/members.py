"""The member set of the product libraries: M member states on one device plus the device table of their addresses.

Every product binding (ensemble, verify, events, tracks, regrid, points, scenarios, spectra, breeding) takes ``members`` and
``table = member_table(members)`` and validates them here, with its own name in front of every message.  The program-driven bindings
(derived, thermo, vertical, aggregate, neighbourhood) do so through ``program.bind``, the prelude they share.
"""
from __future__ import annotations

import torch

from .native import tensor_ptr


def member_table(members) -> torch.Tensor:
    """The device array of member pointers the kernels read (one small upload; keep it while the members keep their storage)."""
    return torch.tensor([t.data_ptr() for t in members], dtype=torch.int64).to(members[0].device)


def member_count(members, what: str, max_members: int, lo: int = 1) -> int:
    """M = len(members), refused outside ``lo..max_members``.  ``member_set`` begins with this; a caller whose next refusal needs no
    member (a count of ops or channels, the rank of a truth) calls it first, so that its refusals keep their order."""
    M = len(members)
    if not lo <= M <= max_members:
        raise ValueError(f"{what}: {M} members; {lo} to {max_members} are supported")
    return M


def member_set(members, table, what: str, max_members: int, lo: int = 1, ndim: int | None = 3, same: str = "shape", dev=None):
    """(M, device, align) of a valid member set: ``lo..max_members`` contiguous float32 tensors on one device -- ``dev``, or that of
    the first -- of rank ``ndim`` (None: any), equal in shape (``same="shape"``) or in element count (``same="numel"``), with ``table``
    the int64 device array of M entries ``member_table`` makes of them.  ``align``: 16 when every member's address is a multiple of 16
    (the kernels may then read four floats at once), otherwise 4.  The CONTENTS of ``table`` (device memory) are not read back: they
    are trusted to be the addresses of ``members`` in order."""
    M = member_count(members, what, max_members, lo)
    first = members[0]
    if ndim is not None and first.dim() != ndim:
        raise ValueError(f"{what}: states are (C, H, W)")
    dev = first.device if dev is None else dev
    align = 16
    for t in members:
        if tensor_ptr(t, f"{what}: member", torch.float32, dev) % 16:
            align = 4
        if (t.numel() != first.numel()) if same == "numel" else (t.shape != first.shape):
            raise ValueError(f"{what}: the members differ in shape")
    if table.dtype != torch.int64 or table.device != dev or table.numel() != M or not table.is_contiguous():
        raise ValueError(f"{what}: table must be member_table(members)")
    return M, dev, align


def fill_channels(d, channels, max_channels: int) -> None:
    """``d.nc`` and ``d.channels[k]`` of a descriptor from the channel indices ``channels``; entries past ``max_channels`` are left out
    (``nc`` still counts them: the caller, or the library, refuses the call)."""
    channels = [int(c) for c in channels]
    d.nc = len(channels)
    for k, c in enumerate(channels[:max_channels]):
        d.channels[k] = c
