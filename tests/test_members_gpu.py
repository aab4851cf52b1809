"""``members.member_set`` and ``member_table`` on the device: what only a device tensor can show -- the alignment class, and the refusals
that lie behind ``tensor_ptr``'s device check."""
from __future__ import annotations

import pytest
import torch

from skyrim_amd.members import member_set, member_table

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SHAPE = (2, 3, 5)


def _members(n=3):
    return [torch.zeros(SHAPE, dtype=torch.float32, device=DEV) for _ in range(n)]


def test_alignment_class_and_the_table():
    mem = _members()
    table = member_table(mem)
    assert table.dtype == torch.int64 and table.device == DEV and table.tolist() == [t.data_ptr() for t in mem]
    assert all(t.data_ptr() % 16 == 0 for t in mem)                                # fresh allocations
    assert member_set(mem, table, "p", 8) == (3, DEV, 16)
    buf = torch.zeros(31, dtype=torch.float32, device=DEV)
    mem[1] = buf[1:31].view(SHAPE)                                                 # contiguous, 4 bytes into its buffer
    assert mem[1].is_contiguous() and mem[1].data_ptr() % 16 == 4
    assert member_set(mem, member_table(mem), "p", 8) == (3, DEV, 4)
    flat = [t.view(-1) for t in mem]
    assert member_set(flat, member_table(flat), "p", 8, ndim=None, same="numel") == (3, DEV, 4)


def test_refusals_behind_the_device_check():
    mem = _members()
    table = member_table(mem)
    with pytest.raises(ValueError, match=rf"^p: member: expected a contiguous float32 tensor on {DEV}$"):
        member_set([mem[0], mem[1].cpu(), mem[2]], table, "p", 8)
    with pytest.raises(ValueError, match=r"^p: the members differ in shape$"):
        member_set([mem[0], mem[1].view(3, 2, 5), mem[2]], table, "p", 8)
    assert member_set([mem[0], mem[1].view(3, 2, 5), mem[2]], table, "p", 8, same="numel") == (3, DEV, 16)
    with pytest.raises(ValueError, match=r"^p: the members differ in shape$"):
        member_set([mem[0], torch.zeros(31, dtype=torch.float32, device=DEV)], table[:2].contiguous(), "p", 8, ndim=None, same="numel")
    with pytest.raises(ValueError, match=r"^p: table must be member_table\(members\)$"):
        member_set(mem, table[:2].contiguous(), "p", 8)
    with pytest.raises(ValueError, match=r"^p: table must be member_table\(members\)$"):
        member_set(mem, table.to(torch.int32), "p", 8)
    with pytest.raises(ValueError, match=r"^p: table must be member_table\(members\)$"):
        member_set(mem, table.cpu(), "p", 8)
