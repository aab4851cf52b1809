"""``torch.ops.skyrim_hip.thermo_fields`` against the numpy float32 restatement (tests/_thermo_reference.py ``fp32``), bit for bit: both
paths, both moisture kinds, both sources, with and without a surface, the planted corner columns, every subset of an op's slots with
the untouched slots and the tail checked, non-finite inputs, and bit-equal repeats."""
from __future__ import annotations

import itertools

import numpy as np
import pytest
import torch

import _thermo_reference as R
from skyrim_amd import thermo as T
from skyrim_amd.members import member_table

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMES = {T.MOIST: ("td", "other", "thetae", "theta"), T.INDEX: ("kx", "tt"), T.FREEZE: ("zdeg0",), T.PARCEL: ("cape", "li", "p_src")}


def chans(L):
    """the channel tuples (t, q, r, z) of ``R.planted``'s layout"""
    return tuple(tuple(range(i * L, (i + 1) * L)) for i in range(4))


def program(L, kind, source, surface):
    """MOIST at the second level, INDEX, FREEZE and PARCEL over all levels: ten slots, slot 10 stays untouched"""
    t, q, r, z = chans(L)
    m = q if kind == R.Q else r
    lv = R.LEVELS[L]
    i7, i5 = min(3, L - 1), min(5, L - 1)
    return [T.Op(T.MOIST, (t[1],), (m[1],), (), (0, 1, 2, 3), kind, (float(lv[1]),)),
            T.Op(T.INDEX, (t[0], t[i7], t[i5]), (m[0], m[i7]), (), (4, 5), kind),
            T.Op(T.FREEZE, t, (), z, (6,)),
            T.Op(T.PARCEL, t, m, z if surface else (), (7, 8, 9), kind, tuple(float(p) for p in lv), source)]


def expect(state, zs, op):
    """{slot: plane} of one op on one (C, H, W) state by the restatement"""
    pick = lambda idx: state[list(idx)]                             # noqa: E731
    if op.kind == T.MOIST:
        only = all(s < 0 for s in op.outputs[:3])
        res = R.fp32.moist(state[op.t[0]], state[op.m[0]] if op.m else state[op.t[0]], op.pressures[0], op.moisture, theta_only=only)
    elif op.kind == T.INDEX:
        res = R.fp32.index(*pick(op.t), *pick(op.m), op.moisture)
    elif op.kind == T.FREEZE:
        res = (R.fp32.freeze(pick(op.t), pick(op.z), zs),)
    else:
        res = R.fp32.parcel(pick(op.t), pick(op.m), op.pressures, op.moisture, op.source, op.p_src_min, op.p_top,
                            z=pick(op.z) if zs is not None else None, zs=zs)
    return {s: v for s, v in zip(op.outputs, res) if s >= 0}


def run_op(states, ops, n_out, misalign=False, zs=None):
    """The (M, n_out, H, W) output of one thermo_fields on the device; the buffer starts as 0xAB bytes and has a tail that must stay so."""
    M, (_, H, W) = len(states), states[0].shape
    members = []
    for s in states:
        if misalign:
            flat = torch.empty(s.size + 1, dtype=torch.float32, device=DEV)
            t = flat[1:].view(s.shape)
            assert t.data_ptr() % 16 == 4
        else:
            t = torch.empty(s.shape, dtype=torch.float32, device=DEV)
        t.copy_(torch.from_numpy(s))
        members.append(t)
    raw = torch.full((M * n_out * H * W * 4 + 256,), 0xAB, dtype=torch.uint8, device=DEV)
    out = raw[:M * n_out * H * W * 4].view(torch.float32).view(M, n_out, H, W)
    ints, floats = T.encode(ops)
    surface = None if zs is None else torch.from_numpy(zs).to(DEV)
    torch.ops.skyrim_hip.thermo_fields(members, member_table(members), ints, floats, out, surface)
    torch.cuda.synchronize()
    assert bool((raw[M * n_out * H * W * 4:] == 0xAB).all()), "bytes beyond the buffer were touched"
    return out.cpu().numpy()


def untouched(plane) -> bool:
    return bool(np.all(np.ascontiguousarray(plane).view(np.uint8) == 0xAB))


def same_bits(got, want, what):
    """NaN where the restatement has NaN, the same bits everywhere else"""
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), (what, "NaN at other points", np.argwhere(np.isnan(got) != nan)[:5])
    diff = (got.view(np.uint32) != want.view(np.uint32)) & ~nan
    assert not diff.any(), (what, int(diff.sum()), np.argwhere(diff)[:5], got[diff][:5], want[diff][:5])


def check(out, states, zs, ops, what):
    for m, s in enumerate(states):
        for op in ops:
            for slot, plane in expect(s, zs, op).items():
                same_bits(out[m, slot], plane, (what, m, NAMES[op.kind][op.outputs.index(slot)]))


# (H, W), M, L, moisture, source, surface, misaligned
CASES = {"3x4 M=1 L=13 q mu": ((3, 4), 1, 13, R.Q, R.SRC_MAX_THETAE, False, False),
         "3x4 M=64 L=13 q sb zs": ((3, 4), 64, 13, R.Q, R.SRC_LOWEST, True, False),
         "5x12 M=3 L=13 r sb zs misaligned": ((5, 12), 3, 13, R.R, R.SRC_LOWEST, True, True),
         "5x12 M=1 L=16 q mu zs misaligned": ((5, 12), 1, 16, R.Q, R.SRC_MAX_THETAE, True, True),
         "9x516 M=3 L=16 q mu zs": ((9, 516), 3, 16, R.Q, R.SRC_MAX_THETAE, True, False),
         "9x516 M=1 L=13 r mu": ((9, 516), 1, 13, R.R, R.SRC_MAX_THETAE, False, False),
         "9x516 M=1 L=2 r sb zs": ((9, 516), 1, 2, R.R, R.SRC_LOWEST, True, False),
         "7x75 M=3 L=2 q mu": ((7, 75), 3, 2, R.Q, R.SRC_MAX_THETAE, False, False),           # 525 points: past a 512-point tile, no multiple of 4
         "7x75 M=1 L=13 r mu zs": ((7, 75), 1, 13, R.R, R.SRC_MAX_THETAE, True, False)}


@pytest.mark.parametrize("case", list(CASES))
def test_every_output_has_the_restatements_bits(case):
    (H, W), M, L, kind, source, surface, misalign = CASES[case]
    made = [R.planted(40 + (m % 3), H, W, R.LEVELS[L]) for m in range(min(M, 3))]
    states = [made[m % 3][0] for m in range(M)]
    zs = made[0][1] if surface else None
    ops = program(L, kind, source, surface)
    out = run_op(states, ops, 11, misalign, zs)
    check(out[:3], states[:3], zs, ops, case)
    for m in range(3, M):                                        # (members 3 .. repeat the first three states)
        assert np.array_equal(out[m].view(np.uint32), out[m % 3].view(np.uint32)), m
    assert all(untouched(out[m, 10]) for m in range(M))
    if surface:                                                  # the planted columns did what they were planted for
        p_src, cape = out[0, 9].ravel(), out[0, 7].ravel()
        lv = R.LEVELS[L]
        assert np.isnan(p_src[5]) and np.isnan(cape[5]) and np.isnan(out[0, 6].ravel()[5])           # all masked
        assert p_src[6] == lv[-1] and cape[6] == 0                                                     # one unmasked level
        assert p_src[3] == lv[max(L - 2, 0)]                                                           # source second from the top
    assert out[0, 7].ravel()[4] == 0 or L == 2                                                         # LCL above the top: no CAPE
    assert np.isfinite(out[0, :10].reshape(10, -1)[:7, :3]).all()                                      # q = 0, r = 130, saturated


@pytest.mark.parametrize("kind", [T.MOIST, T.INDEX, T.FREEZE, T.PARCEL])
def test_every_subset_of_slots_and_untouched_slots(kind):
    L, (H, W) = 13, (5, 12)
    state, zs = R.planted(7, H, W, R.LEVELS[L])
    full = program(L, R.Q, R.SRC_MAX_THETAE, True)[kind - 1]
    n = T.RESULTS[kind]
    for mask in range(1, 1 << n):
        slots = [-1] * n
        for i, k in enumerate([k for k in range(n) if mask >> k & 1]):
            slots[k] = n - i                                     # (slots in descending order, slot 0 never named)
        op = T.Op(full.kind, full.t, full.m, full.z, tuple(slots), full.moisture, full.pressures, full.source)
        out = run_op([state], [op], n + 1, zs=zs)
        check(out, [state], zs, [op], (kind, mask))
        for d in range(n + 1):
            assert untouched(out[0, d]) == (d not in slots), (kind, mask, d)


def test_paths_repeats_and_launch_splits_give_equal_bits():
    L, (H, W) = 13, (9, 516)
    states = [R.planted(20 + m, H, W, R.LEVELS[L])[0] for m in range(2)]
    zs = R.planted(20, H, W, R.LEVELS[L])[1]
    ops = program(L, R.Q, R.SRC_MAX_THETAE, True)
    t, q, r, z = chans(L)
    lv = tuple(float(p) for p in R.LEVELS[L])
    ops.append(T.Op(T.PARCEL, t, q, z, (10, 11, 12), R.Q, lv, R.SRC_LOWEST))                           # shares the first one's table
    ops.append(T.Op(T.PARCEL, t[2:], r[2:], z[2:], (13, -1, 14), R.R, lv[2:], R.SRC_LOWEST, 700.0, 300.0))   # other levels: a second launch
    whole = run_op(states, ops, 15, zs=zs)
    check(whole, states, zs, ops, "seven ops")
    assert np.array_equal(whole.view(np.uint32), run_op(states, ops, 15, zs=zs).view(np.uint32))       # two runs: the same bits
    assert np.array_equal(whole.view(np.uint32), run_op(states, ops, 15, misalign=True, zs=zs).view(np.uint32))   # scalar path
    for op in ops:
        single = run_op(states, [op], 15, zs=zs)
        for s in op.outputs:
            if s >= 0:
                assert np.array_equal(single[:, s].view(np.uint32), whole[:, s].view(np.uint32)), (op.kind, s)


def test_a_non_finite_input_gives_nan_in_its_column_and_nowhere_else():
    L, (H, W) = 13, (5, 12)
    made = [R.planted(30 + m, H, W, R.LEVELS[L]) for m in range(3)]
    states, zs = [s for s, _ in made], made[0][1]
    ops = program(L, R.Q, R.SRC_MAX_THETAE, True)
    t, q, r, z = chans(L)
    ops.append(T.Op(T.MOIST, (t[1],), (), (), (-1, -1, -1, 10), R.Q, (float(R.LEVELS[L][1]),)))      # theta alone reads no moisture
    clean = run_op(states, ops, 11, zs=zs)
    reads = {T.MOIST: {t[1], q[1]}, T.INDEX: {t[0], t[3], t[5], q[0], q[3]}, T.FREEZE: set(t) | set(z), T.PARCEL: set(t) | set(q) | set(z)}
    for ch, (j, i), value in ((t[1], (2, 5), np.nan), (q[1], (4, 11), np.inf), (q[7], (1, 0), -np.inf), (z[12], (3, 7), np.nan), (t[5], (0, 9), np.inf)):
        bad = [s.copy() for s in states]
        bad[1][ch, j, i] = value
        out = run_op(bad, ops, 11, zs=zs)
        assert np.array_equal(out[0].view(np.uint32), clean[0].view(np.uint32)) and np.array_equal(out[2].view(np.uint32), clean[2].view(np.uint32))
        check(out, bad, zs, ops, ("non-finite", ch))
        for op in ops[:4]:
            for s in op.outputs:
                hit = ch in reads[op.kind]
                assert np.isnan(out[1, s, j, i]) == (hit or bool(np.isnan(clean[1, s, j, i]))), (ch, op.kind, s)
                keep = np.ones((H, W), bool)
                keep[j, i] = False
                assert np.array_equal(out[1, s][keep].view(np.uint32), clean[1, s][keep].view(np.uint32)), (ch, op.kind, s)
        assert np.isnan(out[1, 10, j, i]) == (ch == t[1])
    zbad = zs.copy()
    zbad[2, 2] = np.inf
    out = run_op(states, ops, 11, zs=zbad)
    assert np.isnan(out[:, 6:10, 2, 2]).all() and np.isfinite(out[:, :6, 2, 2]).all()                   # FREEZE and PARCEL read the surface
    check(out, states, zbad, ops, "non-finite surface")
