"""``torch.ops.skyrim_hip.vert_fields`` against the numpy float32 restatement (tests/_vert_reference.py ``fp32``), bit for bit: both
paths, the five coordinates, the four field kinds, one and four targets, one and eight fields, with and without a surface, both
``outside`` modes, the planted corner columns, every subset of an op's slots with the untouched slots and the tail checked, non-finite
inputs, launch splits and bit-equal repeats; and against what exists: ``zdeg0`` and ``theta<level>`` of ``thermo_fields``, ``ws<level>``
of ``derive_fields``."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import _vert_reference as R
from skyrim_amd import vertical as V
from skyrim_amd.members import member_table

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TARGETS = {V.P: (700.0, 875.0, 1100.0, 30.0), V.Z: (1500.0, 5000.0, 300.0, 11000.0), V.Z_AGL: (100.0, 5.0, 1500.0, 40.0),
           V.THETA: (320.0, 300.0, 350.0, 285.0), V.T: (-10.0, 0.0, -40.0, 15.0)}      # the first ones are those the corners are planted around
G10, G2 = float(np.float32(9.80665 * 10)), float(np.float32(9.80665 * 2))
NO = (V.NODE_NONE, V.NODE_NONE)


def op_of(L, coord, T, F, surface, outside, slot0=0):
    """One op with slots slot0 + f T + t.  F = 8: t, ws, theta, p, q, u, z, v (all four kinds; above the ground t, ws, u and z have
    their surface nodes); F = 1: ws alone."""
    lay = R.layout(L)
    agl = coord == V.Z_AGL
    slots = lambda f: tuple(slot0 + f * T + t for t in range(T))        # noqa: E731
    ws = lambda f: V.Field(V.SPEED, lay["u"], lay["v"], slots(f), (lay["u10m"], lay["v10m"]) if agl else NO, G10 if agl else 0.0)      # noqa: E731
    if F == 1:
        fields = (ws(0),)
    else:
        fields = (V.Field(V.PLAIN, lay["t"], (), slots(0), (lay["t2m"], V.NODE_NONE) if agl else NO, G2 if agl else 0.0), ws(1),
                  V.Field(V.THETA_F, lay["t"], (), slots(2)), V.Field(V.PRESSURE, (), (), slots(3)), V.Field(V.PLAIN, lay["q"], (), slots(4)),
                  V.Field(V.PLAIN, lay["u"], (), slots(5), (lay["u10m"], V.NODE_NONE) if agl else NO, G10 if agl else 0.0),
                  V.Field(V.PLAIN, lay["z"], (), slots(6), (V.NODE_ZS, V.NODE_NONE) if agl else NO), V.Field(V.PLAIN, lay["v"], (), slots(7)))
    c = {V.P: (), V.Z: lay["z"], V.Z_AGL: lay["z"], V.THETA: lay["t"], V.T: lay["t"]}[coord]
    z = lay["z"] if coord in (V.THETA, V.T) and surface else ()
    return V.Op(coord, tuple(float(p) for p in R.LEVELS[L]), c, z, tuple(V.target_value(coord, x) for x in TARGETS[coord][:T]), fields, outside)


def run_op(states, ops, n_out, misalign=False, zs=None):
    """The (M, n_out, H, W) output of one vert_fields on the device; the buffer starts as 0xAB bytes and has a tail that must stay so."""
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
    ints, floats = V.encode(ops)
    surface = None if zs is None else torch.from_numpy(zs).to(DEV)
    torch.ops.skyrim_hip.vert_fields(members, member_table(members), ints, floats, out, surface)
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


def check(out, states, zs, ops, what, info=None):
    for m, s in enumerate(states):
        for k, op in enumerate(ops):
            for slot, plane in R.fp32.apply(op, s, zs, info=info if m == 0 and k == 0 else None).items():
                same_bits(out[m, slot], plane, (what, m, k, slot))


# (H, W), M, L, T, F, surface, outside, misaligned
SHAPES = {"5x12 M=3 L=13 T=4 F=8 zs nan": ((5, 12), 3, 13, 4, 8, True, V.NAN, False),
          "6x16 M=1 L=13 T=4 F=8 zs nearest": ((6, 16), 1, 13, 4, 8, True, V.NEAREST, False),
          "6x16 M=3 L=16 T=1 F=1 zs nearest misaligned": ((6, 16), 3, 16, 1, 1, True, V.NEAREST, True),
          "5x12 M=1 L=2 T=4 F=8 nan": ((5, 12), 1, 2, 4, 8, False, V.NAN, False),
          "6x16 M=1 L=16 T=1 F=8 nearest": ((6, 16), 1, 16, 1, 8, False, V.NEAREST, False),
          "6x16 M=1 L=2 T=4 F=1 zs nearest": ((6, 16), 1, 2, 4, 1, True, V.NEAREST, False),
          "9x516 M=3 L=13 T=4 F=8 zs nan": ((9, 516), 3, 13, 4, 8, True, V.NAN, False),          # ten tiles a member
          "7x75 M=1 L=13 T=4 F=8 zs nearest": ((7, 75), 1, 13, 4, 8, True, V.NEAREST, False)}     # 525 points: past a tile, no multiple of 4
COORDS = {"P": V.P, "Z": V.Z, "Z_AGL": V.Z_AGL, "THETA": V.THETA, "T": V.T}
_made: dict = {}


def states_of(L, H, W, M):
    """the planted states of a shape, made once and shared; nothing changes them"""
    key = (L, H, W)
    if key not in _made:
        _made[key] = [R.planted(40 + m, H, W, R.LEVELS[L]) for m in range(3)]
    return [_made[key][m][0] for m in range(M)], _made[key][0][1]


@pytest.mark.parametrize("coord", list(COORDS))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_every_output_has_the_restatements_bits(shape, coord):
    (H, W), M, L, T, F, surface, outside, misalign = SHAPES[shape]
    coord = COORDS[coord]
    surface = surface or coord == V.Z_AGL                           # (a height above the ground needs the ground)
    states, zs = states_of(L, H, W, M)
    zs = zs if surface else None
    op = op_of(L, coord, T, F, surface, outside)
    out = run_op(states, [op], T * F + 1, misalign, zs)
    info = {}
    check(out, states, zs, [op], (shape, coord), info)
    assert all(untouched(out[m, T * F]) for m in range(M))
    # the planted columns did what they were planted for (tests/test_vert_cpu.py checks the restatement's side in detail)
    mode = info[(0, 0)][0].ravel()
    if L > 2 and coord in (V.Z, V.T) and surface is False:
        assert mode[0] == R.LAYER and mode[1] == R.LAYER and mode[5] == R.LAYER and mode[2] == (R.LEVEL if outside else R.NONE)
    if coord == V.Z_AGL:
        assert mode[9] == R.NODE_LAYER and mode[10] == R.NODE_LAYER and np.isnan(out[0, 0].ravel()[8]) and np.isnan(out[0, 0].ravel()[14])
    if coord in (V.Z, V.Z_AGL):
        assert np.isnan(out[0, 0].ravel()[12])                       # NaN in a z plane


@pytest.mark.parametrize("coord", ["Z_AGL", "THETA"])
def test_every_subset_of_slots_and_untouched_slots(coord):
    L, (H, W) = 13, (5, 12)
    states, zs = states_of(L, H, W, 1)
    full = op_of(L, COORDS[coord], 2, 8, True, V.NAN)
    fields = (full.fields[1], full.fields[3] if coord == "THETA" else full.fields[0])      # ws with p (on the isentrope) or with t (above the ground)
    for mask in range(1, 16):
        named = [k for k in range(4) if mask >> k & 1]
        slots = [-1] * 4
        for i, k in enumerate(named):
            slots[k] = 4 - i                                         # (slots in descending order, slot 0 never named)
        op = V.Op(full.coord, full.pressures, full.c, full.z, full.targets,
                  tuple(V.Field(f.kind, f.a, f.b, tuple(slots[2 * j:2 * j + 2]), f.node, f.gh) for j, f in enumerate(fields)), full.outside)
        out = run_op(states, [op], 5, zs=zs)
        check(out, states, zs, [op], (coord, mask))
        for d in range(5):
            assert untouched(out[0, d]) == (d not in slots), (coord, mask, d)


def test_paths_repeats_and_launch_splits_give_equal_bits():
    L, (H, W) = 13, (9, 516)
    states, zs = states_of(L, H, W, 2)
    ops = [op_of(L, c, 4, 8, True, V.NEAREST if k % 2 else V.NAN, 32 * k) for k, c in enumerate(COORDS.values())]      # 40 fields: more than a launch holds
    whole = run_op(states, ops, 161, zs=zs)
    check(whole, states, zs, ops, "five ops")
    assert all(untouched(whole[m, 160]) for m in range(2))
    assert np.array_equal(whole.view(np.uint32), run_op(states, ops, 161, zs=zs).view(np.uint32))                      # two runs: the same bits
    assert np.array_equal(whole.view(np.uint32), run_op(states, ops, 161, misalign=True, zs=zs).view(np.uint32))       # the scalar path
    for k, op in enumerate(ops):
        single = run_op(states, [op], 161, zs=zs)
        assert np.array_equal(single[:, 32 * k:32 * k + 32].view(np.uint32), whole[:, 32 * k:32 * k + 32].view(np.uint32)), k


def test_a_non_finite_input_gives_nan_at_its_point_and_nowhere_else():
    L, (H, W) = 13, (5, 12)
    lay = R.layout(L)
    states, zs = states_of(L, H, W, 3)
    ops = [op_of(L, V.Z_AGL, 2, 8, True, V.NAN), op_of(L, V.THETA, 2, 8, True, V.NEAREST, 16), op_of(L, V.P, 2, 1, True, V.NAN, 32)]
    clean = run_op(states, ops, 35, zs=zs)
    infos = [{} for _ in ops]
    for k, op in enumerate(ops):
        R.fp32.apply(op, states[1], zs, info=infos[k])
    layered = np.flatnonzero(infos[0][(4, 0)][0].ravel() == R.LAYER)
    j, i = divmod(int(layered[layered >= len(R.PLANTED)][0]), W)   # a column that is no planted corner, where q@100magl lies in a layer
    lower = int(infos[0][(4, 0)][1][j, i])                          # the level it takes its lower value from
    assert lower < L - 2
    far = L - 1                                                     # the top level: no result at 100 m above the ground reads it
    # (channel, value, the ops whose every result must turn NaN, the ops that do not read the plane at all)
    cases = ((lay["z"][4], np.nan, {0, 1}, {2}), (lay["t"][2], np.inf, {1}, {2}), (lay["q"][lower], -np.inf, {0}, {2}),
             (lay["u10m"], np.nan, {0}, {1, 2}), (lay["v"][6], np.inf, set(), set()))
    for ch, value, must, never in cases:
        bad = [s.copy() for s in states]
        bad[1][ch, j, i] = value
        out = run_op(bad, ops, 35, zs=zs)
        assert np.array_equal(out[0].view(np.uint32), clean[0].view(np.uint32)) and np.array_equal(out[2].view(np.uint32), clean[2].view(np.uint32))
        check(out, bad, zs, ops, ("non-finite", ch))
        keep = np.ones((H, W), bool)
        keep[j, i] = False
        assert np.array_equal(out[1][:34, keep].view(np.uint32), clean[1][:34, keep].view(np.uint32)), ch      # no other point is affected
        for k in range(3):
            sl = slice(16 * k, 16 * k + (16 if k < 2 else 2))
            if k in must:
                assert np.isnan(out[1, sl, j, i]).all(), (ch, k)      # every requested result of the op
            if k in never:
                assert np.array_equal(out[1, sl, j, i].view(np.uint32), clean[1, sl, j, i].view(np.uint32)), (ch, k)
    # a field value at a level no result of the point reads changes nothing there
    quiet = [s.copy() for s in states]
    quiet[1][lay["q"][far], j, i] = np.nan
    op_q = V.Op(ops[0].coord, ops[0].pressures, ops[0].c, ops[0].z, ops[0].targets[:1], (V.Field(V.PLAIN, lay["q"], (), (0,)),))
    assert np.array_equal(run_op(quiet, [op_q], 1, zs=zs).view(np.uint32), run_op(states, [op_q], 1, zs=zs).view(np.uint32))
    zbad = zs.copy()
    zbad[2, 2] = np.inf
    out = run_op(states, ops, 35, zs=zbad)
    assert np.isnan(out[:, :32, 2, 2]).all() and np.array_equal(out[:, 32:34, 2, 2].view(np.uint32), clean[:, 32:34, 2, 2].view(np.uint32))      # P does not read zs
    check(out, states, zbad, ops, "non-finite surface")


# ---- against what exists ------------------------------------------------------------------------------------------------------------------ #
def test_z_on_the_zero_isotherm_is_zdeg0_where_there_is_a_crossing():
    from skyrim_amd import thermo as TH
    L, (H, W) = 13, (6, 16)
    lay = R.layout(L)
    states, zs = states_of(L, H, W, 2)
    for surface in (None, zs):
        freeze = [TH.Op(TH.FREEZE, lay["t"], (), lay["z"], (0,))]
        members = [torch.from_numpy(s).to(DEV) for s in states]
        want = torch.full((2, 1, H, W), float("nan"), device=DEV)
        ints, floats = TH.encode(freeze)
        sdev = None if surface is None else torch.from_numpy(surface).to(DEV)
        torch.ops.skyrim_hip.thermo_fields(members, member_table(members), ints, floats, want, sdev)
        op = V.Op(V.T, tuple(float(p) for p in R.LEVELS[L]), lay["t"], lay["z"] if surface is not None else (), (V.target_value(V.T, 0.0),),
                  (V.Field(V.PLAIN, lay["z"], (), (0,)),))
        got = run_op(states, [op], 1, zs=surface)
        want = want.cpu().numpy()
        crossed = ~np.isnan(got)
        assert crossed.sum() > H * W and np.array_equal(got[crossed].view(np.uint32), want[crossed].view(np.uint32))


def test_fields_on_a_model_level_are_the_levels_own():
    from skyrim_amd import derived as D
    from skyrim_amd import thermo as TH
    L, (H, W) = 13, (6, 16)
    lay = R.layout(L)
    states, _ = states_of(L, H, W, 2)
    k = 3                                                           # 700 hPa, an interior level
    lv = tuple(float(p) for p in R.LEVELS[L])
    op = V.Op(V.P, lv, (), (), (V.target_value(V.P, lv[k]),), (V.Field(V.THETA_F, lay["t"], (), (0,)), V.Field(V.SPEED, lay["u"], lay["v"], (1,))))
    got = run_op(states, [op], 2)
    members = [torch.from_numpy(s).to(DEV) for s in states]
    table = member_table(members)
    want = torch.zeros((2, 2, H, W), device=DEV)
    ints, floats = TH.encode([TH.Op(TH.MOIST, (lay["t"][k],), (), (), (-1, -1, -1, 0), TH.Q, (lv[k],))])
    torch.ops.skyrim_hip.thermo_fields(members, table, ints, floats, want, None)
    ints, floats = D.encode([D.Op(D.SPEED, (lay["u"][k], lay["v"][k]), (1,))])
    torch.ops.skyrim_hip.derive_fields(members, table, ints, floats, want, None, [])
    want = want.cpu().numpy()
    ok = ~np.isnan(want)                                            # (the planted -Inf in t and Inf in u)
    assert np.array_equal(np.isnan(got), ~ok) and np.array_equal(got[ok].view(np.uint32), want[ok].view(np.uint32))
