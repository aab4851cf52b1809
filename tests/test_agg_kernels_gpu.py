"""``torch.ops.skyrim_hip.agg_update`` against the float32 restatement of include/skyrim_agg.h (tests/_agg_reference.py): every output
BIT-EQUAL on inputs in the normal range -- both paths, misaligned pointers, a 0xAB-filled accumulator with untouched slots and tail,
repeats, ties and signed zeros, planted NaN and infinities, infinite and attained thresholds, the derived bound of the mean against
float64, and one full-size case."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import _agg_reference as R
from skyrim_amd import aggregate as A
from skyrim_amd import ensemble as E

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
C = 6
D = 24
SHAPES = [(3, 4), (5, 132), (7, 50), (33, 64)]                 # (7, 50): H W = 350 is no multiple of 4 -- the scalar path


def program():
    """Sixteen ops in one call: all four kinds, MAX and MIN with and without ``when``, several ops per input channel (channel 0: five)."""
    return [A.Op(A.MAX, 0, 0, when=1), A.Op(A.SUM, 0, 2, scale=float(np.float32(1 / 3))), A.Op(A.COUNT_ABOVE, 0, 3, thr=1.5, scale=6.0),
            A.Op(A.MIN, 0, 4), A.Op(A.SUM, 0, 5, scale=1.0),
            A.Op(A.MIN, 1, 6, when=7), A.Op(A.MAX, 1, 8), A.Op(A.COUNT_ABOVE, 1, 9, thr=-20.0, scale=1.0),
            A.Op(A.MAX, 2, 10, when=11), A.Op(A.MIN, 2, 12, when=13),
            A.Op(A.SUM, 3, 14, scale=0.25), A.Op(A.COUNT_ABOVE, 3, 15, thr=0.0, scale=3.0),
            A.Op(A.MAX, 4, 16), A.Op(A.SUM, 4, 17, scale=1.0),
            A.Op(A.MIN, 5, 18, when=19), A.Op(A.COUNT_ABOVE, 5, 20, thr=1e4, scale=6.0)]


UNNAMED = (21, 22, 23)


def phases(n):
    return [(A.FIRST if k == 0 else 0) | (A.LAST if k == n - 1 else 0) for k in range(n)]


def with_phase(ops, phase):
    return [A.Op(o.kind, o.channel, o.out, o.when, phase, o.thr, o.scale) for o in ops]


def device_members(x, misalign=False):
    """The M members of one step as device tensors (x: (M, C, H, W))."""
    members = []
    for s in x:
        if misalign:
            flat = torch.empty(s.size + 1, dtype=torch.float32, device=DEV)
            t = flat[1:].view(s.shape)
            assert t.data_ptr() % 16 == 4
        else:
            t = torch.empty(s.shape, dtype=torch.float32, device=DEV)
            assert t.data_ptr() % 16 == 0
        t.copy_(torch.from_numpy(s))
        members.append(t)
    return members


def fold_device(xs, ops_per_step, stamps, n_slots, misalign_members=False, misalign_acc=False):
    """The (M, n_slots, H, W) accumulator after one agg_update per step; it starts as 0xAB bytes and has a 256-byte tail that must stay so."""
    M, _, H, W = xs[0].shape
    n = M * n_slots * H * W * 4
    off = 4 if misalign_acc else 0
    raw = torch.full((off + n + 256,), 0xAB, dtype=torch.uint8, device=DEV)
    acc = raw[off:off + n].view(torch.float32).view(M, n_slots, H, W)
    assert acc.data_ptr() % 16 == off
    for x, ops, stamp in zip(xs, ops_per_step, stamps):
        members = device_members(x, misalign_members)
        ints, floats = A.encode(ops)
        torch.ops.skyrim_hip.agg_update(members, E.member_table(members), ints, floats, float(stamp), acc)
        torch.cuda.synchronize()
    assert bool((raw[off + n:] == 0xAB).all()) and bool((raw[:off] == 0xAB).all()), "bytes outside the accumulator were touched"
    return acc.cpu().numpy()


def garbage(shape):
    return np.frombuffer(b"\xab" * (4 * int(np.prod(shape))), np.float32).reshape(shape)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def assert_bit_equal(got, want, what=""):
    diff = bits(got) != bits(want)
    assert not diff.any(), f"{what}: {int(diff.sum())} of {diff.size} values differ, first at {tuple(np.argwhere(diff)[0])}"


def reference(xs, ops_per_step, stamps, n_slots):
    M, _, H, W = xs[0].shape
    return R.fold(xs, ops_per_step, stamps, n_slots, fill=garbage((M, n_slots, H, W)))


_cases: dict = {}


def base_case(shape, M, steps):
    """(xs, ops per step, stamps, the restatement's accumulator), made once per (shape, M, steps) and shared."""
    key = (shape, M, steps)
    if key not in _cases:
        xs = R.case(M, C, *shape, steps, seed=hash(key) % 1000)
        ops = [with_phase(program(), p) for p in phases(steps)]
        stamps = [6.0 * (k + 1) for k in range(steps)]
        _cases[key] = (xs, ops, stamps, reference(xs, ops, stamps, D))
    return _cases[key]


@pytest.mark.parametrize("M", [1, 2, 50, 64])
@pytest.mark.parametrize("shape", SHAPES)
def test_bit_equal_to_the_restatement(shape, M):
    steps = 3 + (shape[0] + M) % 3                                # three to five steps: FIRST, middle ..., LAST
    xs, ops, stamps, want = base_case(shape, M, steps)
    got = fold_device(xs, ops, stamps, D)
    assert_bit_equal(got, want, f"{shape} M={M}")
    for d in UNNAMED:                                             # slots no op names keep their bytes
        assert np.all(bits(got[:, d]) == 0xABABABAB)
    for o in program():                                           # ... and every named slot was written (FIRST never reads)
        assert not np.any(bits(got[:, o.out]) == 0xABABABAB)


@pytest.mark.parametrize("shape", SHAPES)
def test_one_step_window(shape):
    xs = R.case(2, C, *shape, 1, seed=5)
    ops = [with_phase(program(), A.FIRST | A.LAST)]
    got = fold_device(xs, ops, [6.0], D)
    assert_bit_equal(got, reference(xs, ops, [6.0], D), f"{shape}")
    assert_bit_equal(got[:, 0], xs[0][:, 0])                      # max of one step is the step, its stamp the step's
    assert np.all(got[:, 1] == 6.0) and np.all(got[:, 7] == 6.0)


@pytest.mark.parametrize("shape", [(5, 132), (7, 50)])
@pytest.mark.parametrize("members,acc", [(True, False), (False, True), (True, True)])
def test_misaligned_pointers_give_the_same_bits(shape, members, acc):
    xs, ops, stamps, want = base_case(shape, 2, 4)
    assert_bit_equal(fold_device(xs, ops, stamps, D, misalign_members=members, misalign_acc=acc), want, f"{shape} {members} {acc}")


def test_two_runs_are_bit_equal():
    xs, ops, stamps, _ = base_case((33, 64), 50, 3 + (33 + 50) % 3)
    assert_bit_equal(fold_device(xs, ops, stamps, D), fold_device(xs, ops, stamps, D))


def test_windows_follow_each_other_without_a_reset():
    """Two windows of two steps in one accumulator: FIRST of the second overwrites the first's result, which is read in between."""
    xs = R.case(3, C, 5, 132, 4, seed=11)
    ops = [with_phase(program(), p) for p in (A.FIRST, A.LAST, A.FIRST, A.LAST)]
    stamps = [6.0, 12.0, 18.0, 24.0]
    got = fold_device(xs, ops, stamps, D)
    assert_bit_equal(got, reference(xs[2:], ops[2:], stamps[2:], D))
    assert_bit_equal(fold_device(xs[:2], ops[:2], stamps[:2], D), reference(xs[:2], ops[:2], stamps[:2], D))


def test_ties_keep_the_first_stamp_and_signed_zeros():
    H, W = 5, 132
    x = np.full((3, 1, 1, H, W), 7.5, np.float32)                  # the same value at every step: the first stamp stays
    x[1, 0, 0, 0, :10] = 9.0                                      # a later, greater value takes over where it occurs
    x[:, 0, 0, 1, 0] = (-0.0, 0.0, -0.0)                          # neither zero is greater or smaller than the other
    x[:, 0, 0, 1, 1] = (0.0, -0.0, 0.0)
    ops = [A.Op(A.MAX, 0, 0, when=1), A.Op(A.MIN, 0, 2, when=3)]
    per = [with_phase(ops, p) for p in phases(3)]
    got = fold_device(list(x), per, [6.0, 12.0, 18.0], 4)
    assert_bit_equal(got, reference(list(x), per, [6.0, 12.0, 18.0], 4))
    assert np.all(got[0, 1, 2:] == 6.0) and np.all(got[0, 3] == 6.0)
    assert np.all(got[0, 0, 0, :10] == 9.0) and np.all(got[0, 1, 0, :10] == 12.0) and np.all(got[0, 1, 0, 10:] == 6.0)
    assert bits(got[0, 0, 1, 0]) == 0x80000000 and bits(got[0, 2, 1, 0]) == 0x80000000            # -0.0 came first and stays
    assert bits(got[0, 0, 1, 1]) == 0 and bits(got[0, 2, 1, 1]) == 0                            # +0.0 came first and stays
    assert np.all(got[0, 1, 1, :2] == 6.0) and np.all(got[0, 3, 1, :2] == 6.0)


@pytest.mark.parametrize("shape", [(5, 132), (7, 50)])
def test_non_finite_values_stay_where_they_are_planted(shape):
    M, steps = 4, 4
    xs = [x.copy() for x in base_case(shape, M, steps)[0]]
    clean = base_case(shape, M, steps)[3]
    plants = {(1, 0, 2, 3): np.nan, (1, 1, 1, 1): np.inf, (1, 2, 0, 2): -np.inf}               # (step, channel, j, i) in member 2
    for (k, c, j, i), v in plants.items():
        xs[k][2, c, j, i] = v
    ops = [with_phase(program(), p) for p in phases(steps)]
    stamps = [6.0 * (k + 1) for k in range(steps)]
    got = fold_device(xs, ops, stamps, D)
    assert_bit_equal(got, reference(xs, ops, stamps, D))
    changed = bits(got) != bits(clean)
    allowed = np.zeros_like(changed)
    for (k, c, j, i) in plants:
        for o in program():
            if o.channel == c:
                allowed[2, o.out, j, i] = True
                if o.when >= 0:
                    allowed[2, o.when, j, i] = True
    assert not np.any(changed & ~allowed), "a planted value changed a slot, member or point that does not read it"
    # the NaN of step 1 is still there after steps 2 and 3, in the value and in the stamp; sums and counts carry it too
    assert all(np.isnan(got[2, d, 2, 3]) for d in (0, 1, 2, 3, 4, 5))
    assert got[2, 8, 1, 1] == np.inf and got[2, 6, 1, 1] != np.inf                              # +inf is the maximum, not the minimum
    assert got[2, 12, 0, 2] == -np.inf and got[2, 13, 0, 2] == 12.0 and got[2, 10, 0, 2] != -np.inf


def test_thresholds_infinite_and_attained():
    H, W = 5, 132
    xs = R.case(2, 1, H, W, 3, seed=3)
    for x in xs:
        x[:, 0, 0, :4] = (2.5, np.inf, -np.inf, 2.5000002)
    ops = [A.Op(A.COUNT_ABOVE, 0, 0, thr=float("inf"), scale=1.0), A.Op(A.COUNT_ABOVE, 0, 1, thr=float("-inf"), scale=1.0),
           A.Op(A.COUNT_ABOVE, 0, 2, thr=2.5, scale=1.0)]
    per = [with_phase(ops, p) for p in phases(3)]
    got = fold_device(xs, per, [1.0, 2.0, 3.0], 3)
    assert_bit_equal(got, reference(xs, per, [1.0, 2.0, 3.0], 3))
    assert np.all(got[:, 0] == 0.0)                                # nothing is above +inf, +inf itself included
    assert np.all(got[:, 1, 0, 2] == 0.0) and np.all(np.delete(got[:, 1].reshape(2, -1), 2, axis=1) == 3.0)      # all but -inf are above -inf
    assert np.all(got[:, 2, 0, 0] == 0.0) and np.all(got[:, 2, 0, 3] == 3.0)                   # > is strict; the next float32 counts


def test_mean_of_forty_steps_is_within_the_derived_bound():
    """|mean - exact| <= (n + 1) 2^-24 sum|x| / n: n - 1 additions and the product with float32(1 / n), whose own rounding is one more."""
    n, M, H, W = 40, 2, 33, 64
    rng = np.random.default_rng(7)
    xs = [rng.uniform(250.0, 310.0, size=(M, 1, H, W)).astype(np.float32) for _ in range(n)]
    ops = [A.Op(A.SUM, 0, 0, scale=float(np.float32(1.0 / n)))]
    per = [with_phase(ops, p) for p in phases(n)]
    stamps = [float(k + 1) for k in range(n)]
    got = fold_device(xs, per, stamps, 1)
    assert_bit_equal(got, reference(xs, per, stamps, 1))
    s, a = R.sum64(xs, 0)
    err = np.abs(got[:, 0].astype(np.float64) - s / n)
    bound = (n + 1) * 2.0 ** -24 * a / n
    print(f"mean of {n} steps: worst share of the bound {float((err / bound).max()):.3f}")
    assert np.all(err <= bound)


def test_full_size():
    """721 x 1440, M = 50, C = 2, three ops, three steps, compared on every point."""
    M, H, W, steps = 50, 721, 1440, 3
    ops = [A.Op(A.MAX, 1, 0, when=3), A.Op(A.SUM, 1, 1, scale=float(np.float32(1 / 3))), A.Op(A.COUNT_ABOVE, 1, 2, thr=15.0, scale=6.0)]
    raw = torch.full((M * 4 * H * W * 4 + 256,), 0xAB, dtype=torch.uint8, device=DEV)
    acc = raw[:M * 4 * H * W * 4].view(torch.float32).view(M, 4, H, W)
    want = np.zeros((M, 4, H, W), np.float32)
    gen = torch.Generator(device=DEV).manual_seed(1)
    for k, p in enumerate(phases(steps)):
        members = [torch.rand((2, H, W), generator=gen, device=DEV) * 30.0 + 1e-3 for _ in range(M)]
        per = with_phase(ops, p)
        ints, floats = A.encode(per)
        torch.ops.skyrim_hip.agg_update(members, E.member_table(members), ints, floats, 6.0 * (k + 1), acc)
        R.update(torch.stack(members).cpu().numpy(), want, per, 6.0 * (k + 1))
    torch.cuda.synchronize()
    assert bool((raw[M * 4 * H * W * 4:] == 0xAB).all())
    assert_bit_equal(acc.cpu().numpy(), want)
