"""``torch.ops.skyrim_hip.nbr_fields`` against the restatement of include/skyrim_nbr.h (tests/_nbr_reference.py): MAX, MIN and FRAC_ABOVE
BIT-EQUAL, MEAN within the header's bound of exact arithmetic (and outside it when one point of a disc is left out) -- sixteen ops over four
radii in one call, misaligned members, a 0xAB-filled output with untouched slots and tail, closed circles, infinite and attained
thresholds, planted NaN and infinities and their containment, repeats, and one full-size case."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import _nbr_reference as R
from skyrim_amd import ensemble as E
from skyrim_amd import neighbourhood as N
from skyrim_amd.tracks import EARTH_RADIUS_KM
from skyrim_amd.verify import area_weights

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
C, D = 4, 20
UNNAMED = (3, 9, 17, 19)
GRIDS = [(9, 12, True), (7, 15, True), (33, 64, True), (32, 64, False), (19, 50, True)]      # (19, 50): H W = 950 is no multiple of 4


def program():
    """Sixteen ops over four radii, every kind on every radius, several ops per input channel (channel 0: six)."""
    return [N.Op(N.MAX, 0, 0, 0), N.Op(N.MAX, 0, 1, 2), N.Op(N.MIN, 0, 2, 1), N.Op(N.FRAC_ABOVE, 0, 4, 2, 1.5), N.Op(N.MEAN, 0, 5, 1),
            N.Op(N.MEAN, 0, 6, 3),
            N.Op(N.MIN, 1, 7, 3), N.Op(N.FRAC_ABOVE, 1, 8, 1, 0.0), N.Op(N.MEAN, 1, 10, 2), N.Op(N.MAX, 1, 11, 1),
            N.Op(N.MAX, 2, 12, 3), N.Op(N.FRAC_ABOVE, 2, 13, 3, 1.25), N.Op(N.MEAN, 2, 14, 0),
            N.Op(N.MIN, 3, 15, 0), N.Op(N.FRAC_ABOVE, 3, 16, 0, -1.5), N.Op(N.MIN, 3, 18, 2)]


def radii_of(lat, lon):
    """Below the smallest step between two nodes off the poles, about 1.5 and about 4 row steps, and the whole sphere."""
    dphi = np.deg2rad(abs(lat[1] - lat[0])) * EARTH_RADIUS_KM
    off_pole = np.abs(lat) < 90
    dlam = EARTH_RADIUS_KM * np.cos(np.deg2rad(lat[off_pole])).min() * np.deg2rad(360.0 / lon.size)
    return [0.5 * min(dphi, dlam), 1.53 * dphi, 4.07 * dphi, 25000.0]


_grids: dict = {}


def setup(H, W, south=True):
    """(lat, lon, tables, weights) of a grid, made once."""
    key = (H, W, south)
    if key not in _grids:
        lat, lon = R.grid(H, W, south)
        _grids[key] = (lat, lon, [N.discs(lat, lon, r) for r in radii_of(lat, lon)], area_weights(lat))
    return _grids[key]


def device_members(x, misalign=False):
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


def run_device(x, ops, tables, weights, n_slots=D, misalign=False):
    """The (M, n_slots, H, W) output of one nbr_fields; it starts as 0xAB bytes and has a 256-byte tail that must stay so."""
    M, _, H, W = x.shape
    n = M * n_slots * H * W * 4
    raw = torch.full((n + 256,), 0xAB, dtype=torch.uint8, device=DEV)
    out = raw[:n].view(torch.float32).view(M, n_slots, H, W)
    members = device_members(x, misalign)
    ints, floats = N.encode(ops)
    half = [torch.from_numpy(h).to(DEV) for _, h in tables]
    torch.ops.skyrim_hip.nbr_fields(members, E.member_table(members), ints, floats, half, torch.from_numpy(weights).to(DEV), out)
    torch.cuda.synchronize()
    assert bool((raw[n:] == 0xAB).all()), "bytes beyond the output were touched"
    return out.cpu().numpy()


def garbage(shape):
    return np.frombuffer(b"\xab" * (4 * int(np.prod(shape))), np.float32).reshape(shape)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def assert_bit_equal(got, want, what=""):
    diff = bits(got) != bits(want)
    assert not diff.any(), f"{what}: {int(diff.sum())} of {diff.size} values differ, first at {tuple(np.argwhere(diff)[0])}"


def check_exact(got, x, ops, tables, what=""):
    """MAX, MIN, FRAC_ABOVE and the unnamed slots, bit for bit; the MEAN slots are left to ``check_mean``."""
    want = R.fields(x, ops, tables, garbage(got.shape))
    keep = [s for s in range(got.shape[1]) if s not in {op.out for op in ops if op.kind == N.MEAN}]
    assert_bit_equal(got[:, keep], want[:, keep], what)


def check_mean(got, x, ops, tables, weights, members=None) -> float:
    """Every MEAN slot within the header's bound of exact arithmetic; returns the largest error / bound."""
    worst = 0.0
    for m in (range(x.shape[0]) if members is None else members):
        for op in ops:
            if op.kind != N.MEAN:
                continue
            exact, bound = R.mean_exact(x[m, op.channel], *tables[op.radius], weights)
            g = got[m, op.out].astype(np.float64)
            assert np.array_equal(np.isnan(g), np.isnan(exact)), f"member {m} slot {op.out}: NaN in other places than the restatement's"
            ok = ~np.isnan(exact)
            if not ok.any():
                continue
            ratio = np.abs(g[ok] - exact[ok]) / bound[ok]
            worst = max(worst, float(ratio.max()))
            assert ratio.max() <= 1.0, f"member {m} slot {op.out}: error / bound = {ratio.max():.3g}"
    return worst


@pytest.mark.parametrize("M,misalign", [(1, False), (3, True)])
@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: f"{g[0]}x{g[1]}")
def test_sixteen_ops_over_four_radii(grid, M, misalign):
    lat, lon, tables, weights = setup(*grid)
    x = R.case(M, C, grid[0], grid[1], seed=grid[0] + M)
    got = run_device(x, program(), tables, weights, misalign=misalign)
    check_exact(got, x, program(), tables, f"{grid} M={M}")
    assert (bits(got[:, list(UNNAMED)]) == 0xABABABAB).all(), "a slot no op names was written"
    worst = check_mean(got, x, program(), tables, weights, members=[M - 1])
    print(f"nbr mean {grid[0]}x{grid[1]} M={M}: largest error / bound = {worst:.3f}")


def test_sixty_four_members():
    lat, lon = R.grid(5, 8)
    tables, weights = [N.discs(lat, lon, r) for r in radii_of(lat, lon)], area_weights(lat)
    x = R.case(64, C, 5, 8, seed=64)
    got = run_device(x, program(), tables, weights)
    check_exact(got, x, program(), tables, "M=64")
    check_mean(got, x, program(), tables, weights, members=[0, 63])


@pytest.mark.parametrize("grid", [(9, 12, True), (33, 64, True)], ids=lambda g: f"{g[0]}x{g[1]}")
def test_mean_without_one_point_lies_outside_the_bound(grid):
    H, W, _ = grid
    lat, lon, tables, weights = setup(*grid)
    x = R.case(1, C, H, W, seed=7)
    ops = [N.Op(N.MEAN, 0, 0, 2)]
    got = run_device(x, ops, tables, weights, n_slots=1)[0, 0].astype(np.float64)
    reach, half = tables[2]
    full, bound = R.mean_exact(x[0, 0], reach, half, weights)
    assert (np.abs(got - full) <= bound).all()
    for (j, i), d in (((H // 2, 3), 1), ((1, 0), -1), ((H // 3, W - 1), 0)):
        point = (j + d, (i + 1) % W if d == 0 else i)
        assert R.table_sets(reach, half, W)[j, i][point], "the point left out must be one of the disc"
        less, lbound = R.mean_exact(x[0, 0], reach, half, weights, skip=((j, i), point))
        assert abs(less[j, i] - full[j, i]) > 2 * max(bound[j, i], lbound[j, i]), "|x| >= 1: a point left out moves the mean by more than the bound"
        assert abs(got[j, i] - less[j, i]) > lbound[j, i]


def test_fraction_where_the_circle_closes_and_at_thresholds():
    H, W = 9, 12
    lat, lon, tables, weights = setup(H, W)
    x = R.case(2, C, H, W, seed=3)
    x[:, 0] = np.abs(x[:, 0]) + 1                      # channel 0: every value above 1.5
    x[:, 2] = np.float32(1.25)                         # channel 2: the threshold of its FRAC_ABOVE is attained everywhere
    x[0, 2, 4, 5] = np.nextafter(np.float32(1.25), np.float32(2))
    inf = float("inf")
    ops = [N.Op(N.FRAC_ABOVE, 0, r, r, 1.5) for r in range(4)] + [N.Op(N.FRAC_ABOVE, 2, 4 + r, r, 1.25) for r in range(4)] \
        + [N.Op(N.FRAC_ABOVE, 1, 8, 1, inf), N.Op(N.FRAC_ABOVE, 1, 9, 1, -inf), N.Op(N.FRAC_ABOVE, 3, 10, 3, inf), N.Op(N.FRAC_ABOVE, 3, 11, 3, -inf)]
    got = run_device(x, ops, tables, weights, n_slots=12)
    check_exact(got, x, ops, tables, "thresholds")
    assert (got[:, 0:4] == 1.0).all(), "a wrap counted twice, or a point missed, where a row of the disc closes the circle"
    assert any((2 * h[h >= 0] + 1 >= W).any() and (2 * h[h >= 0] + 1 < W).any() for _, h in tables[1:3]), "closed and open rows in one table"
    assert (got[1, 4:8] == 0.0).all() and got[0, 4, 4, 5] > 0 and (got[0, 7] == np.float32(1 / (H * W))).all()      # strict >
    assert (got[:, 8] == 0.0).all() and (got[:, 9] == 1.0).all() and (got[:, 10] == 0.0).all() and (got[:, 11] == 1.0).all()


@pytest.mark.parametrize("value", [np.nan, np.inf], ids=["nan", "inf"])
@pytest.mark.parametrize("where", ["mid", "pole", "col0"])
def test_a_non_finite_value_stays_in_the_discs_that_hold_it(where, value):
    H, W = 9, 12
    lat, lon, tables, weights = setup(H, W)
    clean = R.case(2, C, H, W, seed=11)
    base = run_device(clean, program(), tables, weights)
    j, i = {"mid": (4, 7), "pole": (0, 5), "col0": (3, 0)}[where]
    x = clean.copy()
    x[1, 0, j, i] = value
    got = run_device(x, program(), tables, weights)
    check_exact(got, x, program(), tables, f"{where} {value}")
    check_mean(got, x, program(), tables, weights)
    assert_bit_equal(got[0], base[0], "the other member")
    for op in program():
        changed = bits(got[1, op.out]) != bits(base[1, op.out])
        holds = R.table_sets(*tables[op.radius], W)[:, :, j, i]          # the points whose disc holds the planted node
        if op.channel != 0:
            assert not changed.any(), f"slot {op.out} reads another channel"
            continue
        assert not (changed & ~holds).any(), f"slot {op.out}: a value changed outside the discs that hold the planted node"
        if np.isnan(value) or op.kind == N.MEAN:
            assert np.isnan(got[1, op.out][holds]).all() and not np.isnan(got[1, op.out][~holds]).any()
        else:                                                            # an infinity compares as a number
            assert not np.isnan(got[1, op.out]).any()
            if op.kind == N.MAX:
                assert (got[1, op.out][holds] == np.inf).all()


def test_two_runs_give_the_same_bits():
    lat, lon, tables, weights = setup(19, 50)
    x = R.case(3, C, 19, 50, seed=5)
    assert_bit_equal(run_device(x, program(), tables, weights), run_device(x, program(), tables, weights), "second run")


def test_full_size_max_and_fraction_at_100_km():
    H, W = 721, 1440
    lat, lon = R.grid(H, W)
    tables, weights = [N.discs(lat, lon, 100.0)], area_weights(lat)
    rng = np.random.default_rng(721)
    x = rng.uniform(0.0, 30.0, (2, 1, H, W)).astype(np.float32) + np.float32(0.5)
    ops = [N.Op(N.MAX, 0, 0, 0), N.Op(N.FRAC_ABOVE, 0, 1, 0, 25.0)]
    got = run_device(x, ops, tables, weights, n_slots=2)
    check_exact(got, x, ops, tables, "721 x 1440")
