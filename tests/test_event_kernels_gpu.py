"""``event_counts`` at its edges on the MI355X (include/skyrim_event.h) against the numpy restatement on the same float32 inputs.  Every
output is an integer: joint counts, the uint8 planes and the neighbourhood sums are compared with ``np.array_equal``, and whatever was
not requested must still hold the sentinel the buffers were filled with."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import _event_reference as R
from skyrim_amd import events as E

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
hip = torch.ops.skyrim_hip
T = E.MAX_THRESHOLDS
S_COUNT, S_PLANE, S_SUM = -7, 0xAB, -99
SHAPES = [(1, 1, 1), (2, 2, 7), (5, 7, 333), (1, 3, 4097), (3, 49, 192)]
COUNTS = [1, 2, 7, 8, 9, 33, 50, 64]
LATTICE = [0.25, -0.5, 1.0, 0.0]                                  # thresholds ON the lattice of R.case: equal values occur


def _run(x, y, channels, thresholds, hy=(), hx=None, shift=0):
    """One event_counts call -> (counts (E, 4, H, 2, M + 1), planes (E, 4, 2, H, W) uint8, sums (E, 4, S, H, 3)); every buffer is
    pre-filled with its sentinel.  ``shift``: members start that many floats into their allocation (1: the 4-byte path)."""
    from skyrim_amd.ensemble import member_table
    M, C, H, W = x.shape
    En, S = len(channels), len(hy)
    mem = []
    for m in range(M):
        buf = torch.empty(C * H * W + shift, dtype=torch.float32, device=DEV)
        buf[shift:].copy_(torch.from_numpy(x[m]).reshape(-1))
        mem.append(buf[shift:].view(C, H, W))
    counts = torch.full((En, T, H, 2, M + 1), S_COUNT, dtype=torch.int32, device=DEV)
    planes = torch.full((En * T * 2 * H * W,), S_PLANE, dtype=torch.uint8, device=DEV) if S else None
    sums = torch.full((En, T, S, H, 3), S_SUM, dtype=torch.int64, device=DEV) if S else None
    hxd = torch.from_numpy(np.ascontiguousarray(hx, np.int32)).to(DEV) if S else None
    hip.event_counts(mem, member_table(mem), torch.from_numpy(y).to(DEV), list(channels), [len(t) for t in thresholds],
                     [float(v) for t in thresholds for v in t], counts, list(hy), hxd, sums, planes)
    torch.cuda.synchronize()
    return (counts.cpu().numpy(), planes.cpu().numpy().reshape(En, T, 2, H, W) if S else None, sums.cpu().numpy() if S else None)


def _expect(x, y, channels, thresholds, hy=(), hx=None):
    M, C, H, W = x.shape
    En, S = len(channels), len(hy)
    counts = np.full((En, T, H, 2, M + 1), S_COUNT, np.int32)
    planes = np.full((En, T, 2, H, W), S_PLANE, np.uint8)
    sums = np.full((En, T, S, H, 3), S_SUM, np.int64)
    for e, (ch, thr) in enumerate(zip(channels, thresholds)):
        for t, v in enumerate(thr):
            k, o = R.point_counts(x[:, ch], y[ch], v)
            counts[e, t] = R.joint_counts(k, o, M)
            planes[e, t, 0], planes[e, t, 1] = k, o
            for s in range(S):
                sums[e, t, s], _ = R.row_sums(k, o, M, hy[s], np.asarray(hx)[s])
    return counts, planes, sums


def _check(x, y, channels, thresholds, hy=(), hx=None, shift=0, what=""):
    got = _run(x, y, channels, thresholds, hy, hx, shift)
    want = _expect(x, y, channels, thresholds, hy, hx)
    assert np.array_equal(got[0], want[0]), f"{what}: joint counts"
    if len(hy):
        assert np.array_equal(got[1], want[1]), f"{what}: uint8 planes"
        assert np.array_equal(got[2], want[2]), f"{what}: neighbourhood sums"
    H, W = x.shape[2:]
    for e, thr in enumerate(thresholds):
        assert np.all(got[0][e, :len(thr)].sum(axis=(1, 2, 3)) == H * W)
    return got


def _hx(H, W, seed):
    """A row-varying table with entries below 0 and beyond the clamp."""
    rng = np.random.default_rng(seed)
    hx = rng.integers(0, max(2, min(W, 12)), size=H)
    hx[0], hx[-1] = W + 5, -3
    return hx.astype(np.int32)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("M", COUNTS)
def test_counts_planes_and_sums_match_the_restatement(M, shape):
    C, H, W = shape
    x, y = R.case(M, shape, seed=100 * M + C)
    channels = list(range(C))[::-1]                                # every channel, last first
    thresholds = [LATTICE[:1 + (c + M) % T] for c in channels]     # 1 to 4 thresholds, on the lattice
    _check(x, y, channels, thresholds, what=f"M={M} {shape} counts alone")
    hx = np.stack([np.zeros(H, np.int32), _hx(H, W, M)])
    _check(x, y, channels, thresholds, hy=(0, 1), hx=hx, what=f"M={M} {shape} with scales")


def test_full_size_grid_with_fifty_members():
    """(2, 721, 1440) at M = 50 with the windows of 0 and 100 km: more than one pass of a workgroup over a row, every row of a real grid."""
    M, shape = 50, (2, 721, 1440)
    x, y = R.case(M, shape, seed=50)
    lat, lon = np.linspace(90, -90, 721), np.arange(1440) * 0.25
    win = [E.windows(lat, lon, r) for r in (0.0, 100.0)]
    got = _check(x, y, [1, 0], [[0.25, 1.5], [3.0]], hy=[w[0] for w in win], hx=np.stack([w[1] for w in win]), what="721 x 1440, M = 50")
    assert np.array_equal(_run(x, y, [1, 0], [[0.25, 1.5], [3.0]])[0], got[0])            # without planes: the same counts


@pytest.mark.parametrize("M", [1, 9, 50])
def test_equal_values_nan_and_infinite_thresholds(M):
    shape = (3, 7, 333)
    x, y = R.case(M, shape, seed=M)
    thr = np.float32(0.75)
    x[M // 2, 1, 2, ::5] = thr                                     # members and truth EQUAL to the threshold: not above it
    y[1, 3, ::7] = thr
    x[0, 1, 4, 10] = np.nan                                        # a NaN compares false: never above
    y[1, 4, 11] = np.nan
    x[M - 1, 1, 5, 20], y[1, 5, 21] = np.inf, -np.inf
    inf = float("inf")
    got = _check(x, y, [1, 0], [[0.75, -inf, inf], [inf, -inf, 0.0, 0.75]], hy=(1,), hx=_hx(7, 333, M)[None], what=f"M={M} edge values")
    counts = got[0]
    assert counts[1, 0, :, 0, 0].sum() == 7 * 333 and counts[1, 0].sum() == 7 * 333      # +inf: every point in bin (0, 0)
    assert counts[1, 1, :, 1, M].sum() == 7 * 333                                        # -inf on clean data: every point in bin (1, M)
    assert counts[0, 1, :, 1, M].sum() == 7 * 333 - 3                                    # the NaN member, the NaN truth and -inf leave it
    k, o = R.point_counts(x[:, 1], y[1], 0.75)
    assert o[3, 0] == 0 and k[2, 0] < M                            # (the restatement itself: equal is not above)


def test_channel_lists_subset_unordered_and_sixteen():
    M, shape = 7, (5, 7, 333)
    x, y = R.case(M, shape, seed=16)
    _check(x, y, [3], [[0.25]], what="one channel of five")
    _check(x, y, [4, 1, 2], [[0.0, 1.0], [0.25], [-0.5, 0.5, 1.0, 1.5]], hy=(2,), hx=_hx(7, 333, 1)[None], what="a subset, unordered")
    channels = [(3 * i) % 5 for i in range(16)]                    # sixteen event channels (repeats are allowed)
    thresholds = [[0.25 * (i % 5) - 0.5] + LATTICE[:i % T] for i in range(16)]
    _check(x, y, channels, thresholds, hy=(1,), hx=_hx(7, 333, 2)[None], what="sixteen event channels")


@pytest.mark.parametrize("M", [1, 8, 50])
@pytest.mark.parametrize("shape", [(2, 49, 192), (2, 5, 1028)], ids=["49x192", "5x1028"])
def test_scalar_path_equals_vector_path(M, shape):
    x, y = R.case(M, shape, seed=7 * M)
    H, W = shape[1:]
    args = ([1, 0], [[0.25, 1.0], [0.0]], (1, 0), np.stack([_hx(H, W, 3), np.zeros(H, np.int32)]))
    vec = _check(x, y, *args, what=f"M={M} 16-byte aligned members")
    sca = _check(x, y, *args, shift=1, what=f"M={M} members offset by one element")
    for a, b in zip(vec, sca):
        assert np.array_equal(a, b)


def test_what_was_not_requested_keeps_the_sentinel():
    M, shape = 9, (3, 5, 64)
    x, y = R.case(M, shape, seed=9)
    counts, planes, sums = _run(x, y, [2, 0], [[0.25], [0.0, 1.0, 2.0]], hy=(1,), hx=np.ones((1, 5), np.int32))
    assert np.all(counts[0, 1:] == S_COUNT) and np.all(counts[1, 3:] == S_COUNT) and np.all(counts[0, 0] >= 0) and np.all(counts[1, :3] >= 0)
    assert np.all(planes[0, 1:] == S_PLANE) and np.all(planes[1, 3:] == S_PLANE) and np.all(planes[1, :3, 0] <= M) and np.all(planes[:, 0, 1] <= 1)
    assert np.all(sums[0, 1:] == S_SUM) and np.all(sums[1, 3:] == S_SUM) and np.all(sums[0, 0] >= 0)
    counts, planes, sums = _run(x, y, [2], [[0.25]])               # no scales: counts alone
    assert planes is None and sums is None and counts[0, 0].sum() == 5 * 64 and np.all(counts[0, 1:] == S_COUNT)


@pytest.mark.parametrize("case", ["point", "tall", "clamp_even", "clamp_odd", "one_column", "one_row", "windows", "four_scales", "widest"])
def test_scales(case):
    M = 5
    if case == "point":                                            # hy = hx = 0: the point itself
        shape, hy, hx = (1, 6, 40), (0,), np.zeros((1, 6), np.int32)
    elif case == "tall":                                           # hy >= H: every row, with hy = H, H + 3 and far beyond
        shape, hy, hx = (1, 6, 40), (6, 9, 10 ** 5), np.stack([_hx(6, 40, s) for s in range(3)])
    elif case == "clamp_even":                                     # hx beyond (W - 1) // 2 = 19: the circle once, one column short
        shape, hy, hx = (1, 4, 40), (1,), np.array([[19, 20, 21, 400]], np.int32)
    elif case == "clamp_odd":                                      # (W - 1) // 2 = 20: the whole circle
        shape, hy, hx = (1, 4, 41), (1,), np.array([[20, 21, 41, 2 ** 31 - 1]], np.int32)
    elif case == "one_column":
        shape, hy, hx = (2, 9, 1), (2, 0), np.array([[0, 1, 2, 3, 4, 5, 6, 7, 8], [0] * 9], np.int32)
    elif case == "one_row":
        shape, hy, hx = (2, 1, 333), (0, 3), np.array([[7], [166]], np.int32)
    elif case == "windows":                                        # the row-varying table of windows() on a global grid
        shape = (1, 49, 192)
        lat, lon = np.linspace(90, -90, 49), np.arange(192) * 1.875
        win = [E.windows(lat, lon, r) for r in (500.0, 1500.0)]
        hy, hx = [w[0] for w in win], np.stack([w[1] for w in win])
    elif case == "four_scales":
        shape, hy, hx = (2, 7, 333), (0, 1, 2, 7), np.stack([_hx(7, 333, s) for s in range(4)])
    else:                                                          # the widest grid the neighbourhood pass holds in LDS
        M, shape, hy, hx = 2, (1, 2, 8192), (1,), np.array([[4095, 3]], np.int32)
    C, H, W = shape
    x, y = R.case(M, shape, seed=len(case))
    channels, thresholds = list(range(C)), [[0.25, 1.0]] * C
    _, _, sums = _check(x, y, channels, thresholds, hy=hy, hx=hx, what=case)
    if case == "point":
        k, o = R.point_counts(x[:, 0], y[0], 0.25)
        assert np.array_equal(sums[0, 0, 0, :, 0], ((k - M * o) ** 2).sum(axis=1))


def test_an_event_on_the_date_line():
    """A block of observed events across the first and last columns, forecast two columns further east: windows must wrap."""
    M, H, W = 4, 5, 36
    y = np.zeros((1, H, W), np.float32)
    x = np.zeros((M, 1, H, W), np.float32)
    y[0, 1:4, [W - 2, W - 1, 0, 1]] = 1.0
    for m in range(M):
        x[m, 0, 1:4, [W - 1, 0, 1, 2 + (m % 2)]] = 1.0
    hx = np.array([[0] * H, [1] * H, [3] * H, [17] * H], np.int32)
    _, planes, sums = _check(x, y, [0], [[0.5]], hy=(0, 0, 1, 2), hx=hx, what="date line")
    assert planes[0, 0, 1, 2, W - 1] == 1 and planes[0, 0, 1, 2, 0] == 1 and planes[0, 0, 0, 2, 0] == M
    flipped = _run(np.roll(x, W // 2, axis=-1), np.roll(y, W // 2, axis=-1), [0], [[0.5]], hy=(0, 0, 1, 2), hx=hx)
    assert np.array_equal(flipped[2], sums)                        # the same event in mid-grid: the same sums
