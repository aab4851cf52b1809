"""``torch.ops.skyrim_hip.point_gather`` against the float32 restatement of include/skyrim_point.h (tests/_point_reference.py): every output
bit-equal, over grids, point counts, member counts and channel lists that reach every tail of the kernel; the untouched parts of the
output buffer; the order of the records; non-finite inputs; the nodes of a regrid target against ``torch.ops.skyrim_hip.regrid``; and one
full-size case, also within the header's bound of float64.  Only records ``skpoint_validate`` accepts go to the device: the kernel's
clamps are read in the code, not provoked."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import _point_reference as R
from skyrim_amd import ensemble as E
from skyrim_amd import points as P
from skyrim_amd import regrid as G

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
C = 6


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def field(M, H, W, seed, c=C):
    """(M, c, H, W) float32 of mixed magnitude: a temperature, a geopotential, winds of both signs, a tiny humidity."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((M, c, H, W), dtype=np.float32)
    scale = np.array([250.0, 54000.0, 25.0, 8.0, 1e-3, 1e-30, 1e5, 3.0, 0.02] * 8)[:c]
    shift = np.array([250.0, 5e4, 0.0, 0.0, 5e-3, 0.0, 1e5, -3.0, 0.0] * 8)[:c]
    x *= scale.astype(np.float32)[None, :, None, None]
    x += shift.astype(np.float32)[None, :, None, None]
    return x


def random_records(H, W, n, seed):
    """n validated records: all four (nr, ncol) combinations, weights of both signs and mixed size; the first ones are the edge cases
    col = W - 1 with two taps (the wrap), row = H - 2 with two taps, row = H - 1 with one."""
    rng = np.random.default_rng(seed)
    rec = np.zeros(n, R.REC)
    rec["nr"], rec["ncol"] = rng.integers(1, 3, n), rng.integers(1, 3, n)
    if H == 1:
        rec["nr"] = 1
    rec["row"] = np.where(rec["nr"] == 2, rng.integers(0, max(H - 1, 1), n), rng.integers(0, H, n))
    rec["col"] = rng.integers(0, W, n)
    for k in ("wr0", "wr1", "wc0", "wc1"):
        w = rng.normal(0, 0.6, n).astype(np.float32) + np.float32(0.25)
        w[w == 0] = 0.5
        rec[k] = w
    rec["wr0"][::5], rec["wc0"][::7] = 1.0, 1.0
    edge = [(0, W - 1, 1, 2), (H - 2, 0, 2, 1), (H - 1, W - 1, 1, 2), (H - 2, W - 1, 2, 2), (H - 1, 0, 1, 1)]
    for i, (r, c, a, b) in enumerate(edge[:n]):
        rec["row"][i], rec["col"][i], rec["nr"][i], rec["ncol"][i] = r, c, a, b
    rec["wr1"][rec["nr"] == 1] = 0.0
    rec["wc1"][rec["ncol"] == 1] = 0.0
    P.validate_records(rec, H, W)                                           # nothing else goes to the device
    return rec


def run_op(x, channels, rec, misalign=False, gap=0):
    """(M, nc, P) of one gather.  The output buffer starts as 0xAB bytes, each member's part is ``gap`` elements longer than nc P and a
    256-byte tail follows: gap and tail must still hold 0xAB."""
    members = []
    for s in x:
        if misalign:
            flat = torch.empty(s.size + 1, dtype=torch.float32, device=DEV)
            t = flat[1:].view(s.shape)
            assert t.data_ptr() % 16 == 4
        else:
            t = torch.empty(s.shape, dtype=torch.float32, device=DEV)
        t.copy_(torch.from_numpy(np.ascontiguousarray(s)))
        members.append(t)
    M, nc, n = len(members), len(channels), rec.size
    stride = nc * n + gap
    raw = torch.full((M * stride * 4 + 256,), 0xAB, dtype=torch.uint8, device=DEV)
    out = raw[:M * stride * 4].view(torch.float32).view(M, stride)
    torch.ops.skyrim_hip.point_gather(members, E.member_table(members), list(channels), P.device_records(rec, DEV), out)
    torch.cuda.synchronize()
    host = raw.cpu().numpy()
    assert np.all(host[M * stride * 4:] == 0xAB), "bytes beyond the buffer were touched"
    per = host[:M * stride * 4].reshape(M, stride * 4)
    assert np.all(per[:, nc * n * 4:] == 0xAB), "the gap between the members' parts was touched"
    return per[:, :nc * n * 4].copy().view(np.float32).reshape(M, nc, n)


def assert_bits(got, ref, what):
    bad = bits(got) != bits(ref)
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4].tolist())


@pytest.mark.parametrize("H,W", [(3, 4), (5, 132), (7, 50), (33, 64)])
@pytest.mark.parametrize("M", [1, 3])
def test_bit_equal_over_grids_point_counts_and_channel_lists(H, W, M):
    x = field(M, H, W, 7 * H + M)
    for n in (1, 63, 64, 65, 257, 1000):
        rec = random_records(H, W, n, n + W)
        if n >= 64:
            assert {(a, b) for a, b in zip(rec["nr"].tolist(), rec["ncol"].tolist())} == {(1, 1), (1, 2), (2, 1), (2, 2)}
            assert np.any((rec["col"] == W - 1) & (rec["ncol"] == 2)) and np.any((rec["row"] == H - 2) & (rec["nr"] == 2))
            assert np.any((rec["row"] == H - 1) & (rec["nr"] == 1))
        channels = {1: [4], 63: [5, 4, 3, 2, 1, 0], 64: [2, 2, 0], 65: list(range(C)), 257: [3], 1000: [1, 5]}[n]
        got = run_op(x, channels, rec, misalign=(n % 2 == 1), gap=(3 if n != 64 else 0))
        assert_bits(got, R.gather(x, channels, rec), (H, W, M, n))


def test_more_channels_than_a_chunk_with_repeats_and_reversed_order():
    H, W, M = 7, 50, 2
    x = field(M, H, W, 3)
    rec = random_records(H, W, 300, 11)
    for channels in ([5, 4, 3, 2, 1, 0] * 3 + [0],                        # 19: two full chunks and a tail of three
                     list(range(C)) + [0, 1, 2],                          # 9: one chunk and one channel
                     [2] * P.CHUNK, [1] * (P.CHUNK + 1), list(range(C))[::-1] + [3, 3, 3, 3, 3, 3, 3]):
        assert len(channels) >= P.CHUNK
        got = run_op(x, channels, rec, misalign=True, gap=5)
        assert_bits(got, R.gather(x, channels, rec), len(channels))
    full = run_op(x, list(range(C)), rec)
    part = run_op(x, [3, 0, 3, 4], rec)
    assert_bits(part, full[:, [3, 0, 3, 4]], "subset")


def test_the_order_of_the_records_does_not_change_a_point():
    H, W, M = 33, 64, 3
    x = field(M, H, W, 5)
    rec = random_records(H, W, 777, 9)
    base = run_op(x, [0, 3, 5], rec)
    srt = np.lexsort((rec["col"], rec["row"]))
    rng = np.random.default_rng(1)
    for what, order in (("sorted", srt), ("reversed", srt[::-1].copy()), ("shuffled", rng.permutation(rec.size))):
        got = run_op(x, [0, 3, 5], rec[order])
        assert_bits(got, base[:, :, order], what)


def test_non_finite_inputs_reach_exactly_the_points_that_read_them():
    H, W, M = 7, 50, 2
    x = field(M, H, W, 8)
    x[1, 1, 2, 10], x[0, 1, 5, 0], x[1, 1, 0, 7] = np.inf, -np.inf, -0.0
    x.view(np.uint32)[0, 1, 3, 49] = 0x7FC12345                            # a quiet NaN with a payload
    rec = random_records(H, W, 600, 13)
    single = np.zeros(4, R.REC)
    for i, (r, c) in enumerate([(3, 49), (2, 10), (5, 0), (0, 7)]):
        single[i] = (r, c, 1, 1, 1.0, 0.0, 1.0, 0.0)
    rec = np.concatenate([single, rec])
    P.validate_records(rec, H, W)
    got = run_op(x, [1, 0], rec)
    ref = R.gather(x, [1, 0], rec)
    # single taps of weight 1 copy the bits: the NaN's payload, the infinities, the sign of zero
    for i, (m, r, c) in enumerate([(0, 3, 49), (1, 2, 10), (0, 5, 0), (1, 0, 7)]):
        assert bits(got[m, 0, i]) == bits(x[m, 1, r, c]), i
    assert bits(got[0, 0, 0]) == 0x7FC12345 and bits(got[1, 0, 3]) == 0x80000000
    # which taps a point reads
    row, row1, col, col1, two_r, two_c = R._taps(rec, H, W)
    for m, (r, c) in ((0, (3, 49)),):
        reads = ((row == r) | (two_r & (row1 == r))) & ((col == c) | (two_c & (col1 == c)))
        assert reads.sum() >= 1 and np.array_equal(np.isnan(got[m, 0]), reads)
        assert not np.isnan(got[m, 1]).any() and not np.isnan(got[1 - m]).any()
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan)
    assert not np.any((bits(got) != bits(ref)) & ~nan)                      # (two NaN operands: the payload that survives is the hardware's)


def nodes(dlat, dlon):
    return P.Points([(f"n{j}_{i}", la, lo) for j, la in enumerate(dlat) for i, lo in enumerate(dlon)])


@pytest.mark.parametrize("method", ["bilinear", "nearest"])
def test_nodes_of_a_regrid_target_equal_regridding_bit_for_bit(method):
    H, W, M = 33, 64, 3
    lat, lon = np.linspace(90.0, -90.0, H), np.arange(W) * (360.0 / W)
    dlat, dlon = G.target_grid(7.5, lat, lon)                                # the "1.5deg" construction, scaled: 25 x 48 nodes
    dlon = np.mod(dlon + 1.0, 360.0)                                         # off the source columns: two column taps
    assert (dlat.size, dlon.size) == (25, 48)
    t = G.tables(lat, lon, dlat, dlon, method)
    x = field(M, H, W, 21)
    members = [torch.from_numpy(s).to(DEV) for s in x]
    out = torch.empty((M, 3, dlat.size, dlon.size), dtype=torch.float32, device=DEV)
    torch.ops.skyrim_hip.regrid(members, E.member_table(members), [4, 0, 2], *t.on(DEV), out)
    rec = P.records(nodes(dlat, dlon), lat, lon, method)
    if method == "bilinear":
        assert set(rec["nr"].tolist()) == {1, 2} and set(rec["ncol"].tolist()) == {2}
    got = run_op(x, [4, 0, 2], rec)
    assert_bits(got, out.cpu().numpy().reshape(M, 3, -1), method)
    assert_bits(got, R.gather(x, [4, 0, 2], rec), method + " restatement")


def test_full_size_bit_equal_and_within_the_bound():
    H, W, Cf, M, n = 721, 1440, 69, 2, 4096
    rng = np.random.default_rng(4)
    x = field(M, H, W, 2, c=Cf)
    lat, lon = np.linspace(90.0, -90.0, H), np.arange(W) * 0.25
    pts = P.Points([(f"s{i}", la, lo) for i, (la, lo) in enumerate(zip(rng.uniform(-90, 90, n), rng.uniform(-180, 360, n)))])
    rec = P.records(pts, lat, lon)
    channels = [68, 0, 33, 12, 12, 50, 7, 1]
    got = run_op(x, channels, rec, gap=1)
    assert_bits(got, R.gather(x, channels, rec), "full size")
    exact, S = R.gather64(x, channels, rec)
    share = np.abs(got.astype(np.float64) - exact) / R.bound(rec, S)
    print(f"full size: worst share of the bound {share.max():.3f}")
    assert share.max() <= 1.0
