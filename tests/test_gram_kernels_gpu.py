"""``torch.ops.skyrim_hip.gram`` against the float64 restatement of include/skyrim_gram.h (tests/_scenario_reference.py), entry by entry
within the header's bound, over member counts on both sides of the one-block / three-block switch, tile tails, rows on both sides of the
workgroup cap, regions that wrap, channel lists and a misaligned member; that the bound has teeth; bitwise symmetry and reproducibility;
the untouched parts of the output buffer and of the workspace; non-finite inputs; ``member_combine`` bit-equal to its fp32 restatement;
and one full-size case.  The header puts products that underflow fp32 outside the bound, so the smallest channel here is 1e-12, not
the 1e-30 of the point tests."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import _scenario_reference as R
from skyrim_amd import ensemble as E
from skyrim_amd import scenarios as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
C = 3
TILE = S.TILE


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def field(M, H, W, seed, c=C):
    """(M, c, H, W) float32 of mixed magnitude: a temperature, a geopotential, a tiny humidity, winds of both signs."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((M, c, H, W), dtype=np.float32)
    scale = np.array([250.0, 54000.0, 1e-12, 25.0, 8.0, 1e-3] * 8)[:c]
    shift = np.array([250.0, 5e4, 0.0, 0.0, -3.0, 5e-3] * 8)[:c]
    x *= scale.astype(np.float32)[None, :, None, None]
    x += shift.astype(np.float32)[None, :, None, None]
    return x


def upload(x, misalign=None):
    """The members as device tensors; member ``misalign`` starts 4 bytes past a 16-byte boundary."""
    members = []
    for m, s in enumerate(x):
        if m == misalign:
            flat = torch.empty(s.size + 1, dtype=torch.float32, device=DEV)
            t = flat[1:].view(s.shape)
            assert t.data_ptr() % 16 == 4
        else:
            t = torch.empty(s.shape, dtype=torch.float32, device=DEV)
        t.copy_(torch.from_numpy(np.ascontiguousarray(s)))
        members.append(t)
    return members


def weights(H, seed=0):
    """Positive weights of different sizes, like the areas of latitude rows."""
    return np.random.default_rng(1000 + seed).uniform(0.05, 1.0, H)


def run_gram(members, truth, channels, region, w, gap=3):
    """(nc, M', M') of one call.  The output buffer starts as 0xAB bytes with a 64-byte head, ``gap`` doubles between the matrices and a
    256-byte tail, the workspace has a 256-byte tail: all of them must still hold 0xAB."""
    M, nc = len(members), len(channels)
    Mp = M + (truth is not None)
    stride = Mp * Mp + gap
    raw = torch.full((64 + nc * stride * 8 + 256,), 0xAB, dtype=torch.uint8, device=DEV)
    out = raw[64:64 + nc * stride * 8].view(torch.float64).view(nc, stride)
    need = S.workspace_bytes(Mp, nc, region[1], region[3])
    assert need > 0
    ws_raw = torch.full((need + 256,), 0xAB, dtype=torch.uint8, device=DEV)
    torch.ops.skyrim_hip.gram(members, E.member_table(members), truth, list(channels), list(region), torch.from_numpy(w).to(DEV), out,
                              ws_raw[:need])
    torch.cuda.synchronize()
    host, ws = raw.cpu().numpy(), ws_raw.cpu().numpy()
    assert (host[:64] == 0xAB).all() and (host[64 + nc * stride * 8:] == 0xAB).all(), "head or tail of the output buffer written"
    body = host[64:64 + nc * stride * 8].reshape(nc, stride * 8)
    assert (body[:, Mp * Mp * 8:] == 0xAB).all(), "the gap between two matrices written"
    assert (ws[need:] == 0xAB).all(), "the workspace written beyond workspace_bytes"
    return body[:, :Mp * Mp * 8].copy().view(np.float64).reshape(nc, Mp, Mp)


def check(x, y, channels, region, seed=0, misalign=None):
    """One call against the float64 reference within the header's bound, entry by entry; symmetric bit for bit."""
    H = x.shape[2]
    w = weights(H, seed)
    members = upload(x, misalign)
    truth = None if y is None else upload([y])[0]
    got = run_gram(members, truth, channels, region, w)
    want, Sabs = R.gram(list(x), y, channels, region, w)
    err, lim = np.abs(got - want), S.bound_factor() * Sabs
    assert np.isfinite(got).all()
    assert (err <= lim).all(), f"worst entry at {float((err / np.maximum(lim, 1e-300)).max()):.3f} of the bound"
    assert np.array_equal(got.view(np.uint64), np.transpose(got, (0, 2, 1)).copy().view(np.uint64)), "not bitwise symmetric"
    assert not got[:, 0].any() and not got[:, :, 0].any()                      # d_0 is exactly 0
    return got


# M on both sides of 32 (one block / three blocks), with and without the truth column where M' <= 64
@pytest.mark.parametrize("M,truth", [(2, False), (2, True), (3, False), (3, True), (31, False), (31, True), (32, False), (32, True), (33, False),
                                     (33, True), (50, False), (50, True), (63, False), (63, True), (64, False)])
def test_member_counts_with_and_without_truth(M, truth):
    H, W = 5, TILE + 1
    x = field(M + 1, H, W, seed=M)
    check(x[:M], x[M] if truth else None, [1, 0], (0, H, 0, W), seed=M)


# tile tails in W, more rows than workgroups (H = 300 and 600 at W = 8: 300 and 600 tiles for at most 512 workgroups) and fewer
@pytest.mark.parametrize("H,W", [(5, TILE - 1), (5, TILE), (1, TILE + 1), (5, 8), (5, 70), (1, 8), (300, 8), (600, 8), (3, 2 * TILE + 70)])
@pytest.mark.parametrize("M", [5, 40])
def test_grid_sizes_and_tile_tails(H, W, M):
    x = field(M + 1, H, W, seed=H + W)
    check(x[:M], x[M], [2, 1, 0], (0, H, 0, W), seed=W)


@pytest.mark.parametrize("region", ["one column", "all columns from the middle", "wrap", "rows", "one point", "wrap over a tile"])
def test_regions(region):
    H, W = 7, 300
    reg = {"one column": (0, H, 17, 1), "all columns from the middle": (0, H, 123, W), "wrap": (2, 3, W - 1, 40), "rows": (4, 3, 0, W),
           "one point": (6, 1, W - 1, 1), "wrap over a tile": (1, 5, 250, 299)}[region]
    for M in (4, 37):
        x = field(M + 1, H, W, seed=len(region))
        check(x[:M], x[M], [0, 2], reg, seed=3)


def test_channel_lists_a_repeated_channel_and_a_misaligned_member():
    H, W, M = 5, 70, 6
    x = field(M + 1, H, W, seed=9, c=6)
    one = check(x[:M], x[M], [4], (1, 3, 60, 30))
    three = check(x[:M], x[M], [4, 0, 4], (1, 3, 60, 30))
    assert np.array_equal(three[0], one[0]) and np.array_equal(three[2], one[0])          # the same channel: the same bits
    mis = check(x[:M], x[M], [4, 0, 4], (1, 3, 60, 30), misalign=3)
    assert np.array_equal(mis, three)                                          # alignment changes no operation
    big = field(41, H, W, seed=10, c=6)
    assert np.array_equal(check(big[:40], big[40], [5, 3], (0, H, 0, W), misalign=0), check(big[:40], big[40], [5, 3], (0, H, 0, W)))


def test_the_bound_has_teeth():
    """4096 points: the reference with ONE region point left out lies outside the bound of the device result, on every diagonal entry
    of every member but 0.  That this is a property of the inputs is checked on the reference alone first."""
    H, W, M = 16, 256, 34
    x = field(M, H, W, seed=77)
    j, i = 9, 131                                                              # the point left out: every member four sigmas from member 0 there
    x[1:, :, j, i] = x[0, :, j, i] + 4 * x.std(axis=(0, 2, 3))
    w = weights(H, 5)
    region = (0, H, 0, W)
    want, Sabs = R.gram(list(x), None, [0, 1], region, w)
    dropped = []
    for cc, c in enumerate([0, 1]):
        d = R.differences(list(x), None, c, region)
        dropped.append(want[cc] - w[j] * np.outer(d[:, j, i], d[:, j, i]))
    dropped = np.stack(dropped)
    lim = S.bound_factor() * Sabs
    diag = np.arange(1, M)
    assert (np.abs(want - dropped)[:, diag, diag] > 3 * lim[:, diag, diag]).all()          # the reference alone: beyond three bounds
    got = run_gram(upload(x), None, [0, 1], region, w)
    assert (np.abs(got - want) <= lim).all()
    assert (np.abs(got - dropped)[:, diag, diag] > lim[:, diag, diag]).all()


def test_two_calls_give_the_same_bits():
    for M, H, W in ((50, 40, 300), (7, 600, 8)):
        x = field(M + 1, H, W, seed=21)
        members, truth, w = upload(x[:M]), upload([x[M]])[0], weights(H)
        a = run_gram(members, truth, [0, 1, 2], (0, H, 0, W), w)
        b = run_gram(members, truth, [0, 1, 2], (0, H, 0, W), w)
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64))


@pytest.mark.parametrize("M", [5, 40])
def test_non_finite_values_reach_exactly_their_rows_and_columns(M):
    H, W = 5, 300
    x = field(M + 1, H, W, seed=31)
    w = weights(H)
    region = (1, 3, 290, 50)
    clean = run_gram(upload(x[:M]), upload([x[M]])[0], [0, 1], region, w)
    bad = x.copy()
    a, b = 2, M - 1                                                            # (M = 40: one in each operand half)
    bad[a, 0, 2, 5] = np.nan
    bad[b, 0, 3, 295] = np.inf
    bad[M, 0, 1, 0] = -np.inf                                                  # the truth: column M
    bad[1, 0, 0, 7] = np.nan                                                   # outside the region: no effect
    bad[1, 0, 2, 100] = np.nan
    got = run_gram(upload(bad[:M]), upload([bad[M]])[0], [0, 1], region, w)
    hit = np.zeros((M + 1, M + 1), bool)
    for m in (a, b, M):
        hit[m, :] = hit[:, m] = True
    assert not np.isfinite(got[0][hit]).any() and np.isfinite(got[0][~hit]).all()
    assert np.array_equal(got[0][~hit], clean[0][~hit])                        # every other entry: the same bits
    assert np.array_equal(got[1].view(np.uint64), clean[1].view(np.uint64))    # no other channel is touched
    zero = x.copy()
    zero[0, 1, 2, 20] = np.inf                                                 # member 0: every difference of the channel
    got = run_gram(upload(zero[:M]), upload([zero[M]])[0], [0, 1], region, w)
    assert not np.isfinite(got[1]).any() and np.array_equal(got[0].view(np.uint64), clean[0].view(np.uint64))


# ---- member_combine ---------------------------------------------------------------------------------------------------------------------- #
def run_combine(members, channels, coef, b):
    K, nc = coef.shape[0], len(channels)
    _, H, W = members[0].shape
    n = K * nc * H * W
    raw = torch.full((64 + n * 4 + 256,), 0xAB, dtype=torch.uint8, device=DEV)
    out = raw[64:64 + n * 4].view(torch.float32).view(K, nc, H, W)
    torch.ops.skyrim_hip.member_combine(members, E.member_table(members), list(channels), torch.from_numpy(coef).to(DEV),
                                        torch.from_numpy(b).to(DEV), out)
    torch.cuda.synchronize()
    host = raw.cpu().numpy()
    assert (host[:64] == 0xAB).all() and (host[64 + n * 4:] == 0xAB).all(), "head or tail of the output buffer written"
    return host[64:64 + n * 4].copy().view(np.float32).reshape(K, nc, H, W)


@pytest.mark.parametrize("K", [1, 8])
@pytest.mark.parametrize("M", [2, 50])
@pytest.mark.parametrize("H,W", [(5, 70), (3, TILE + 1), (2, TILE)])
def test_member_combine_equals_its_restatement_bit_for_bit(K, M, H, W):
    x = field(M, H, W, seed=K + M)
    rng = np.random.default_rng(K * 100 + M)
    coef = rng.normal(0, 0.5, (K, M)).astype(np.float32)
    members = upload(x, misalign=1)
    for b in (np.zeros(K, np.float32), np.ones(K, np.float32), rng.normal(0, 1, K).astype(np.float32)):
        got = run_combine(members, [2, 0, 2], coef, b)
        want = R.combine(list(x), [2, 0, 2], coef, b)
        assert not np.any(bits(got) != bits(want))
    if K == 1:                                                                 # b = 1, coefficients 0: a bit copy of member 0
        got = run_combine(members, [1], np.zeros((1, M), np.float32), np.ones(1, np.float32))
        assert not np.any(bits(got[0, 0]) != bits(x[0, 1]))


def test_member_combine_other_counts_and_a_non_finite_value():
    H, W, M = 4, 130, 11
    x = field(M, H, W, seed=5)
    x[3, 0, 1, 7] = np.nan
    members = upload(x)
    rng = np.random.default_rng(8)
    for K in (2, 3, 5, 7):
        coef, b = rng.normal(0, 1, (K, M)).astype(np.float32), rng.normal(0, 1, K).astype(np.float32)
        got, want = run_combine(members, [0, 1], coef, b), R.combine(list(x), [0, 1], coef, b)
        assert np.isnan(got[:, 0, 1, 7]).all() and np.isfinite(np.delete(got.reshape(K, -1), 1 * W + 7, axis=1)).all()
        assert not np.any(bits(np.nan_to_num(got)) != bits(np.nan_to_num(want)))


# ---- full size --------------------------------------------------------------------------------------------------------------------------- #
def test_full_size_within_the_bound():
    """721 x 1440, 50 members, one channel of a one-channel state: 4326 tiles on 512 workgroups, three blocks."""
    H, W, M = 721, 1440, 50
    rng = np.random.default_rng(2024)
    base = rng.standard_normal((H, W), dtype=np.float32) * np.float32(500.0) + np.float32(54000.0)
    members = []
    d = np.empty((M, H * W), np.float64)
    for m in range(M):
        xm = base + rng.standard_normal((H, W), dtype=np.float32) * np.float32(40.0) if m else base
        t = torch.from_numpy(xm[None]).to(DEV)
        members.append(t)
        d[m] = (xm - base).astype(np.float32).reshape(-1)                      # the fp32 difference, exactly as the header states it
    from skyrim_amd.verify import area_weights
    w = area_weights(np.linspace(90.0, -90.0, H))
    got = run_gram(members, None, [0], (0, H, 0, W), w, gap=0)[0]
    wp = np.repeat(w, W)
    want = (d * wp) @ d.T
    np.abs(d, out=d)
    Sabs = (d * wp) @ d.T
    err, lim = np.abs(got - want), S.bound_factor() * Sabs
    assert (err <= lim).all(), f"worst entry at {float((err / np.maximum(lim, 1e-300)).max()):.3f} of the bound"
    assert np.array_equal(got, got.T) and got[1, 1] > 0
