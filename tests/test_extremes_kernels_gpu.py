"""The two kernels of include/skyrim_clim.h on the GPU against the numpy restatements of tests/_extremes_reference.py, bit for bit."""
import itertools
import math

import numpy as np
import pytest
import torch

import _extremes_reference as R
from skyrim_amd import climate as K
from skyrim_amd.members import member_table
from skyrim_amd.ops import hip

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GRIDS = [(1, 4), (3, 7), (5, 64), (9, 260)]
TAIL = 37                                    # floats behind every output: must stay 0xAB


def levels_of(Q):
    return np.linspace(0.0, 1.0, Q)


def upload_members(x, align):
    """x (M, C, H, W) -> M device tensors whose addresses are multiples of 16, or 4 bytes past one."""
    out = []
    for m in range(x.shape[0]):
        buf = torch.empty(x[m].size + 8, dtype=torch.float32, device=DEV)
        off = (-(buf.data_ptr() // 4) % 4 + (1 if align == 4 else 0))
        t = buf[off:off + x[m].size].view(x[m].shape)
        t.copy_(torch.from_numpy(x[m]))
        assert t.data_ptr() % 16 == (4 if align == 4 else 0)
        out.append(t)
    return out


def guarded(shape):
    """(view of `shape`, whole buffer) pre-filled with 0xAB bytes, TAIL floats behind the view."""
    n = int(np.prod(shape))
    buf = torch.full((n + TAIL,), 0, dtype=torch.float32, device=DEV)
    buf.view(torch.uint8).fill_(0xAB)
    return buf[:n].view(shape), buf


def untouched(buf, n):
    return bool((buf[n:].view(torch.uint8) == 0xAB).all().item())


def requests(levels, M, n_sot, n_prob):
    Q = len(levels)
    tails = [0.9, 0.1, 0.75, 0.3][:n_sot]
    sot = []
    for s, q in enumerate(tails):                   # any levels of the climate: the kernel takes indices
        h = (M - 1) * q
        k = min(int(math.floor(h)), M - 1)
        sot.append((k, h - k, (Q - 1 - s) % Q, (Q // 2 + s) % Q))
    prob = [((3 * t + 1) % Q, t % 2 == 1) for t in range(n_prob)]
    return sot, prob


def call(members, channels, clim, levels, floor, sot, prob, want=(True, True, True)):
    """The op with guarded outputs; returns ({name: array}, every guard untouched)."""
    nf, (_, H, W) = len(channels), members[0].shape
    table = member_table(members)
    shapes = dict(efi=(nf, H, W), sot=(len(sot), nf, H, W), prob=(len(prob), nf, H, W))
    on = dict(efi=want[0], sot=want[1] and len(sot) > 0, prob=want[2] and len(prob) > 0)
    out = {k: guarded(shapes[k]) if on[k] else (None, None) for k in shapes}
    hip.clim_extremes(members, table, channels, clim, [float(v) for v in levels], [float(v) for v in floor],
                      [r[0] for r in sot] if on["sot"] else [], [float(r[1]) for r in sot] if on["sot"] else [],
                      [r[2] for r in sot] if on["sot"] else [], [r[3] for r in sot] if on["sot"] else [],
                      [r[0] for r in prob] if on["prob"] else [], [bool(r[1]) for r in prob] if on["prob"] else [],
                      out["efi"][0], out["sot"][0], out["prob"][0])
    torch.cuda.synchronize()
    ok = all(untouched(b, int(np.prod(shapes[k]))) for k, (v, b) in out.items() if v is not None)
    return {k: None if v is None else v.cpu().numpy() for k, (v, b) in out.items()}, ok


def reference(x, channels, clim, levels, floor, sot, prob):
    """The restatement per listed field: dict of (nf, H W) / (S, nf, H W) / (T, nf, H W)."""
    M, C, H, W = x.shape
    refs = [R.extremes32(x[:, ch].reshape(M, -1), clim[f].reshape(len(levels), -1), levels, floor[f], sot, prob)
            for f, ch in enumerate(channels)]
    return dict(efi=np.stack([r["efi"] for r in refs]), sot=np.stack([r["sot"] for r in refs], axis=1),
                prob=np.stack([r["prob"] for r in refs], axis=1))


def same(got, ref, names=("efi", "sot", "prob")):
    for k in names:
        if got[k] is not None:
            g, r = R.bits(got[k]).reshape(-1), R.bits(ref[k]).reshape(-1)
            assert g.size == r.size and np.array_equal(g, r), (k, int((g != r).sum()), g.size)


def make_case(M, Q, H, W, C, seed):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((M, C, H, W)) * 1.2 + 0.3).astype(np.float32)
    return x, rng


def make_clim(rng, nf, Q, H, W):
    return np.sort(rng.standard_normal((nf, Q, H, W)).astype(np.float32), axis=1)


@pytest.mark.parametrize("align", [4, 16])
@pytest.mark.parametrize("grid", GRIDS)
def test_extremes_grids_members_alignment(grid, align):
    """Every bucket edge of M on every grid, at both alignments, with 4 SOT tails and 8 percentiles, all outputs."""
    H, W = grid
    Q, C, channels = 11, 4, [2, 0, 2]
    for M in (1, 2, 7, 8, 9, 16, 17, 33, 50, 64):
        x, rng = make_case(M, Q, H, W, C, 100 + M)
        clim = make_clim(rng, len(channels), Q, H, W)
        sot, prob = requests(levels_of(Q), M, 4, 8)
        floor = [-np.inf, -0.2, 0.4]
        got, ok = call(upload_members(x, align), channels, torch.from_numpy(clim).to(DEV), levels_of(Q), floor, sot, prob)
        assert ok, "a guard was written"
        same(got, reference(x, channels, clim, levels_of(Q), floor, sot, prob))


@pytest.mark.parametrize("Q", [2, 3, 101, 128])
@pytest.mark.parametrize("nf", [1, 3, 16])
def test_extremes_levels_and_fields(Q, nf):
    H, W, C, M = 3, 7, 5, 9
    x, rng = make_case(M, Q, H, W, C, 7 * Q + nf)
    channels = [int(c) for c in rng.integers(0, C, nf)]                 # repeated and reordered
    clim = make_clim(rng, nf, Q, H, W)
    sot, prob = requests(levels_of(Q), M, 4, 8)
    floor = [(-np.inf if f % 2 else 0.0) for f in range(nf)]
    for align in (4, 16):
        got, ok = call(upload_members(x, align), channels, torch.from_numpy(clim).to(DEV), levels_of(Q), floor, sot, prob)
        assert ok
        same(got, reference(x, channels, clim, levels_of(Q), floor, sot, prob))


def test_extremes_every_combination_of_outputs():
    """NULL outputs are not computed, nothing else is written: every combination of (efi, sot, prob) with 0 / 4 tails and 0 / 8 percentiles."""
    H, W, C, M, Q = 5, 64, 3, 12, 11
    x, rng = make_case(M, Q, H, W, C, 5)
    channels, floor = [1, 2], [-np.inf, -np.inf]
    clim = make_clim(rng, 2, Q, H, W)
    dclim = torch.from_numpy(clim).to(DEV)
    sot, prob = requests(levels_of(Q), M, 4, 8)
    ref = reference(x, channels, clim, levels_of(Q), floor, sot, prob)
    for align in (4, 16):
        mem = upload_members(x, align)
        for want in itertools.product((False, True), repeat=3):
            if not any(want):
                continue
            got, ok = call(mem, channels, dclim, levels_of(Q), floor, sot, prob, want)
            assert ok and [got[k] is not None for k in ("efi", "sot", "prob")] == list(want)
            same(got, ref)


def test_extremes_constructed_cases():
    H, W, C, Q = 1, 8, 1, 11
    lev = levels_of(Q)
    rng = np.random.default_rng(3)
    c1 = np.sort(rng.standard_normal((1, Q, H, W)).astype(np.float32), axis=1)
    run = lambda x, c, floor, sot=(), prob=(): (call(upload_members(x, 16), [0], torch.from_numpy(c).to(DEV), lev, floor, list(sot), list(prob)),   # noqa: E731
                                                 reference(x, [0], c, lev, floor, list(sot), list(prob)))
    # members exactly on climate values: <= against <
    M = 5
    x = np.stack([c1[0, k] for k in (0, 3, 3, 7, 10)])[:, None]          # (M, 1, H, W)
    prob = [(3, False), (3, True), (0, True), (10, False)]
    (got, ok), ref = run(x, c1, [-np.inf], [(2, 0.5, 9, 5)], prob)
    assert ok
    same(got, ref)
    assert np.all(got["prob"][0] == np.float32(2) / np.float32(5)) and np.all(got["prob"][1] == np.float32(1) / np.float32(5))
    assert np.all(got["prob"][2] == 0) and np.all(got["prob"][3] == 0)
    # a flat climate: SOT NaN, EFI from the counts; 0 only when the floor switches every interval off
    flat = np.full((1, Q, H, W), 2.0, np.float32)
    xs = (rng.standard_normal((M, 1, H, W)) + 2.0).astype(np.float32)
    for floor, zero in ((-np.inf, False), (1.0, False), (2.0, True), (5.0, True)):
        (got, ok), ref = run(xs, flat, [floor], [(2, 0.5, 9, 5)], [(4, False)])
        assert ok
        same(got, ref)
        assert np.all(R.bits(got["sot"]) == 0x7FC00000)
        assert np.all(R.bits(got["efi"]) == 0) == zero
    # a floor that deactivates some, none and all intervals
    xs = (rng.standard_normal((7, 1, H, W))).astype(np.float32)
    for floor in (float(c1[0, 5].max()), -np.inf, float(c1.max()) + 1):
        (got, ok), ref = run(xs, c1, [floor])
        assert ok
        same(got, ref)
    assert np.all(R.bits(got["efi"]) == 0)                               # all off: exactly +0
    # all members above the top level: exactly 1; all at or below the bottom level: -1 (exact in real arithmetic; to the header's bound in fp32)
    (got, ok), ref = run(np.full((6, 1, H, W), 50.0, np.float32), c1, [-np.inf])
    same(got, ref)
    assert np.all(got["efi"] == np.float32(1.0))
    xb = np.broadcast_to(c1[0, 0], (6, H, W))[:, None].copy()            # ON the bottom level
    (got, ok), ref = run(xb, c1, [-np.inf])
    same(got, ref)
    bound = R.extremes64(xb[:, 0].reshape(6, -1), c1[0].reshape(Q, -1), lev)["efi_bound"]
    print("all at or below the bottom level: efi =", sorted(set(got["efi"].reshape(-1).tolist())))
    assert np.all(got["efi"] >= -1) and np.all(np.abs(got["efi"].reshape(-1).astype(np.float64) + 1) <= bound)
    # +-0 in both inputs
    xz = np.array([0.0, -0.0, 0.0, -0.0, 1.0], np.float32)[:, None, None, None] * np.ones((1, 1, H, W), np.float32)
    cz = c1.copy()
    cz[0, 4], cz[0, 5] = -0.0, 0.0
    cz[0, :4] = -np.abs(cz[0, :4]) - 1
    cz[0, 6:] = np.abs(cz[0, 6:]) + 2
    cz = np.sort(cz, axis=1)
    (got, ok), ref = run(xz, cz, [-np.inf], [(0, 0.0, 5, 3), (1, 0.25, 4, 5)], [(4, False), (4, True), (5, True)])
    assert ok
    same(got, ref)
    assert np.all(got["prob"][0] == np.float32(1) / np.float32(5)) and np.all(got["prob"][1:] == 0)      # 0 is never above or below -0
    assert np.all(R.bits(got["sot"][1]) == 0x7FC00000)                   # -0 and +0 are one level: no denominator


def test_extremes_nan_poisons_its_own_point_only():
    H, W, C, M, Q = 3, 7, 2, 9, 11
    x, rng = make_case(M, Q, H, W, C, 11)
    channels, floor = [0, 1], [-np.inf, -np.inf]
    clim = make_clim(rng, 2, Q, H, W)
    x[4, 0, 1, 2] = np.nan                     # a member: field 0, point (1, 2)
    x[2, 1, 0, 0] = np.inf
    clim[1, 6, 2, 5] = np.nan                  # a climate value: field 1, point (2, 5)
    sot, prob = requests(levels_of(Q), M, 2, 3)
    got, ok = call(upload_members(x, 4), channels, torch.from_numpy(clim).to(DEV), levels_of(Q), floor, sot, prob)
    assert ok
    same(got, reference(x, channels, clim, levels_of(Q), floor, sot, prob))
    nan = np.isnan(got["efi"])
    assert set(zip(*np.nonzero(nan))) == {(0, 1, 2), (1, 0, 0), (1, 2, 5)}
    assert np.all(R.bits(got["efi"][nan]) == 0x7FC00000) and np.all(R.bits(got["prob"][:, nan]) == 0x7FC00000)


def test_extremes_full_width():
    """721 x 1440, M = 50, Q = 101, one field: bit-equal to the restatement on about 40 sampled rows, and within the header's bounds of
    the float64 formula there."""
    H, W, M, Q = 721, 1440, 50, 101
    lev = levels_of(Q)
    g = torch.Generator(device=DEV).manual_seed(1)
    mem = [torch.randn((1, H, W), generator=g, device=DEV) * 1.3 + 0.2 for _ in range(M)]
    clim = torch.sort(torch.randn((1, Q, H, W), generator=g, device=DEV), dim=1).values.contiguous()
    sot = [K.sot_request(lev, 0.9, M), K.sot_request(lev, 0.1, M)]
    prob = [(K.level_index(lev, 0.99, "t"), False), (K.level_index(lev, 0.05, "t"), True)]
    got, ok = call(mem, [0], clim, lev, [-np.inf], sot, prob)
    assert ok
    rows = sorted(set([0, 1, H - 1, H - 2] + [int(r) for r in np.linspace(2, H - 3, 36)]))
    flat = np.concatenate([np.arange(r * W, (r + 1) * W) for r in rows])
    flat = np.union1d(flat, np.arange(256 * 100 - 700, 256 * 100 + 700))       # across a workgroup boundary inside a row
    x = torch.stack([t.reshape(-1)[torch.from_numpy(flat).to(DEV)] for t in mem]).cpu().numpy()
    c = clim.reshape(Q, -1)[:, torch.from_numpy(flat).to(DEV)].cpu().numpy()
    ref = R.extremes32(x, c, lev, -np.inf, sot, prob)
    for k in ("efi", "sot", "prob"):
        assert np.array_equal(R.bits(got[k].reshape(got[k].shape[0], -1)[..., flat]).reshape(-1), R.bits(ref[k]).reshape(-1)), k
    ex = R.extremes64(x, c, lev, -np.inf, sot)
    e_efi = np.abs(ref["efi"].astype(np.float64) - ex["efi"]) / ex["efi_bound"]
    e_sot = np.abs(ref["sot"].astype(np.float64) - ex["sot"]) / ex["sot_bound"]
    print(f"full width: largest |efi - exact| / bound = {e_efi.max():.3e}, largest |sot - exact| / bound = {np.nanmax(e_sot):.3e}")
    assert e_efi.max() <= 1.0 and np.nanmax(e_sot) <= 1.0


# ---- the builder ----------------------------------------------------------------------------------------------------------------------- #
def quantiles(s, channels, levels):
    """s (N, C, H, W) -> the op's (nf, Q, H, W) with a guard behind it."""
    samples = [torch.from_numpy(np.ascontiguousarray(s[n])).to(DEV) for n in range(s.shape[0])]
    out, buf = guarded((len(channels), len(levels), *s.shape[2:]))
    hip.clim_quantiles(samples, member_table(samples), channels, [float(v) for v in levels], out)
    torch.cuda.synchronize()
    assert untouched(buf, out.numel())
    return out.cpu().numpy()


def quantiles_ref(s, channels, levels):
    N, C, H, W = s.shape
    return np.stack([R.quantiles32(s[:, ch].reshape(N, -1), levels).reshape(len(levels), H, W) for ch in channels])


QLEVELS = {1: [0.37], 2: [0.0, 1.0], 101: np.linspace(0, 1, 101)}


@pytest.mark.parametrize("N", [1, 2, 3, 63, 64, 65, 101, 257, 1000, 2048])
def test_quantiles_sizes(N):
    """Every N on the small grids and on one tile of points plus one, every Q, mixed magnitudes; planes non-decreasing; float64 bound."""
    T = K.tile_points(N)
    for (H, W), Q in (((1, 4), 1), ((3, 7), 2), ((1, T + 1), 101)):
        s = R.field(N, 3, H, W, N + Q)
        channels = [2, 0]
        got = quantiles(s, channels, QLEVELS[Q])
        assert np.array_equal(R.bits(got), R.bits(quantiles_ref(s, channels, QLEVELS[Q])))
        assert np.all(np.diff(got, axis=1) >= 0)
        for f, ch in enumerate(channels):
            exact, bound = R.quantile_bound(s[:, ch].reshape(N, -1), QLEVELS[Q])
            assert np.all(np.abs(got[f].reshape(len(QLEVELS[Q]), -1) - exact) <= bound)


def test_quantiles_ties_zeros_and_poison():
    rng = np.random.default_rng(9)
    N, H, W = 65, 3, 7
    lev = QLEVELS[101]
    s = rng.integers(0, 4, (N, 2, H, W)).astype(np.float32)             # heavy ties
    s[:, 1] = 5.5                                                        # all equal
    s[::3, 0, 0, 0], s[1::3, 0, 0, 0], s[2::3, 0, 0, 0] = 0.0, -0.0, 0.0      # +-0
    got = quantiles(s, [0, 1], lev)
    assert np.array_equal(R.bits(got), R.bits(quantiles_ref(s, [0, 1], lev)))
    assert np.all(got[1] == 5.5) and np.all(R.bits(got[0, :, 0, 0]) == 0)
    s = R.field(N, 2, H, W, 4)
    s[7, 0, 1, 3] = np.nan
    s[60, 1, 2, 6] = -np.inf
    got = quantiles(s, [0, 1], lev)
    assert np.array_equal(R.bits(got), R.bits(quantiles_ref(s, [0, 1], lev)))
    nan = np.isnan(got).any(axis=1)
    assert set(zip(*np.nonzero(nan))) == {(0, 1, 3), (1, 2, 6)} and np.all(R.bits(got[:, :, 1, 3][0]) == 0x7FC00000)


def test_builder_output_feeds_extremes():
    """The two layouts agree: a climate built from N <= 64 samples, fed unchanged to clim_extremes with the samples as members, gives the
    restatement's EFI.  It is small, since the members ARE the climate's sample: the fraction of them at or below their own level-p
    quantile is within 1 / N of p, so |efi| <= (2 / pi) pi / N = 2 / N, plus rounding (not a physical claim)."""
    N, C, H, W = 50, 3, 3, 7
    lev = QLEVELS[101]
    s = R.field(N, C, H, W, 21)
    channels = [2, 1]
    samples = [torch.from_numpy(s[n]).to(DEV) for n in range(N)]
    clim = torch.empty((2, 101, H, W), device=DEV)
    hip.clim_quantiles(samples, member_table(samples), channels, [float(v) for v in lev], clim)
    got, ok = call(samples, channels, clim, lev, [-np.inf, -np.inf], [], [])
    assert ok
    ref = reference(s, channels, clim.cpu().numpy(), lev, [-np.inf, -np.inf], [], [])
    same(got, ref)
    print("efi of a sample against its own climate: max |efi| =", float(np.abs(got["efi"]).max()))
    assert np.abs(got["efi"]).max() <= 2.0 / N + 1e-3
