"""libskyrim_spec.so on the MI355X against the float64 restatement of tests/_spectra_reference.py, inside the header's bound for every
slot, band and wavenumber: every radix alone and mixed (W = 30, 45, 48, 64), W = 1440, the 512-lane instantiation (W = 2048), the
largest W (4096, more than 64 KiB of LDS), several chunks per segment; M = 1, 2, 3, 64 with and without a truth; a repeated channel,
overlapping bands, a one-row band and a band of all rows.  Also: equal members give a spread of exactly 0, the identities between the
slots, bit-equal repeats, the teeth of the bound, a NaN stays in its channel and bands, and sentinels round output and workspace."""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

import _spectra_reference as R
from skyrim_amd import ensemble as E
from skyrim_amd import ops  # noqa: F401  (registers torch.ops.skyrim_hip)
from skyrim_amd import spectra as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64                                                                     # sentinel doubles before and after a buffer
SENTINEL = -1.2345e300
CHANNELS = [0, 2, 0]                                                           # nc = 3 of C = 3 with a repeated channel


def bands_of(H):
    return [(0, H), (1, 3), (2, 3)] if H < 8 else [(0, H), (3, H - 3), (2, 3)]  # all rows, an overlapping band, a one-row band


def weights_of(H):
    return np.cos(np.linspace(-1.2, 1.3, H)) + 0.1


@functools.lru_cache(maxsize=None)
def inputs(W, H, M, truth, white=False):
    """The case and its reference: computed once, shared, left unchanged."""
    members, y = R.case(W, H, M, truth, white=white)
    out, lim = R.spectra(members, y, CHANNELS, bands_of(H), weights_of(H))
    return members, y, out, lim


def guarded(n):
    buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.float64, device=DEV)
    return buf, buf[GUARD:GUARD + n]


def intact(buf, n):
    host = buf.cpu().numpy()
    return bool((host[:GUARD] == SENTINEL).all() and (host[GUARD + n:] == SENTINEL).all())


def launch(members, y, channels, bands, w, via_op=False):
    """One launch on fresh guarded buffers; returns the (nc, nb, slots, K) result on the host."""
    states = [torch.from_numpy(np.ascontiguousarray(m)).to(DEV) for m in members]
    truth = None if y is None else torch.from_numpy(np.ascontiguousarray(y)).to(DEV)
    table = E.member_table(states)
    C, H, W = states[0].shape
    slots = 6 if y is not None else 3
    shape = (len(channels), len(bands), slots, W // 2 + 1)
    n = int(np.prod(shape))
    need = S.workspace_bytes(len(states), H, W, len(channels), bands, y is not None)
    assert need > 0 and need % 8 == 0
    obuf, out = guarded(n)
    wbuf, ws = guarded(need // 8)
    wd = torch.from_numpy(np.asarray(w, np.float64)).to(DEV)
    if via_op:
        torch.ops.skyrim_hip.zonal_spectra(states, table, truth, list(channels), [v for b in bands for v in b], wd, out.view(shape), ws)
    else:
        S.zonal(states, table, truth, channels, bands, wd, out.view(shape), ws)
    torch.cuda.synchronize()
    res = out.view(shape).cpu().numpy().copy()
    assert intact(obuf, n) and intact(wbuf, need // 8), "the kernel wrote outside its output or workspace"
    return res


def worst(got, out, lim):
    """The largest error / bound; entries whose bound is 0 (a single member's spread) must be exact."""
    err = np.abs(got - out)
    assert np.isfinite(got).all()
    assert not err[lim == 0].any()
    return float((err[lim > 0] / lim[lim > 0]).max())


SHAPES = [(30, 5), (45, 5), (48, 5), (64, 5), (1440, 4)]


@pytest.mark.parametrize("truth", [False, True])
@pytest.mark.parametrize("M", [1, 2, 3, 64])
@pytest.mark.parametrize("W,H", SHAPES)
def test_every_slot_band_and_wavenumber_lies_within_the_headers_bound(W, H, M, truth):
    members, y, out, lim = inputs(W, H, M, truth)
    got = launch(members, y, CHANNELS, bands_of(H), weights_of(H))
    assert got.shape == out.shape == (3, 3, 6 if truth else 3, W // 2 + 1)
    ratio = worst(got, out, lim)
    print(f"spectra W={W} H={H} M={M} truth={truth}: worst error / bound = {ratio:.4f}")
    assert ratio <= 1.0
    assert np.array_equal(got[0], got[2])                                      # the repeated channel: the same bits
    if M == 1:
        assert not got[:, :, 2].any()                                          # spread: exactly 0


@pytest.mark.parametrize("W,H,M,truth", [(2048, 2, 3, True), (4096, 2, 2, False), (4096, 1, 3, True), (48, 20, 3, True), (2, 3, 3, True)])
def test_the_other_paths_512_lanes_the_largest_w_several_chunks_the_smallest_w(W, H, M, truth):
    members, y = R.case(W, H, M, truth)
    bands = [(0, H)] if H < 3 else bands_of(H)
    w = weights_of(H)
    out, lim = R.spectra(members, y, CHANNELS, bands, w)
    ratio = worst(launch(members, y, CHANNELS, bands, w), out, lim)
    print(f"spectra W={W} H={H} M={M} truth={truth}: worst error / bound = {ratio:.4f}")
    assert ratio <= 1.0


def test_two_channels_that_are_one_channel_give_the_same_bits_within_the_bound():
    members, y, _, _ = inputs(45, 5, 3, True)
    out, lim = R.spectra(members, y, [1, 1], bands_of(5), weights_of(5))
    got = launch(members, y, [1, 1], bands_of(5), weights_of(5))                # nc = 2: chunks of two rows
    assert worst(got, out, lim) <= 1.0 and np.array_equal(got[0], got[1])


def test_white_noise_differences_lie_within_the_bound():
    members, y, out, lim = inputs(48, 5, 3, True, True)
    ratio = worst(launch(members, y, CHANNELS, bands_of(5), weights_of(5)), out, lim)
    print(f"spectra white W=48: worst error / bound = {ratio:.4f}")
    assert ratio <= 1.0
    members, y = R.case(1440, 4, 4, True, white=True)
    out, lim = R.spectra(members, y, [1], bands_of(4), weights_of(4))
    ratio = worst(launch(members, y, [1], bands_of(4), weights_of(4)), out, lim)
    print(f"spectra white W=1440: worst error / bound = {ratio:.4f}")
    assert ratio <= 1.0


def test_equal_members_give_a_spread_of_exactly_zero_and_two_calls_the_same_bits():
    members, y, _, _ = inputs(1440, 4, 3, True)
    same = [members[1].copy() for _ in range(5)]
    got = launch(same, y, CHANNELS, bands_of(4), weights_of(4))
    assert not got[:, :, 2].any() and got[:, :, 0].all()
    assert np.allclose(got[:, :, 0], got[:, :, 1], rtol=1e-14, atol=0) and np.allclose(got[:, :, 4], got[:, :, 5], rtol=1e-14, atol=0)
    a = launch(members, y, CHANNELS, bands_of(4), weights_of(4))
    b = launch(members, y, CHANNELS, bands_of(4), weights_of(4), via_op=True)
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64))


@pytest.mark.parametrize("W,H,M", [(45, 5, 3), (1440, 4, 64)])
def test_the_identities_between_the_slots_hold_within_the_summed_bounds(W, H, M):
    members, y, _, lim = inputs(W, H, M, True)
    got = launch(members, y, CHANNELS, bands_of(H), weights_of(H))
    f = (M - 1) / M
    assert (np.abs(got[:, :, 0] - got[:, :, 1] - f * got[:, :, 2]) <= lim[:, :, 0] + lim[:, :, 1] + f * lim[:, :, 2]).all()
    assert (np.abs(got[:, :, 5] - got[:, :, 4] - f * got[:, :, 2]) <= lim[:, :, 5] + lim[:, :, 4] + f * lim[:, :, 2]).all()


def test_the_bound_has_teeth_one_value_changed_by_one_row_rms_lies_ten_bounds_away():
    """W = 1440, a one-row band: one value of member 0 moved by the row's rms shifts every coefficient by rms / 1440 = 1.2e4 u rms.  The
    row's phases lie within +-1 rad and the changed value is the row's first, so that the shift is never orthogonal to a coefficient."""
    W, H, M = 1440, 3, 2
    rng = np.random.default_rng(7)
    base = 5.5e4 + R.red_rows(rng, (1, H), W, 1e3, phase_span=1.0)
    members = [base.astype(np.float32), (base + R.red_rows(rng, (1, H), W)).astype(np.float32)]
    bands, w = [(1, 2)], np.ones(H)
    out, lim = R.spectra(members, None, [0], bands, w)
    row = members[0][0, 1].astype(np.float64)
    moved = [members[0].copy(), members[1]]
    moved[0][0, 1, 0] += np.float32(np.sqrt(((row - row.mean()) ** 2).mean()))
    out2, _ = R.spectra(moved, None, [0], bands, w)
    away = np.abs(out2[0, 0, 0] - out[0, 0, 0]) / lim[0, 0, 0]
    print(f"spectra teeth: the changed row lies {away.min():.1f} to {away.max():.1f} bounds away")
    assert away.min() >= 10.0
    got = launch(members, None, [0], bands, w)
    assert worst(got, out, lim) <= 1.0
    assert (np.abs(got[0, 0, 0] - out2[0, 0, 0]) / lim[0, 0, 0]).min() >= 9.0


def test_a_nan_poisons_only_its_channels_slots_in_the_bands_that_hold_its_row():
    members, y, out, lim = inputs(48, 5, 3, True)
    bad = [m.copy() for m in members]
    bad[1][2, 2, 17] = np.nan                                                  # member 1, channel 2, row 2
    got = launch(bad, y, CHANNELS, bands_of(5), weights_of(5))
    for cc, ch in enumerate(CHANNELS):
        for b, (j0, j1) in enumerate(bands_of(5)):
            hit = ch == 2 and j0 <= 2 < j1
            for s in range(6):
                if hit and s != 3:
                    assert np.isnan(got[cc, b, s]).all(), (cc, b, s)
                else:                                                          # the truth's own spectrum does not depend on member 1
                    assert (np.abs(got[cc, b, s] - out[cc, b, s]) <= lim[cc, b, s]).all(), (cc, b, s)
    bad = [m.copy() for m in members]
    bad[0][0, 4, 0] = np.inf                                                   # member 0 reaches every slot of its row's bands
    got = launch(bad, y, CHANNELS, [(0, 5), (0, 4)], weights_of(5))
    assert np.isnan(got[0, 0]).all() and np.isnan(got[2, 0]).all() and np.isfinite(got[1]).all() and np.isfinite(got[:, 1]).all()
    bad_y = y.copy()
    bad_y[0, 1, 5] = np.nan                                                    # the truth: truth, error_mean, error_member
    got = launch(members, bad_y, CHANNELS, [(0, 5), (2, 5)], weights_of(5))
    assert np.isnan(got[0, 0, 3:]).all() and np.isfinite(got[0, 0, :3]).all() and np.isfinite(got[1]).all() and np.isfinite(got[:, 1]).all()
