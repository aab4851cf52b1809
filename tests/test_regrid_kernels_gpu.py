"""``torch.ops.skyrim_hip.regrid`` against the float64 restatement (tests/_regrid_reference.py): every output within the header's bound
(the worst share is printed), the vector and the scalar path, bit-equal repeats, the bit-exact crop, the untouched parts of the output
buffer and NaN propagation.  No test hands the kernel a bad table: its clamps are read in the code, not provoked."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import _regrid_reference as R
from skyrim_amd import ensemble as E
from skyrim_amd import regrid as G

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
C, M = 5, 3


def grid(n_lat, n_lon, rows=None, ascending=False):
    lat = np.linspace(90.0, -90.0, n_lat)[:rows]
    return (lat[::-1].copy() if ascending else lat), np.arange(n_lon) * (360.0 / n_lon)


def state(lat, lon, seed):
    """(C, H, W) float32: smooth fields plus noise of realistic magnitude (a temperature, a geopotential, two winds, a humidity)."""
    rng = np.random.default_rng(seed)
    la, lo = np.radians(lat)[:, None], np.radians(lon)[None, :]
    shape = (lat.size, lon.size)
    s = np.empty((C,) + shape)
    s[0] = 250.0 + 40.0 * np.cos(la) ** 2 + 3.0 * np.sin(2 * lo + seed) + rng.normal(0, 1.0, shape)
    s[1] = 54000.0 + 3000.0 * np.cos(la) ** 2 + 200.0 * np.sin(2 * lo) + rng.normal(0, 30.0, shape)
    s[2] = 25.0 * np.cos(la) * (1 + 0.3 * np.sin(3 * lo + seed)) + rng.normal(0, 2.0, shape)
    s[3] = 8.0 * np.sin(2 * la) * np.cos(2 * lo - seed) + rng.normal(0, 2.0, shape)
    s[4] = np.clip(0.02 * np.cos(la) ** 2 * (1 + 0.5 * np.sin(2 * lo)) + rng.normal(0, 5e-4, shape), 0, 0.02)
    return s.astype(np.float32)


def host_tables(t):
    return (t.rows.start, t.rows.count, t.rows.weight), (t.cols.start, t.cols.count, t.cols.weight)


def run_op(states, rows, cols, channels, misalign=False):
    """The (M, nc, Ho, Wo) output of one regrid on the device; the buffer starts as 0xAB bytes and has a tail that must stay so."""
    members = []
    for s in states:
        if misalign:
            flat = torch.empty(s.size + 1, dtype=torch.float32, device=DEV)
            t = flat[1:].view(s.shape)
            assert t.data_ptr() % 16 == 4
        else:
            t = torch.empty(s.shape, dtype=torch.float32, device=DEV)
            assert t.data_ptr() % 16 == 0
        t.copy_(torch.from_numpy(s))
        members.append(t)
    Ho, Wo, nc = len(rows[0]), len(cols[0]), len(channels)
    n = len(states) * nc * Ho * Wo * 4
    raw = torch.full((n + 256,), 0xAB, dtype=torch.uint8, device=DEV)
    out = raw[:n].view(torch.float32).view(len(states), nc, Ho, Wo)
    dev = [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in (*rows, *cols)]
    torch.ops.skyrim_hip.regrid(members, E.member_table(members), list(channels), *dev, out)
    torch.cuda.synchronize()
    assert bool((raw[n:] == 0xAB).all()), "bytes beyond the buffer were touched"
    return out.cpu().numpy()


def check(states, rows, cols, channels, what, **kw):
    """Every output within the header's bound; returns (the output, the worst share of a bound)."""
    got = run_op(states, rows, cols, channels, **kw)
    worst = 0.0
    for m, s in enumerate(states):
        for k, ch in enumerate(channels):
            exact, bound = R.apply(s[ch], rows, cols)
            share = np.abs(got[m, k].astype(np.float64) - exact) / bound
            assert np.all(np.isfinite(got[m, k])) and share.max() <= 1.0, (what, m, ch, float(share.max()))
            worst = max(worst, float(share.max()))
    print(f"{what}: worst share of the bound {worst:.3f}")
    return got, worst


REGION = dict(region=(-15.0, 15.0, 341.0, 18.0))              # 9 x 20 points of the 49 x 192 grid, across the date line
CASES = {
    "conservative 49x192 -> 13x48": (grid(49, 192), grid(13, 48), "conservative"),
    "conservative 48x192 -> 13x48": (grid(49, 192, rows=48), grid(13, 48), "conservative"),
    "conservative 37x90 -> 7x18 (W % 4 != 0)": (grid(37, 90), grid(7, 18), "conservative"),
    "bilinear 13x48 -> 25x96 (upsampling)": (grid(13, 48), grid(25, 96), "bilinear"),
    "date-line region 9x20": (grid(49, 192), REGION, "conservative"),
    "date-line region bilinear": (grid(49, 192), dict(region=(-15.0, 15.0, 341.0, 17.0), res=2.0), "bilinear"),
    "ascending 49x192 -> 13x48": (grid(49, 192, ascending=True), grid(13, 48, ascending=True), "conservative"),
}


@pytest.mark.parametrize("name", list(CASES))
def test_outputs_within_the_bound(name):
    (lat, lon), spec, method = CASES[name]
    dlat, dlon = G.target_grid(spec, lat, lon)
    if name == "date-line region 9x20":
        assert (dlat.size, dlon.size) == (9, 20) and dlon[0] > dlon[-1]
    if "W % 4" in name:
        assert lon.size % 4 != 0
    if "upsampling" in name:
        assert dlon.size > lon.size
    t = G.tables(lat, lon, dlat, dlon, method)
    states = [state(lat, lon, 10 + m) for m in range(M)]
    check(states, *host_tables(t), list(range(C)), name)


def synthetic_tables(H, W, Ho, Wo, seed):
    """32 taps on both axes, signed weights of mixed size; the column taps wrap."""
    rng = np.random.default_rng(seed)
    def axis(n_out, n_src, periodic):                         # noqa: E306
        start = rng.integers(0, n_src if periodic else n_src - 32 + 1, n_out).astype(np.int32)
        count = np.full(n_out, 32, np.int32)
        count[1::3] = rng.integers(1, 33, count[1::3].size)
        w = (rng.normal(0, 0.2, (n_out, 32)) + 0.03).astype(np.float32)
        w[w == 0] = 0.5
        for o in range(n_out):
            w[o, count[o]:] = 0.0
        return start, count, w
    return axis(Ho, H, False), axis(Wo, W, True)


def test_thirty_two_taps_on_both_axes():
    lat, lon = grid(49, 192)
    rows, cols = synthetic_tables(49, 192, 11, 70, 5)
    assert rows[1].max() == 32 and cols[1].max() == 32 and (cols[0] + cols[1]).max() > 192
    states = [state(lat, lon, 20 + m) for m in range(M)]
    check(states, rows, cols, list(range(C)), "32 x 32 taps")
    check([s[:, :, :40].copy() for s in states], rows, synthetic_tables(49, 40, 11, 70, 6)[1], [0, 2], "32 taps wrapping a 40-column circle")


def test_channel_lists_subset_and_out_of_order():
    lat, lon = grid(49, 192)
    t = G.tables(lat, lon, *grid(13, 48), "conservative")
    states = [state(lat, lon, 30 + m) for m in range(M)]
    full, _ = check(states, *host_tables(t), list(range(C)), "all channels")
    part, _ = check(states, *host_tables(t), [3, 0, 3, 4], "channels 3, 0, 3, 4")
    assert np.array_equal(part, full[:, [3, 0, 3, 4]])


def test_vector_and_scalar_paths_and_repeats_bit_equal():
    lat, lon = grid(49, 192)
    states = [state(lat, lon, 40 + m) for m in range(M)]
    for method, spec in (("conservative", grid(13, 48)), ("bilinear", "7.5deg")):
        t = G.tables(lat, lon, *G.target_grid(spec, lat, lon), method)
        a = run_op(states, *host_tables(t), list(range(C)))
        b = run_op(states, *host_tables(t), list(range(C)), misalign=True)
        c = run_op(states, *host_tables(t), list(range(C)))
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), method
        assert np.array_equal(a.view(np.uint32), c.view(np.uint32)), method


def test_nearest_region_is_a_bit_exact_crop():
    lat, lon = grid(49, 192)
    dlat, dlon = G.target_grid(REGION, lat, lon)
    t = G.tables(lat, lon, dlat, dlon, "nearest")
    assert (dlat.size, dlon.size) == (9, 20)
    states = [state(lat, lon, 50 + m) for m in range(M)]
    j0, i0 = int(t.rows.start[0]), int(t.cols.start[0])
    states[0][1, j0 + 2, (i0 + 3) % 192] = -0.0
    states[1][0, j0, i0] = np.nan
    states[2][4, j0 + 8, (i0 + 19) % 192] = np.float32(1e-42)                       # a subnormal
    for misalign in (False, True):
        got = run_op(states, *host_tables(t), list(range(C)), misalign=misalign)
        jj, ii = j0 + np.arange(9), (i0 + np.arange(20)) % 192
        for m, s in enumerate(states):
            want = torch.from_numpy(s)[:, jj][:, :, ii].numpy()
            assert np.array_equal(got[m].view(np.uint32), want.view(np.uint32)), (m, misalign)
        assert np.signbit(got[0, 1, 2, 3]) and got[0, 1, 2, 3] == 0 and np.isnan(got[1, 0, 0, 0]) and np.isnan(got).sum() == 1


def test_only_the_planes_of_each_member_are_written():
    lat, lon = grid(37, 90)
    t = G.tables(lat, lon, *grid(7, 12), "conservative")
    rows, cols = host_tables(t)
    states = [state(lat, lon, 60 + m) for m in range(M)]
    members = [torch.from_numpy(s).to(DEV) for s in states]
    nc, Ho, Wo, gap = 2, 7, 12, 40                             # a member stride larger than its planes
    stride = nc * Ho * Wo + gap
    raw = torch.full((M * stride * 4 + 256,), 0xAB, dtype=torch.uint8, device=DEV)
    d = G.describe(M, C, 37, 90, Ho, Wo, [4, 1], stride, 16 if all(x.data_ptr() % 16 == 0 for x in members) else 4)
    table = E.member_table(members)
    dev = [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in (*rows, *cols)]
    d.members, d.out = table.data_ptr(), raw.data_ptr()
    d.rows.start, d.rows.count, d.rows.weight, d.cols.start, d.cols.count, d.cols.weight = (x.data_ptr() for x in dev)
    import ctypes
    from skyrim_amd import native
    assert G.load_library().skregrid_run(ctypes.byref(d), native.stream(torch.device(DEV))) == 0
    torch.cuda.synchronize()
    host = raw.cpu().numpy()
    body = host[:M * stride * 4].view(np.float32).reshape(M, stride)
    want = run_op(states, rows, cols, [4, 1])
    assert np.array_equal(body[:, :nc * Ho * Wo].view(np.uint32), want.reshape(M, -1).view(np.uint32))
    assert np.all(body[:, nc * Ho * Wo:].view(np.uint8) == 0xAB) and np.all(host[M * stride * 4:] == 0xAB)


def test_nan_reaches_exactly_the_outputs_whose_taps_read_it():
    lat, lon = grid(49, 192)
    off = (np.linspace(88.0, -88.0, 23), np.arange(48) * 7.5 + 6.5)            # between the source's points; the last column wraps
    for method, spec, (j, i) in (("conservative", grid(13, 48), (20, 3)), ("bilinear", off, (None, 191)), ("conservative", grid(13, 48), (0, 100))):
        t = G.tables(lat, lon, *G.target_grid(spec, lat, lon), method)
        rows, cols = host_tables(t)
        if j is None:                                          # the second tap of an output row between two source rows
            assert rows[1][10] == 2 and cols[1][47] == 2 and cols[0][47] == 191
            j = int(rows[0][10]) + 1
        states = [state(lat, lon, 70 + m) for m in range(M)]
        states[1][2, j, i] = np.nan
        got = run_op(states, rows, cols, list(range(C)))
        hit = R.reached(rows, cols, 49, 192, j, i)
        assert hit.any() and not hit.all()
        bad = ~np.isfinite(got)
        assert np.array_equal(bad[1, 2], hit), (method, j, i)
        bad[1, 2] = False
        assert not bad.any()
