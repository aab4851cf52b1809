"""``torch.ops.skyrim_hip.derive_fields`` against the float64 restatement (tests/_derive_reference.py): every output within the header's
bound (the worst share is printed), both paths, every edge treatment, untouched slots, bit-equal repeats and NaN propagation."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import _derive_reference as R
from skyrim_amd import derived as D
from skyrim_amd import ensemble as E

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
L = 8
C = 4 + 3 * L                                    # u, v, z_a, z_b, then q, u, v of L levels
CH = dict(u=0, v=1, za=2, zb=3, q=4, ul=4 + L, vl=4 + 2 * L)
WEIGHTS = tuple(float(np.float32(w)) for w in R.column_weights([300, 400, 500, 600, 700, 850, 925, 1000]))
FIELDS = ("speed", "diff", "ivtu", "ivtv", "ivt", "iwv", "vo", "div")


def grid(n_lat, n_lon, rows=None, ascending=False):
    lat = np.linspace(90.0, -90.0, n_lat)[:rows]
    return (lat[::-1].copy() if ascending else lat), np.arange(n_lon) * (360.0 / n_lon)


def state(lat, lon, seed, white=False):
    """(C, H, W) float32: smooth fields plus noise of realistic magnitude (winds in m/s, geopotential, q in [0, 0.02]); ``white``:
    the two wind planes are white noise, so that the differences of vorticity and divergence cancel."""
    rng = np.random.default_rng(seed)
    la, lo = np.radians(lat)[:, None], np.radians(lon)[None, :]
    s = np.empty((C, lat.size, lon.size))
    s[CH["u"]] = 25.0 * np.cos(la) * (1 + 0.3 * np.sin(3 * lo + seed)) + rng.normal(0, 2.0, (lat.size, lon.size))
    s[CH["v"]] = 8.0 * np.sin(2 * la) * np.cos(2 * lo - seed) + rng.normal(0, 2.0, (lat.size, lon.size))
    if white:
        s[CH["u"]], s[CH["v"]] = rng.normal(0, 15.0, (2, lat.size, lon.size))
    s[CH["za"]] = 54000.0 + 3000.0 * np.cos(la) ** 2 + 200.0 * np.sin(2 * lo) + rng.normal(0, 30.0, (lat.size, lon.size))
    s[CH["zb"]] = 1000.0 + 800.0 * np.cos(la) * np.cos(lo) + rng.normal(0, 30.0, (lat.size, lon.size))
    for k in range(L):
        s[CH["q"] + k] = np.clip(0.02 * (k + 1) / L * np.cos(la) ** 2 * (1 + 0.5 * np.sin(2 * lo + k)) + rng.normal(0, 5e-4, (lat.size, lon.size)), 0, 0.02)
        s[CH["ul"] + k] = (10.0 + 3 * (L - k)) * np.cos(la) * np.cos(lo + 0.3 * k) + rng.normal(0, 3.0, (lat.size, lon.size))
        s[CH["vl"] + k] = 6.0 * np.sin(2 * la) * np.sin(2 * lo + 0.2 * k) + rng.normal(0, 3.0, (lat.size, lon.size))
    return s.astype(np.float32)


def column_op(levels=L, outputs=(2, 3, 4, 5)):
    lv = tuple(range(levels))
    pick = lambda base: tuple(base + (k % L) for k in lv)      # noqa: E731  (more than L levels: the planes are read again)
    w = tuple(WEIGHTS[k % L] for k in lv)
    return D.Op(D.COLUMN, (pick(CH["q"]), pick(CH["ul"]), pick(CH["vl"])), tuple(outputs), w)


def program():
    return [D.Op(D.SPEED, (CH["u"], CH["v"]), (0,)), D.Op(D.DIFF, (CH["za"], CH["zb"]), (1,)), column_op(), D.Op(D.VORTDIV, (CH["u"], CH["v"]), (6, 7))]


def run_op(states, lat, lon, ops, n_out, misalign=False):
    """The (M, n_out, H, W) output of one derive_fields on the device; the buffer starts as 0xAB bytes and has a tail that must stay so."""
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
    rowc, e0, e1 = D.row_table(lat, lon)
    ints, floats = D.encode(ops)
    torch.ops.skyrim_hip.derive_fields(members, E.member_table(members), ints, floats, out, torch.from_numpy(rowc).to(DEV), [e0, e1])
    torch.cuda.synchronize()
    assert bool((raw[M * n_out * H * W * 4:] == 0xAB).all()), "bytes beyond the buffer were touched"
    return out.cpu().numpy()


def untouched(plane) -> bool:
    return bool(np.all(np.ascontiguousarray(plane).view(np.uint8) == 0xAB))


def reference(s, lat, lon, levels=L, weights=None):
    """{field: (value, bound)} of one state for the program above."""
    rowc, e0, e1 = R.row_table(lat, lon)
    out = {}
    v, S = R.speed(s[CH["u"]], s[CH["v"]])
    out["speed"] = (v, R.bound(R.K_SPEED, S, R.TINY_SPEED))
    v, S = R.diff(s[CH["za"]], s[CH["zb"]])
    out["diff"] = (v, R.bound(R.K_DIFF, S, R.TINY_DIFF))
    lv = [k % L for k in range(levels)]
    w = np.array([WEIGHTS[k] for k in lv], np.float32) if weights is None else weights
    col = R.column(s[[CH["q"] + k for k in lv]], s[[CH["ul"] + k for k in lv]], s[[CH["vl"] + k for k in lv]], w)
    for name, (v, S, k, tiny) in col.items():
        out[name] = (v, R.bound(k, S, tiny))
    vd = R.vortdiv(s[CH["u"]], s[CH["v"]], rowc, e0, e1)
    out["vo"], out["div"] = vd["vo"], vd["div"]
    return out


def shares(got, ref, what):
    """The worst share of its bound per field; every output must lie within."""
    worst = {}
    for name, (val, bnd) in ref.items():
        if name not in got:
            continue
        err = np.abs(got[name].astype(np.float64) - val)
        with np.errstate(divide="ignore", invalid="ignore"):
            share = np.where(bnd > 0, err / bnd, np.where(err == 0, 0.0, np.inf))
        worst[name] = max(worst.get(name, 0.0), float(share.max()))
    print(f"{what}: worst share of the bound " + " ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert all(v <= 1 for v in worst.values()), (what, worst)
    return worst


CASES = {"33x64 M=1": (grid(33, 64), 1, False), "33x64 M=3": (grid(33, 64), 3, False), "49x192 M=3": (grid(49, 192), 3, False),
         "33x66 scalar": (grid(33, 66), 2, False), "33x64 misaligned": (grid(33, 64), 2, True), "32of33x64 one-sided": (grid(33, 64, rows=32), 2, False),
         "ascending": (grid(33, 64, ascending=True), 2, False), "17x8": (grid(17, 8), 2, False), "17x6 scalar": (grid(17, 6), 1, False)}


@pytest.mark.parametrize("case", list(CASES))
def test_every_output_within_its_bound(case):
    (lat, lon), M, misalign = CASES[case]
    states = [state(lat, lon, 10 + m, white=(m == 1)) for m in range(M)]
    out = run_op(states, lat, lon, program(), len(FIELDS), misalign)
    H, W = lat.size, lon.size
    for m, s in enumerate(states):
        ref = reference(s, lat, lon)
        got = {name: out[m, d] for d, name in enumerate(FIELDS)}
        shares(got, ref, f"{case} member {m}")
        for name in ("vo", "div"):                              # the seam columns and the first and last row, explicitly
            val, bnd = ref[name]
            for idx in ((slice(None), 0), (slice(None), W - 1), (0, slice(None)), (H - 1, slice(None))):
                assert np.all(np.abs(got[name][idx].astype(np.float64) - val[idx]) <= bnd[idx]), (case, m, name, idx)
        _, e0, e1 = R.row_table(lat, lon)
        for j, flag in ((0, e0), (H - 1, e1)):
            if flag == R.POLE:
                assert np.all(got["vo"][j] == got["vo"][j, 0]) and np.all(got["div"][j] == got["div"][j, 0])
    if case == "33x64 M=3":                                     # both paths do the same arithmetic: bit-equal
        assert np.array_equal(out, run_op(states, lat, lon, program(), len(FIELDS), misalign=True))


@pytest.mark.parametrize("levels", [2, 8, 16])
def test_column_levels_and_switched_off_outputs(levels):
    lat, lon = grid(33, 64)
    s = state(lat, lon, 3)
    ref = reference(s, lat, lon, levels)
    names = ("ivtu", "ivtv", "ivt", "iwv")
    for mask in range(1, 16):
        slots = [-1] * 4
        for n, k in enumerate([k for k in range(4) if mask >> k & 1]):
            slots[k] = 4 - n                                   # (slots in descending order, slot 0 never named)
        out = run_op([s], lat, lon, [column_op(levels, slots)], 5)
        got = {names[k]: out[0, slots[k]] for k in range(4) if slots[k] >= 0}
        shares(got, {k: ref[k] for k in got}, f"L={levels} outputs {sorted(got)}")
        for d in range(5):
            assert untouched(out[0, d]) == (d not in slots), (levels, mask, d)


def test_vorticity_alone_and_divergence_alone():
    lat, lon = grid(33, 64)
    s = state(lat, lon, 4, white=True)
    ref = reference(s, lat, lon)
    both = run_op([s], lat, lon, [D.Op(D.VORTDIV, (CH["u"], CH["v"]), (0, 1))], 2)
    vo = run_op([s], lat, lon, [D.Op(D.VORTDIV, (CH["u"], CH["v"]), (1, -1))], 2)
    dv = run_op([s], lat, lon, [D.Op(D.VORTDIV, (CH["u"], CH["v"]), (-1, 0))], 2)
    shares(dict(vo=both[0, 0], div=both[0, 1]), ref, "white noise, vo and div")
    assert np.array_equal(vo[0, 1], both[0, 0]) and untouched(vo[0, 0])
    assert np.array_equal(dv[0, 0], both[0, 1]) and untouched(dv[0, 1])


def test_sixteen_ops_equal_one_at_a_time_and_repeat():
    lat, lon = grid(33, 64)
    states = [state(lat, lon, 20 + m) for m in range(2)]
    ops = []
    for d in range(16):
        k = d % L
        ops.append([D.Op(D.SPEED, (CH["ul"] + k, CH["vl"] + k), (d,)), D.Op(D.DIFF, (CH["za"], CH["q"] + k), (d,)),
                    column_op(16 if d == 2 else 8, (-1, -1, d, -1)), D.Op(D.VORTDIV, (CH["ul"] + k, CH["vl"] + k), (d, -1) if d % 8 < 4 else (-1, d))][d % 4])
    whole = run_op(states, lat, lon, ops, 16)
    assert np.array_equal(whole, run_op(states, lat, lon, ops, 16))                     # two runs: the same bits
    assert np.isfinite(whole).all()
    for d, op in enumerate(ops):
        single = run_op(states, lat, lon, [op], 16)
        assert np.array_equal(single[:, d], whole[:, d]), d
        assert all(untouched(single[:, e]) for e in range(16) if e != d)


def test_a_nan_reaches_exactly_the_points_that_read_it():
    lat, lon = grid(33, 64)
    states = [state(lat, lon, 30 + m) for m in range(3)]
    clean = run_op(states, lat, lon, program(), len(FIELDS))
    for ch, (j, i) in ((CH["u"], (7, 0)), (CH["v"], (1, 63)), (CH["q"] + 3, (16, 31)), (CH["ul"] + 5, (32, 5)), (CH["zb"], (0, 0))):
        bad = [s.copy() for s in states]
        bad[1][ch, j, i] = np.nan
        out = run_op(bad, lat, lon, program(), len(FIELDS))
        assert np.array_equal(out[0], clean[0]) and np.array_equal(out[2], clean[2])
        ref = reference(bad[1], lat, lon)
        hit = 0
        for d, name in enumerate(FIELDS):
            want = ~np.isfinite(ref[name][0])
            assert np.array_equal(~np.isfinite(out[1, d]), want), (ch, name)
            assert np.array_equal(out[1, d][~want], clean[1, d][~want]), (ch, name)
            hit += int(want.sum())
        assert hit >= 1
