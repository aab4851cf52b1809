"""``score_fields`` at its edges on the MI355X (include/skyrim_score.h) against the float64 restatement on the same float32 inputs:
member counts across every bucket, grid shapes down to one point, field magnitudes, a truth 1e-3, 1 and 30 sigma away from the
control, channel sub-ranges, 4-byte aligned members, both latitude orientations.  Every slot is held to the header's bound
(k u + 2^-40) S, k <= 2M + 7, which stays under the cap (64 + 2M) u S; rank counts are bit-exact."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import _score_reference as R
from skyrim_amd import verify as V

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
hip = torch.ops.skyrim_hip
SENTINEL = -12345.678
KINDS = {"z": (2e5, 3e3), "q": (1e-5, 3e-3), "t": (250.0, 15.0)}      # (base, sigma) as _members of test_ens_kernels_gpu.py builds them
SHAPES = [(3, 721, 1440), (2, 720, 1440), (3, 49, 192), (5, 7, 333), (1, 1, 1), (2, 2, 7), (1, 3, 4097)]
COUNTS = [1, 2, 7, 8, 9, 33, 50, 64]
ALL = V.DET | V.VAR | V.CRPS | V.ACC | V.RANK


def _case(M, shape, dist, seed, scale=1e-3, kinds="zqt"):
    """Members (M, C, H, W): a control plus ``scale`` sigma of noise per member (member 0 the control), channel c of kind kinds[c % 3];
    the truth ``dist`` sigma of noise away from the control; the climatology a smooth field a few sigma from the truth."""
    C, H, W = shape
    rng = np.random.default_rng(seed)
    x = np.empty((M, C, H, W), np.float32)
    y, c = np.empty((C, H, W), np.float32), np.empty((C, H, W), np.float32)
    for ch in range(C):
        kind = kinds[ch % len(kinds)]
        base, sigma = KINDS[kind]
        ctrl = base + sigma * rng.standard_normal((H, W)) * (1.0 if kind != "q" else 1e-3)
        m = ctrl[None] + scale * sigma * rng.standard_normal((M, H, W))
        m[0] = ctrl
        x[:, ch] = m
        y[ch] = ctrl + dist * sigma * rng.standard_normal((H, W))
        c[ch] = base + 0.5 * sigma * rng.standard_normal((H, W))
    return x, y, c


def _lat(H, ascending=False):
    lat = np.linspace(90, -90, 721)[:720] if H == 720 else (np.linspace(90, -90, H) if H > 1 else np.zeros(1))
    return lat[::-1].copy() if ascending else lat


def _run(x, y, c, w, flags=ALL, c0=0, nc=None, shift=0):
    """One score_fields call -> (out (nc, 10) float64 host, counts (nc, H, M + 1) int32 host or None); buffers pre-filled with a sentinel."""
    from skyrim_amd.ensemble import member_table
    M, C, H, W = x.shape
    nc = C - c0 if nc is None else nc
    mem = []
    for m in range(M):
        buf = torch.empty(C * H * W + shift, dtype=torch.float32, device=DEV)
        buf[shift:].copy_(torch.from_numpy(x[m]).reshape(-1))
        mem.append(buf[shift:].view(C, H, W))
    out = torch.full((nc, len(V.SLOTS)), SENTINEL, dtype=torch.float64, device=DEV)
    counts = torch.full((nc, H, M + 1), -7, dtype=torch.int32, device=DEV)
    ws = torch.empty(C * H * V.PARTIALS, dtype=torch.float64, device=DEV)
    hip.score_fields(mem, member_table(mem), torch.from_numpy(y).to(DEV), torch.from_numpy(np.asarray(w, np.float64)).to(DEV),
                     out if flags & ~V.RANK else None, ws, flags, torch.from_numpy(c).to(DEV) if flags & V.ACC else None,
                     counts if flags & V.RANK else None, c0, nc)
    return out.cpu().numpy(), counts.cpu().numpy()


def _check(x, y, c, w, out, counts, what, c0=0):
    """-> the worst share of the bound over slots and channels (asserted <= 1); rank counts bit-exact."""
    M = x.shape[0]
    worst = {}
    for ch in range(out.shape[0]):                                # channel by channel: the float64 copies of 64 full-size members are large
        k = c0 + ch
        val, bound, ref_counts = R.scores(x[:, k:k + 1], y[k:k + 1], w, c[k:k + 1])
        assert np.array_equal(counts[ch], ref_counts[0]), f"{what}: rank counts of channel {k}"
        for slot, name in enumerate(V.SLOTS):
            err = abs(out[ch, slot] - val[name][0])
            share = err / bound[name][0] if bound[name][0] > 0 else (0.0 if err == 0 else np.inf)
            worst[name] = max(worst.get(name, 0.0), share)
    print(f"{what}: share of the bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert max(worst.values()) <= 1, (what, worst)
    return worst


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("M", COUNTS)
def test_scores_match_the_restatement(M, shape):
    C, H, W = shape
    for i, dist in enumerate((1e-3, 1.0, 30.0)):
        kinds = "zqt"[i:] + "zqt"[:i]                              # every magnitude meets every distance, also where C < 3
        x, y, c = _case(M, shape, dist, seed=1000 * M + i, kinds=kinds)
        w = V.area_weights(_lat(H, ascending=bool(i & 1)))         # descending, ascending, descending
        out, counts = _run(x, y, c, w)
        _check(x, y, c, w, out, counts, f"M={M} {C}x{H}x{W} truth {dist} sigma away ({kinds})")
        if M > 1:
            assert counts.sum() == C * H * W


@pytest.mark.parametrize("M", [1, 7, 9, 50])
def test_channel_sub_range_alignment_and_spread_of_one_sigma(M):
    """A channel sub-range (the same bits as in the full call), member pointers shifted by one float (the 4-byte path: the same scores
    up to the order of the float64 sums) and members one sigma apart."""
    shape = (5, 49, 192)
    x, y, c = _case(M, shape, 1.0, seed=M, scale=1.0)
    w = V.area_weights(_lat(49))
    full, full_counts = _run(x, y, c, w)
    _check(x, y, c, w, full, full_counts, f"M={M} members 1 sigma apart")
    for c0, nc in ((1, 3), (4, 1), (0, 2)):
        out, counts = _run(x, y, c, w, c0=c0, nc=nc)
        assert np.array_equal(out, full[c0:c0 + nc]) and np.array_equal(counts, full_counts[c0:c0 + nc]), (c0, nc)
    out, counts = _run(x, y, c, w, shift=1)
    assert np.allclose(out, full, rtol=1e-12, atol=0) and np.array_equal(counts, full_counts)
    _check(x, y, c, w, out, counts, f"M={M} on 4-byte aligned members")
    flipped = [a[..., ::-1, :].copy() for a in (x, y, c)]          # the same fields on an ascending axis: the same scores
    out, counts = _run(*flipped, w[::-1].copy())
    _check(flipped[0], flipped[1], flipped[2], w[::-1], out, counts, f"M={M} ascending latitudes")
    assert np.allclose(out, full, rtol=1e-12, atol=0) and np.array_equal(counts[:, ::-1], full_counts)


@pytest.mark.parametrize("M", [1, 2, 9, 50])
def test_ties_equal_members_and_exact_zeros(M):
    shape = (3, 7, 333)
    x, y, c = _case(M, shape, 1.0, seed=7 * M)
    w = V.area_weights(_lat(7))
    x[M // 2, :, 2, ::5] = y[:, 2, ::5]                            # a member equal to the truth: rank is a strict comparison
    x[:, 1, 4] = x[0, 1, 4]                                        # a row of equal members
    out, counts = _run(x, y, c, w)
    _check(x, y, c, w, out, counts, f"M={M} with ties")
    xe = np.repeat(x[:1], M, axis=0)                               # all members equal
    out, counts = _run(xe, y, c, w)
    s = {k: out[:, i] for i, k in enumerate(V.SLOTS)}
    assert np.all(s["var"] == 0) and np.all(s["pair"] == 0) and np.array_equal(s["crps"], s["mae"]) and np.array_equal(s["abs"], s["mae"])
    assert counts[..., 1:M].sum() == 0 and np.all(counts[..., 0] + counts[..., M] == 333)      # all members on one side of the truth
    _check(xe, y, c, w, out, counts, f"M={M} equal members")
    xt = np.repeat(y[None], M, axis=0)                             # all members equal to the truth: every error slot exactly 0
    out, counts = _run(xt, y, c, w)
    assert np.all(out[:, :7] == 0) and np.all(counts[..., 0] == 333) and np.all(counts[..., 1:] == 0)


@pytest.mark.parametrize("M", [1, 8, 50])
def test_non_finite_values_stay_in_their_channel(M):
    shape = (3, 49, 192)
    x, y, c = _case(M, shape, 1.0, seed=3 * M)
    w = V.area_weights(_lat(49))
    clean, clean_counts = _run(x, y, c, w)
    for where, value in (("member", np.nan), ("member", np.inf), ("truth", np.nan), ("truth", -np.inf)):
        xb, yb = x.copy(), y.copy()
        if where == "member":
            xb[M // 2, 1, 17, 100] = value
        else:
            yb[1, 17, 100] = value
        out, counts = _run(xb, yb, c, w)
        want = out[1] if M > 1 else np.delete(out[1], [3, 6])      # (M = 1: VARIANCE and PAIR are the constant 0)
        assert not np.isfinite(want).any(), (where, value, out[1])
        assert np.array_equal(out[[0, 2]], clean[[0, 2]]) and np.array_equal(counts[[0, 2]], clean_counts[[0, 2]]), (where, value)
    cb = c.copy()
    cb[1, 3, 3] = np.nan                                           # the climatology reaches the ACC slots only
    out, counts = _run(x, y, cb, w)
    assert not np.isfinite(out[1, 7:]).any() and np.array_equal(out[1, :7], clean[1, :7]) and np.array_equal(out[[0, 2]], clean[[0, 2]])


@pytest.mark.parametrize("M", [1, 9, 50])
def test_outputs_not_requested_are_not_written(M):
    shape = (2, 49, 192)
    x, y, c = _case(M, shape, 1.0, seed=11 * M)
    w = V.area_weights(_lat(49))
    full, full_counts = _run(x, y, c, w)
    groups = {V.DET: [0, 1, 2], V.VAR: [3], V.CRPS: [4, 5, 6], V.ACC: [7, 8, 9]}
    for flags in (V.DET, V.VAR, V.CRPS, V.ACC, V.RANK, V.DET | V.ACC, V.VAR | V.RANK, V.DET | V.VAR | V.CRPS, V.CRPS | V.RANK):
        out, counts = _run(x, y, c, w, flags=flags)
        for g, slots in groups.items():
            if flags & g:
                assert np.allclose(out[:, slots], full[:, slots], rtol=1e-6, atol=0), (flags, g)   # (another instantiation may contract another product)
            else:
                assert np.all(out[:, slots] == SENTINEL), (flags, g)
        assert np.array_equal(counts, full_counts) if flags & V.RANK else np.all(counts == -7), flags


def test_full_size_is_reproducible_bit_for_bit():
    """M = 50 at 69 x 721 x 1440 from ens_perturb members: two runs give the same bits, and z500 / t850 / t2m are within the bound."""
    from skyrim_amd.ensemble import member_table
    from skyrim_amd.pangu.spec import CHANNELS, PanguGeometry, synthetic_state
    g = PanguGeometry(721, 1440)
    M, hw = 50, 721 * 1440
    x0 = synthetic_state(g, 0).to(DEV).contiguous()
    std = x0.reshape(69, -1).std(dim=1).contiguous()
    mem = []
    for m in range(M):
        t = torch.empty_like(x0)
        hip.ens_perturb(x0, std, t, hw, 1e-3, 0, m)
        mem.append(t)
    truth = synthetic_state(g, 1).to(DEV).contiguous()
    clim = synthetic_state(g, 2).to(DEV).contiguous()
    w_host = V.area_weights(np.asarray(g.lat))
    w = torch.from_numpy(w_host).to(DEV)
    ws = torch.empty(69 * 721 * V.PARTIALS, dtype=torch.float64, device=DEV)
    table = member_table(mem)
    runs = []
    for _ in range(2):
        out = torch.full((69, len(V.SLOTS)), SENTINEL, dtype=torch.float64, device=DEV)
        counts = torch.full((69, 721, M + 1), -7, dtype=torch.int32, device=DEV)
        ws.fill_(float("nan"))
        hip.score_fields(mem, table, truth, w, out, ws, ALL, clim, counts, 0, 69)
        runs.append((out.cpu().numpy(), counts.cpu().numpy()))
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])
    assert np.isfinite(runs[0][0]).all() and np.all(runs[0][1].sum(axis=(1, 2)) == hw)
    for name in ("z500", "t850", "t2m"):
        k = CHANNELS.index(name)
        x = np.stack([t[k:k + 1].cpu().numpy() for t in mem])
        _check(x, truth[k:k + 1].cpu().numpy(), clim[k:k + 1].cpu().numpy(), w_host, runs[0][0][k:k + 1], runs[0][1][k:k + 1], f"full size M=50 {name}")
