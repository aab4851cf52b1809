"""ms of the event count pass (include/skyrim_event.h) at 721 x 1440 with M = 50 synthetic states (no model), for 1 and for 4 event
channels with one threshold each, in two regimes: thresholds at each channel's median (the points spread over the (o, k) bins) and a
threshold no member exceeds (every point in bin (0, 0): the case in which per-lane LDS adds to one word would serialise) -- next to
``ens_stats(exceed=...)`` on the same channels of the same members (the same bytes in, 4 B per point and threshold out, one call per
channel as ``ensemble.run`` makes them) and to a plain torch chain that forms the same joint counts.  The ``ens_stats`` case is in the
alternation TWICE: the difference of its two medians is the run-to-run spread the other differences are read against.  One more case
times the count pass with the planes plus the neighbourhood pass over three scales.  The measurements alternate in one process, each
between device events, after warm-up; prints the medians and one JSON line.

    timeout -k 10 600 python tools/event_time.py [--reps 10] [--warmup 2] [--members 50]
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from skyrim_amd import ensemble as E  # noqa: E402
from skyrim_amd import events as EV  # noqa: E402
from skyrim_amd.pangu.spec import CHANNELS, PanguGeometry, synthetic_state  # noqa: E402

NAMES = ("t2m", "u10m", "z500", "t850")


def _timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def torch_counts(members, truth, channels, thresholds):
    """The same joint counts per latitude row as whole-tensor torch ops: a running sum of comparisons over the member list, then one
    bincount per channel over (row, o, k)."""
    M, (H, W) = len(members), truth.shape[1:]
    rows = torch.arange(H, device=truth.device).view(H, 1) * (2 * (M + 1))
    out = []
    for ch, thr in zip(channels, thresholds):
        k = torch.zeros((H, W), dtype=torch.int64, device=truth.device)
        for m in members:
            k += m[ch] > thr
        o = (truth[ch] > thr).to(torch.int64)
        out.append((rows + o * (M + 1) + k).flatten().bincount(minlength=H * 2 * (M + 1)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--members", type=int, default=50)
    args = ap.parse_args()
    dev, M = "cuda:0", args.members
    g = PanguGeometry(721, 1440)
    C, H, W = 69, g.n_lat, g.n_lon
    hw = H * W
    x0 = synthetic_state(g, 0).to(dev).contiguous()
    std = x0.reshape(C, -1).std(dim=1).contiguous()
    members = [torch.empty_like(x0) for _ in range(M)]
    for m, t in enumerate(members):
        E.perturb(x0, std, t, hw, 1e-3, 0, m)
    truth = synthetic_state(g, 1).to(dev).contiguous()
    table = E.member_table(members)
    idx = [CHANNELS.index(n) for n in NAMES]
    median = [float(x0[c].median().item()) for c in idx]
    never = [float(max(t[c].max().item() for t in members)) + 1.0 for c in idx]
    counts = torch.zeros((4, EV.MAX_THRESHOLDS, H, 2, M + 1), dtype=torch.int32, device=dev)
    exceed = torch.empty((1, H, W), dtype=torch.float32, device=dev)
    radii = (0.0, 100.0, 300.0)
    win = [EV.windows(np.asarray(g.lat), np.asarray(g.lon), r) for r in radii]
    hy, hx = [w[0] for w in win], torch.from_numpy(np.stack([w[1] for w in win])).to(dev)
    sums = torch.zeros((1, EV.MAX_THRESHOLDS, len(radii), H, 3), dtype=torch.int64, device=dev)
    planes = torch.empty(EV.MAX_THRESHOLDS * 2 * hw, dtype=torch.uint8, device=dev)

    def count(n, thr):
        return lambda: EV.run(members, table, truth, idx[:n], [[v] for v in thr[:n]], counts[:n])

    def stats(n, thr):
        def fn():
            for c, v in zip(idx[:n], thr[:n]):
                E.stats(members, table, c * hw, hw, exceed=exceed, thresholds=[v])
        return fn

    cases = {}
    for n in (1, 4):
        moved = n * (M + 1) * hw * 4
        cases[f"event counts, {n} ch, median"] = (count(n, median), moved)
        cases[f"event counts, {n} ch, never exceeded"] = (count(n, never), moved)
        cases[f"ens_stats exceed, {n} ch, median"] = (stats(n, median), n * (M + 1) * hw * 4)
        cases[f"ens_stats exceed, {n} ch, median (repeat)"] = (stats(n, median), n * (M + 1) * hw * 4)
        cases[f"ens_stats exceed, {n} ch, never exceeded"] = (stats(n, never), n * (M + 1) * hw * 4)
        cases[f"torch chain, {n} ch, median"] = (lambda n=n: torch_counts(members, truth, idx[:n], median[:n]), None)
    cases["event counts + 3 scales, 1 ch, median"] = (
        lambda: EV.run(members, table, truth, idx[:1], [[median[0]]], counts[:1], hy, hx, sums, planes), None)
    times = {k: [] for k in cases}
    for _ in range(args.warmup):
        for fn, _b in cases.values():
            fn()
    torch.cuda.synchronize()
    for _ in range(args.reps):                       # alternating: every case sees the same clocks and the same neighbours
        for k, (fn, _b) in cases.items():
            times[k].append(_timed(fn))
    res = {}
    for k, (fn, nbytes) in cases.items():
        med = statistics.median(times[k])
        res[k] = {"ms_median": round(med, 4), "ms_min": round(min(times[k]), 4), "ms_max": round(max(times[k]), 4)}
        line = f"{k:>46}: median {med:8.3f} ms (min {min(times[k]):.3f}, max {max(times[k]):.3f})"
        if nbytes is not None:
            res[k]["bytes_read"] = nbytes
            line += f"; {nbytes / 1e6:.0f} MB read, {nbytes / (med * 1e-3) / 1e12:.2f} TB/s"
        print(line)
    ratios = {}
    for n in (1, 4):
        ms = lambda k: res[f"{k}, {n} ch, " + "median"]["ms_median"]      # noqa: E731
        a, b = ms("ens_stats exceed"), res[f"ens_stats exceed, {n} ch, median (repeat)"]["ms_median"]
        ratios[f"{n}ch_ens_stats_spread"] = round(abs(a - b) / min(a, b), 4)
        ratios[f"{n}ch_counts_over_ens_stats_median"] = round(ms("event counts") / min(a, b), 3)
        ratios[f"{n}ch_counts_over_ens_stats_never"] = round(res[f"event counts, {n} ch, never exceeded"]["ms_median"]
                                                             / res[f"ens_stats exceed, {n} ch, never exceeded"]["ms_median"], 3)
        ratios[f"{n}ch_counts_never_over_median"] = round(res[f"event counts, {n} ch, never exceeded"]["ms_median"] / ms("event counts"), 3)
        ratios[f"{n}ch_torch_over_counts"] = round(ms("torch chain") / ms("event counts"), 2)
    for k, v in ratios.items():
        print(f"{k}: {v}")
    print(json.dumps({"tool": "event_time", "grid": [H, W], "members": M, "reps": args.reps, "ratios": ratios, "cases": res}))


if __name__ == "__main__":
    main()
