"""ms of one ``point_gather`` launch at 721 x 1440 x 69 with M = 50 synthetic member states (no model), 8 channels, P = 1 000 and 100 000
random points with bilinear records (two taps per axis), the records sorted by (row, col) and in the order given, next to the torch chain
on the same tensors (advanced indexing of the four neighbours straight out of each member, no plane is copied first; weights and sum) and
to the copy of ONE member to the host, which is what ``keep_members=True`` pays per member and lead time.  The measurements alternate in
one process, each between device events, after warm-up.  A measurement is a batch of calls sized so that its window is some milliseconds
long whatever the case (``--window_ms``; at least ``--batch`` calls): a window of a few launches would measure the clock and the scheduler.
Prints the medians and spreads, the ratios, whether the kernel and the chain agree, and one JSON line.

    timeout -k 10 600 python tools/point_time.py [--reps 20] [--warmup 3] [--members 50] [--batch 10] [--window_ms 20]
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
from skyrim_amd import points as P  # noqa: E402

H, W, C = 721, 1440, 69
CHANNELS = [68, 65, 66, 0, 13, 26, 39, 52]


def _timed(fn, batch):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(batch):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / batch


def random_records(n, seed):
    """n bilinear records of points spread evenly over the sphere's latitudes and longitudes: two taps on both axes."""
    rng = np.random.default_rng(seed)
    rec = np.zeros(n, P.REC)
    rec["row"], rec["col"] = rng.integers(0, H - 1, n), rng.integers(0, W, n)
    rec["nr"], rec["ncol"] = 2, 2
    t, s = rng.uniform(0.05, 0.95, n).astype(np.float32), rng.uniform(0.05, 0.95, n).astype(np.float32)
    rec["wr0"], rec["wr1"], rec["wc0"], rec["wc1"] = 1 - t, t, 1 - s, s
    P.validate_records(rec, H, W)
    return rec


def torch_chain(members, rec_dev, ch, out):
    """The same sampling with torch ops, member after member: four advanced-indexing gathers of (nc, P) values straight out of the member
    (``ch``: the channel indices as a column, so no plane is copied), weights and sums in the header's order."""
    row, row1, col, col1, wr0, wr1, wc0, wc1 = rec_dev
    for m, s in enumerate(members):
        v0 = wr0 * s[ch, row, col] + wr1 * s[ch, row1, col]
        v1 = wr0 * s[ch, row, col1] + wr1 * s[ch, row1, col1]
        out[m] = wc0 * v0 + wc1 * v1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--members", type=int, default=50)
    ap.add_argument("--batch", type=int, default=10)
    ap.add_argument("--window_ms", type=float, default=20.0)
    args = ap.parse_args()
    dev, M = torch.device("cuda:0"), args.members
    gen = torch.Generator(device=dev).manual_seed(0)
    base = torch.rand((C, H, W), generator=gen, device=dev) * 30.0
    members = [base * (1.0 + 1e-3 * m) for m in range(M)]
    table = E.member_table(members)
    ch = torch.tensor(CHANNELS, device=dev)[:, None]
    pinned = torch.empty((C, H, W), dtype=torch.float32, pin_memory=True)
    cases, agree = {}, {}
    for n in (1000, 100000):
        rec = random_records(n, n)
        order = np.lexsort((rec["col"], rec["row"]))
        for label, r in (("sorted", rec[order]), ("unsorted", rec)):
            rd = P.device_records(r, dev)
            out = torch.empty((M, len(CHANNELS), n), dtype=torch.float32, device=dev)
            cases[f"point_gather P={n} {label}"] = (lambda rd=rd, out=out: P.run(members, table, CHANNELS, rd, out))
            row, col = torch.from_numpy(r["row"].astype(np.int64)).to(dev), torch.from_numpy(r["col"].astype(np.int64)).to(dev)
            parts = (row, row + 1, col, (col + 1) % W, *(torch.from_numpy(r[k].copy()).to(dev) for k in ("wr0", "wr1", "wc0", "wc1")))
            ref = torch.empty_like(out)
            cases[f"torch chain P={n} {label}"] = (lambda parts=parts, ref=ref: torch_chain(members, parts, ch, ref))
            agree[f"P={n} {label}"] = (out, ref)
    cases["one member to the host (pinned)"] = lambda: pinned.copy_(members[0], non_blocking=True)
    for _ in range(args.warmup):
        for fn in cases.values():
            fn()
    torch.cuda.synchronize()
    batch = {}
    for k, fn in cases.items():                      # one probe per case sizes its batch: every timed window is about window_ms long
        probe = _timed(fn, args.batch)
        batch[k] = max(args.batch, min(2000, int(round(args.window_ms / max(probe, 1e-4)))))
    # (the chain contracts nothing either, but torch may fuse a product and a sum differently: report, do not assume)
    differ = {k: float((a - b).abs().max().item()) for k, (a, b) in agree.items()}
    times = {k: [] for k in cases}
    for _ in range(args.reps):                       # alternating: every case sees the same clocks and the same neighbours
        for k, fn in cases.items():
            times[k].append(_timed(fn, batch[k]))
    res = {}
    for k in cases:
        med = statistics.median(times[k])
        res[k] = {"ms_median": round(med, 4), "ms_min": round(min(times[k]), 4), "ms_max": round(max(times[k]), 4), "batch": batch[k]}
        print(f"{k:>36}: median {med:9.4f} ms (min {min(times[k]):.4f}, max {max(times[k]):.4f}; {batch[k]} calls per measurement)")
    for n in (1000, 100000):
        g, u = res[f"point_gather P={n} sorted"]["ms_median"], res[f"point_gather P={n} unsorted"]["ms_median"]
        c = res[f"torch chain P={n} sorted"]["ms_median"]
        copy = res["one member to the host (pinned)"]["ms_median"]
        print(f"P={n}: unsorted / sorted {u / g:.2f} x; torch chain / point_gather {c / g:.1f} x; {M} members to the host / point_gather "
              f"{M * copy / g:.0f} x; largest difference kernel - chain {differ[f'P={n} sorted']:.3g}")
    print(json.dumps({"tool": "point_time", "grid": [H, W, C], "members": M, "channels": len(CHANNELS), "reps": args.reps, "window_ms": args.window_ms,
                      "max_abs_difference": differ, "cases": res}))


if __name__ == "__main__":
    main()
