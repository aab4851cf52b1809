"""ms of one ``nbr_fields`` launch at 721 x 1440 with M = 50 synthetic member states (no model): max + frac_above of one channel over the
discs of 100 km and of 300 km, next to a torch chain on the same tensors (per row offset a periodic ``max_pool1d`` / ``avg_pool1d`` over
the rows that share a half-width -- a restatement of the same discs by rows, whole rows left out, so it does LESS work than the kernel;
it makes thousands of small launches per member, so it is timed on CHAIN_MEMBERS members and scaled to M) and next to the bytes the call
must move (per member one input plane in and two planes out) divided by the measured copy rate.  The measurements alternate in one process, each between device events, after warm-up; prints the medians and one JSON line.

    timeout -k 10 600 python tools/nbr_time.py [--reps 10] [--warmup 2] [--members 50]
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
from skyrim_amd import neighbourhood as N  # noqa: E402
from skyrim_amd.verify import area_weights  # noqa: E402

COPY_RATE = 6.29e12          # bytes / s: the measured device-to-device copy rate of an MI355X (tools/ens_time.py)
THRESHOLD = 25.0
CHAIN_MEMBERS = 2
OPS = [N.Op(N.MAX, 1, 0, 0), N.Op(N.FRAC_ABOVE, 1, 1, 0, THRESHOLD)]


def _timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def torch_chain(members, reach, half, out):
    """Max and count above over the open ranges of the discs with torch ops, member after member: per row offset d and per half-width n
    that occurs, a periodic pooling of the rows that have it.  Rows that close the circle are skipped."""
    H, W = half.shape[0], members[0].shape[-1]
    groups = []
    for d in range(-reach, reach + 1):
        col = half[:, reach + d]
        for n in np.unique(col[(col >= 0) & (2 * col + 1 < W)]):
            rows = np.nonzero(col == n)[0]
            groups.append((d, int(n), torch.from_numpy(rows).to(out.device)))
    for m, s in enumerate(members):
        x = s[1]
        above = (x > THRESHOLD).float()
        mx = torch.full_like(x, -float("inf"))
        cnt = torch.zeros_like(x)
        for d, n, rows in groups:
            src = rows + d
            xs, ab = x[src], above[src]
            if n:
                xs = torch.cat([xs[:, -n:], xs, xs[:, :n]], dim=1)
                ab = torch.cat([ab[:, -n:], ab, ab[:, :n]], dim=1)
                xs = torch.nn.functional.max_pool1d(xs[None], 2 * n + 1, 1)[0]
                ab = torch.nn.functional.avg_pool1d(ab[None], 2 * n + 1, 1)[0] * (2 * n + 1)
            mx[rows] = torch.maximum(mx[rows], xs)
            cnt[rows] += ab
        out[m, 0], out[m, 1] = mx, cnt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--members", type=int, default=50)
    args = ap.parse_args()
    dev, M, H, W = "cuda:0", args.members, 721, 1440
    lat, lon = np.linspace(90.0, -90.0, H), np.arange(W) * (360.0 / W)
    gen = torch.Generator(device=dev).manual_seed(0)
    base = torch.rand((2, H, W), generator=gen, device=dev) * 30.0                 # a wind speed of 0 .. 30 m/s in channel 1
    members = [base * (1.0 + 1e-3 * m) for m in range(M)]
    table = E.member_table(members)
    weights = torch.from_numpy(area_weights(lat)).to(dev)
    out, ref = (torch.empty((M, len(OPS), H, W), dtype=torch.float32, device=dev) for _ in range(2))
    nbytes = M * (1 + len(OPS)) * H * W * 4
    res = {}
    for km in (100, 300):
        reach, half = N.discs(lat, lon, float(km))
        halves = [torch.from_numpy(half).to(dev)]
        cases = {f"nbr_fields {km} km": (lambda: N.run(members, table, OPS, halves, weights, out), nbytes),
                 f"torch chain {km} km": (lambda: torch_chain(members[:CHAIN_MEMBERS], reach, half, ref), None)}
        times = {k: [] for k in cases}
        for _ in range(args.warmup):
            for fn, _b in cases.values():
                fn()
        torch.cuda.synchronize()
        for _ in range(args.reps):                   # alternating: every case sees the same clocks and the same neighbours
            for k, (fn, _b) in cases.items():
                times[k].append(_timed(fn))
        for k, (fn, nb) in cases.items():
            if nb is None:                           # the chain ran on CHAIN_MEMBERS members: scaled to M
                times[k] = [t * M / min(M, CHAIN_MEMBERS) for t in times[k]]
            med = statistics.median(times[k])
            res[k] = {"ms_median": round(med, 4), "ms_min": round(min(times[k]), 4), "ms_max": round(max(times[k]), 4), "reach": reach,
                      "mean_points": round(float(N.disc_points(half, W).mean()), 1)}
            line = f"{k:>22}: median {med:9.3f} ms (min {min(times[k]):.3f}, max {max(times[k]):.3f})"
            if nb is not None:
                floor = nb / COPY_RATE * 1e3
                res[k].update(bytes=nb, ms_at_copy_rate=round(floor, 4), times_the_copy_floor=round(med / floor, 2))
                line += f"; {nb / 1e6:.1f} MB in and out = {floor:.3f} ms at the copy rate, the launch takes {med / floor:.1f} x that"
            print(line)
        ratio = res[f"torch chain {km} km"]["ms_median"] / res[f"nbr_fields {km} km"]["ms_median"]
        res[f"ratio_torch_over_kernel_{km}km"] = round(ratio, 3)
        print(f"torch chain / nbr_fields at {km} km: {ratio:.2f} x")
    print(json.dumps({"tool": "nbr_time", "grid": [H, W], "members": M, "ops": ["max", "frac_above"], "reps": args.reps, "cases": res}))


if __name__ == "__main__":
    main()
