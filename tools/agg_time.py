"""ms of the ``agg_update`` launches of one window at 721 x 1440 with M = 50 synthetic member states (no model): max + mean + hours-above
of one channel over 4 steps (FIRST, two middle steps, LAST), next to a torch chain that folds the same tensors (``torch.maximum``,
``add_``, a comparison).  The measurements alternate in one process, each between device events, after warm-up; prints the medians, the
bytes the four calls must move (per member and call one input plane, per op the write of its slot and, without FIRST, its read), their
share of the measured copy rate, the ratio to the torch chain, and one JSON line.

    timeout -k 10 600 python tools/agg_time.py [--reps 20] [--warmup 3] [--members 50]
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from dataclasses import replace
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from skyrim_amd import aggregate as A  # noqa: E402
from skyrim_amd import ensemble as E  # noqa: E402

COPY_RATE = 6.29e12          # bytes / s: the measured device-to-device copy rate of an MI355X (tools/ens_time.py)
STEPS, THRESHOLD, DT = 4, 15.0, 6.0
OPS = [A.Op(A.MAX, 1, 0), A.Op(A.SUM, 1, 1, scale=float(np.float32(1.0 / STEPS))), A.Op(A.COUNT_ABOVE, 1, 2, thr=THRESHOLD, scale=DT)]


def _timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def phase(k: int) -> int:
    return (A.FIRST if k == 0 else 0) | (A.LAST if k == STEPS - 1 else 0)


def kernel_window(steps, tables, acc):
    for k, (members, table) in enumerate(zip(steps, tables)):
        A.run(members, table, [replace(op, phase=phase(k)) for op in OPS], acc, DT * (k + 1))


def torch_chain(steps, acc):
    """The same window with torch ops, member after member."""
    for k, members in enumerate(steps):
        for m, s in enumerate(members):
            x = s[1]
            if k == 0:
                acc[m, 0].copy_(x)
                acc[m, 1].copy_(x)
                acc[m, 2].copy_(x > THRESHOLD)
            else:
                torch.maximum(acc[m, 0], x, out=acc[m, 0])
                acc[m, 1].add_(x)
                acc[m, 2].add_(x > THRESHOLD)
            if k == STEPS - 1:
                acc[m, 1].mul_(1.0 / STEPS)
                acc[m, 2].mul_(DT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--members", type=int, default=50)
    args = ap.parse_args()
    dev, M, H, W = "cuda:0", args.members, 721, 1440
    gen = torch.Generator(device=dev).manual_seed(0)
    base = torch.rand((2, H, W), generator=gen, device=dev) * 30.0                 # a wind speed of 0 .. 30 m/s in channel 1
    steps = [[base * (1.0 + 1e-3 * m + 0.05 * k) for m in range(M)] for k in range(STEPS)]
    tables = [E.member_table(members) for members in steps]
    acc = torch.empty((M, len(OPS), H, W), dtype=torch.float32, device=dev)
    ref = torch.empty_like(acc)
    planes = STEPS + len(OPS) * (2 * STEPS - 1)                                    # reads of the input, writes and reads of the slots
    nbytes = M * planes * H * W * 4
    cases = {"agg_update (four launches)": (lambda: kernel_window(steps, tables, acc), nbytes),
             "torch chain": (lambda: torch_chain(steps, ref), None)}
    times = {k: [] for k in cases}
    for _ in range(args.warmup):
        for fn, _b in cases.values():
            fn()
    torch.cuda.synchronize()
    agree = float((acc - ref).abs().max().item())                                  # (the chain adds in the same order: only 1 / n differs)
    for _ in range(args.reps):                       # alternating: every case sees the same clocks and the same neighbours
        for k, (fn, _b) in cases.items():
            times[k].append(_timed(fn))
    res = {}
    for k, (fn, nb) in cases.items():
        med = statistics.median(times[k])
        res[k] = {"ms_median": round(med, 4), "ms_min": round(min(times[k]), 4), "ms_max": round(max(times[k]), 4)}
        line = f"{k:>30}: median {med:8.3f} ms (min {min(times[k]):.3f}, max {max(times[k]):.3f})"
        if nb is not None:
            rate = nb / (med * 1e-3)
            res[k].update(bytes=nb, share_of_copy_rate=round(rate / COPY_RATE, 4))
            line += f"; {nb / 1e6:.1f} MB moved, {rate / 1e12:.2f} TB/s = {100 * rate / COPY_RATE:.1f} % of the copy rate"
        print(line)
    ratio = res["torch chain"]["ms_median"] / res["agg_update (four launches)"]["ms_median"]
    print(f"torch chain / agg_update: {ratio:.2f} x; largest difference between the two results {agree:.3g}")
    print(json.dumps({"tool": "agg_time", "grid": [H, W], "members": M, "steps": STEPS, "ops": ["max", "mean", "hours_above"], "planes_moved": planes,
                      "reps": args.reps, "ratio_torch_over_kernel": round(ratio, 3), "max_abs_difference": agree, "cases": res}))


if __name__ == "__main__":
    main()
