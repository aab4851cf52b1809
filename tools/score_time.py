"""ms of the verification kernel at 69 x 721 x 1440 with M = 50 and M = 1 synthetic states (no model): the deterministic scores, the
ensemble scores without CRPS and rank, and the full set -- next to ``ens_stats (mean, spread)`` on the same members (one state fewer in,
two more out) and to a plain torch chain that computes the same scores on the same tensors.  The measurements alternate in one process,
each between device events, after warm-up; prints the medians, the bytes each moves, its share of the measured copy rate, and one JSON
line.

    timeout -k 10 900 python tools/score_time.py [--reps 10] [--warmup 2] [--members 50]
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
from skyrim_amd import verify as V  # noqa: E402
from skyrim_amd.pangu.spec import PanguGeometry, synthetic_state  # noqa: E402

COPY_RATE = 6.29e12          # bytes / s: the measured device-to-device copy rate of an MI355X


def _timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def torch_scores(members, truth, w, full: bool):
    """The same scores as a chain of whole-tensor torch ops on the (C, H, W) states: float32 per-point terms, row sums accumulated in
    float64 (``sum(dtype=float64)``: no float64 copy of a field is made), weights and the sum over rows in float64.  The members stay
    the separate tensors they are in a forecast, so the member sums are running sums over the list (two passes for the variance);
    only the sort of the pair term needs the members of a point side by side, and stacks them one channel at a time (the stack of 50
    whole states would not fit next to the members)."""
    M, C = len(members), truth.shape[0]
    norm = truth.shape[2] * w.sum()
    out = torch.zeros((C, 7), dtype=torch.float64, device=truth.device)

    def mean(t):
        return (t.sum(dim=-1, dtype=torch.float64) * w).sum(dim=-1) / norm
    if M == 1:
        eb = members[0] - truth
        absum = eb.abs()
    else:
        eb = members[0] - truth
        absum = eb.abs() if full else None
        for m in members[1:]:
            e = m - truth
            eb += e
            if full:
                absum += e.abs()
        eb /= M
        if full:
            absum /= M
    out[:, 0], out[:, 1], out[:, 2] = mean(eb), mean(eb.abs()), mean(eb * eb)
    if M > 1:
        xb = eb + truth
        v = torch.zeros_like(truth)
        for m in members:
            v += (m - xb) ** 2
        out[:, 3] = mean(v) / (M - 1)
    if full:
        out[:, 5] = mean(absum)
        if M > 1:
            coef = (2 * torch.arange(M, device=truth.device, dtype=torch.float32) - M + 1).view(M, 1, 1)
            for c in range(C):
                x = torch.stack([m[c] for m in members])
                s = torch.sort(x, dim=0).values
                out[c, 6] = mean((coef * (s - truth[c])).sum(dim=0)) / (M * (M - 1))
                (x < truth[c]).sum(dim=0).flatten().bincount(minlength=M + 1)
        out[:, 4] = out[:, 5] - out[:, 6]
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
    state = x0.numel() * 4
    members = [torch.empty_like(x0) for _ in range(M)]
    for m, t in enumerate(members):
        E.perturb(x0, std, t, hw, 1e-3, 0, m)
    truth = synthetic_state(g, 1).to(dev).contiguous()
    table, table1 = E.member_table(members), E.member_table(members[:1])
    w = torch.from_numpy(V.area_weights(np.asarray(g.lat))).to(dev)
    out = torch.zeros((C, len(V.SLOTS)), dtype=torch.float64, device=dev)
    counts = torch.zeros((C, H, M + 1), dtype=torch.int32, device=dev)
    ws = torch.empty(C * H * V.PARTIALS, dtype=torch.float64, device=dev)
    mean, spread = torch.empty_like(x0), torch.empty_like(x0)
    n = x0.numel()
    cases = {
        "score deterministic (M = 1)": (lambda: V.score(members[:1], table1, truth, w, out, ws, V.DET | V.CRPS), 2 * state),
        f"score ensemble, no CRPS / rank (M = {M})": (lambda: V.score(members, table, truth, w, out, ws, V.DET | V.VAR), (M + 1) * state),
        f"score full set (M = {M})": (lambda: V.score(members, table, truth, w, out, ws, V.DET | V.VAR | V.CRPS | V.RANK, counts=counts),
                                      (M + 1) * state + counts.numel() * 4),
        f"ens_stats mean, spread (M = {M})": (lambda: E.stats(members, table, 0, n, mean=mean, spread=spread), (M + 2) * state),
        "torch deterministic (M = 1)": (lambda: torch_scores(members[:1], truth, w, True), None),
        f"torch ensemble, no CRPS / rank (M = {M})": (lambda: torch_scores(members, truth, w, False), None),
        f"torch full set (M = {M})": (lambda: torch_scores(members, truth, w, True), None),
    }
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
        line = f"{k:>44}: median {med:9.3f} ms (min {min(times[k]):.3f}, max {max(times[k]):.3f})"
        if nbytes is not None:
            rate = nbytes / (med * 1e-3)
            res[k].update(bytes=nbytes, share_of_copy_rate=round(rate / COPY_RATE, 4))
            line += f"; {nbytes / 1e6:.1f} MB moved, {rate / 1e12:.2f} TB/s = {100 * rate / COPY_RATE:.1f} % of the copy rate"
        print(line)
    keys = list(cases)
    ratios = {"torch_over_kernel_" + name: round(res[keys[4 + i]]["ms_median"] / res[keys[i]]["ms_median"], 3)
              for i, name in enumerate(("deterministic", "ensemble", "full"))}
    ratios["full_over_ens_stats"] = round(res[keys[2]]["ms_median"] / res[keys[3]]["ms_median"], 3)
    ratios["ensemble_over_ens_stats"] = round(res[keys[1]]["ms_median"] / res[keys[3]]["ms_median"], 3)
    for k, v in ratios.items():
        print(f"{k}: {v:.2f} x")
    print(json.dumps({"tool": "score_time", "grid": [C, H, W], "members": M, "reps": args.reps, "ratios": ratios, "cases": res}))
    slower = [n for n in ("deterministic", "ensemble", "full") if ratios["torch_over_kernel_" + n] <= 1]
    if slower:
        raise SystemExit(f"the kernel is not faster than the torch chain for: {slower}")


if __name__ == "__main__":
    main()
