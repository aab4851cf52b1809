"""ms of the ensemble kernels at 69 x 721 x 1440 with M = 50 synthetic member states (no model): ``ens_perturb`` per member, ``ens_stats``
for (mean, spread), for (mean, spread, min, max) and for one channel's three quantiles, and the torch chain of
``pangu.ensemble.ensemble_mean_spread`` on the same 50 tensors.  The measurements alternate in one process, each between device events,
after warm-up; prints the medians, the bytes each moves, its share of the measured copy rate, and one JSON line.

    timeout -k 10 600 python tools/ens_time.py [--reps 20] [--warmup 3] [--members 50]
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from skyrim_amd import ensemble as E  # noqa: E402
from skyrim_amd.pangu.ensemble import ensemble_mean_spread  # noqa: E402
from skyrim_amd.pangu.spec import PanguGeometry, synthetic_state  # noqa: E402

COPY_RATE = 6.29e12          # bytes / s: the measured device-to-device copy rate of an MI355X


def _timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--members", type=int, default=50)
    args = ap.parse_args()
    dev, M = "cuda:0", args.members
    g = PanguGeometry(721, 1440)
    hw = g.n_lat * g.n_lon
    x0 = synthetic_state(g, 0).to(dev).contiguous()
    std = x0.reshape(69, -1).std(dim=1).contiguous()
    state = x0.numel() * 4
    members = [torch.empty_like(x0) for _ in range(M)]
    for m, t in enumerate(members):
        E.perturb(x0, std, t, hw, 1e-3, 0, m)
    table = E.member_table(members)
    out = [torch.empty_like(x0) for _ in range(4)]
    quant = torch.empty((3, g.n_lat, g.n_lon), dtype=torch.float32, device=dev)
    scratch = torch.empty_like(x0)
    n = x0.numel()
    cases = {
        "ens_perturb (one member)": (lambda: E.perturb(x0, std, scratch, hw, 1e-3, 0, 1), 2 * state),
        "ens_stats mean, spread": (lambda: E.stats(members, table, 0, n, mean=out[0], spread=out[1]), (M + 2) * state),
        "ens_stats mean, spread, min, max": (lambda: E.stats(members, table, 0, n, mean=out[0], spread=out[1], min=out[2], max=out[3]), (M + 4) * state),
        "ens_stats 3 quantiles of one channel": (lambda: E.stats(members, table, 68 * hw, hw, quant=quant, levels=[0.1, 0.5, 0.9]), (M + 3) * hw * 4),
        "torch ensemble_mean_spread": (lambda: ensemble_mean_spread(members, M), None),
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
        line = f"{k:>40}: median {med:8.3f} ms (min {min(times[k]):.3f}, max {max(times[k]):.3f})"
        if nbytes is not None:
            rate = nbytes / (med * 1e-3)
            res[k].update(bytes=nbytes, share_of_copy_rate=round(rate / COPY_RATE, 4))
            line += f"; {nbytes / 1e6:.1f} MB moved, {rate / 1e12:.2f} TB/s = {100 * rate / COPY_RATE:.1f} % of the copy rate"
        print(line)
    ratio = res["torch ensemble_mean_spread"]["ms_median"] / res["ens_stats mean, spread"]["ms_median"]
    print(f"torch chain / ens_stats (mean, spread): {ratio:.2f} x")
    print(json.dumps({"tool": "ens_time", "grid": [69, g.n_lat, g.n_lon], "members": M, "reps": args.reps, "ratio_torch_over_kernel": round(ratio, 3),
                      "cases": res}))


if __name__ == "__main__":
    main()
