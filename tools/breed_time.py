"""ms of the two breeding launches at 69 x 721 x 1440 with M = 50 synthetic states (the control and 49 members; no model):
``breed_norms`` and ``breed_apply`` against a torch chain on the same tensors and against the device-to-device copy rate, which this
script measures itself.  The measurements alternate in one process, each between device events, after warm-up; prints the medians, the
bytes each launch has to move (M states read for the norms; M + 1 read and M - 1 written for the apply), its share of the copy rate,
and one JSON line.

    timeout -k 10 600 python tools/breed_time.py [--reps 20] [--warmup 3] [--members 50]
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

from skyrim_amd import breeding as B  # noqa: E402
from skyrim_amd import ensemble as E  # noqa: E402
from skyrim_amd.pangu.spec import PanguGeometry, synthetic_state  # noqa: E402
from skyrim_amd.verify import area_weights  # noqa: E402


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
    C, H, W = 69, g.n_lat, g.n_lon
    hw = H * W
    x0 = synthetic_state(g, 0).to(dev).contiguous()
    std = x0.reshape(C, -1).std(dim=1).contiguous()
    state = x0.numel() * 4
    y0 = torch.empty_like(x0)
    E.perturb(x0, std, y0, hw, 1e-2, 1, 1)                                 # a stand-in for the control forecast
    ys = [torch.empty_like(x0) for _ in range(M - 1)]                      # the members' forecasts
    for m, t in enumerate(ys):
        E.perturb(y0, std, t, hw, 1e-3, 0, m + 1)
    outs = [torch.empty_like(x0) for _ in range(M - 1)]
    y_table, o_table = E.member_table(ys), E.member_table(outs)
    w_host = area_weights(np.asarray(g.lat, np.float64))
    w = torch.from_numpy(w_host).to(dev)
    S = torch.empty((M - 1, C), dtype=torch.float64, device=dev)
    work = torch.empty(B.workspace_bytes(M - 1, C, H, W) // 8, dtype=torch.float64, device=dev)
    f = B.factors(torch.ones_like(S), std, 1e-3, "total", None, float(w_host.sum()), W)
    copy_src, copy_dst = torch.empty(8 * x0.numel(), dtype=torch.float32, device=dev), torch.empty(8 * x0.numel(), dtype=torch.float32, device=dev)
    w32 = w.float().reshape(1, H, 1)

    def torch_norms():
        return torch.stack([(((t - y0).double() ** 2).sum(dim=2) * w).sum(dim=1) for t in ys])

    def torch_norms_fp32():                                                # what one would write first: fp32 throughout, not the same numbers
        return torch.stack([(((t - y0) ** 2) * w32).sum(dim=(1, 2)) for t in ys])

    def torch_apply():
        for m, t in enumerate(ys):
            torch.add(x0, (t - y0) * f[m].reshape(C, 1, 1), out=outs[m])

    cases = {
        "copy (8 states)": (lambda: copy_dst.copy_(copy_src), 2 * 8 * state),
        "breed_norms": (lambda: B.norms(y0, ys, y_table, w, S, work), M * state),
        "breed_apply": (lambda: B.apply(x0, y0, ys, y_table, f, outs, o_table), (M + 1) * state + (M - 1) * state),
        "torch norms (float64 squares)": (torch_norms, None),
        "torch norms (fp32 throughout)": (torch_norms_fp32, None),
        "torch apply": (torch_apply, None),
    }
    times = {k: [] for k in cases}
    for _ in range(args.warmup):
        for fn, _b in cases.values():
            fn()
    torch.cuda.synchronize()
    for _ in range(args.reps):                       # alternating: every case sees the same clocks and the same neighbours
        for k, (fn, _b) in cases.items():
            times[k].append(_timed(fn))
    copy_rate = cases["copy (8 states)"][1] / (statistics.median(times["copy (8 states)"]) * 1e-3)
    res = {}
    for k, (fn, nbytes) in cases.items():
        med = statistics.median(times[k])
        res[k] = {"ms_median": round(med, 4), "ms_min": round(min(times[k]), 4), "ms_max": round(max(times[k]), 4)}
        line = f"{k:>34}: median {med:8.3f} ms (min {min(times[k]):.3f}, max {max(times[k]):.3f})"
        if nbytes is not None:
            rate = nbytes / (med * 1e-3)
            res[k].update(bytes=nbytes, share_of_copy_rate=round(rate / copy_rate, 4))
            line += f"; {nbytes / 1e6:.1f} MB moved, {rate / 1e12:.2f} TB/s = {100 * rate / copy_rate:.1f} % of the copy rate"
        print(line)
    r_norms = res["torch norms (float64 squares)"]["ms_median"] / res["breed_norms"]["ms_median"]
    r_apply = res["torch apply"]["ms_median"] / res["breed_apply"]["ms_median"]
    print(f"torch chain / kernel: norms {r_norms:.2f} x, apply {r_apply:.2f} x; copy rate {copy_rate / 1e12:.2f} TB/s")
    print(json.dumps({"tool": "breed_time", "grid": [C, H, W], "members": M, "reps": args.reps, "copy_rate_TBps": round(copy_rate / 1e12, 3),
                      "torch_over_kernel": {"norms": round(r_norms, 3), "apply": round(r_apply, 3)}, "cases": res}))


if __name__ == "__main__":
    main()
