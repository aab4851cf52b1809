"""ms of ONE cyclone-detection launch at 721 x 1440 with M = 50 synthetic states and the default ``TrackerConfig`` (no model) -- next to
``ens_stats (mean, spread)`` on the same members and to what the feature replaces: copying the seven channels of the 50 members to the
host with ``.cpu()``.  The measurements alternate in one process, the device ones between device events, the copy on the host clock
around a synchronised copy; prints the medians, the candidates found, the bytes the kernels should move and one JSON line.

    timeout -k 10 900 python tools/track_time.py [--reps 10] [--warmup 2] [--members 50]
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from skyrim_amd import ensemble as E  # noqa: E402
from skyrim_amd import tracks as T  # noqa: E402
from skyrim_amd.pangu.spec import CHANNELS, PanguGeometry, synthetic_state  # noqa: E402


def _timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def _host_timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--members", type=int, default=50)
    args = ap.parse_args()
    dev, M = "cuda:0", args.members
    g = PanguGeometry(721, 1440)
    H, W = g.n_lat, g.n_lon
    x0 = synthetic_state(g, 0).to(dev).contiguous()
    C = x0.shape[-3]
    x0 = x0.reshape(C, H, W)
    std = x0.reshape(C, -1).std(dim=1).contiguous()
    members = [torch.empty_like(x0) for _ in range(M)]
    for m, t in enumerate(members):
        E.perturb(x0, std, t, H * W, 1e-3, 0, m)
    table = E.member_table(members)
    tracker = T.LeadTracker("pangu", CHANNELS, g.lat, g.lon, M, None, dev)
    b, p, c, geo = tracker._buffers(), tracker.plan, tracker.cfg, tracker.geo
    tabs = b["g"]
    seven = torch.tensor([p.msl, p.u10, p.v10, p.u850, p.v850, p.z_up, p.z_lo], device=dev)
    mean, spread = torch.empty_like(x0), torch.empty_like(x0)
    n = x0.numel()

    def detect():
        T.detect(members, table, (p.msl, p.u10, p.v10, p.u850, p.v850, p.z_up, p.z_lo), (geo.j0, geo.j1),
                 (c.thr_msl, c.thr_vort, c.thr_wind, c.thr_core), tabs["msl"], tabs["vort"], tabs["wind"], tabs["core"], tabs["rowc"],
                 b["records"], b["count"], b["ws"])

    def to_host():
        for t in members:
            t[seven].cpu()

    cases = {"track_detect": (detect, _timed), "ens_stats mean, spread": (lambda: E.stats(members, table, 0, n, mean=mean, spread=spread), _timed),
             "seven channels to the host": (to_host, _host_timed)}
    times = {k: [] for k in cases}
    for _ in range(args.warmup):
        for fn, _t in cases.values():
            fn()
    torch.cuda.synchronize()
    for _ in range(args.reps):                       # alternating: every case sees the same clocks and the same neighbours
        for k, (fn, timer) in cases.items():
            times[k].append(timer(fn))
    detect()
    torch.cuda.synchronize()
    found = int(b["count"].item())
    survivors = int(b["ws"][:4].view(torch.int32).item())
    # what the kernels should move: M x the msl band (with its two halo rows), then per survivor its msl window, and per candidate that
    # passes, the windows of the later criteria (2 + 2 + 2 fields; the vorticity stencil's neighbours come from the same lines)
    Hb = geo.j1 - geo.j0
    window = {k: float((2 * np.maximum(geo.h[k], -0.5) + 1).sum(axis=1).mean()) for k in geo.h}
    should = M * (Hb + 2) * W * 4 + survivors * window["msl"] * 4
    res = {}
    for k in cases:
        med = statistics.median(times[k])
        res[k] = {"ms_median": round(med, 4), "ms_min": round(min(times[k]), 4), "ms_max": round(max(times[k]), 4)}
        print(f"{k:>28}: median {med:9.3f} ms (min {min(times[k]):.3f}, max {max(times[k]):.3f})")
    print(f"prefilter survivors {survivors}, candidates {found}; mean window points " + ", ".join(f"{k} {v:.0f}" for k, v in window.items()))
    print(f"bytes the detection should move: {should / 1e6:.1f} MB (band {M * (Hb + 2) * W * 4 / 1e6:.1f} MB); the host copy moves "
          f"{M * 7 * H * W * 4 / 1e6:.1f} MB")
    print(json.dumps({"tool": "track_time", "grid": [C, H, W], "members": M, "reps": args.reps, "survivors": survivors, "candidates": found,
                      "window_points": window, "bytes_should": should, "bytes_host_copy": M * 7 * H * W * 4, "cases": res}))


if __name__ == "__main__":
    main()
