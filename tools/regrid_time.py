"""ms of ONE ``regrid`` launch at 721 x 1440 -> 121 x 240 (first-order conservative, 1.5 degrees) with M = 50 synthetic member states on
Pangu's channel layout (no model), every channel, next to a torch chain that computes the same map (``Wr @ x @ Wc^T`` with dense weight
matrices) on the same tensors.  The measurements alternate in one process, each between device events, after warm-up; prints the medians,
the bytes the kernel must move (M x C x (H W + Ho Wo) x 4), its share of the copy rate (the constant of tools/ens_time.py), the ratio to
the torch chain, and one JSON line.

    timeout -k 10 600 python tools/regrid_time.py [--reps 20] [--warmup 3] [--members 50]
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
from skyrim_amd import regrid as G  # noqa: E402
from skyrim_amd.pangu.spec import CHANNELS, PanguGeometry, synthetic_state  # noqa: E402

COPY_RATE = 6.29e12          # bytes / s: the measured device-to-device copy rate of an MI355X (tools/ens_time.py)


def _timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def torch_chain(members, wr, wct, out):
    """The same map with two batched matrix products per member."""
    for m, s in enumerate(members):
        torch.matmul(torch.matmul(wr, s), wct, out=out[m])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--members", type=int, default=50)
    args = ap.parse_args()
    dev, M = "cuda:0", args.members
    g = PanguGeometry(721, 1440)
    H, W, C = g.n_lat, g.n_lon, len(CHANNELS)
    lat, lon = np.linspace(90.0, -90.0, H), np.arange(W) * (360.0 / W)
    x0 = synthetic_state(g, 0).to(dev).reshape(C, H, W).contiguous()
    members = [x0 * (1.0 + 1e-3 * m) for m in range(M)]
    table = E.member_table(members)
    rg = G.LeadRegridder(CHANNELS, lat, lon, M, "1.5deg", "conservative", device=dev)
    Ho, Wo = rg.lat_out.size, rg.lon_out.size
    nbytes = M * C * (H * W + Ho * Wo) * 4
    wr = torch.from_numpy(rg.tables.rows.dense().astype(np.float32)).to(dev)
    wct = torch.from_numpy(rg.tables.cols.dense().astype(np.float32).T.copy()).to(dev)
    out = torch.empty((M, C, Ho, Wo), dtype=torch.float32, device=dev)
    cases = {"regrid (one launch)": (lambda: rg.add(members, table), nbytes),
             "torch chain": (lambda: torch_chain(members, wr, wct, out), None)}
    times = {k: [] for k in cases}
    for _ in range(args.warmup):
        for fn, _b in cases.values():
            fn()
    torch.cuda.synchronize()
    got = rg.add(members, table)[0][M - 1]
    dev_err = float((got - out[M - 1]).abs().max() / out[M - 1].abs().max())
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
    ratio = res["torch chain"]["ms_median"] / res["regrid (one launch)"]["ms_median"]
    print(f"torch chain / regrid: {ratio:.2f} x; largest difference between the two, relative to the largest value: {dev_err:.2e}")
    print(json.dumps({"tool": "regrid_time", "grid": [H, W], "target": [Ho, Wo], "members": M, "channels": C, "reps": args.reps,
                      "ratio_torch_over_kernel": round(ratio, 3), "cases": res}))


if __name__ == "__main__":
    main()
