"""ms of ONE ``derive_fields`` launch at 721 x 1440 with M = 50 synthetic member states on Pangu's channel layout (no model) for
["ws10m", "ivt", "iwv", "vo850", "div850"], next to a torch chain that computes the same fields on the same tensors.  The measurements
alternate in one process, each between device events, after warm-up; prints the medians, the bytes the kernel must move
(M x (input planes + output planes) x H x W x 4), its share of the measured copy rate, the ratio to the torch chain, and one JSON line.

    timeout -k 10 600 python tools/derive_time.py [--reps 20] [--warmup 3] [--members 50]
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

from skyrim_amd import derived as D  # noqa: E402
from skyrim_amd import ensemble as E  # noqa: E402
from skyrim_amd.pangu.spec import CHANNELS, PanguGeometry, synthetic_state  # noqa: E402

COPY_RATE = 6.29e12          # bytes / s: the measured device-to-device copy rate of an MI355X (tools/ens_time.py)
FIELDS = ["ws10m", "ivt", "iwv", "vo850", "div850"]


def _timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def torch_chain(members, plan, rowc, out):
    """The same fields with torch ops, member after member (interior rows of vo / div; the pole rows are left out: less work)."""
    names = list(CHANNELS)
    w = torch.tensor([float(np.float32(x)) for x in plan.weights], device=rowc.device).view(-1, 1, 1)
    q, u, v = ([names.index(f"{x}{l}") for l in plan.levels] for x in "quv")
    A, Bp, Bm = rowc[:, 0:1], rowc[:, 1:2], rowc[:, 2:3]
    for m, s in enumerate(members):
        out[m, 0] = torch.sqrt(s[names.index("u10m")] ** 2 + s[names.index("v10m")] ** 2)
        t = w * s[q]
        out[m, 1] = torch.sqrt((t * s[u]).sum(0) ** 2 + (t * s[v]).sum(0) ** 2)
        out[m, 2] = t.sum(0)
        u8, v8 = s[names.index("u850")], s[names.index("v850")]
        un, us, vn, vs = torch.roll(u8, -1, 0), torch.roll(u8, 1, 0), torch.roll(v8, -1, 0), torch.roll(v8, 1, 0)
        out[m, 3] = A * (torch.roll(v8, -1, 1) - torch.roll(v8, 1, 1)) - (Bp * un - Bm * us)
        out[m, 4] = A * (torch.roll(u8, -1, 1) - torch.roll(u8, 1, 1)) + (Bp * vn - Bm * vs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--members", type=int, default=50)
    args = ap.parse_args()
    dev, M = "cuda:0", args.members
    g = PanguGeometry(721, 1440)
    H, W = g.n_lat, g.n_lon
    lat, lon = np.linspace(90.0, -90.0, H), np.arange(W) * (360.0 / W)
    x0 = synthetic_state(g, 0).to(dev).reshape(len(CHANNELS), H, W).contiguous()
    members = [x0 * (1.0 + 1e-3 * m) for m in range(M)]
    table = E.member_table(members)
    deriver = D.LeadDeriver(CHANNELS, lat, lon, M, FIELDS, dev)
    plan = deriver.plan
    planes_in = len({c for f in FIELDS for c in plan.inputs[f]})
    nbytes = M * (planes_in + len(FIELDS)) * H * W * 4
    rowc = torch.from_numpy(plan.rowc).to(dev)
    out = torch.empty((M, len(FIELDS), H, W), dtype=torch.float32, device=dev)
    cases = {"derive_fields (one launch)": (lambda: deriver.add(members, table), nbytes),
             "torch chain": (lambda: torch_chain(members, plan, rowc, out), None)}
    times = {k: [] for k in cases}
    for _ in range(args.warmup):
        for fn, _b in cases.values():
            fn()
    torch.cuda.synchronize()
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
    ratio = res["torch chain"]["ms_median"] / res["derive_fields (one launch)"]["ms_median"]
    print(f"torch chain / derive_fields: {ratio:.2f} x")
    print(json.dumps({"tool": "derive_time", "grid": [H, W], "members": M, "fields": FIELDS, "input_planes": planes_in, "reps": args.reps,
                      "ratio_torch_over_kernel": round(ratio, 3), "cases": res}))


if __name__ == "__main__":
    main()
