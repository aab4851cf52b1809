"""ms of one ``gram`` launch at 721 x 1440 with M = 50 synthetic member states of one channel (no model) over the globe -- the
three-block path, 4326 tiles -- and at M = 32 (one block), next to the torch chain on the same tensors (stack the members' planes,
subtract member 0, weigh the rows, ``A @ A.T`` in float32: one more pass over the members plus the allocation, then a vendor GEMM whose
summation order is its own), to one ``member_combine`` of 3 patterns, and to the copy of ONE member plane to the host, which is what
clustering on the host would pay per member, channel and lead time.  The measurements alternate in one process, each between device
events, after warm-up.  A measurement is a batch of calls sized so that its window is about ``--window_ms`` long (at least ``--batch``
calls).  Consecutive calls of a case read DIFFERENT member sets (``--sets`` copies of the 208 MB, rotated; 4 sets = 830 MB): one set alone
would stay in the 256 MiB Infinity Cache from call to call, which the members of a forecast, just rewritten by a model step, do not.
Prints the medians and spreads, the ratios, how far the kernel and the chain are apart relative to the diagonal, and one JSON line.

    timeout -k 10 600 python tools/gram_time.py [--reps 20] [--warmup 3] [--batch 5] [--window_ms 100] [--sets 4]
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
from skyrim_amd import scenarios as S  # noqa: E402
from skyrim_amd.verify import area_weights  # noqa: E402

H, W = 721, 1440


def _timed(fn, batch):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(batch):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / batch


def torch_chain(members, w, out):
    """Stack, subtract member 0, weigh, multiply: float32 throughout, the product accumulated by the vendor GEMM."""
    A = torch.stack([m[0] for m in members]).reshape(len(members), -1)
    A = A - A[0]
    out.copy_((A * w) @ A.T)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=5)
    ap.add_argument("--window_ms", type=float, default=100.0)
    ap.add_argument("--sets", type=int, default=4)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    base = torch.randn((1, H, W), generator=gen, device=dev) * 500.0 + 54000.0
    every = [base + (torch.randn((1, H, W), generator=gen, device=dev) * 40.0 if m else 0.0) for m in range(50)]
    sets = [every] + [[t.clone() for t in every] for _ in range(max(args.sets, 1) - 1)]      # the same values at other addresses
    turn = {}

    def rotating(key, fns):
        """One callable that runs fns[0], fns[1], ... in turn: consecutive calls touch different member sets."""
        turn[key] = 0

        def call():
            fns[turn[key] % len(fns)]()
            turn[key] += 1
        return call

    wrow = area_weights(np.linspace(90.0, -90.0, H))
    w64 = torch.from_numpy(wrow).to(dev)
    w32 = torch.from_numpy(np.repeat(wrow, W).astype(np.float32)).to(dev)
    pinned = torch.empty((H, W), dtype=torch.float32, pin_memory=True)
    cases, agree = {}, {}
    for M in (50, 32):
        out = torch.empty((1, M, M), dtype=torch.float64, device=dev)
        ws = torch.empty(S.workspace_bytes(M, 1, H, W) // 8, dtype=torch.float64, device=dev)
        ref = torch.empty((M, M), dtype=torch.float32, device=dev)
        subs = [(s[:M], E.member_table(s[:M])) for s in sets]
        cases[f"gram M={M}"] = rotating(f"gram{M}", [(lambda mm=mm, tb=tb, out=out, ws=ws: S.gram(mm, tb, None, [0], (0, H, 0, W), w64, out, ws))
                                                     for mm, tb in subs])
        cases[f"torch chain M={M}"] = rotating(f"chain{M}", [(lambda mm=mm, ref=ref: torch_chain(mm, w32, ref)) for mm, _ in subs])
        agree[f"M={M}"] = (out, ref)
    full = [(s, E.member_table(s)) for s in sets]
    coef = torch.randn((3, 50), generator=gen, device=dev)
    pat = torch.empty((3, 1, H, W), dtype=torch.float32, device=dev)
    zero = torch.zeros(3, dtype=torch.float32, device=dev)
    cases["member_combine K=3 M=50"] = rotating("combine", [(lambda mm=mm, tb=tb: S.combine(mm, tb, [0], coef, zero, pat)) for mm, tb in full])
    cases["one member plane to the host (pinned)"] = lambda: pinned.copy_(every[0][0], non_blocking=True)
    for _ in range(args.warmup):
        for fn in cases.values():
            fn()
    torch.cuda.synchronize()
    batch = {}
    for k, fn in cases.items():                      # one probe per case sizes its batch: every timed window is about window_ms long
        probe = _timed(fn, args.batch)
        batch[k] = max(args.batch, min(2000, int(round(args.window_ms / max(probe, 1e-4)))))
    for k in turn:                                   # the comparison below: both paths on the same set
        turn[k] = 0
    for M in (50, 32):
        cases[f"gram M={M}"]()
        cases[f"torch chain M={M}"]()
    differ = {k: float(((a[0] - b.double()).abs().max() / a[0].diagonal().max()).item()) for k, (a, b) in agree.items()}
    times = {k: [] for k in cases}
    for _ in range(args.reps):                       # alternating: every case sees the same clocks and the same neighbours
        for k, fn in cases.items():
            times[k].append(_timed(fn, batch[k]))
    res = {}
    for k in cases:
        med = statistics.median(times[k])
        res[k] = {"ms_median": round(med, 4), "ms_min": round(min(times[k]), 4), "ms_max": round(max(times[k]), 4), "batch": batch[k]}
        print(f"{k:>40}: median {med:9.4f} ms (min {min(times[k]):.4f}, max {max(times[k]):.4f}; {batch[k]} calls per measurement)")
    copy = res["one member plane to the host (pinned)"]["ms_median"]
    for M in (50, 32):
        g, c = res[f"gram M={M}"]["ms_median"], res[f"torch chain M={M}"]["ms_median"]
        gbs = M * H * W * 4 / (g * 1e-3) / 1e9
        print(f"M={M}: torch chain / gram {c / g:.2f} x; {M} planes to the host / gram {M * copy / g:.0f} x; gram reads {gbs:.0f} GB/s; "
              f"largest difference kernel - chain {differ[f'M={M}']:.3g} of the largest diagonal entry")
    print(json.dumps({"tool": "gram_time", "grid": [H, W], "reps": args.reps, "window_ms": args.window_ms, "sets": len(sets),
                      "relative_difference": differ,
                      "cases": res}))


if __name__ == "__main__":
    main()
