"""ms of one ``clim_extremes`` launch (50 members, 101 levels, one field at 721 x 1440; EFI alone, and with two SOT tails and two
percentiles) and of one ``clim_quantiles`` launch (1000 samples, 101 levels, the same grid), next to the torch chains on the same tensors --
``(x[:, None] <= c[None]).sum(0)`` plus the closed form of the index, and ``torch.quantile`` over the samples in the largest pieces it
takes -- and to the tool's own measured device copy rate.  The measurements alternate in one process, each between device events, after
warm-up; a measurement is a batch of calls sized so that its window is some milliseconds long (``--window_ms``).  Prints the medians, the
ratios, the fraction of the copy rate the extremes kernel's bytes reach, and one JSON line.

    timeout -k 10 600 python tools/extremes_time.py [--reps 10] [--warmup 2] [--members 50] [--levels 101] [--samples 1000]
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

from skyrim_amd import climate as K  # noqa: E402
from skyrim_amd.members import member_table  # noqa: E402

H, W = 721, 1440


def _timed(fn, batch):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(batch):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / batch


def torch_efi(x, c, tab, M):
    """The index with torch ops: the counts as one broadcast comparison, then the header's closed form over the intervals."""
    F = (x[:, None] <= c[None]).sum(0).to(torch.float32) / M               # (Q, HW)
    p, A, B, rdp = tab
    b = (F[1:] - F[:-1]) * rdp[:, None]
    a = F[:-1] - b * p[:-1, None]
    t = (B[:, None] - a * A[:, None]) - b * B[:, None]
    return (t.sum(0) / B.sum()).clamp(-1, 1)


def torch_quantiles(s, levels, piece):
    out = torch.empty((levels.numel(), s.shape[1]), dtype=torch.float32, device=s.device)
    for i in range(0, s.shape[1], piece):                                  # torch.quantile refuses more than 2^24 elements
        out[:, i:i + piece] = torch.quantile(s[:, i:i + piece], levels, dim=0)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--members", type=int, default=50)
    ap.add_argument("--levels", type=int, default=101)
    ap.add_argument("--samples", type=int, default=1000)
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--window_ms", type=float, default=20.0)
    args = ap.parse_args()
    dev, M, Q, N = torch.device("cuda:0"), args.members, args.levels, args.samples
    lev = np.linspace(0.0, 1.0, Q)
    gen = torch.Generator(device=dev).manual_seed(0)
    members = [torch.randn((1, H, W), generator=gen, device=dev) * 1.3 + 0.2 for _ in range(M)]
    clim = torch.sort(torch.randn((1, Q, H, W), generator=gen, device=dev), dim=1).values.contiguous()
    table = member_table(members)
    efi, efi2 = torch.empty((1, H, W), device=dev), torch.empty((1, H, W), device=dev)
    sot, prob = torch.empty((2, 1, H, W), device=dev), torch.empty((2, 1, H, W), device=dev)
    sreq = [K.sot_request(lev, 0.9, M), K.sot_request(lev, 0.1, M)]
    preq = [(K.level_index(lev, 0.99, "t"), False), (K.level_index(lev, 0.05, "t"), True)]
    x, c = torch.stack([m.reshape(-1) for m in members]), clim.reshape(Q, -1)
    t = K.tables(lev)
    tab = tuple(torch.from_numpy(t[k].astype(np.float32)).to(dev) for k in ("p", "A", "B", "rdp"))
    samples = [torch.randn((1, H, W), generator=gen, device=dev) for _ in range(N)]
    stable = member_table(samples)
    built = torch.empty((1, Q, H, W), device=dev)
    s2, tlev = torch.stack([s.reshape(-1) for s in samples]), torch.from_numpy(lev.astype(np.float32)).to(dev)
    src, dst = torch.empty(1 << 28, device=dev), torch.empty(1 << 28, device=dev)              # 1 GiB each
    cases = {
        "clim_extremes efi": lambda: K.run_extremes(members, table, [0], clim, lev, efi=efi),
        "clim_extremes efi + 2 sot + 2 odds": lambda: K.run_extremes(members, table, [0], clim, lev, None, sreq, preq, efi2, sot, prob),
        "torch chain efi": lambda: torch_efi(x, c, tab, M),
        "clim_quantiles": lambda: K.run_quantiles(samples, stable, [0], lev, built),
        "torch.quantile": lambda: torch_quantiles(s2, tlev, (1 << 24) // N),
        "device copy 1 GiB": lambda: dst.copy_(src),
    }
    for _ in range(args.warmup):
        for fn in cases.values():
            fn()
    torch.cuda.synchronize()
    differ = {"efi": float((efi.reshape(-1) - torch_efi(x, c, tab, M)).abs().max().item()),
              "quantiles": float((built.reshape(Q, -1) - torch_quantiles(s2, tlev, (1 << 24) // N)).abs().max().item())}
    batch = {}
    for k, fn in cases.items():
        probe = _timed(fn, 1)
        batch[k] = max(1, min(500, int(round(args.window_ms / max(probe, 1e-4)))))
    times = {k: [] for k in cases}
    for _ in range(args.reps):
        for k, fn in cases.items():
            times[k].append(_timed(fn, batch[k]))
    res = {}
    for k in cases:
        med = statistics.median(times[k])
        res[k] = {"ms_median": round(med, 4), "ms_min": round(min(times[k]), 4), "ms_max": round(max(times[k]), 4), "batch": batch[k]}
        print(f"{k:>36}: median {med:10.4f} ms (min {min(times[k]):.4f}, max {max(times[k]):.4f}; {batch[k]} calls per measurement)")
    rate = 2 * 4 * (1 << 28) / (res["device copy 1 GiB"]["ms_median"] * 1e-3)                 # bytes read + written per second
    k_ms = res["clim_extremes efi"]["ms_median"]
    k_bytes = (M + Q + 1) * 4 * H * W
    k_pairs = Q * (8 if M <= 8 else 16 if M <= 16 else 32 if M <= 32 else 64) * H * W
    summary = {"copy_GBps": round(rate / 1e9, 1), "extremes_fraction_of_copy_rate": round(k_bytes / (k_ms * 1e-3) / rate, 3),
               "extremes_compare_pairs_per_ns": round(k_pairs / (k_ms * 1e6), 1),
               "torch_chain_over_extremes": round(res["torch chain efi"]["ms_median"] / k_ms, 1),
               "torch_quantile_over_quantiles": round(res["torch.quantile"]["ms_median"] / res["clim_quantiles"]["ms_median"], 1)}
    print(f"copy rate {summary['copy_GBps']} GB/s; clim_extremes moves its {k_bytes / 1e6:.0f} MB at {summary['extremes_fraction_of_copy_rate']:.2f} of it, "
          f"{summary['extremes_compare_pairs_per_ns']} compare-and-add pairs per ns; torch chain / clim_extremes {summary['torch_chain_over_extremes']} x; "
          f"torch.quantile / clim_quantiles {summary['torch_quantile_over_quantiles']} x; largest differences {differ}")
    print(json.dumps({"tool": "extremes_time", "grid": [H, W], "members": M, "levels": Q, "samples": N, "reps": args.reps,
                      "max_abs_difference": differ, "cases": res, **summary}))


if __name__ == "__main__":
    main()
