"""ms of one ``zonal_spectra`` launch at 721 x 1440 with M = 1, 32 and 50 synthetic member states plus a truth (no model), the four default
bands, for 1 and for 8 channels, next to the torch chain on the same tensors (per member ``torch.fft.rfft`` along the longitudes,
``abs() ** 2``, weigh the rows, sum: the ``member`` slot of one band only, float32, each member's planes read once more and a complex
intermediate written per member), and to the copy of ONE member plane to the device's own memory, which gives the copy rate the launch
is compared with.  The measurements alternate in one process, each between device events, after warm-up.  A measurement is a batch of
calls sized so that its window is about ``--window_ms`` long (at least ``--batch`` calls).  Consecutive calls of a case read DIFFERENT
member sets (``--sets`` copies, rotated): one set alone could stay in the 256 MiB Infinity Cache from call to call, which the members of a
forecast, just rewritten by a model step, do not.  Prints the medians and spreads, the ratios, the bytes the launch reads per second,
how far kernel and chain are apart, and one JSON line.

    timeout -k 10 600 python tools/spectra_time.py [--reps 10] [--warmup 2] [--batch 3] [--window_ms 100] [--sets 2]
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
from skyrim_amd import spectra as S  # noqa: E402
from skyrim_amd.verify import area_weights  # noqa: E402

H, W, C = 721, 1440, 8
K = W // 2 + 1


def _timed(fn, batch):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(batch):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / batch


def torch_chain(members, nc, w, ck, out):
    """The ``member`` slot of the globe: per member rfft, |.|^2, weigh the rows, sum; float32 / complex64 throughout."""
    acc = torch.zeros((nc, K), dtype=torch.float32, device=w.device)
    for m in members:
        f = torch.fft.rfft(m[:nc], dim=-1, norm="forward")
        acc += ((f.abs() ** 2) * w[None, :, None]).sum(dim=1)
    out.copy_(acc * ck / (w.sum() * len(members)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=3)
    ap.add_argument("--window_ms", type=float, default=100.0)
    ap.add_argument("--sets", type=int, default=2)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    base = torch.randn((C, H, W), generator=gen, device=dev) * 500.0 + 54000.0
    every = [base + (torch.randn((C, H, W), generator=gen, device=dev) * 40.0 if m else 0.0) for m in range(50)]
    truth = base + torch.randn((C, H, W), generator=gen, device=dev) * 60.0
    sets = [every] + [[t.clone() for t in every] for _ in range(max(args.sets, 1) - 1)]      # the same values at other addresses
    turn = {}

    def rotating(key, fns):
        turn[key] = 0

        def call():
            fns[turn[key] % len(fns)]()
            turn[key] += 1
        return call

    lat = np.linspace(90.0, -90.0, H)
    wrow = area_weights(lat)
    w64 = torch.from_numpy(wrow).to(dev)
    w32 = w64.float()
    ck = torch.full((K,), 2.0, device=dev)
    ck[0] = ck[-1] = 1.0
    rows = [S.band_rows(lat, b) for b in S.DEFAULT_BANDS.values()]
    spare = torch.empty((H, W), dtype=torch.float32, device=dev)
    cases, agree = {}, {}
    for M in (1, 32, 50):
        for nc in (1, 8):
            out = torch.empty((nc, len(rows), 6, K), dtype=torch.float64, device=dev)
            ws = torch.empty(S.workspace_bytes(M, H, W, nc, rows, True) // 8, dtype=torch.float64, device=dev)
            ref = torch.empty((nc, K), dtype=torch.float32, device=dev)
            subs = [(s[:M], E.member_table(s[:M])) for s in sets]
            key = f"M={M} nc={nc}"
            cases[f"zonal_spectra {key}"] = rotating(f"spec{key}", [(lambda mm=mm, tb=tb, out=out, ws=ws, nc=nc: S.zonal(mm, tb, truth, list(range(nc)), rows, w64, out, ws))
                                                                    for mm, tb in subs])
            cases[f"torch chain {key}"] = rotating(f"chain{key}", [(lambda mm=mm, ref=ref, nc=nc: torch_chain(mm, nc, w32, ck, ref)) for mm, _ in subs])
            agree[key] = (out, ref)
    cases["one member plane copied on the device"] = lambda: spare.copy_(every[1][0])
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
    for key in agree:
        cases[f"zonal_spectra {key}"]()
        cases[f"torch chain {key}"]()
    torch.cuda.synchronize()
    globe = list(S.DEFAULT_BANDS).index("globe")
    differ = {k: float(((a[:, globe, 0] - b.double()).abs() / a[:, globe, 0]).max().item()) for k, (a, b) in agree.items()}
    times = {k: [] for k in cases}
    for _ in range(args.reps):                       # alternating: every case sees the same clocks and the same neighbours
        for k, fn in cases.items():
            times[k].append(_timed(fn, batch[k]))
    res = {}
    for k in cases:
        med = statistics.median(times[k])
        res[k] = {"ms_median": round(med, 4), "ms_min": round(min(times[k]), 4), "ms_max": round(max(times[k]), 4), "batch": batch[k]}
        print(f"{k:>40}: median {med:9.4f} ms (min {min(times[k]):.4f}, max {max(times[k]):.4f}; {batch[k]} calls per measurement)")
    copy = res["one member plane copied on the device"]["ms_median"]
    plane = H * W * 4
    print(f"copy rate: {2 * plane / (copy * 1e-3) / 1e9:.0f} GB/s (read + write of one plane)")
    for key in agree:
        M, nc = (int(v.split("=")[1]) for v in key.split())
        g, c = res[f"zonal_spectra {key}"]["ms_median"], res[f"torch chain {key}"]["ms_median"]
        gbs = (M + 1) * nc * plane / (g * 1e-3) / 1e9
        print(f"{key}: torch chain (one slot, one band) / zonal_spectra (six slots, four bands) {c / g:.2f} x; the launch reads {gbs:.0f} GB/s of members "
              f"and truth; largest relative difference of the member slot, kernel - chain, {differ[key]:.3g}")
    print(json.dumps({"tool": "spectra_time", "grid": [H, W], "reps": args.reps, "window_ms": args.window_ms, "sets": len(sets),
                      "relative_difference": differ, "cases": res}))


if __name__ == "__main__":
    main()
