"""ms of the three weather-object launches at 721 x 1440 with M = 50 synthetic planes (no model), one threshold and then four, on a smooth
field (a few large objects), a noisy field (many small ones) and a field that is ONE object (every point above the threshold: the
worst case for the atomics of the attributes) -- next to two baselines: the measured device copy rate over the bytes each launch must
move, and what the feature replaces: copying the planes to the host and labelling them there (``scipy.ndimage.label`` + ``ndimage.sum``
when scipy imports, else the numpy flood fill of tests/_object_reference.py), measured on ``--host_members`` members and scaled to M.
The device measurements alternate in one process between device events; prints the medians and one JSON line.

    timeout -k 10 600 python tools/object_time.py [--reps 5] [--warmup 1] [--members 50] [--host_members 2]
"""
from __future__ import annotations

import argparse
import json
import math
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from skyrim_amd import objects as O  # noqa: E402
from skyrim_amd.members import member_table  # noqa: E402

HOST_COPY_MS = 5.0                                              # one member (69 x 721 x 1440 fp32) to pinned host memory, docs/experiments.md


def _timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def fields(kind, M, H, W, dev):
    """M (1, H, W) planes with values around 0: ``smooth`` -- a few waves per member; ``noisy`` -- the same plus white noise of equal
    size; ``one`` -- the smooth field lifted above every threshold."""
    gen = torch.Generator(device=dev).manual_seed(1)
    la = torch.linspace(math.pi / 2, -math.pi / 2, H, device=dev)[:, None]
    lo = torch.arange(W, device=dev)[None, :] * (2 * math.pi / W)
    out = []
    for m in range(M):
        x = torch.zeros((H, W), device=dev)
        for k in range(1, 5):
            ph = torch.rand(2, generator=gen, device=dev) * 2 * math.pi
            x += torch.cos(k * lo + ph[0] + 0.1 * m) * torch.cos((k + 1) * la + ph[1]) / k
        if kind == "noisy":
            x += torch.randn((H, W), generator=gen, device=dev)
        if kind == "one":
            x += 100.0
        out.append(x[None].contiguous())
    return out


def host_route(members, thresholds, n):
    """ms per member of: the plane to the host, then per threshold the labels, the point counts and the value sums there."""
    try:
        from scipy import ndimage
        eight = np.ones((3, 3), int)

        def work(v, thr):
            lab, k = ndimage.label(v >= thr, eight)
            ndimage.sum(v, lab, np.arange(1, k + 1))
        how = "scipy.ndimage.label + ndimage.sum"
    except ImportError:
        sys.path.insert(0, str(ROOT / "tests"))
        import _object_reference as R

        def work(v, thr):
            ids, k, _ = R.number(R.flood_labels(v >= thr, 8, False), 1, 1 << 20)
            np.bincount(ids.ravel(), weights=v.ravel())
        how = "numpy flood fill (scipy does not import)"
    torch.cuda.synchronize()
    t = time.perf_counter()
    for m in range(n):
        v = members[m][0].cpu().numpy()
        for thr in thresholds:
            work(v, thr)
    return (time.perf_counter() - t) * 1e3 / n, how


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--members", type=int, default=50)
    ap.add_argument("--host_members", type=int, default=2)
    args = ap.parse_args()
    dev, M, H, W, cap = torch.device("cuda:0"), args.members, 721, 1440, 1 << 17
    N = H * W
    g = O.tables(np.linspace(90.0, -90.0, H), np.arange(W) * 360.0 / W)
    row, col = torch.from_numpy(g.row).to(dev), torch.from_numpy(g.col).to(dev)
    # the copy rate: a device-to-device copy of 512 MiB reads and writes that many bytes
    src = torch.empty(512 << 20, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    for _ in range(2):
        dst.copy_(src)
    rate = 2 * src.numel() / (statistics.median(_timed(lambda: dst.copy_(src)) for _ in range(5)) * 1e-3)       # bytes / s
    del src, dst
    print(f"device copy rate {rate / 1e12:.2f} TB/s (read + write); one member to the host takes {HOST_COPY_MS} ms")
    res, notes = {}, []
    for P in (1, 4):
        thresholds = [0.5, 0.0, 1.0, -0.5][:P]
        spec = [(0, float(t), 1, 8, O.value_scale(t)) for t in thresholds]
        labels = torch.empty((M, P, H, W), dtype=torch.int32, device=dev)
        ids = torch.empty_like(labels)
        n_found = torch.empty((M, P), dtype=torch.int32, device=dev)
        ws = torch.empty(O.workspace_bytes(M, P, H, W), dtype=torch.uint8, device=dev)
        records = torch.empty(M * P * cap * 128, dtype=torch.uint8, device=dev)
        keep = torch.ones((M, P, cap + 1), dtype=torch.uint8, device=dev)
        keep[:, :, 0] = 0
        counts = torch.empty((P, H, W), dtype=torch.int32, device=dev)
        # what each launch must move at the least: the field once per plane, the planes it writes or reads once
        must = {"label": M * P * N * 4 * 3, "attributes": M * P * N * 4 * 2, "probability": (M + 1) * P * N * 4}
        for kind in ("smooth", "noisy", "one"):
            members = fields(kind, M, H, W, dev)
            table = member_table(members)
            cases = {"label": lambda: O.label(members, table, spec, True, 1, cap, labels, ids, n_found, ws),
                     "attributes": lambda: O.attributes(members, table, spec, cap, labels, ids, n_found, row, col, records),
                     "probability": lambda: O.probability(ids, keep, counts)}
            times = {k: [] for k in cases}
            for _ in range(args.warmup):
                for fn in cases.values():
                    fn()
            torch.cuda.synchronize()
            for _ in range(args.reps):                          # alternating: every case sees the same clocks and the same neighbours
                for k, fn in cases.items():
                    times[k].append(_timed(fn))
            found = n_found.cpu().numpy()
            host_ms, how = host_route(members, thresholds, min(args.host_members, M)) if kind != "one" else (None, "")
            total = 0.0
            for k in cases:
                med = statistics.median(times[k])
                total += med
                share = 100.0 * (must[k] / rate * 1e3) / med
                res[f"P={P} {kind} {k}"] = {"ms_median": round(med, 4), "ms_min": round(min(times[k]), 4), "ms_max": round(max(times[k]), 4),
                                            "bytes_must": must[k], "percent_of_copy_rate": round(share, 1)}
                print(f"P={P} {kind:>6} {k:>12}: median {med:9.3f} ms (min {min(times[k]):.3f}, max {max(times[k]):.3f}), must move "
                      f"{must[k] / 1e6:7.1f} MB: {share:5.1f} % of the copy rate")
                if med > HOST_COPY_MS:
                    notes.append(f"P={P} {kind} {k}: {med:.2f} ms is longer than copying one member to the host ({HOST_COPY_MS} ms)")
            print(f"P={P} {kind:>6}: objects found per member and plane: mean {found.mean():.0f}, max {found.max()}"
                  + (f" (capacity {cap}: {int((found > cap).sum())} entries truncated)" if (found > cap).any() else ""))
            if host_ms is not None:
                res[f"P={P} {kind} host route"] = {"ms_per_member": round(host_ms, 2), "ms_all_members": round(host_ms * M, 1), "how": how,
                                                   "device_speedup": round(host_ms * M / total, 1)}
                print(f"P={P} {kind:>6}   host route ({how}): {host_ms:.1f} ms per member, {host_ms * M:.0f} ms for {M}: "
                      f"{host_ms * M / total:.0f} x the {total:.2f} ms of the three launches")
            del members, table
        one, smooth = res[f"P={P} one attributes"]["ms_median"], res[f"P={P} smooth attributes"]["ms_median"]
        notes.append(f"P={P}: attributes on ONE object per plane take {one / smooth:.2f} x the time of the smooth field"
                     + (": atomic-bound on the one record" if one > 1.5 * smooth else ": the wave reduction keeps the one record out of the way"))
        del labels, ids, ws, records
    for n in notes:
        print(n)
    print(json.dumps({"tool": "object_time", "grid": [H, W], "members": M, "reps": args.reps, "copy_rate_TBps": round(rate / 1e12, 3),
                      "cases": res, "notes": notes}))


if __name__ == "__main__":
    main()
