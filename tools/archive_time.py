"""ms of ``pack_range``, ``pack_quantize`` (50 members x 69 channels at 721 x 1440) and ``pack_unpack`` (one state), next to a torch chain
that makes the same codes member by member (``amin`` / ``amax``, subtract, multiply, round, clamp, ``to(int16)``, byte swap), to the
tool's own measured device copy rate, and to what the packing saves: the device-to-host copy of the same members as float32 into pinned
memory (and of the int16 image, half the bytes).  The measurements alternate in one process, each between device events (the copies: a
host clock around work that ends in a synchronise), after warm-up; a measurement is a batch of calls sized so that its window is some
milliseconds long (``--window_ms``).  With ``--ensemble`` (synthetic weights and initial condition) it then times a saving ensemble of the
full-size Pangu with no archive, with ``float32`` and with ``int16``: ms per lead, host clock, files into ``--dir``.  Prints the medians,
the ratios and one JSON line.

    timeout -k 10 900 python tools/archive_time.py [--reps 7] [--warmup 2] [--members 50] [--channels 69] [--ensemble] [--dir DIR]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import tempfile
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
os.environ.setdefault("SKYRIM_SYNTHETIC_IC", "1")
os.environ.setdefault("SKYRIM_SYNTHETIC_WEIGHTS", "1")

from skyrim_amd import archive as A  # noqa: E402
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


def _clocked(fn, batch):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(batch):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3 / batch


def torch_codes(x, out):
    """The codes of one state (C, H, W) with torch ops, as big-endian int16 in ``out`` (C, H W): the arithmetic of the header in double
    would double the traffic again; this chain stays in float32, which is what a user would write (the codes differ in a few places)."""
    v = x.reshape(x.shape[0], -1)
    lo, hi = v.amin(dim=1, keepdim=True), v.amax(dim=1, keepdim=True)
    d = hi - lo
    inv = torch.where(d > 0, 65534.0 / d, torch.ones_like(d))
    c = ((v - (0.5 * lo + 0.5 * hi)) * inv).round().clamp(-32767, 32767).to(torch.int16)
    out.copy_((c << 8) | ((c >> 8) & 0xFF))


def ensemble_ms(kind, members, steps, directory):
    """ms per lead of ``ensemble_forecast(save=True)`` of the full-size Pangu with synthetic weights: ``kind`` None, "float32" or "int16"."""
    from skyrim_amd.core.models.pangu import PanguModel
    from skyrim_amd.pangu.engine import DEFAULT_PRECISION
    from skyrim_amd.pangu.spec import PanguGeometry, init_synthetic
    import datetime
    g = PanguGeometry(H, W)
    model = ensemble_ms.model = getattr(ensemble_ms, "model", None) or PanguModel(
        ic_source="synthetic", geom=g, params=init_synthetic(g, 0), precision=DEFAULT_PRECISION, device=torch.device("cuda", 0))
    kw = dict(n_steps=steps, n_members=members, products=("mean", "spread"), save=True, save_config=dict(output_dir=str(directory)))
    if kind is not None:
        kw["archive"] = dict(packing=kind)
    torch.cuda.synchronize()
    t = time.perf_counter()
    model.ensemble_forecast(datetime.datetime(2024, 5, 13, 18, 0), **kw)
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3 / (steps + 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--members", type=int, default=50)
    ap.add_argument("--channels", type=int, default=69)
    ap.add_argument("--window_ms", type=float, default=50.0)
    ap.add_argument("--ensemble", action="store_true", help="also time a saving ensemble (synthetic weights) with and without an archive")
    ap.add_argument("--ens_members", type=int, default=4)
    ap.add_argument("--ens_steps", type=int, default=2)
    ap.add_argument("--dir", type=str, default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("archive_time measures on a GPU: none is visible")
    dev, M, C = torch.device("cuda:0"), args.members, args.channels
    gen = torch.Generator(device=dev).manual_seed(0)
    scale = torch.logspace(-3, 5, C, device=dev)[:, None, None]
    members = [torch.randn((C, H, W), generator=gen, device=dev) * scale + scale for _ in range(M)]
    table, ch = member_table(members), list(range(C))
    tab = A.new_table(M, C, dev)
    ws = torch.empty(A.workspace_bytes(M, C, H, W), dtype=torch.uint8, device=dev)
    image = torch.empty((M, 2 * C * H * W), dtype=torch.uint8, device=dev)
    back = torch.empty((C, H, W), dtype=torch.float32, device=dev)
    timage = torch.empty((C, H * W), dtype=torch.int16, device=dev)
    src, dst = torch.empty(1 << 28, device=dev), torch.empty(1 << 28, device=dev)              # 1 GiB each
    pin32 = torch.empty(C * H * W, dtype=torch.float32).pin_memory()
    pin16 = torch.empty(2 * C * H * W, dtype=torch.uint8).pin_memory()

    def chain():
        for x in members:
            torch_codes(x, timage)

    def d2h32():
        for x in members:
            pin32.copy_(x.reshape(-1), non_blocking=True)

    def d2h16():
        for m in range(M):
            pin16.copy_(image[m], non_blocking=True)
    cases = {
        "pack_range": (lambda: A.run_range(members, table, ch, tab, ws), _timed),
        "pack_quantize": (lambda: A.run_quantize(members, table, ch, tab, image), _timed),
        "pack_unpack (one state)": (lambda: A.run_unpack(image[0], tab[0], back), _timed),
        "torch chain": (chain, _timed),
        "device copy 1 GiB": (lambda: dst.copy_(src), _timed),
        "float32 members to pinned host": (d2h32, _clocked),
        "int16 image to pinned host": (d2h16, _clocked),
    }
    for _ in range(args.warmup):
        for fn, _t in cases.values():
            fn()
    torch.cuda.synchronize()
    torch_codes(members[0], timage)
    mine = image[0].view(torch.int16).view(C, H * W)
    differ = float((mine != timage).float().mean().item())          # the fraction of codes where the float32 chain rounds otherwise
    batch = {}
    for k, (fn, timer) in cases.items():
        probe = timer(fn, 1)
        batch[k] = max(1, min(500, int(round(args.window_ms / max(probe, 1e-4)))))
    times = {k: [] for k in cases}
    for _ in range(args.reps):
        for k, (fn, timer) in cases.items():
            times[k].append(timer(fn, batch[k]))
    res = {}
    for k in cases:
        med = statistics.median(times[k])
        res[k] = {"ms_median": round(med, 4), "ms_min": round(min(times[k]), 4), "ms_max": round(max(times[k]), 4), "batch": batch[k]}
        print(f"{k:>34}: median {med:10.4f} ms (min {min(times[k]):.4f}, max {max(times[k]):.4f}; {batch[k]} calls per measurement)")
    n = M * C * H * W
    rate = 2 * 4 * (1 << 28) / (res["device copy 1 GiB"]["ms_median"] * 1e-3)                 # bytes read + written per second
    ms = {k: v["ms_median"] for k, v in res.items()}
    pack = ms["pack_range"] + ms["pack_quantize"]
    summary = {"copy_GBps": round(rate / 1e9, 1),
               "range_fraction_of_copy_rate": round(4 * n / (ms["pack_range"] * 1e-3) / rate, 3),
               "quantize_fraction_of_copy_rate": round(6 * n / (ms["pack_quantize"] * 1e-3) / rate, 3),
               "unpack_fraction_of_copy_rate": round(6 * C * H * W / (ms["pack_unpack (one state)"] * 1e-3) / rate, 3),
               "torch_chain_over_pack": round(ms["torch chain"] / pack, 1),
               "float32_d2h_GBps": round(4 * n / (ms["float32 members to pinned host"] * 1e-3) / 1e9, 1),
               "float32_d2h_over_pack": round(ms["float32 members to pinned host"] / pack, 1),
               "pack_plus_int16_d2h_over_float32_d2h": round((pack + ms["int16 image to pinned host"]) / ms["float32 members to pinned host"], 3),
               "codes_differing_from_float32_chain": differ}
    print(f"copy rate {summary['copy_GBps']} GB/s; range / quantize / unpack move their bytes at {summary['range_fraction_of_copy_rate']:.2f} / "
          f"{summary['quantize_fraction_of_copy_rate']:.2f} / {summary['unpack_fraction_of_copy_rate']:.2f} of it; torch chain / (range + quantize) "
          f"{summary['torch_chain_over_pack']} x; the float32 copy to the host ({summary['float32_d2h_GBps']} GB/s) takes "
          f"{summary['float32_d2h_over_pack']} x the two pack launches; pack + int16 copy = {summary['pack_plus_int16_d2h_over_float32_d2h']:.2f} of it")
    ens = None
    if args.ensemble:
        del members, image, src, dst, ws
        torch.cuda.empty_cache()
        ens = {}
        for label, kind, members, steps in (("warm-up", None, 2, 1), ("none", None, args.ens_members, args.ens_steps),
                                            ("float32", "float32", args.ens_members, args.ens_steps),
                                            ("int16", "int16", args.ens_members, args.ens_steps),
                                            ("none again", None, args.ens_members, args.ens_steps)):
            with tempfile.TemporaryDirectory(dir=args.dir or None) as d:                      # (each run's files go before the next one starts)
                ens[label] = round(ensemble_ms(kind, members, steps, d), 1)
            print(f"saving ensemble [{label}], {members} members, {steps + 1} leads: {ens[label]} ms per lead", flush=True)
    print(json.dumps({"tool": "archive_time", "grid": [H, W], "members": M, "channels": C, "reps": args.reps, "cases": res, **summary,
                      "ensemble_ms_per_lead": ens}))


if __name__ == "__main__":
    main()
