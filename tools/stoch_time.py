"""ms of one member's stochastic step at 69 x 721 x 1440 and lmax 256, with the coefficient states of M = 50 members allocated (49
perturbed members: 1.8 GB with the additive term's 69 fields): ``stoch_evolve`` of the additive fields (F = 69) and of the SPPT pattern
(F = 1), the two-GEMM synthesis of each, and ``stoch_apply`` for each kind -- against the device-to-device copy rate, which this script
measures itself, and against a torch chain of the same arithmetic on the same tensors (the autoregressive step given the fresh draw, and
the SPPT / additive step).  No model runs.  The measurements alternate in one process, each between device events, after warm-up;
prints the medians, the bytes each launch has to move, its share of the copy rate, and one JSON line.

    timeout -k 10 600 python tools/stoch_time.py [--reps 20] [--warmup 3] [--members 50]
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
from skyrim_amd import noise as N  # noqa: E402
from skyrim_amd import stochastic as S  # noqa: E402
from skyrim_amd.pangu.spec import PanguGeometry, synthetic_state  # noqa: E402


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
    ap.add_argument("--lmax", type=int, default=256)
    args = ap.parse_args()
    dev, M, lmax = "cuda:0", args.members, args.lmax
    g = PanguGeometry(721, 1440)
    C, H, W = 69, g.n_lat, g.n_lon
    hw = H * W
    xp = synthetic_state(g, 0).to(dev).contiguous().reshape(C, H, W)
    std = xp.reshape(C, -1).std(dim=1).contiguous()
    xn = torch.empty_like(xp)
    E.perturb(xp, std, xn, hw, 1e-2, 1, 1)                                  # a stand-in for the model's step
    out = torch.empty_like(xp)
    state = xp.numel() * 4
    sigma64 = N.spectrum(lmax)
    e = N.scale_exponent(sigma64)
    sigma = torch.from_numpy((sigma64 * 2.0 ** e).astype(np.float32)).to(dev)
    synth = N.synthesis(dev, H, H, W, lmax)
    phi, psi = S.ar1(6.0, 6.0)
    gs = torch.full((C,), float(np.float32(0.3 * 2.0 ** -e)), dtype=torch.float32, device=dev)
    ga = N.amplitudes(std, 1e-3, e)
    buf = {}
    for name, F, f_first in (("additive", C, 0), ("sppt", 1, C)):
        nc, nt, ny = synth.sizes(F)
        coef = torch.empty((M - 1, nc), dtype=torch.float32, device=dev)   # every member's state, as the rollout holds them
        S.coeffs(coef, sigma, F, f_first, 0, 1, 1)
        buf[name] = dict(F=F, f_first=f_first, coef=coef, t=torch.empty(nt, dtype=torch.float32, device=dev),
                         y=torch.empty(ny, dtype=torch.float32, device=dev), fresh=torch.empty(nc, dtype=torch.float32, device=dev), nc=nc)
        S.coeffs(buf[name]["fresh"], sigma, F, f_first, 0, 1, 2)
        synth.run(coef[0], buf[name]["t"], buf[name]["y"], F)
    held = sum(b["coef"].numel() * 4 for b in buf.values())
    r, y = buf["sppt"]["y"], buf["additive"]["y"]
    copy_src, copy_dst = torch.empty(8 * xp.numel(), dtype=torch.float32, device=dev), torch.empty(8 * xp.numel(), dtype=torch.float32, device=dev)
    gs3, ga3, r3, y3 = gs.reshape(C, 1, 1), ga.reshape(C, 1, 1), r.reshape(1, H, W), y.reshape(C, H, W)
    draw = [2]

    def evolve(name):
        b = buf[name]
        draw[0] += 1
        S.evolve(b["coef"][0], sigma, b["F"], b["f_first"], 0, 1, draw[0], phi, psi)

    def torch_ar1():                                                       # the autoregressive arithmetic alone, the fresh draw given
        b = buf["additive"]
        b["coef"][1].mul_(phi).add_(b["fresh"] * psi)

    def torch_apply(sppt, add):
        t = xn
        if sppt:
            t = torch.addcmul(xn, (gs3 * r3).clamp(-0.9, 0.9), xn - xp)
        if add:
            t = torch.addcmul(t, ga3, y3)
        out.copy_(t)

    cases = {
        "copy (8 states)": (lambda: copy_dst.copy_(copy_src), 2 * 8 * state),
        "stoch_evolve F=69": (lambda: evolve("additive"), 2 * buf["additive"]["nc"] * 4),
        "stoch_evolve F=1": (lambda: evolve("sppt"), 2 * buf["sppt"]["nc"] * 4),
        "synthesis F=69": (lambda: synth.run(buf["additive"]["coef"][0], buf["additive"]["t"], y, C), None),
        "synthesis F=1": (lambda: synth.run(buf["sppt"]["coef"][0], buf["sppt"]["t"], r, 1), None),
        "stoch_apply sppt": (lambda: S.apply(xp, xn, r, None, gs, None, 0.9, out, hw), 3 * state + hw * 4),
        "stoch_apply additive": (lambda: S.apply(None, xn, None, y, None, ga, 0.9, out, hw), 3 * state),
        "stoch_apply both": (lambda: S.apply(xp, xn, r, y, gs, ga, 0.9, out, hw), 4 * state + hw * 4),
        "torch ar1 F=69 (fresh given)": (torch_ar1, None),
        "torch apply sppt": (lambda: torch_apply(True, False), None),
        "torch apply additive": (lambda: torch_apply(False, True), None),
        "torch apply both": (lambda: torch_apply(True, True), None),
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
        line = f"{k:>30}: median {med:8.3f} ms (min {min(times[k]):.3f}, max {max(times[k]):.3f})"
        if nbytes is not None:
            rate = nbytes / (med * 1e-3)
            res[k].update(bytes=nbytes, share_of_copy_rate=round(rate / copy_rate, 4))
            line += f"; {nbytes / 1e6:.1f} MB moved, {rate / 1e12:.2f} TB/s = {100 * rate / copy_rate:.1f} % of the copy rate"
        print(line)
    ms = lambda k: res[k]["ms_median"]               # noqa: E731
    ratios = {k: round(ms(f"torch apply {k}") / ms(f"stoch_apply {k}"), 3) for k in ("sppt", "additive", "both")}
    per_member = {"sppt": ms("stoch_evolve F=1") + ms("synthesis F=1") + ms("stoch_apply sppt"),
                  "additive": ms("stoch_evolve F=69") + ms("synthesis F=69") + ms("stoch_apply additive"),
                  "both": ms("stoch_evolve F=1") + ms("synthesis F=1") + ms("stoch_evolve F=69") + ms("synthesis F=69") + ms("stoch_apply both")}
    print(f"torch chain / kernel (apply): {ratios}; copy rate {copy_rate / 1e12:.2f} TB/s; coefficient states held: {held / 1e9:.2f} GB")
    print("per member and step (evolve + synthesis + apply): " + ", ".join(f"{k} {v:.2f} ms" for k, v in per_member.items()))
    print(json.dumps({"tool": "stoch_time", "grid": [C, H, W], "lmax": lmax, "members": M, "reps": args.reps,
                      "copy_rate_TBps": round(copy_rate / 1e12, 3), "coefficient_state_GB": round(held / 1e9, 3),
                      "torch_over_kernel_apply": ratios, "ms_per_member_step": {k: round(v, 3) for k, v in per_member.items()}, "cases": res}))


if __name__ == "__main__":
    main()
