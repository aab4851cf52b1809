"""ms of ONE ``thermo_fields`` launch at 721 x 1440 with M = 50 synthetic member states on Pangu's channel layout (no model) for
["mucape", "thetae850"] -- one PARCEL op over the 13 levels and one MOIST op -- next to a torch chain that makes the same fields with
torch.exp / torch.log on ``--chain-members`` of the same tensors (the chain is some ten thousand small launches per member, so it is
timed on a few members and scaled to M; the line says so).  The measurements alternate in one process, each between device events,
after warm-up; prints the medians, the operations of include/skyrim_thermo.h the launch performs per second (``OPS_PER_COLUMN``: the
header's + - * / comparisons, selects and conversions of a column whose every node is saturated, a division counted once: a NOMINAL
count made by hand, not a measured instruction rate -- the kernel skips unsaturated nodes and layers below the source) as a share of
the peak fp32 rate of the vector ALUs, the ratio to the torch chain, and one JSON line.

    timeout -k 10 600 python tools/thermo_time.py [--reps 10] [--warmup 2] [--members 50] [--chain-members 2]
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

PEAK_VALU = 78.6e12          # fp32 lane-operations / s of an MI355X: 256 CUs x 128 lanes x 2.4 GHz (an fma would count as one; none is used)
FIELDS = ["mucape", "thetae850"]
NSUB, NITER = 8, 3
# operations of the header per node: four thetae_sat (es 32, w 6, thetae 69, the difference) = 432, three secant updates 24, the guess,
# the environment, the parcel's tv and the trapezoid 64; per level 16, per candidate source 140, the source's constants 170
OPS_PER_NODE, OPS_PER_LEVEL, OPS_PER_CANDIDATE, OPS_SOURCE, OPS_MOIST = 520, 16, 140, 170, 210
EPS, KAPPA, RD = 0.622, 0.2854, 287.04


def _timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def _es(T):
    return 6.112 * torch.exp(17.67 * (T - 273.15) / (T - 29.65))


def _w(e, p):
    e = torch.minimum(e, 0.5 * p) if torch.is_tensor(p) else torch.clamp(e, max=0.5 * p)
    return EPS * e / (p - e)


def _tv(T, w):
    return T * (1 + w / EPS) / (1 + w)


def _tl(T, e):
    le = torch.log(e / 6.112)
    td = 243.5 * le / (17.67 - le) + 273.15
    return 1 / (1 / (td - 56) + torch.log(T / td) / 800) + 56


def _thetae(T, TL, lq, w):
    return T * torch.exp(KAPPA * (1 - 0.28 * w) * lq) * torch.exp((3.376 / TL - 0.00254) * (w * 1000) * (1 + 0.81 * w))


def torch_chain(members, names, levels, out):
    """The same two fields with torch ops, member after member: the algorithm of include/skyrim_thermo.h, the functions torch's own."""
    p = [float(l) for l in levels]
    lnp = [float(np.log(x)) for x in p]
    ln1000 = float(np.log(1000.0))
    ti, qi = ([names.index(f"{x}{l}") for l in levels] for x in "tq")
    ktop = max(k for k in range(len(p)) if p[k] >= 100.0)
    for m, s in enumerate(members):
        t, q = s[ti], s[qi]
        pl = torch.tensor(p, device=s.device).view(-1, 1, 1)
        e = torch.clamp(q * pl / (EPS + 0.378 * q), min=1e-10)
        w = _w(e, pl)
        tve = _tv(t, w)
        cand = [k for k in range(len(p)) if p[k] >= 700.0]
        the_k = torch.stack([_thetae(t[k], _tl(t[k], e[k]), ln1000 - lnp[k], w[k]) for k in cand])
        src = torch.argmax(the_k, 0, keepdim=True)
        T0, e0, w0 = (torch.gather(a[cand], 0, src)[0] for a in (t, e, w))
        lnp_s = torch.tensor(lnp, device=s.device)[src[0]]
        lq_s = ln1000 - lnp_s
        TL = _tl(T0, e0)
        the = _thetae(T0, TL, lq_s, w0)
        th0 = T0 * torch.exp(KAPPA * lq_s)
        lq_lcl = lq_s - torch.log(TL / T0) / KAPPA
        tot, prevB, Tprev = torch.zeros_like(T0), torch.zeros_like(T0), T0.clone()
        lp_prev = None
        for k in range(ktop):
            act = src[0] <= k
            for n in range(1, NSUB + 1):
                lp = lnp[k] + n / NSUB * (lnp[k + 1] - lnp[k])
                pp, lq = float(np.exp(lp)), ln1000 - lp
                tenv = tve[k] + n / NSUB * (tve[k + 1] - tve[k])
                Ta, Tb = Tprev, Tprev * float(np.exp(KAPPA * (lp - (lnp[k] if n == 1 else lp_prev))))
                Fa = _thetae(Ta, Ta, lq, _w(_es(Ta), pp)) - the
                for _ in range(NITER):
                    Fb = _thetae(Tb, Tb, lq, _w(_es(Tb), pp)) - the
                    d = Fb - Fa
                    step = torch.where(d != 0, Fb * (Tb - Ta) / torch.where(d != 0, d, torch.ones_like(d)), torch.zeros_like(d))
                    Ta, Fa, Tb = Tb, Fb, Tb - step
                sat = lq > lq_lcl
                T = torch.where(sat, Tb, th0 * float(np.exp(KAPPA * (lp - ln1000))))
                B = torch.clamp(_tv(T, torch.where(sat, _w(_es(T), pp), w0)) - tenv, min=0)
                tot = torch.where(act, tot + 0.5 * (B + prevB) * ((lnp[k] - lnp[k + 1]) / NSUB), tot)
                prevB, Tprev = torch.where(act, B, prevB), torch.where(act, T, Tprev)
                lp_prev = lp
        out[m, 0] = RD * tot
        t8, q8 = s[names.index("t850")], s[names.index("q850")]
        e8 = torch.clamp(q8 * 850.0 / (EPS + 0.378 * q8), min=1e-10)
        out[m, 1] = _thetae(t8, _tl(t8, e8), ln1000 - float(np.log(850.0)), _w(e8, 850.0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--members", type=int, default=50)
    ap.add_argument("--chain-members", type=int, default=2)
    args = ap.parse_args()
    dev, M = "cuda:0", args.members
    g = PanguGeometry(721, 1440)
    H, W = g.n_lat, g.n_lon
    lat, lon = np.linspace(90.0, -90.0, H), np.arange(W) * (360.0 / W)
    names = list(CHANNELS)
    x0 = synthetic_state(g, 0).to(dev).reshape(len(CHANNELS), H, W).contiguous()
    for c, n in enumerate(names):                                # the synthetic humidity is mean + noise: keep it physical
        if n[0] == "q" and n[1:].isdigit():
            x0[c].clamp_(min=1e-6)
    members = [x0 * (1.0 + 1e-3 * m) for m in range(M)]
    table = E.member_table(members)
    deriver = D.LeadDeriver(CHANNELS, lat, lon, M, FIELDS, dev)
    plan = deriver.plan
    levels = plan.column["parcel"]
    layers = max(k for k, l in enumerate(levels) if l >= 100)
    candidates = sum(1 for l in levels if l >= 700)
    ops_per_column = layers * NSUB * OPS_PER_NODE + len(levels) * OPS_PER_LEVEL + candidates * OPS_PER_CANDIDATE + OPS_SOURCE + OPS_MOIST
    n_ops = M * H * W * ops_per_column
    planes_in = len({c for f in FIELDS for c in plan.inputs[f]})
    nbytes = M * (planes_in + len(FIELDS)) * H * W * 4
    cm = max(1, min(args.chain_members, M))
    out = torch.empty((cm, len(FIELDS), H, W), dtype=torch.float32, device=dev)
    cases = {"thermo_fields (one launch)": lambda: deriver.add(members, table),
             f"torch chain ({cm} members)": lambda: torch_chain(members[:cm], names, levels, out)}
    times = {k: [] for k in cases}
    for _ in range(args.warmup):
        for fn in cases.values():
            fn()
    torch.cuda.synchronize()
    got = deriver.add(members, table)[0]
    torch.cuda.synchronize()
    cape = got[0][0]
    print(f"mucape of member 0: max {float(cape.max()):.1f} J/kg, {float((cape > 0).float().mean()):.3f} of the columns unstable, "
          f"{int(torch.isnan(cape).sum())} NaN")
    for _ in range(args.reps):                       # alternating: every case sees the same clocks and the same neighbours
        for k, fn in cases.items():
            times[k].append(_timed(fn))
    res = {}
    for k in cases:
        med = statistics.median(times[k])
        res[k] = {"ms_median": round(med, 4), "ms_min": round(min(times[k]), 4), "ms_max": round(max(times[k]), 4)}
        print(f"{k:>30}: median {med:9.3f} ms (min {min(times[k]):.3f}, max {max(times[k]):.3f})")
    kern, chain = res["thermo_fields (one launch)"], res[f"torch chain ({cm} members)"]
    rate = n_ops / (kern["ms_median"] * 1e-3)
    kern.update(ops_per_column=ops_per_column, ops_per_s=rate, share_of_peak_valu=round(rate / PEAK_VALU, 4), bytes=nbytes,
                bytes_per_s=nbytes / (kern["ms_median"] * 1e-3))
    print(f"nominal: {ops_per_column} header operations per column (every node saturated) x {M * H * W} columns: {rate / 1e12:.2f} T ops/s = "
          f"{100 * rate / PEAK_VALU:.1f} % of the peak fp32 rate of the vector ALUs; {nbytes / 1e9:.2f} GB moved at {kern['bytes_per_s'] / 1e12:.3f} TB/s")
    scaled = chain["ms_median"] * M / cm
    ratio = scaled / kern["ms_median"]
    print(f"torch chain scaled to {M} members: {scaled:.1f} ms; torch chain / thermo_fields: {ratio:.1f} x")
    print(json.dumps({"tool": "thermo_time", "grid": [H, W], "members": M, "chain_members": cm, "fields": FIELDS, "levels": levels,
                      "input_planes": planes_in, "reps": args.reps, "ratio_torch_over_kernel": round(ratio, 2), "cases": res}))


if __name__ == "__main__":
    main()
