"""ms of ONE ``vert_fields`` launch at 721 x 1440 with M = 50 synthetic member states on Pangu's channel layout (no model), 13 levels, for

    agl    ["ws@100magl"]                                                  (one coordinate pass, one SPEED field with its 10-m node)
    z      t, u, v, q on 1500 m and 3000 m                                 (four fields x two targets on one coordinate pass)
    theta  ["u@320K", "v@320K", "p@320K"]

next to a torch chain that makes the same fields on ``--chain-members`` of the same tensors (a top-down loop over the layers with
``torch.where``: some twenty launches a layer, so it is timed on a few members and scaled to M; the line says so) and next to the time
the tool's own measured device-to-device copy rate would need for the bytes the kernel must move (``BYTES``: every coordinate plane
once, two values per field component and target, the node planes, the output planes).  The measurements alternate in one process, each
between device events, after warm-up; prints the medians and one JSON line.

    timeout -k 10 900 python tools/vert_time.py [--reps 10] [--warmup 2] [--members 50] [--chain-members 2]
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
from skyrim_amd import vertical as V  # noqa: E402
from skyrim_amd.pangu.spec import CHANNELS, PanguGeometry, synthetic_state  # noqa: E402

CASES = {"agl": ["ws@100magl"],
         "z": [f"{x}@{h}m" for h in (1500, 3000) for x in "tuvq"],
         "theta": ["u@320K", "v@320K", "p@320K"]}


def _timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def bytes_moved(plan, M, H, W) -> int:
    """What the kernel must move for the plan's vert ops: coordinate and mask planes once, two values per component and requested
    (field, target), the node planes, the surface and the outputs"""
    planes = 0
    for op in plan.vert_ops:
        planes += len(op.c) + len(op.z) + (1 if op.coord == V.Z_AGL or op.z else 0)
        for fd in op.fields:
            wanted = sum(1 for s in fd.outputs if s >= 0)
            planes += 2 * wanted * {V.PLAIN: 1, V.THETA_F: 1, V.SPEED: 2, V.PRESSURE: 0}[fd.kind] + sum(1 for c in fd.node if c >= 0) + wanted
    return planes * M * H * W * 4


def torch_chain(members, plan, zs, out):
    """The same fields with torch ops, member after member: the search of include/skyrim_vert.h as a loop over the layers"""
    for m, s in enumerate(members):
        for op in plan.vert_ops:
            L = len(op.pressures)
            lnp = [float(np.log(p)) for p in op.pressures]
            ex = [float((1000.0 / p) ** 0.2854) for p in op.pressures]
            if op.coord == V.THETA:
                c = s[list(op.c)] * torch.tensor(ex, device=s.device).view(-1, 1, 1)
            else:
                c = s[list(op.c)]
            masked = zs is not None and op.coord != V.P
            z = s[list(op.z)] if op.z else c
            for t, target in enumerate(op.targets):
                tau = zs + target if op.coord == V.Z_AGL else torch.full_like(c[0], target)
                found = torch.zeros_like(c[0], dtype=torch.bool)
                frac = torch.zeros_like(c[0])
                kl = torch.zeros_like(c[0], dtype=torch.long)
                ku = torch.zeros_like(kl)
                have = torch.zeros_like(found)
                cu, klast = torch.zeros_like(c[0]), torch.zeros_like(kl)
                for k in range(L - 1, -1, -1):
                    ok = ~(z[k] < zs) if masked else torch.ones_like(found)
                    a, b = c[k] - tau, cu - tau
                    hit = ok & have & ~found & (((a >= 0) & (b <= 0)) | ((a <= 0) & (b >= 0))) & (a != b)
                    frac = torch.where(hit, a / (a - b), frac)
                    kl, ku = torch.where(hit, k, kl), torch.where(hit, klast, ku)
                    found |= hit
                    cu, klast = torch.where(ok, c[k], cu), torch.where(ok, k, klast)
                    have |= ok
                for fd in op.fields:
                    slot = fd.outputs[t]
                    if slot < 0:
                        continue
                    nodes = []
                    if fd.node[0] >= 0:                              # the node's layer, for the columns no layer above crossed
                        a, b = (zs + fd.gh) - tau, cu - tau
                        take = ~found & have & (((a >= 0) & (b <= 0)) | ((a <= 0) & (b >= 0))) & (a != b)
                        nfrac = a / (a - b)
                        nodes = [s[ch] for ch in fd.node if ch >= 0]
                    if fd.kind == V.PRESSURE:
                        lp = torch.tensor(lnp, device=s.device)
                        res = torch.exp(lp[kl] + (lp[ku] - lp[kl]) * frac)
                    else:
                        vals = []
                        for comp, chans in enumerate((fd.a, fd.b) if fd.kind == V.SPEED else (fd.a,)):
                            planes = s[list(chans)]
                            vl, vu = torch.gather(planes, 0, kl[None])[0], torch.gather(planes, 0, ku[None])[0]
                            v = vl + (vu - vl) * frac
                            if nodes:
                                vn = torch.gather(planes, 0, klast[None])[0]
                                v = torch.where(take, nodes[comp] + (vn - nodes[comp]) * nfrac, v)
                            vals.append(v)
                        res = torch.sqrt(vals[0] * vals[0] + vals[1] * vals[1]) if fd.kind == V.SPEED else vals[0]
                    ok = found | take if nodes else found
                    out[m, slot] = torch.where(ok, res, torch.full_like(res, float("nan")))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--members", type=int, default=50)
    ap.add_argument("--chain-members", type=int, default=2)
    ap.add_argument("--lat", type=int, default=721)
    ap.add_argument("--lon", type=int, default=1440)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("vert_time measures on the GPU: none found")
    dev, M = "cuda:0", args.members
    g = PanguGeometry(args.lat, args.lon)
    H, W = g.n_lat, g.n_lon
    lat, lon = np.linspace(90.0, -90.0, H), np.arange(W) * (360.0 / W)
    names = list(CHANNELS)
    x0 = synthetic_state(g, 0).to(dev).reshape(len(CHANNELS), H, W).contiguous()
    members = [x0 * (1.0 + 1e-3 * m) for m in range(M)]
    table = E.member_table(members)
    zs_host = (x0[names.index("z1000")] - 9.80665 * 60.0).cpu().numpy()      # the ground some 60 m below the 1000-hPa surface of member 0
    zs = torch.from_numpy(zs_host).to(dev)
    cm = max(1, min(args.chain_members, M))
    # the copy rate this device gives a plain device-to-device copy of a gigabyte: read + write
    src = torch.empty(1 << 28, dtype=torch.float32, device=dev)
    dst = torch.empty_like(src)
    for _ in range(3):
        dst.copy_(src)
    torch.cuda.synchronize()
    copy_ms = statistics.median(_timed(lambda: dst.copy_(src)) for _ in range(10))
    copy_rate = 2 * src.numel() * 4 / (copy_ms * 1e-3)
    del src, dst
    print(f"device-to-device copy: {copy_rate / 1e12:.3f} TB/s (read + write)")
    results = {}
    for case, fields in CASES.items():
        deriver = D.LeadDeriver(CHANNELS, lat, lon, M, fields, dev, surface=zs_host if case == "agl" else None)
        plan = deriver.plan
        out = torch.empty((cm, len(fields), H, W), dtype=torch.float32, device=dev)
        surface = zs if case == "agl" else None
        runs = {"vert_fields (one launch)": lambda: deriver.add(members, table),
                f"torch chain ({cm} members)": lambda: torch_chain(members[:cm], plan, surface, out)}
        for _ in range(args.warmup):
            for fn in runs.values():
                fn()
        torch.cuda.synchronize()
        got = deriver.add(members, table)[0]
        torch.cuda.synchronize()
        torch_chain(members[:cm], plan, surface, out)
        both = torch.isfinite(out[0]) & torch.isfinite(got[0])
        print(f"{case}: {fields}: {float(torch.isnan(got[0]).float().mean()):.3f} of member 0's results NaN; largest difference from the torch "
              f"chain {float((out[0] - got[0])[both].abs().max()):.3g}")
        times = {k: [] for k in runs}
        for _ in range(args.reps):                   # alternating: every case sees the same clocks and the same neighbours
            for k, fn in runs.items():
                times[k].append(_timed(fn))
        nbytes = bytes_moved(plan, M, H, W)
        kern = statistics.median(times["vert_fields (one launch)"])
        chain = statistics.median(times[f"torch chain ({cm} members)"]) * M / cm
        floor = nbytes / copy_rate * 1e3
        for k in runs:
            print(f"{k:>30}: median {statistics.median(times[k]):9.3f} ms (min {min(times[k]):.3f}, max {max(times[k]):.3f})")
        print(f"  {nbytes / 1e9:.2f} GB to move: {floor:.3f} ms at the copy rate, the launch takes {kern / floor:.2f} x that "
              f"({nbytes / (kern * 1e-3) / 1e12:.3f} TB/s); torch chain scaled to {M} members {chain:.1f} ms = {chain / kern:.1f} x the launch")
        results[case] = dict(fields=fields, ms_median=round(kern, 4), ms_min=round(min(times["vert_fields (one launch)"]), 4),
                             ms_max=round(max(times["vert_fields (one launch)"]), 4), bytes=nbytes, ms_at_copy_rate=round(floor, 4),
                             chain_ms_scaled=round(chain, 2), ratio_torch_over_kernel=round(chain / kern, 2))
    print(json.dumps({"tool": "vert_time", "grid": [H, W], "members": M, "chain_members": cm, "reps": args.reps,
                      "copy_TB_per_s": round(copy_rate / 1e12, 4), "cases": results}))


if __name__ == "__main__":
    main()
