"""Time of one member's spherical perturbation at 721 x 1440 x 69 (Pangu's state): coefficients + synthesis (two GEMMs) + apply, for
lmax 128 / 256 / 720, next to ``skens_perturb`` (white noise) on the same state.  Prints one JSON line per case: median and minimum of
``--repeat`` timed runs after ``--warmup`` untimed ones, device time from events around the member's launches.

    python tools/noise_time.py [--lmax 128 256 720] [--fields 69] [--repeat 20] [--warmup 3]
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import torch  # noqa: E402


def timed(fn, warmup: int, repeat: int) -> list[float]:
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeat):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--lmax", type=int, nargs="+", default=[128, 256, 720])
    ap.add_argument("--fields", type=int, default=69)
    ap.add_argument("--n_lat", type=int, default=721)
    ap.add_argument("--n_lon", type=int, default=1440)
    ap.add_argument("--repeat", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    from skyrim_amd import ensemble, noise
    from skyrim_amd.pangu.spec import PanguGeometry
    dev = torch.device("cuda:0")
    C, H, W = a.fields, a.n_lat, a.n_lon
    x0 = torch.randn(1, 1, C, H, W, device=dev)
    std = torch.rand(C, device=dev) + 0.5
    out = torch.empty_like(x0)
    ms = timed(lambda: ensemble.perturb(x0, std, out, H * W, 1e-3, 0, 1), a.warmup, a.repeat)
    print(json.dumps(dict(case="white (skens_perturb)", fields=C, grid=[H, W], median_ms=statistics.median(ms), min_ms=min(ms))))
    model = type("M", (), dict(grid=PanguGeometry(H, W), in_channel_names=[str(c) for c in range(C)]))
    for lmax in a.lmax:
        p = noise.plan(model, "spherical", lmax=lmax)
        pert = noise.Perturber(p, x0, std, 1e-3, 0)
        parts = {}
        parts["coeffs"] = timed(lambda: noise.coeffs(pert.coef, pert.sigma, pert.F, 0, 0, 1), a.warmup, a.repeat)
        parts["synthesis"] = timed(lambda: pert.synth.run(pert.coef, pert.t, pert.y, pert.F), a.warmup, a.repeat)
        parts["apply"] = timed(lambda: noise.apply(x0, pert.y, pert.g, out, H * W), a.warmup, a.repeat)
        ms = timed(lambda: pert.member(1, out), a.warmup, a.repeat)
        macs = 2 * C * (sum(lmax - (m // 32) * 32 for m in range(lmax)) * H + H * 2 * lmax * W)
        print(json.dumps(dict(case="spherical", lmax=lmax, e=p.e, fields=C, grid=[H, W], median_ms=statistics.median(ms), min_ms=min(ms),
                              parts_median_ms={k: statistics.median(v) for k, v in parts.items()}, gemm_macs=macs,
                              matrices_mb=round(2 * 2 * (pert.synth.syn.plane + pert.synth.idft.plane) / 2 ** 20, 1))))
        del pert
        noise.release()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
