"""ms per FourCastNet v1 step at 720 x 1440 (synthetic parameters): warm-up steps, then timed steps between HIP events; prints the
median, the spread and one JSON line.  Also times the stages of one step (patch embedding, spectral filters, token MLPs, head).

    python tools/fcn_time.py [--steps 20] [--warmup 3]
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from skyrim_amd.fcn.engine import FcnEngine  # noqa: E402
from skyrim_amd.fcn.spec import FcnConfig, flops_per_step, init_synthetic, synthetic_state  # noqa: E402


def _timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    cfg = FcnConfig()
    eng = FcnEngine(cfg, "cuda:0")
    eng.load_params(init_synthetic(cfg, 0))
    x = synthetic_state(cfg, 0).to("cuda:0")
    y = torch.empty_like(x)
    for _ in range(args.warmup):
        eng.step(x, y)
    torch.cuda.synchronize()
    ms = [_timed(lambda: eng.step(x, y)) for _ in range(args.steps)]
    a, b = eng.t
    stages = {
        "patch_embed": _timed(lambda: eng.patch_embed(x, a)),
        "spectral x depth": _timed(lambda: [eng.spectral(i, a) for i in range(cfg.depth)]),
        "token_mlp x depth": _timed(lambda: [eng.token_mlp(i, a, b) for i in range(cfg.depth)]),
        "head": _timed(lambda: eng.head(a, y)),
    }
    med = statistics.median(ms)
    print(f"fcn 720x1440: median {med:.2f} ms/step over {len(ms)} steps (min {min(ms):.2f}, max {max(ms):.2f}); "
          f"{flops_per_step(cfg) / med / 1e9:.0f} TFLOP/s algorithmic")
    for k, v in stages.items():
        print(f"  {k:>18}: {v:.2f} ms")
    print(json.dumps({"model": "fourcastnet", "grid": [cfg.n_lat, cfg.n_lon], "ms_per_step_median": round(med, 3), "ms_min": round(min(ms), 3),
                      "ms_max": round(max(ms), 3), "steps": len(ms), "stages_ms": {k: round(v, 3) for k, v in stages.items()}}))


if __name__ == "__main__":
    main()
