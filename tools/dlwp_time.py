"""ms per DLWP 12-h step at 721 x 1440 / 6 x 64 x 64 (synthetic parameters): warm-up calls, then timed calls between HIP events;
prints the median, the spread and one JSON line.  Also times the stages of one call (ingest, each conv, egress).

    python tools/dlwp_time.py [--steps 20] [--warmup 3]
"""
from __future__ import annotations

import argparse
import datetime
import json
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from skyrim_amd.dlwp.engine import DlwpEngine  # noqa: E402
from skyrim_amd.dlwp.spec import DlwpConfig, flops_per_call, init_synthetic, synthetic_state  # noqa: E402


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
    cfg = DlwpConfig()
    eng = DlwpEngine(cfg, "cuda:0")
    eng.load_params(init_synthetic(cfg, 0))
    x0, x1 = synthetic_state(cfg, 0).to("cuda:0"), synthetic_state(cfg, 1).to("cuda:0")
    t = datetime.datetime(2024, 1, 1)
    for _ in range(args.warmup):
        eng.call(x0, x1, t)
    torch.cuda.synchronize()
    ms = [_timed(lambda: eng.call(x0, x1, t)) for _ in range(args.steps)]
    y6, y12 = torch.empty_like(x0), torch.empty_like(x0)
    days = eng.tisr_days(t)
    stages = {"ingest": _timed(lambda: eng.ingest(x0, x1, *days))}
    for i, L in enumerate(eng.layers):
        stages[f"conv {L['name']}"] = _timed(lambda i=i: eng.conv(i))
    stages["egress"] = _timed(lambda: eng.egress(y6, y12))
    med = statistics.median(ms)
    print(f"dlwp 721x1440 / 6x{cfg.face}x{cfg.face}: median {med:.3f} ms per 12-h step over {len(ms)} steps (min {min(ms):.3f}, "
          f"max {max(ms):.3f}); {flops_per_call(cfg) / med / 1e9:.0f} TFLOP/s algorithmic")
    for k, v in stages.items():
        print(f"  {k:>20}: {v:.3f} ms")
    print(json.dumps({"model": "dlwp", "grid": [cfg.n_lat, cfg.n_lon], "face": cfg.face, "ms_per_step_median": round(med, 4),
                      "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4), "steps": len(ms),
                      "stages_ms": {k: round(v, 4) for k, v in stages.items()}}))


if __name__ == "__main__":
    main()
