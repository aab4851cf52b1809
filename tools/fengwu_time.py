"""ms per FengWu call at 721 x 1440, default network (synthetic parameters): warm-up calls, then timed calls between HIP events; prints
the median, the spread, the algorithmic rate next to the three-term MFMA bound, and one JSON line.  Also times the stages of one call
(embedding, encoders, fuser, decoders, recovery) and the launches of one Swin block of each kind.

    python tools/fengwu_time.py [--steps 20] [--warmup 3] [--peak-tflops 2500]

``--peak-tflops``: the dense fp16 MFMA peak the bound is taken from (three MFMA terms per product: bound = peak / 3).
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from skyrim_amd.fengwu.engine import FengwuEngine  # noqa: E402
from skyrim_amd.fengwu.spec import FengwuConfig, flops_per_call, init_synthetic, n_launches, synthetic_state  # noqa: E402


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
    ap.add_argument("--peak-tflops", type=float, default=2500.0)
    args = ap.parse_args()
    cfg = FengwuConfig()
    eng = FengwuEngine(cfg, "cuda:0")
    eng.load_params(init_synthetic(cfg, 0, "cuda:0"))
    x0, x1 = synthetic_state(cfg, 0).to("cuda:0"), synthetic_state(cfg, 1).to("cuda:0")
    for _ in range(args.warmup):
        eng.call(x0, x1)
    torch.cuda.synchronize()
    ms = [_timed(lambda: eng.call(x0, x1)) for _ in range(args.steps)]
    y = torch.empty_like(x0)
    b, W = eng.buf, eng.w
    stages = {"embed + LN": _timed(lambda: eng.embed_stage(x0, x1)), "encoders": _timed(eng.encoders), "fuser": _timed(eng.fuser),
              "decoders (no recovery)": _timed(lambda: ([eng.swin_block(B, b["x2"], "s1") for B in W["dec1"]],
                                                        eng.expand_skip(b["x2"], b["xe"], b["xd"]),
                                                        [eng.swin_block(B, b["xd"], "s0") for B in W["dec0"]])),
              "recovery": _timed(lambda: eng.recover(b["xd"], y))}
    blocks = {"2-D block 181x360 (x6 modalities)": _timed(lambda: eng.swin_block(W["enc0"][1], b["xe"], "s0")),
              "2-D block 91x180 (x6 modalities)": _timed(lambda: eng.swin_block(W["enc1"][1], b["x2"], "s1")),
              "3-D fuser block": _timed(lambda: eng.swin_block(W["fuser"][1], b["x2"], "fuser"))}
    rows = cfg.grid2[0] * cfg.grid2[1] * cfg.n_mod
    F = W["fuser"][1]
    fuser = {"qkv": _timed(lambda: eng.linear(b["h"], F["qkv"], F["qkv_b"], b["qkv"], rows)),
             "attention (shifted)": _timed(lambda: eng.attention(b["qkv"], F["qkv_b"], F["table"], b["att"], "fuser", F["shift"], F["types"])),
             "proj + residual": _timed(lambda: eng.linear(b["att"], F["proj"], F["proj_b"], b["x2"], rows, res=b["x2"])),
             "fc1 + GELU": _timed(lambda: eng.linear(b["h"], F["fc1"], F["fc1_b"], b["hid"], rows, act=1)),
             "fc2 + residual": _timed(lambda: eng.linear(b["hid"], F["fc2"], F["fc2_b"], b["x2"], rows, res=b["x2"])),
             "LayerNorm": _timed(lambda: eng.layer_norm(b["x2"], F["n1_g"], F["n1_b"], b["h"], rows, 1, cfg.dims[1]))}
    med = statistics.median(ms)
    fl = flops_per_call(cfg)
    bound = args.peak_tflops / 3
    print(f"fengwu 721x1440, dims {cfg.dims}, {n_launches(cfg)} launches: median {med:.2f} ms per call over {len(ms)} calls (min {min(ms):.2f}, "
          f"max {max(ms):.2f}); {fl / 1e12:.2f} TFLOP -> {fl / med / 1e9:.0f} TFLOP/s algorithmic; three-term bound {bound:.0f} TFLOP/s = "
          f"{fl / bound / 1e9:.2f} ms ({fl / bound / 1e9 / med:.2f} of it)")
    for k, v in {**stages, **blocks}.items():
        print(f"  {k:>36}: {v:.3f} ms")
    print("  one fuser block:")
    for k, v in fuser.items():
        print(f"  {k:>36}: {v:.3f} ms")
    print(json.dumps({"model": "fengwu", "grid": [cfg.n_lat, cfg.n_lon], "dims": list(cfg.dims), "launches": n_launches(cfg),
                      "ms_per_call_median": round(med, 3), "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3), "calls": len(ms),
                      "tflop_per_call": round(fl / 1e12, 3), "tflops_algorithmic": round(fl / med / 1e9, 1),
                      "three_term_bound_ms": round(fl / bound / 1e9, 2), "fraction_of_bound": round(fl / bound / 1e9 / med, 3),
                      "stages_ms": {k: round(v, 3) for k, v in stages.items()}, "blocks_ms": {k: round(v, 3) for k, v in blocks.items()},
                      "fuser_block_ms": {k: round(v, 3) for k, v in fuser.items()}}))


if __name__ == "__main__":
    main()
