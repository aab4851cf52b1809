"""ms per FuXi call at 721 x 1440, full width and depth (synthetic parameters of all three stages): warm-up calls, then timed calls
between HIP events; prints the median, the spread, the algorithmic rate next to the three-term MFMA bound, and one JSON line.  Also times
the stages of one call (embedding, down block, the Swin blocks, up block, head).

    python tools/fuxi_time.py [--steps 20] [--warmup 3] [--peak-tflops 2500]

``--peak-tflops``: the dense fp16 MFMA peak the bound is taken from (three MFMA terms per product: bound = peak / 3).
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

from skyrim_amd.fuxi.engine import FuxiEngine  # noqa: E402
from skyrim_amd.fuxi.spec import FuxiConfig, flops_per_call, init_synthetic, synthetic_state, time_encoding  # noqa: E402


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
    cfg = FuxiConfig()
    eng = FuxiEngine(cfg, "cuda:0")
    eng.load_params(init_synthetic(cfg, 0, "cuda:0"))
    x0, x1 = synthetic_state(cfg, 0).to("cuda:0"), synthetic_state(cfg, 1).to("cuda:0")
    t = datetime.datetime(2024, 1, 1)
    for _ in range(args.warmup):
        eng.call(x0, x1, t, "short")
    torch.cuda.synchronize()
    ms = [_timed(lambda: eng.call(x0, x1, t, "short")) for _ in range(args.steps)]
    S, b, (g0, g1) = eng.stages["short"], eng.buf, (cfg.grid0, cfg.grid1)
    t0 = g0[0] * g0[1]
    y = torch.empty_like(x0)

    def embed():
        eng.embed(x0, x1, time_encoding(t), "short")
        eng.layer_norm(b["emb"], S["en_g"], S["en_b"], b["h0"], t0)

    def down():
        eng.conv(b["h0"], S["down"], S["down_b"], b["d0"], g0, g1, stride=2)
        eng.res_block(b["d0"], S["down_res"], b["d"], g1, b["ra1"], b["rb1"])

    def up():
        eng.conv(b["d"], S["up"], S["up_b"], b["u0"], g1, g1, taps=1, src1=b["x"], shuffle=1)
        eng.res_block(b["u0"], S["up_res"], b["u"], g0, b["ra0"], b["rb0"])

    def head():
        eng.linear(b["u"], S["head"], S["head_b"], b["head"], t0, head=True)
        eng.resample(b["head"], y)

    stages = {"embed + LN": _timed(embed), "down block": _timed(down),
              "swin blocks": _timed(lambda: [eng.swin_block(i, "short") for i in range(cfg.depth)]), "up block": _timed(up), "head": _timed(head)}
    rows = g1[0] * g1[1]
    B = S["blocks"][1]
    swin = {"qkv": _timed(lambda: eng.linear(b["x"], B["qkv"], B["qkv_b"], b["qkv"], rows)),
            "attention (shifted)": _timed(lambda: eng.attention(b["qkv"], b["att"], B["cpb"], B["scale"], g1, cfg.window[0] // 2, cfg.window[1] // 2)),
            "proj": _timed(lambda: eng.linear(b["att"], B["proj"], B["proj_b"], b["y"], rows)),
            "fc1 + GELU": _timed(lambda: eng.linear(b["x"], B["fc1"], B["fc1_b"], b["hid"], rows, act=1)),
            "fc2": _timed(lambda: eng.linear(b["hid"], B["fc2"], B["fc2_b"], b["y"], rows)),
            "residual LN": _timed(lambda: eng.layer_norm(b["y"], B["n1_g"], B["n1_b"], b["att"], rows, res=b["x"]))}
    med = statistics.median(ms)
    fl = flops_per_call(cfg)
    bound = args.peak_tflops / 3
    print(f"fuxi 721x1440, C {cfg.embed}, depth {cfg.depth}: median {med:.1f} ms per call over {len(ms)} calls (min {min(ms):.1f}, max {max(ms):.1f}); "
          f"{fl / 1e12:.1f} TFLOP -> {fl / med / 1e9:.0f} TFLOP/s algorithmic; three-term bound {bound:.0f} TFLOP/s = {fl / bound / 1e9:.1f} ms")
    for k, v in stages.items():
        print(f"  {k:>22}: {v:.2f} ms")
    print("  one Swin block:")
    for k, v in swin.items():
        print(f"  {k:>22}: {v:.3f} ms")
    print(json.dumps({"model": "fuxi", "grid": [cfg.n_lat, cfg.n_lon], "embed": cfg.embed, "depth": cfg.depth, "ms_per_call_median": round(med, 3),
                      "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3), "calls": len(ms), "tflop_per_call": round(fl / 1e12, 2),
                      "tflops_algorithmic": round(fl / med / 1e9, 1), "three_term_bound_ms": round(fl / bound / 1e9, 2),
                      "stages_ms": {k: round(v, 3) for k, v in stages.items()}, "swin_block_ms": {k: round(v, 3) for k, v in swin.items()}}))


if __name__ == "__main__":
    main()
