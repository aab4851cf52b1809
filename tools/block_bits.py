"""Bit-level fingerprint of Pangu's block kernels on the toy case of tests/test_pangu_gpu.py: sha256 of ``eng.block(layer, 0, x)`` for
layers 1-4 and of ``eng.step(x)``, for the three-term engines and a ladder of term plans.  The toy grid's token counts (4992 and 1344) are
no multiples of the 256- / 128-token tiles, so dead tiles run at both widths.  Two builds that compute the same thing print the same lines:

    python tools/block_bits.py > a.txt        # in one tree
    python tools/block_bits.py > b.txt        # in the other
    cmp a.txt b.txt
"""
import hashlib
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from oracle import pangu_oracle as O  # noqa: E402
from skyrim_amd.pangu.engine import PanguEngine  # noqa: E402
from skyrim_amd.pangu.spec import PanguGeometry, init_synthetic, synthetic_state  # noqa: E402

ENGINES = [("f16x3q", p) for p in (0x000, 0x00F, 0x0FF, 0x66F, 0xFFF)] + [("bf16x3", None)]


def sha(t):
    return hashlib.sha256(t.detach().float().cpu().contiguous().numpy().tobytes()).hexdigest()


def main():
    torch.manual_seed(0)
    g = PanguGeometry(49, 192)
    params, x = init_synthetic(g, 0), synthetic_state(g, 0)
    taps = {}
    O.forward(params, x, taps=taps)
    for prec, plan in ENGINES:
        tag = prec if plan is None else f"{prec} plan 0x{plan:03X}"
        try:
            eng = PanguEngine(g, prec, "cuda:0", term_plan=plan)
        except RuntimeError as e:
            if "skpangu_create failed" not in str(e):
                raise
            print(f"{tag}: rejected ({e})", flush=True)       # a plan the library does not take
            continue
        eng.load_params(params)
        print(f"{tag}: plan in effect 0x{eng.term_plan_in_effect:03X}", flush=True)
        for layer, tap in ((1, "embed"), (2, "down"), (3, "down"), (4, "up")):
            print(f"{tag}: block {layer}.0 {sha(eng.block(layer, 0, taps[tap].float().cuda().contiguous()))}", flush=True)
        print(f"{tag}: step      {sha(eng.step(x.cuda()))}", flush=True)
        eng.release()


if __name__ == "__main__":
    main()
