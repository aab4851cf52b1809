"""Writes tests/golden/fcn_toy_16x48.npz: one FourCastNet v1 toy configuration (16 x 48 grid, patch 4 -> 4 x 12 tokens, embed 192 in two
spectral blocks, depth 2), seeded parameters and state, the float64 CPU restatement's outputs after one and two steps.

    python tests/golden/make_golden_fcn.py
"""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
sys.path.insert(1, str(ROOT / "tests"))

import _fcn_reference as R  # noqa: E402
from skyrim_amd.fcn.spec import FcnConfig, init_synthetic, synthetic_state  # noqa: E402

CFG = FcnConfig(n_lat=16, n_lon=48, patch=4, embed_dim=192, depth=2, num_blocks=2)
SEED = 3
PATH = Path(__file__).resolve().parent / "fcn_toy_16x48.npz"


def main():
    p = init_synthetic(CFG, SEED)
    x = synthetic_state(CFG, SEED)
    y1 = R.forward(p, x.double(), CFG)
    y2 = R.forward(p, y1, CFG)
    np.savez_compressed(PATH, x=x.numpy(), y1=y1.float().numpy(), y2=y2.float().numpy(), seed=np.int64(SEED),
                        grid=np.array([CFG.n_lat, CFG.n_lon, CFG.patch, CFG.embed_dim, CFG.depth, CFG.num_blocks]))
    print(f"wrote {PATH}")


if __name__ == "__main__":
    main()
