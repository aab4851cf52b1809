"""numpy restatement of include/skyrim_agg.h, written from the header: float32 arrays, the same comparisons in the same order, so it is
exact (bit for bit) for the kernel's outputs.  ``sum64`` is the float64 sum the bound of the mean is measured against.

An op is anything with the fields kind, channel, out, when, phase, thr, scale (``skyrim_amd.aggregate.Op``)."""
from __future__ import annotations

import numpy as np

MAX, MIN, SUM, COUNT_ABOVE = 1, 2, 3, 4
FIRST, LAST = 1, 2
F = np.float32


def update(x: np.ndarray, acc: np.ndarray, ops, stamp: float) -> None:
    """One skagg_update on the host: x (M, C, H, W) float32, acc (M, D, H, W) float32, changed in place."""
    assert x.dtype == np.float32 and acc.dtype == np.float32
    stamp = F(stamp)
    with np.errstate(invalid="ignore", over="ignore"):
        for op in ops:
            v = x[:, op.channel]
            first, last = bool(op.phase & FIRST), bool(op.phase & LAST)
            nan = v != v
            if op.kind in (MAX, MIN):
                w_new = np.where(nan, v, stamp).astype(F)
                if first:
                    acc[:, op.out] = v
                    if op.when >= 0:
                        acc[:, op.when] = w_new
                else:
                    a = acc[:, op.out]
                    take = ((v > a) if op.kind == MAX else (v < a)) | nan
                    acc[:, op.out] = np.where(take, v, a)
                    if op.when >= 0:
                        acc[:, op.when] = np.where(take, w_new, acc[:, op.when])
            else:
                if op.kind == SUM:
                    b = v
                else:
                    b = np.where(nan, v, np.where(v > F(op.thr), F(1.0), F(0.0))).astype(F)
                r = b.copy() if first else (acc[:, op.out] + b).astype(F)
                if last:
                    r = (r * F(op.scale)).astype(F)
                acc[:, op.out] = r


def fold(xs, ops_per_step, stamps, D: int, fill=None) -> np.ndarray:
    """The accumulator after the calls xs[k] (M, C, H, W), ops_per_step[k], stamps[k]; it starts as ``fill`` (a float32 bit pattern
    given as an array or None: NaN-free garbage is not needed, slots are only compared where the test wrote them)."""
    M, _, H, W = xs[0].shape
    acc = np.zeros((M, D, H, W), np.float32) if fill is None else fill.copy()
    for x, ops, s in zip(xs, ops_per_step, stamps):
        update(x, acc, ops, s)
    return acc


def sum64(xs, channel: int) -> np.ndarray:
    """(sum over steps, sum of absolute values) of one channel in float64: (M, H, W) each."""
    s = np.zeros(xs[0][:, channel].shape, np.float64)
    a = np.zeros_like(s)
    for x in xs:
        s += x[:, channel].astype(np.float64)
        a += np.abs(x[:, channel].astype(np.float64))
    return s, a


def case(M: int, C: int, H: int, W: int, steps: int, seed: int = 0) -> list:
    """``steps`` states (M, C, H, W) float32 in the normal range: magnitudes between 1e-3 and 1e5, both signs, with repeated values from
    step to step at a tenth of the points so that ties occur."""
    rng = np.random.default_rng(seed)
    xs = []
    for k in range(steps):
        mag = 10.0 ** rng.uniform(-3, 5, size=(M, C, H, W))
        x = (mag * rng.choice([-1.0, 1.0], size=mag.shape)).astype(np.float32)
        if k:
            same = rng.random(size=x.shape) < 0.1
            x[same] = xs[k - 1][same]
        xs.append(x)
    return xs
