"""numpy restatement of include/skyrim_pack.h, operation by operation in float32 and float64: what the kernels (tests/test_pack_kernels_gpu.py),
the file format and the archive are compared with bit for bit.  numpy keeps fp32 subnormals, as the library does."""
from __future__ import annotations

import numpy as np

FILL = -32768
ENTRY = np.dtype([("offset", "<f8"), ("scale", "<f8"), ("inv", "<f8"), ("lo", "<f4"), ("hi", "<f4"), ("n_bad", "<i4"), ("pad", "<i4")])


def entry(plane) -> tuple:
    """(offset, scale, inv, lo, hi, n_bad) of one plane, any shape, float32."""
    x = np.asarray(plane, np.float32).reshape(-1)
    fin = np.isfinite(x)
    n_bad = int(x.size - np.count_nonzero(fin))
    if not fin.any():
        return 0.0, 1.0, 1.0, np.float32(0), np.float32(0), n_bad
    lo = np.float32(x[fin].min() + np.float32(0.0))          # -0 becomes +0
    hi = np.float32(x[fin].max() + np.float32(0.0))
    lo64, hi64 = np.float64(lo), np.float64(hi)
    offset = np.float64(0.5) * lo64 + np.float64(0.5) * hi64
    d = hi64 - lo64
    if d == 0.0:
        return float(offset), 1.0, 1.0, lo, hi, n_bad
    return float(offset), float(d / np.float64(65534.0)), float(np.float64(65534.0) / d), lo, hi, n_bad


def table(states, channels) -> np.ndarray:
    """The (M, nc) record array (dtype ENTRY, the layout of skpack_entry) of the listed channels of M states (C, H, W)."""
    out = np.zeros((len(states), len(channels)), ENTRY)
    for m, s in enumerate(states):
        for k, c in enumerate(channels):
            out[m, k] = entry(np.asarray(s)[c]) + (0,)
    return out


def codes(planes, records) -> np.ndarray:
    """int16 codes of ``planes`` (nc, H, W) float32 with their nc records."""
    x = np.asarray(planes, np.float32)
    out = np.empty(x.shape, np.int16)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(x.shape[0]):
            e = x[k].astype(np.float64) - np.float64(records[k]["offset"])
            q = np.rint(e * np.float64(records[k]["inv"]))            # half to even
            q = np.clip(q, -32767.0, 32767.0)
            fin = np.isfinite(x[k])
            out[k] = np.where(fin, np.where(fin, q, 0.0).astype(np.int32), FILL).astype(np.int16)
    return out


def quantize(states, channels, tab=None) -> list:
    """The big-endian bytes of every member's image: M ``bytes`` of 2 nc H W each."""
    tab = table(states, channels) if tab is None else tab
    return [codes(np.asarray(s, np.float32)[list(channels)], tab[m]).astype(">i2").tobytes() for m, s in enumerate(states)]


def decode(c, records) -> np.ndarray:
    """float32 (nc, H, W) of int16 codes (native order) and their nc records."""
    c = np.asarray(c, np.int16)
    out = np.empty(c.shape, np.float32)
    for k in range(c.shape[0]):
        v = (c[k].astype(np.float64) * np.float64(records[k]["scale"]) + np.float64(records[k]["offset"])).astype(np.float32)
        out[k] = v
    out.view(np.uint32)[c == FILL] = 0x7FC00000
    return out


def unpack(image, records, shape) -> np.ndarray:
    """float32 ``shape`` = (nc, H, W) of a big-endian image (bytes or uint8 array)."""
    return decode(np.frombuffer(bytes(image), ">i2").reshape(shape).astype(np.int16), records)


def bound(x, rec) -> np.ndarray:
    """The header's bound on |x' - x| for finite x of a plane with record ``rec``, in float64."""
    big = max(abs(float(rec["lo"])), abs(float(rec["hi"])))
    return np.full(np.shape(x), 0.5 * float(rec["scale"]) * (1.0 + 2.0 ** -20) + 2.0 ** -24 * big + 2.0 ** -149)
