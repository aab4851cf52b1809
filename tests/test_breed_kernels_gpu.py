"""``breed_norms`` and ``breed_apply`` on the MI355X against tests/_breed_reference.py: the norms entry by entry inside the header's bound,
their reproducibility, the unaligned path, zeros, non-finite values and a lost point; the apply bit for bit, with negative and zero
factors, unaligned and in place."""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

import _breed_reference as BR
from skyrim_amd import breeding as B
from skyrim_amd.ensemble import member_table

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# the issue's shapes, and two where THIS kernel takes another path: a row of more than one 256-point tile that is a multiple of four
# (the four-floats-at-a-time path with a short last tile), and more tiles than workgroups per channel (G = 256 < 300 tiles)
SHAPES = BR.SHAPES + [(3, 2, 3, 260), (2, 1, 300, 8)]


@functools.lru_cache(maxsize=None)
def _case(shape):
    y0, mem, w = BR.inputs(*shape)
    S, T = BR.norms(y0, mem, w)
    for a in (y0, mem, w, S, T):
        a.setflags(write=False)
    return y0, mem, w, S, T


def _offset(a: np.ndarray, off: int) -> torch.Tensor:
    """``a`` on the device at ``off`` elements past a 16-byte boundary (a view into a larger allocation)."""
    buf = torch.empty(a.size + 8, dtype=torch.float32, device=DEV)
    assert buf.data_ptr() % 16 == 0
    v = buf[off:off + a.size].view(a.shape)
    v.copy_(torch.from_numpy(np.array(a, np.float32)))
    return v


def _norms(y0, mem, w, off=0):
    M, C, H, W = mem.shape
    yd = _offset(y0, off)
    md = [_offset(mem[m], off) for m in range(M)]
    S = torch.full((M, C), -1.0, dtype=torch.float64, device=DEV)
    guard = torch.full((B.workspace_bytes(M, C, H, W) // 8 + 4,), 7.0, dtype=torch.float64, device=DEV)
    torch.ops.skyrim_hip.breed_norms(yd, md, member_table(md), torch.from_numpy(np.array(w)).to(DEV), S, guard)
    torch.cuda.synchronize()
    assert torch.all(guard[-4:] == 7.0)                                     # nothing past the stated workspace is written
    return S.cpu().numpy()


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_norms(shape):
    y0, mem, w, S, T = _case(shape)
    M, C, H, W = shape
    got = _norms(y0, mem, w)
    k = B.bound_k(C, H, W)
    bound = k * BR.U53 * T + 2.0 ** -1070                                   # (+ the smallest float64: an all-zero entry compares 0 <= 0)
    ratio = np.abs(got - S) / bound
    print(f"{shape}: k = {k}, worst |S - exact| / bound = {ratio.max():.3f}")
    assert np.all(np.isfinite(got)) and np.all(ratio <= 1.0), (shape, float(ratio.max()))
    assert np.array_equal(_norms(y0, mem, w), got)                          # two calls: the same bits
    assert np.array_equal(_norms(y0, mem, w, off=1), got)                   # members 4 bytes off a 16-byte boundary: the same bits


def test_norms_zero_weight_row_and_equal_states():
    shape = (3, 2, 5, 67)
    y0, mem, w, S, T = _case(shape)
    same = np.array(mem)
    same[1] = y0                                                            # y_m == y_0: exactly 0
    got = _norms(y0, same, w)
    assert np.all(got[1] == 0.0) and np.all(got[[0, 2]] > 0)
    w0 = np.array(w)
    w0[2] = 0.0
    wild = np.array(mem)
    wild[:, :, 2, :] *= 1e3                                                 # whatever row 2 holds, it contributes nothing
    ref, T0 = BR.norms(y0, mem, w0)
    for m_ in (mem, wild):
        got = _norms(y0, m_, w0)
        assert np.all(np.abs(got - ref) <= B.bound_k(2, 5, 67) * BR.U53 * T0)


def test_norms_non_finite_values_stay_where_they_are():
    shape = (5, 3, 9, 257)
    y0, mem, w, S, T = _case(shape)
    bad = np.array(mem)
    bad[2, 1, 4, 256] = np.nan                                              # the one point past the first tile of its row
    got = _norms(y0, bad, w)
    fin = np.isfinite(got)
    assert not fin[2, 1] and fin.sum() == fin.size - 1
    clean = np.ones_like(fin)
    clean[2, 1] = False
    assert np.array_equal(got[clean], _norms(y0, mem, w)[clean])            # every other entry: the bits of the clean run
    bad0 = np.array(y0)
    bad0[0, 8, 0] = np.nan
    got = _norms(bad0, mem, w)
    fin = np.isfinite(got)
    assert not fin[:, 0].any() and fin[:, 1:].all()


def test_norms_bound_notices_a_lost_point():
    """4 096 points; the reference with ONE point of 4 sigma left out lies outside the bound around the device's result."""
    M, C, H, W = 2, 1, 4, 1024
    rng = np.random.default_rng(11)
    y0 = rng.standard_normal((C, H, W)).astype(np.float32)
    mem = (y0[None] + 1e-2 * rng.standard_normal((M, C, H, W))).astype(np.float32)
    mem[1, 0, 2, 517] = y0[0, 2, 517] + np.float32(4e-2)
    w = np.array([0.3, 1.0, 0.9, 0.2])
    got = _norms(y0, mem, w)
    S, T = BR.norms(y0, mem, w)
    bound = B.bound_k(C, H, W) * BR.U53 * T
    assert np.all(np.abs(got - S) <= bound)
    lost = np.array(mem)
    lost[1, 0, 2, 517] = y0[0, 2, 517]
    S_lost, _ = BR.norms(y0, lost, w)
    assert abs(got[1, 0] - S_lost[1, 0]) > 1e6 * bound[1, 0] and got[0, 0] == _norms(y0, lost, w)[0, 0]


def _apply(x0, y0, mem, f, off=0, in_place=False):
    M = mem.shape[0]
    xd, yd = _offset(x0, off), _offset(y0, off)
    md = [_offset(mem[m], off) for m in range(M)]
    out = md if in_place else [torch.full_like(md[0], 9.0) if off == 0 else _offset(np.full_like(x0, 9.0), off) for _ in range(M)]
    torch.ops.skyrim_hip.breed_apply(xd, yd, md, member_table(md), torch.from_numpy(f).to(DEV), out, member_table(out))
    torch.cuda.synchronize()
    assert xd.cpu().numpy().tobytes() == x0.tobytes() and yd.cpu().numpy().tobytes() == y0.tobytes()      # the inputs are left alone
    return np.stack([o.cpu().numpy() for o in out])


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_apply(shape):
    M, C, H, W = shape
    y0, mem, w, _, _ = _case(shape)
    rng = np.random.default_rng([3, *shape])
    x0 = rng.standard_normal((C, H, W)).astype(np.float32)
    f = rng.uniform(0.5, 40.0, (M, C)).astype(np.float32)
    f[::2] *= -1.0                                                          # negative factors: the mirrored members
    if M * C > 2:
        f[M - 1, C - 1] = 0.0
    ref = BR.apply(x0, y0, mem, f)
    for kw in (dict(), dict(off=1), dict(in_place=True), dict(off=3, in_place=True)):
        got = _apply(x0, y0, mem, f, **kw)
        assert got.tobytes() == ref.tobytes(), (shape, kw)


def test_apply_zero_factor_is_a_bit_copy():
    M, C, H, W = 3, 2, 5, 67
    y0, mem, w, _, _ = _case((M, C, H, W))
    x0 = np.array(np.random.default_rng(2).standard_normal((C, H, W)), np.float32)
    x0[0, 0, :8] = [-0.0, 0.0, np.inf, -np.inf, np.nan, 1e-45, -1e-45, 3.0]
    wild = np.array(mem)
    wild[:, 0, 0, :8] = [np.nan, np.inf, 1.0, np.nan, 2.0, -np.inf, np.nan, np.inf]       # a non-finite t where f is 0
    f = np.array([[0.0, 2.0], [-0.0, 0.0], [0.0, -3.0]], np.float32)
    ref = BR.apply(x0, y0, wild, f)
    for kw in (dict(), dict(off=1), dict(in_place=True)):
        got = _apply(x0, y0, wild, f, **kw)
        assert got.tobytes() == ref.tobytes()
        for m, c in ((0, 0), (1, 0), (1, 1), (2, 0)):
            assert got[m, c].tobytes() == x0[c].tobytes()                   # the sign of a zero, the payload of a NaN: bits of x_0
    # where f is non-zero a non-finite input reaches exactly the elements that read it
    wild2 = np.array(mem)
    wild2[0, 1, 3, 5] = np.inf
    got = _apply(x0, y0, wild2, f)
    clean = _apply(x0, y0, mem, f)
    diff = got.view(np.uint32) != clean.view(np.uint32)
    assert diff.sum() == 1 and diff[0, 1, 3, 5] and np.isinf(got[0, 1, 3, 5])


def test_apply_refuses_aliasing():
    M, C, H, W = 2, 1, 4, 64
    y0, mem, w, _, _ = _case((64, 2, 4, 64))
    xd, yd = _offset(y0[:1], 0), _offset(y0[:1], 0)
    md = [_offset(mem[m, :1], 0) for m in range(M)]
    f = torch.ones((M, C), device=DEV)
    for out in ([xd, md[1]], [md[0], yd], [md[1], md[0]]):
        with pytest.raises(ValueError, match="overlaps"):
            torch.ops.skyrim_hip.breed_apply(xd, yd, md, member_table(md), f, out, member_table(out))
