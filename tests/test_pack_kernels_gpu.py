"""libskyrim_pack.so on the device against tests/_pack_reference.py: the table, the bytes of every image (and every byte around them) and
the unpacked floats are BIT-equal.  The shapes are the smallest at which each path is taken: 1 x 2 (fewer values than a lane takes), 5 x 7
(an odd plane: every second plane begins in the middle of a 32-bit word; with three channels an odd total), 33 x 64 (one tile, 16-byte
groups), 181 x 360 (several tiles of both passes, the last one short) and 721 x 1440 once."""
import numpy as np
import pytest
import torch

import _pack_reference as R
from skyrim_amd import archive as A
from skyrim_amd.members import member_table

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
C = 9
FULL = [8, 2, 3, 4, 5, 6, 0, 1, 7, 2]          # out of order, one repeat, every special plane of states()
PAD = 0xAB


def states(M, H, W, seed):
    """M states (C, H, W) of mixed magnitude (field() of tests/test_point_kernels_gpu.py) with, in member 0, a constant plane (2), a
    subnormal one (3), one of NaN only (4), one with +Inf, -Inf and a NaN among finite values (5), one of -0 only (6); in the last member
    the extremes at the first and the last element (0), on either side of the border of the code tiles (1, elements 8191 | 8192) and of
    the range tiles (7, elements 16383 | 16384), or around the middle of a plane smaller than that."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((M, C, H, W), dtype=np.float32)
    scale = np.array([250.0, 54000.0, 25.0, 8.0, 1e-3, 1e-30, 1e5, 3.0, 0.02])
    shift = np.array([250.0, 5e4, 0.0, 0.0, 5e-3, 0.0, 1e5, -3.0, 0.0])
    x *= scale.astype(np.float32)[None, :, None, None]
    x += shift.astype(np.float32)[None, :, None, None]
    HW = H * W
    flat = x.reshape(M, C, HW)
    flat[0, 2] = 3.25
    flat[0, 3] = (rng.standard_normal(HW) * 1e-41).astype(np.float32)
    flat[0, 4] = np.nan
    flat[0, 5, HW // 2] = np.inf
    flat[0, 5, 0] = -np.inf
    flat[0, 5, HW - 1] = np.nan
    flat[0, 6] = -0.0
    flat[-1, 0, 0], flat[-1, 0, HW - 1] = 2000.0, -2000.0
    for c, border in ((1, 8192), (7, 16384)):
        b = border if HW > border else max(HW // 2, 1)
        flat[-1, c, b - 1], flat[-1, c, b % HW] = 1e6, -1e6
    return x


def on_device(x, skew):
    """The members of x (M, C, H, W) as device tensors; ``skew``: member m begins 4 (m even) or 12 (m odd) bytes behind a 16-byte
    boundary, or only the odd members do (``"odd"``)."""
    out = []
    for m, s in enumerate(x):
        off = 0 if not skew or (skew == "odd" and m % 2 == 0) else (1, 3)[m % 2]
        buf = torch.zeros(s.size + 4, dtype=torch.float32, device=DEV)
        t = buf[off:off + s.size].view(s.shape)
        t.copy_(torch.from_numpy(s))
        assert t.is_contiguous() and t.data_ptr() % 16 == 4 * off
        out.append(t)
    return out


def pack(members, channels, lead, gap, tail=64):
    """range + quantize into a buffer of PAD bytes: ``lead`` bytes in front of member 0's image, ``gap`` bytes between images, ``tail``
    behind the last.  Returns (buffer bytes, table records, device buffer, device table, stride)."""
    M, (_, H, W), nc = len(members), members[0].shape, len(channels)
    need = 2 * nc * H * W
    stride = need + gap
    buf = torch.full((lead + (M - 1) * stride + need + tail,), PAD, dtype=torch.uint8, device=DEV)
    table = member_table(members)
    tab = A.new_table(M, nc, DEV)
    tab.fill_(float("nan"))
    ws = torch.full((max(A.workspace_bytes(M, nc, H, W), 4),), 0xFF, dtype=torch.uint8, device=DEV)      # needs no preparation
    torch.ops.skyrim_hip.pack_range(members, table, channels, tab, ws)
    torch.ops.skyrim_hip.pack_quantize(members, table, channels, tab, buf[lead:], stride)
    torch.cuda.synchronize()
    return buf.cpu().numpy(), A.table_of(tab), buf, tab, stride


def expected(x, channels, lead, gap, tail=64):
    M, (_, H, W), nc = len(x), x[0].shape, len(channels)
    need = 2 * nc * H * W
    stride = need + gap
    tab = R.table(list(x), channels)
    buf = np.full(lead + (M - 1) * stride + need + tail, PAD, np.uint8)
    for m, img in enumerate(R.quantize(list(x), channels, tab)):
        buf[lead + m * stride:lead + m * stride + need] = np.frombuffer(img, np.uint8)
    return buf, tab


def unpack_all(x, channels, buf, tab, lead, stride, skew):
    """Every member's image, read where quantize left it (so at an odd 2-byte offset under ``skew``), through pack_unpack."""
    M, (_, H, W), nc = len(x), x[0].shape, len(channels)
    outs = []
    for m in range(M):
        flat = torch.zeros(nc * H * W + 4, dtype=torch.float32, device=DEV)
        off = (m % 3) if skew else 0                              # the output 16-byte aligned or 4 / 8 bytes behind
        out = flat[off:off + nc * H * W].view(nc, H, W)
        codes = buf[lead + m * stride:lead + m * stride + 2 * nc * H * W]
        torch.ops.skyrim_hip.pack_unpack(codes, tab[m].contiguous(), out)
        outs.append(out)
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in outs]


def check(M, H, W, channels, skew, seed, lead=None, gap=None):
    x = states(M, H, W, seed)
    lead = (2 if skew else 0) if lead is None else lead           # out + 2: 2-byte aligned only
    gap = (6 if skew else 0) if gap is None else gap              # every second image 2 bytes off a 4-byte boundary on top of that
    members = on_device(x, skew)
    got, gtab, buf, tab, stride = pack(members, channels, lead, gap)
    want, wtab = expected(x, channels, lead, gap)
    assert gtab.tobytes() == wtab.tobytes(), np.argwhere(gtab != wtab)[:4]
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]          # the images AND every PAD byte around them
    worst = 0.0
    for m, dec in enumerate(unpack_all(x, channels, buf, tab, lead, stride, skew)):
        need = 2 * len(channels) * H * W
        ref = R.unpack(want[lead + m * stride:lead + m * stride + need], wtab[m], (len(channels), H, W))
        assert np.array_equal(dec.view(np.uint32), ref.view(np.uint32))
        for k, c in enumerate(channels):                          # the header's bound, on what the device gave
            fin = np.isfinite(x[m, c])
            assert np.array_equal(np.isnan(dec[k]), ~fin)
            err = np.abs(dec[k][fin].astype(np.float64) - x[m, c][fin].astype(np.float64))
            if err.size:
                worst = max(worst, float((err / R.bound(err, wtab[m, k])).max()))
    assert worst <= 1.0
    return worst, (members, channels, lead, gap, got, gtab)


@pytest.mark.parametrize("skew", [False, True], ids=["aligned", "skewed"])
@pytest.mark.parametrize("M,H,W,channels", [
    (1, 1, 2, [0]), (3, 1, 2, FULL), (3, 5, 7, [6, 0, 6]), (64, 5, 7, FULL), (3, 33, 64, FULL), (64, 33, 64, [1, 0]),
    (3, 181, 360, FULL), (1, 181, 360, [5, 5, 3])])
def test_table_image_and_unpack_are_bit_equal_to_the_reference(M, H, W, channels, skew):
    check(M, H, W, channels, skew, seed=M + H)


def test_full_size_once():
    """721 x 1440, M = 2, nc = 3: member 0 and the images 16-byte aligned (the wide loads and stores of the body), member 1 four bytes
    behind (single loads), a gap of 16 bytes between the images.  Prints the largest error over the header's bound."""
    worst, _ = check(2, 721, 1440, [1, 7, 0], "odd", seed=7, lead=0, gap=16)
    print(f"pack: largest |x' - x| / bound at 721 x 1440: {worst:.4f}")


def test_special_planes_have_the_records_the_header_states():
    _, (_, channels, _, _, _, tab) = check(3, 33, 64, FULL, False, seed=11)
    rec = {c: tab[0, k] for k, c in enumerate(channels)}
    assert (rec[2]["lo"], rec[2]["hi"], rec[2]["scale"], rec[2]["inv"], rec[2]["offset"]) == (3.25, 3.25, 1.0, 1.0, 3.25)
    assert 0 < rec[3]["hi"] < 1.2e-38 and rec[3]["n_bad"] == 0 and rec[3]["scale"] > 0                  # subnormals are kept
    assert tuple(rec[4])[:5] == (0.0, 1.0, 1.0, 0.0, 0.0) and rec[4]["n_bad"] == 33 * 64
    assert rec[5]["n_bad"] == 3 and np.isfinite(rec[5]["hi"])
    assert rec[6]["lo"].tobytes() == np.float32(0.0).tobytes() == rec[6]["hi"].tobytes() and rec[6]["scale"] == 1.0      # -0 is +0


def test_running_twice_gives_the_same_bits():
    x = states(3, 181, 360, 5)
    members = on_device(x, True)
    a = pack(members, FULL, 2, 6)
    b = pack(members, FULL, 2, 6)
    assert np.array_equal(a[0], b[0]) and a[1].tobytes() == b[1].tobytes()


def test_refusals_of_the_binding():
    x = on_device(states(2, 5, 7, 0), False)
    table = member_table(x)
    tab, ws = A.new_table(2, 1, DEV), torch.empty(64, dtype=torch.uint8, device=DEV)
    out = torch.empty(2 * 2 * 35, dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError, match="channel index"):
        A.run_range(x, table, [9], tab, ws)
    with pytest.raises(ValueError, match="workspace"):
        A.run_range(x, table, [0], tab, ws[:8])
    with pytest.raises(ValueError, match="table must hold"):
        A.run_range(x, table, [0, 1], tab, ws)
    with pytest.raises(ValueError, match="member_stride_bytes"):
        A.run_quantize(x, table, [0], tab, out, 69)
    with pytest.raises(ValueError, match="out holds"):
        A.run_quantize(x, table, [0], tab, out[:100])
    with pytest.raises(ValueError, match="codes must hold"):
        A.run_unpack(out[:68], tab[0], torch.empty((1, 5, 7), device=DEV))
