"""``torch.ops.skyrim_hip.object_label`` / ``object_attributes`` / ``object_probability`` against the numpy restatement
(tests/_object_reference.py): label planes, id planes and counts are equal, the records are equal field by field, every integer included,
and what the kernels must not touch keeps its fill.  Shapes: 19 x 70 (neither side a multiple of the 16 x 64 tile or of 64), 33 x 200
(several tiles both ways) and one 721 x 1440 plane."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import _object_reference as R
from skyrim_amd import objects as O
from skyrim_amd.members import member_table

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FILL = 0xAB
GUARD = 1024                                                    # bytes behind the record buffer that must keep their fill
hip = torch.ops.skyrim_hip


def grid(H, W):
    return np.linspace(90.0, -90.0, H), np.arange(W) * (360.0 / W)


def upload(states, misalign=False):
    """The states on the device, at addresses that are multiples of 16 or, with ``misalign``, 4 beyond one."""
    members, want = [], 4 if misalign else 0
    for s in states:
        s = np.ascontiguousarray(s, np.float32)
        flat = torch.empty(s.size + 8, dtype=torch.float32, device=DEV)
        off = ((want - flat.data_ptr()) % 16) // 4
        t = flat[off:off + s.size].view(s.shape)
        assert t.data_ptr() % 16 == want
        t.copy_(torch.from_numpy(s))
        members.append(t)
    return members


def run(states, planes, periodic, min_pixels, capacity, misalign=False, attributes=True):
    """One object_label (and object_attributes) on the device.  ``planes``: tuples (channel, threshold, direction, connectivity, scale)."""
    M, (C, H, W), P = len(states), states[0].shape, len(planes)
    members = upload(states, misalign)
    table = member_table(members)
    args = [[p[k] for p in planes] for k in range(5)]
    labels = torch.full((M, P, H, W), -7, dtype=torch.int32, device=DEV)
    ids = torch.full((M, P, H, W), -7, dtype=torch.int32, device=DEV)
    n_found = torch.full((M, P), -7, dtype=torch.int32, device=DEV)
    ws = torch.full((O.workspace_bytes(M, P, H, W),), FILL, dtype=torch.uint8, device=DEV)
    hip.object_label(members, table, *args, periodic, min_pixels, capacity, labels, ids, n_found, ws)
    out = dict(members=members, table=table, args=args, labels=labels, ids=ids, n_found=n_found)
    if attributes:
        lat, lon = grid(H, W)
        g = O.tables(lat, lon)
        row, col = torch.from_numpy(g.row).to(DEV), torch.from_numpy(g.col).to(DEV)
        nbytes = M * P * capacity * 128
        buf = torch.full((nbytes + GUARD,), FILL, dtype=torch.uint8, device=DEV)
        hip.object_attributes(members, table, *args, capacity, labels, ids, n_found, row, col, buf[:nbytes])
        out.update(buf=buf, row=g.row, col=g.col, tensors=(row, col))
    torch.cuda.synchronize()
    return out


def reference(states, planes, periodic, min_pixels, capacity, row=None, col=None):
    M, (C, H, W), P = len(states), states[0].shape, len(planes)
    labels, ids = np.zeros((M, P, H, W), np.int32), np.zeros((M, P, H, W), np.int32)
    n_found, recs = np.zeros((M, P), np.int32), {}
    for m in range(M):
        for p, (ch, thr, direction, conn, scale) in enumerate(planes):
            labels[m, p] = R.flood_labels(R.mask_of(states[m][ch], thr, direction), conn, periodic)
            ids[m, p], n_found[m, p], roots = R.number(labels[m, p], min_pixels, capacity)
            if row is not None:
                recs[m, p] = R.records(states[m][ch], ids[m, p], row, col, direction, scale, m, p)
                np.testing.assert_array_equal(recs[m, p]["root"], roots)
    return labels, ids, n_found, recs


def check(states, planes, periodic, min_pixels=1, capacity=64, misalign=False):
    """Everything the two calls write against the reference; returns (device results, reference records)."""
    got = run(states, planes, periodic, min_pixels, capacity, misalign)
    labels, ids, n_found, recs = reference(states, planes, periodic, min_pixels, capacity, got["row"], got["col"])
    np.testing.assert_array_equal(got["labels"].cpu().numpy(), labels)
    np.testing.assert_array_equal(got["ids"].cpu().numpy(), ids)
    np.testing.assert_array_equal(got["n_found"].cpu().numpy(), n_found)
    M, P = n_found.shape
    buf = got["buf"].cpu().numpy()
    assert np.all(buf[-GUARD:] == FILL), "written past the record buffer"
    slots = buf[:-GUARD].reshape(M, P, capacity, 128)
    for (m, p), ref in recs.items():
        n = min(int(n_found[m, p]), capacity)
        assert len(ref) == n
        dev = np.ascontiguousarray(slots[m, p, :n]).view(R.RECORD).reshape(n)
        for name in R.RECORD.names:
            np.testing.assert_array_equal(dev[name].view(np.int32) if name == "ext_value" else dev[name],
                                          ref[name].view(np.int32) if name == "ext_value" else ref[name], err_msg=f"member {m} plane {p} {name}")
        assert np.all(slots[m, p, n:] == FILL), "an unused record slot was touched"
    return got, recs


def plane_of(mask, inside=2.0, outside=0.0):
    return np.where(mask, inside, outside).astype(np.float32)[None]


def wrap_mask(H=19, W=70):
    m = np.zeros((H, W), bool)
    m[3:7, W - 4:] = m[3:7, :4] = True                          # a block across the wrap column
    m[10, W - 1] = m[11, 0] = True                              # a purely diagonal contact across it
    m[14, W - 1] = m[13, 0] = True                              # and the other diagonal
    m[16:18, 30:40] = True
    return m


@pytest.mark.parametrize("connectivity", [4, 8])
def test_object_across_the_wrap_column(connectivity):
    got, recs = check([plane_of(wrap_mask())], [(0, 1.0, 1, connectivity, 1.0)], True)
    n = int(got["n_found"][0, 0])
    assert n == (4 if connectivity == 8 else 6)                 # the block is one object; the diagonal pairs only under 8-connectivity
    assert recs[0, 0]["n_pixels"][0] == 32 and recs[0, 0]["root"][0] == 3 * 70


@pytest.mark.parametrize("connectivity", [4, 8])
def test_regional_box_splits_at_the_wrap_column(connectivity):
    got, recs = check([plane_of(wrap_mask())], [(0, 1.0, 1, connectivity, 1.0)], False)
    assert int(got["n_found"][0, 0]) == 7 and sorted(recs[0, 0]["n_pixels"].tolist()) == [1, 1, 1, 1, 16, 16, 20]


@pytest.mark.parametrize("periodic", [False, True])
def test_serpentine_through_every_tile(periodic):
    H, W = 33, 200
    m = np.zeros((H, W), bool)
    m[0::2, 1:W - 1] = True                                     # (columns 0 and W - 1 stay free: the wrap is no short cut)
    for k, j in enumerate(range(1, H, 2)):
        m[j, W - 2 if k % 2 == 0 else 1] = True
    got, recs = check([plane_of(m)], [(0, 1.0, 1, 4, 1.0)], periodic)
    assert int(got["n_found"][0, 0]) == 1 and recs[0, 0]["n_pixels"][0] == int(m.sum()) == 17 * 198 + 16
    assert recs[0, 0]["jmin"][0] == 0 and recs[0, 0]["jmax"][0] == H - 1


def test_checkerboard_one_object_or_one_per_point():
    H, W = 19, 70
    m = (np.add.outer(np.arange(H), np.arange(W)) % 2) == 0
    got, recs = check([plane_of(m)], [(0, 1.0, 1, 8, 1.0)], True, capacity=16)
    assert int(got["n_found"][0, 0]) == 1 and recs[0, 0]["n_pixels"][0] == H * W // 2
    got, recs = check([plane_of(m)], [(0, 1.0, 1, 4, 1.0)], True, capacity=16)      # (check: 16 records, fill beyond, guard intact)
    ids = got["ids"].cpu().numpy()[0, 0]
    assert int(got["n_found"][0, 0]) == H * W // 2 and len(recs[0, 0]) == 16 and ids.max() == 16 and (ids > 0).sum() == 16
    assert np.array_equal(np.flatnonzero(ids.ravel()), np.flatnonzero(m.ravel())[:16])      # the id plane is zero beyond the sixteenth object


@pytest.mark.parametrize("fill", ["true", "false", "nan"])
def test_uniform_planes(fill):
    H, W = 33, 200
    x = np.full((1, H, W), dict(true=2.0, false=0.0, nan=np.nan)[fill], np.float32)
    got, recs = check([x], [(0, 1.0, 1, 8, 1.0), (0, 1.0, -1, 4, 1.0)], True)
    n = got["n_found"].cpu().numpy()[0].tolist()
    assert n == dict(true=[1, 0], false=[0, 1], nan=[0, 0])[fill]
    if fill != "nan":
        r = recs[0, 0 if fill == "true" else 1]
        assert r["n_pixels"][0] == H * W and abs(int(r["area"][0]) - 2 ** 52) <= H * W and r["root"][0] == 0


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("H,W", [(19, 70), (33, 200)])
def test_noise_at_its_median_with_min_pixels(H, W, connectivity):
    x = np.random.default_rng(H * W + connectivity).standard_normal((1, H, W)).astype(np.float32)
    thr = float(np.median(x))
    got, recs = check([x], [(0, thr, 1, connectivity, O.value_scale(thr))], True, min_pixels=4, capacity=256)
    ids, labels = got["ids"].cpu().numpy()[0, 0], got["labels"].cpu().numpy()[0, 0]
    n = int(got["n_found"][0, 0])
    assert 1 <= n <= 256 and np.array_equal(np.unique(ids), np.arange(n + 1))        # dense numbering
    assert np.any((labels > 0) & (ids == 0))                    # components below min_pixels are labelled and are 0 in the id plane
    assert recs[0, 0]["n_pixels"].min() >= 4


def test_members_planes_channels_directions_and_unaligned_members():
    rng = np.random.default_rng(11)
    states = [rng.standard_normal((3, 19, 70)).astype(np.float32) for _ in range(3)]
    check(states, [(2, 0.25, 1, 8, 0.25), (0, -0.5, -1, 4, 0.5)], True, min_pixels=2, misalign=True)
    check(states, [(1, 0.0, -1, 8, 1.0), (1, 0.0, 1, 8, 1.0), (2, 1.0, 1, 4, 1.0)], False)


def test_saturated_points_are_counted_and_clamped():
    H, W = 19, 70
    x = np.full((1, H, W), 0.0, np.float32)
    x[0, 4:9, 10:30] = 3.0
    x[0, 5, 12], x[0, 6, 20], x[0, 8, 29] = 4096.5 * 2.0, np.inf, 1e30          # beyond 4096 value_scale at three points
    x[0, 4, 10] = 4096.0 * 2.0                                  # exactly at the clamp: not saturated
    got, recs = check([x], [(0, 2.0, 1, 8, 2.0)], True)
    assert recs[0, 0]["saturated"].tolist() == [3] and recs[0, 0]["ext_index"][0] == 6 * W + 20


def smooth_field(H, W, seed, waves=6):
    rng = np.random.default_rng(seed)
    lat, lon = grid(H, W)
    la, lo = np.radians(lat)[:, None], np.radians(lon)[None, :]
    x = np.zeros((H, W))
    for _ in range(waves):
        k, l, ph = rng.integers(1, 5), rng.integers(1, 6), rng.uniform(0, 2 * np.pi, 2)
        x += rng.uniform(0.5, 1.0) * np.cos(k * lo + ph[0]) * np.cos(l * la + ph[1])
    return x


def test_sum_v_within_the_headers_bound():
    """The area-weighted mean from sum_v against float64 on the same inputs: |mean - exact| <= 0.5 n_pixels 2^-40 value_scale /
    area_fraction plus the float64 rounding of the comparison itself.  Largest error / bound ratio measured on an MI355X over the 20
    objects of this test: 0.738, at an object of one point (one rounding, up to the whole bound); 0.11 at most for the objects of more
    than 100 points (the roundings of the terms are independent, so their sum grows like sqrt(n_pixels), not like n_pixels)."""
    H, W = 33, 200
    x = (250.0 + 120.0 * smooth_field(H, W, 3) + np.random.default_rng(4).standard_normal((H, W))).astype(np.float32)[None]
    thr, scale = 300.0, O.value_scale(300.0)
    got, recs = check([x], [(0, thr, 1, 8, scale), (0, 200.0, -1, 8, 256.0)], True)
    worst = 0.0
    for p, s in ((0, scale), (1, 256.0)):
        ids = got["ids"].cpu().numpy()[0, p]
        rec = recs[0, p]
        assert len(rec) >= 1
        for r in rec:
            exact, n, area = R.mean_exact(x[0], ids, got["row"], r["id"])
            assert n == r["n_pixels"] and area == r["area"] and r["saturated"] == 0
            mean = s * float(r["sum_v"]) / (float(r["area"]) / 4096.0)
            bound = 0.5 * n * 2.0 ** -40 * s / (area / 2.0 ** 52)
            err = abs(mean - exact)
            print(f"plane {p} object {r['id']}: n {n} mean {mean:.9f} error {err:.3e} bound {bound:.3e} ratio {err / bound:.3f}")
            assert err <= bound + 4 * np.finfo(np.float64).eps * abs(exact)
            worst = max(worst, err / bound)
    print(f"largest error / bound: {worst:.3f}")


def test_two_launches_give_identical_bytes():
    x = np.random.default_rng(2).standard_normal((2, 33, 200)).astype(np.float32)
    planes = [(0, 0.1, 1, 8, 0.125), (1, -0.1, -1, 4, 0.125)]
    a = run([x, x[::-1].copy()], planes, True, 2, 128)
    b = run([x, x[::-1].copy()], planes, True, 2, 128)
    for k in ("labels", "ids", "n_found", "buf"):
        assert torch.equal(a[k], b[k]), k
    # and a second launch into the same buffers, over the first one's results
    members, table, args = a["members"], a["table"], a["args"]
    ws = torch.empty(O.workspace_bytes(2, 2, 33, 200), dtype=torch.uint8, device=DEV)
    before = {k: a[k].clone() for k in ("labels", "ids", "n_found", "buf")}
    hip.object_label(members, table, *args, True, 2, 128, a["labels"], a["ids"], a["n_found"], ws)
    hip.object_attributes(members, table, *args, 128, a["labels"], a["ids"], a["n_found"], *a["tensors"], a["buf"][:-GUARD])
    torch.cuda.synchronize()
    for k, v in before.items():
        assert torch.equal(a[k], v), k


def test_probability_counts():
    rng = np.random.default_rng(9)
    states = [rng.standard_normal((2, 19, 70)).astype(np.float32) for _ in range(5)]
    planes = [(0, 0.0, 1, 8, 1.0), (1, 0.3, -1, 4, 0.5), (1, 1.0, 1, 8, 1.0)]
    cap = 8                                                     # fewer than the objects found: ids beyond it are 0 in the planes
    got = run(states, planes, True, 1, cap, attributes=False)
    ids = got["ids"].cpu().numpy()
    assert ids.max() == cap and got["n_found"].max().item() > cap
    keep = (rng.random((5, 3, cap + 1)) < 0.5).astype(np.uint8)
    keep[:, :, 0] = 0
    counts = torch.full((3, 19, 70), -7, dtype=torch.int32, device=DEV)
    hip.object_probability(got["ids"], torch.from_numpy(keep).to(DEV), counts)
    np.testing.assert_array_equal(counts.cpu().numpy(), R.probability_counts(ids, keep))
    assert 0 < counts.max().item() <= 5
    hip.object_probability(got["ids"], torch.zeros((5, 3, cap + 1), dtype=torch.uint8, device=DEV), counts)
    assert not counts.any().item()


def test_full_size_plane():
    H, W = 721, 1440
    states = [(smooth_field(H, W, 20 + m, waves=8))[None].astype(np.float32) for m in range(2)]
    thr = float(np.quantile(states[0], 0.93))
    got, recs = check(states, [(0, thr, 1, 8, O.value_scale(thr))], True, min_pixels=4, capacity=64)
    n = got["n_found"].cpu().numpy()
    assert n.min() >= 2 and n.max() <= 64
    big = max(int(r["n_pixels"].max()) for r in recs.values())
    assert big > 64 * 64                                        # an object of many tiles, whose inner waves add once per wave
