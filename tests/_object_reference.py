"""Numpy restatement of the weather objects (include/skyrim_object.h, skyrim_amd/objects.py) on the same fp32 inputs.

The labels come from a flood fill with an explicit stack, seeded in raster order, so a component's first point is its smallest index;
the integer sums are np.rint of one float64 product per term, added in int64; the extreme is the maximum of the header's 64-bit key.
Nothing here reads the product's label or id planes.  ``host_properties`` restates the float64 formulas of ``objects.properties``.
"""
from __future__ import annotations

import numpy as np

R_KM = 6371.0
CLAMP = 4096.0
SUMS = ("area", "sx", "sy", "sz", "sxx", "sxy", "sxz", "syy", "syz", "szz", "sum_v")
RECORD = np.dtype([(k, "<i4") for k in ("member", "plane", "id", "root", "n_pixels", "jmin", "jmax", "saturated")]
                  + [(k, "<i8") for k in SUMS] + [("ext_value", "<f4"), ("ext_index", "<i4")])


def mask_of(v, threshold, direction):
    """fp32 comparison; a NaN is background."""
    v = np.asarray(v, np.float32)
    with np.errstate(invalid="ignore"):
        return v >= np.float32(threshold) if direction > 0 else v <= np.float32(threshold)


def flood_labels(mask, connectivity, periodic):
    """int32 (H, W): 1 + the smallest index of the point's component, 0 on background."""
    H, W = mask.shape
    fg = mask.ravel().tolist()
    lab = [0] * (H * W)
    offs = [(0, -1), (0, 1), (-1, 0), (1, 0)]
    if connectivity == 8:
        offs += [(-1, -1), (-1, 1), (1, -1), (1, 1)]
    for q0 in np.flatnonzero(mask.ravel()).tolist():
        if lab[q0]:
            continue
        lab[q0] = q0 + 1
        stack = [q0]
        while stack:
            j, i = divmod(stack.pop(), W)
            for dj, di in offs:
                jj, ii = j + dj, i + di
                if jj < 0 or jj >= H:
                    continue                                    # rows are not joined across the poles
                if ii < 0 or ii >= W:
                    if not periodic:
                        continue
                    ii %= W
                r = jj * W + ii
                if fg[r] and not lab[r]:
                    lab[r] = q0 + 1
                    stack.append(r)
    return np.array(lab, np.int32).reshape(H, W)


def number(labels, min_pixels, capacity):
    """(ids int32 (H, W), n_found, roots of the kept objects): the components of at least ``min_pixels`` points numbered in ascending
    order of their smallest index; ids above ``capacity`` are 0 in the plane, n_found counts them all."""
    roots, counts = np.unique(labels[labels > 0], return_counts=True)
    good = roots[counts >= min_pixels]                          # ascending
    ids = np.zeros(labels.shape, np.int32)
    if good.size:
        pos = np.searchsorted(good, labels)
        pos = np.minimum(pos, good.size - 1)
        hit = (labels > 0) & (good[pos] == labels)
        ids[hit] = (pos[hit] + 1).astype(np.int32)
    ids[ids > capacity] = 0
    return ids, int(good.size), (good[:capacity] - 1).astype(np.int64)


def ordered_key(v, direction, index):
    """The header's 64-bit key of fp32 values ``v`` at point indices ``index``."""
    k = np.asarray(v, np.float32).view(np.uint32).astype(np.uint64)
    o = np.where(k >> np.uint64(31), k ^ np.uint64(0xffffffff), k ^ np.uint64(0x80000000))
    if direction < 0:
        o = o ^ np.uint64(0xffffffff)
    return (o << np.uint64(32)) | (np.uint64(0xffffffff) - np.asarray(index, np.uint64))


def key_value(key, direction):
    o = np.uint64(key) >> np.uint64(32)
    if direction < 0:
        o = o ^ np.uint64(0xffffffff)
    bits = o ^ np.uint64(0x80000000) if o >> np.uint64(31) else o ^ np.uint64(0xffffffff)
    return np.array([bits], np.uint64).astype(np.uint32).view(np.float32)[0], int(np.uint64(0xffffffff) - (np.uint64(key) & np.uint64(0xffffffff)))


def records(v, ids, row, col, direction, scale, member=0, plane=0):
    """The RECORD array of one (member, plane): ``v`` fp32 (H, W), ``ids`` the id plane, ``row`` (6, H) and ``col`` (5, W) the float64
    tables.  Integer sums in int64 of np.rint(one float64 product)."""
    H, W = ids.shape
    n = int(ids.max()) if ids.size else 0
    out = np.zeros(n, RECORD)
    jj, ii = np.nonzero(ids > 0)
    k = ids[jj, ii].astype(np.int64) - 1
    rint = lambda a: np.rint(a).astype(np.int64)                # noqa: E731
    R, C = row[:, jj], col[:, ii]
    area = rint(R[0])
    x = np.asarray(v, np.float32)[jj, ii].astype(np.float64) / float(scale)
    sat = np.abs(x) > CLAMP
    terms = dict(area=area, sx=rint(R[1] * C[0]), sy=rint(R[1] * C[1]), sz=rint(R[2]), sxx=rint(R[3] * C[2]), sxy=rint(R[3] * C[3]),
                 sxz=rint(R[4] * C[0]), syy=rint(R[3] * C[4]), syz=rint(R[4] * C[1]), szz=rint(R[5]),
                 sum_v=rint(np.clip(x, -CLAMP, CLAMP) * (area.astype(np.float64) * 2.0 ** -12)))
    for name, t in terms.items():
        acc = np.zeros(n, np.int64)
        np.add.at(acc, k, t)
        out[name] = acc
    out["member"], out["plane"], out["id"] = member, plane, np.arange(1, n + 1)
    out["n_pixels"] = np.bincount(k, minlength=n)
    out["saturated"] = np.bincount(k, weights=sat, minlength=n).astype(np.int32)
    jmin, jmax = np.full(n, H, np.int64), np.full(n, -1, np.int64)
    np.minimum.at(jmin, k, jj)
    np.maximum.at(jmax, k, jj)
    out["jmin"], out["jmax"] = jmin, jmax
    idx = jj * W + ii
    root = np.full(n, H * W, np.int64)
    np.minimum.at(root, k, idx)
    out["root"] = root
    key = np.zeros(n, np.uint64)
    np.maximum.at(key, k, ordered_key(np.asarray(v, np.float32)[jj, ii], direction, idx))
    for q in range(n):
        out["ext_value"][q], out["ext_index"][q] = key_value(key[q], direction)
    return out


def probability_counts(ids, keep):
    """int32 (P, H, W) from ids (M, P, H, W) and keep (M, P, capacity + 1)."""
    M, P = ids.shape[:2]
    out = np.zeros(ids.shape[1:], np.int32)
    for m in range(M):
        for p in range(P):
            out[p] += keep[m, p][ids[m, p]]
    return out


def mean_exact(v, ids, row, k):
    """The area-weighted mean of object k in float64 with the weights rint(row[0]) 2^-12 the kernels use, and the header's bound's
    n_pixels / area term's inputs: (mean, n_pixels, area integer)."""
    jj, ii = np.nonzero(ids == k)
    w = np.rint(row[0][jj])
    x = np.asarray(v, np.float32)[jj, ii].astype(np.float64)
    return float((x * w).sum() / w.sum()), jj.size, int(w.sum())


def host_properties(rec, lat, lon, scale):
    """dict of float64 arrays: area_km2, lat, lon (centroid), mean -- the formulas of ``objects.properties`` restated."""
    area = rec["area"].astype(np.float64)
    mu = np.stack([rec["sx"], rec["sy"], rec["sz"]]).astype(np.float64) / area
    return dict(area_km2=4 * np.pi * R_KM ** 2 * area / 2.0 ** 52, lat=np.degrees(np.arctan2(mu[2], np.hypot(mu[0], mu[1]))),
                lon=np.degrees(np.arctan2(mu[1], mu[0])) % 360.0, mean=float(scale) * rec["sum_v"].astype(np.float64) / (area / 4096.0))


def tables(lat, lon):
    """(row (6, H), col (5, W)) of the header, with the cell fractions from the rows' mid-latitudes (half cells at a pole row)."""
    lat, lon = np.asarray(lat, np.float64), np.asarray(lon, np.float64)
    edges = np.concatenate([[lat[0] - (lat[1] - lat[0]) / 2], (lat[1:] + lat[:-1]) / 2, [lat[-1] + (lat[-1] - lat[-2]) / 2]])
    a = np.abs(np.diff(np.sin(np.radians(np.clip(edges, -90, 90))))) / 2 * abs(lon[1] - lon[0]) / 360.0 * 2.0 ** 52
    phi, lam = np.radians(lat), np.radians(lon)
    c, s, cl, sl = np.cos(phi), np.sin(phi), np.cos(lam), np.sin(lam)
    return np.stack([a, a * c, a * s, a * (c * c), a * (c * s), a * (s * s)]), np.stack([cl, sl, cl * cl, cl * sl, sl * sl])
