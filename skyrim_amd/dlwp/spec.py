"""Shapes, parameter layout, cube geometry and synthetic inputs of the DLWP (cubed-sphere U-Net) call.

The network is modulus's ``DLWP`` as earth2mip's ``networks/dlwp.py`` wraps it (the reference's skyrim/core/models/dlwp.py:25):
the 7-channel state is normalised on the lat-lon grid, regridded to a 6 x 64 x 64 cubed sphere, joined by TISR, the land-sea mask and
topography (18 channels), run through a depth-2 U-Net of cube-padded 3 x 3 convolutions (equatorial weights on faces 0-3, polar
weights on faces 4-5), and the 14 output channels (t+6 h, t+12 h) are regridded back and de-normalised.  Parameter slots are keyed by
modulus's module names (checkpoint.py maps a package onto them).

Everything the kernels and the float64 restatement (tests/_dlwp_reference.py) must agree on is stated once here: the conv list
(``convs``), the padding table (``PAD``), the corner rule, the polar mirror and TISR.  None of it could be checked against the real
package offline; DESIGN.md 14 lists these points.
"""
from __future__ import annotations

import datetime
import math
from dataclasses import dataclass

import numpy as np
import torch

CHANNELS = ["t850", "z1000", "z700", "z500", "z300", "tcwv", "t2m"]
# (center, scale) of the synthetic data: ERA5-like magnitudes per channel
_STATS = {"t850": (275.0, 15.0), "z1000": (800.0, 900.0), "z700": (29500.0, 700.0), "z500": (55000.0, 2500.0),
          "z300": (89000.0, 3800.0), "tcwv": (19.0, 16.0), "t2m": (278.0, 21.0)}
J2000 = datetime.datetime(2000, 1, 1, 12, 0)


@dataclass(frozen=True)
class DlwpConfig:
    n_lat: int = 721                        # 90 .. -90
    n_lon: int = 1440                       # 0 .. 359.75
    face: int = 64                          # cube face size (cells per side)
    channels: int = 7
    n_history: int = 2                      # input levels: t - history_hours, t
    history_hours: float = 6.0
    step_hours: float = 12.0                # one call returns t + 6 h and t + 12 h; the loop advances 12 h
    nr_initial_channels: int = 64
    depth: int = 2
    leaky_slope: float = 0.1
    clamp_max: float = 10.0
    polar_flip_face: int = 5                # this face is mirrored in rows before its polar conv and back after it
    tisr_offsets_h: tuple = (-6.0, 0.0)     # TISR time of each history level relative to the newest level (point 1)
    topo_center: float = 3.724e3            # topography channel = (z - topo_center) / topo_scale
    topo_scale: float = 8.349e3

    @property
    def in_ch(self):                        # 18: per level the fields + TISR, then mask and topography
        return self.n_history * (self.channels + 1) + 2

    @property
    def out_ch(self):                       # 14: t + 6 h, then t + 12 h
        return 2 * self.channels

    @property
    def cells(self):
        return 6 * self.face * self.face

    @property
    def points(self):
        return self.n_lat * self.n_lon


# ---- the U-Net ------------------------------------------------------------------------------------------------------------------- #
# One entry per conv in call order: (name, level, cin, cout, kernel, input).  level l runs at face / 2**l.  input:
#   "x"       the ingest activations (18 channels, padded to a multiple of 8 in HBM)
#   "prev"    the previous conv's output at the same level
#   "pool"    2 x 2 average of the previous conv's output one level up
#   "up+skip" nearest x 2 upsampling of the previous conv's output one level down, concatenated with the skip of this level
def convs(cfg: DlwpConfig) -> list[tuple]:
    if cfg.depth != 2:
        raise ValueError(f"this build runs the depth-2 U-Net (got depth {cfg.depth})")
    c = cfg.nr_initial_channels
    return [("downsample.0", 0, cfg.in_ch, c, 3, "x"), ("downsample.1", 0, c, c, 3, "prev"),
            ("downsample.2", 1, c, 2 * c, 3, "pool"), ("downsample.3", 1, 2 * c, 2 * c, 3, "prev"),
            ("mid_layers.0", 2, 2 * c, 4 * c, 3, "pool"), ("mid_layers.1", 2, 4 * c, 2 * c, 3, "prev"),
            ("upsample.0", 1, 4 * c, 2 * c, 3, "up+skip"), ("upsample.1", 1, 2 * c, c, 3, "prev"),
            ("upsample.2", 0, 2 * c, c, 3, "up+skip"), ("upsample.3", 0, c, c, 3, "prev"),
            ("last", 0, c, cfg.out_ch, 1, "prev")]


SKIP_OF = {"upsample.0": "downsample.3", "upsample.2": "downsample.1"}      # the encoder output each concatenation appends


def param_spec(cfg: DlwpConfig) -> list[tuple[str, tuple]]:
    n = cfg.face
    spec = [("center", (cfg.channels,)), ("scale", (cfg.channels,)), ("lsm", (6, n, n)), ("topography", (6, n, n)),
            ("cube_lat", (6, n, n)), ("cube_lon", (6, n, n))]
    for name, _, cin, cout, k, _ in convs(cfg):
        for kind in ("equatorial", "polar"):
            spec += [(f"{kind}_{name}.weight", (cout, cin, k, k)), (f"{kind}_{name}.bias", (cout,))]
    return spec


MAP_SLOTS = ("ll_to_cs", "cs_to_ll")        # sparse maps: "<map>.row", "<map>.col" (0-based int64), "<map>.S" (float64)


def n_parameters(cfg: DlwpConfig) -> int:
    return sum(int(np.prod(s)) for name, s in param_spec(cfg) if name.startswith(("equatorial_", "polar_")))


def flops_per_call(cfg: DlwpConfig) -> float:
    """Multiply-adds x 2 of the convolutions of one call (the regrids are bandwidth, not FLOPs)."""
    total = 0.0
    for _, lvl, cin, cout, k, _ in convs(cfg):
        total += 2.0 * cfg.cells / 4 ** lvl * cout * cin * k * k
    return total


# ---- cube padding ------------------------------------------------------------------------------------------------------------------ #
# PAD[f][side] = (g, k), sides (top, bottom, left, right) = (row -1, row n, column -1, column n): the halo strip on that side of face
# f is the facing edge of R = torch.rot90(face g, k, dims=(rows, cols)):
#     top (-1, x) = R[n-1, x]     bottom (n, x) = R[0, x]     left (y, -1) = R[y, n-1]     right (y, n) = R[y, 0]
# with R[i, j] = G[i, j] (k = 0), G[j, n-1-i] (1), G[n-1-i, n-1-j] (2), G[n-1-j, i] (3).  Faces 0-3 run east along the equator from
# longitude 0, face 4 is the north pole, face 5 the south pole (``face_frames``); the test checks every halo cell of this table against
# the nearest cell of the geometry.  Corners (both indices outside) are the mean of the two halo cells next to them.
PAD = ((( 4, 0), (5, 0), (3, 0), (1, 0)),
       (( 4, 3), (5, 1), (0, 0), (2, 0)),
       (( 4, 2), (5, 2), (1, 0), (3, 0)),
       (( 4, 1), (5, 3), (2, 0), (0, 0)),
       (( 2, 2), (0, 0), (3, 3), (1, 1)),
       (( 0, 0), (2, 2), (3, 1), (1, 3)))


def halo_source(f: int, y: int, x: int, n: int) -> tuple[int, int, int]:
    """(g, row, col) of a non-corner halo cell (y, x) of face f (exactly one of y, x in {-1, n})."""
    side = 0 if y < 0 else 1 if y >= n else 2 if x < 0 else 3
    g, k = PAD[f][side]
    i, j = ((n - 1, x), (0, x), (y, n - 1), (y, 0))[side]
    if k == 1:
        i, j = j, n - 1 - i
    elif k == 2:
        i, j = n - 1 - i, n - 1 - j
    elif k == 3:
        i, j = n - 1 - j, i
    return g, i, j


def padded_sources(n: int):
    """Gather form of the padding: (idx [6, n+2, n+2, 2] flat cell indices f n^2 + y n + x, wt [6, n+2, n+2, 2]); a padded cell is
    wt[..., 0] * cell[idx[..., 0]] + wt[..., 1] * cell[idx[..., 1]] (interior and edge halo: one source of weight 1)."""
    idx = np.zeros((6, n + 2, n + 2, 2), dtype=np.int64)
    wt = np.zeros((6, n + 2, n + 2, 2))
    flat = lambda g, i, j: (g * n + i) * n + j          # noqa: E731
    for f in range(6):
        for py in range(n + 2):
            for px in range(n + 2):
                y, x = py - 1, px - 1
                yin, xin = 0 <= y < n, 0 <= x < n
                if yin and xin:
                    idx[f, py, px] = flat(f, y, x)
                    wt[f, py, px, 0] = 1.0
                elif yin or xin:
                    idx[f, py, px] = flat(*halo_source(f, y, x, n))
                    wt[f, py, px, 0] = 1.0
                else:                                   # corner: the two halo cells next to it
                    a = halo_source(f, y, 0 if x < 0 else n - 1, n)
                    b = halo_source(f, 0 if y < 0 else n - 1, x, n)
                    idx[f, py, px] = (flat(*a), flat(*b))
                    wt[f, py, px] = 0.5
    return idx, wt


def pad_table_i32() -> torch.Tensor:
    """PAD as the kernels read it: int32 [6][4][2]."""
    return torch.tensor(PAD, dtype=torch.int32).contiguous()


# ---- geometry ------------------------------------------------------------------------------------------------------------------------ #
def face_frames():
    """(centre, column axis, row axis) of each face as float64 [6, 3] arrays: a face point at gnomonic (a, b) is centre + a col + b row."""
    c, e, d = [], [], []
    for f in range(4):
        lam = math.radians(90.0 * f)
        c.append([math.cos(lam), math.sin(lam), 0.0])
        e.append([-math.sin(lam), math.cos(lam), 0.0])
        d.append([0.0, 0.0, -1.0])
    c += [[0.0, 0.0, 1.0], [0.0, 0.0, -1.0]]
    e += [[0.0, 1.0, 0.0], [0.0, 1.0, 0.0]]
    d += [[1.0, 0.0, 0.0], [-1.0, 0.0, 0.0]]
    return np.array(c), np.array(e), np.array(d)


def gnomonic(n: int, lo: int = 0, hi: int | None = None) -> np.ndarray:
    """tan of the equiangular cell-centre angles of indices lo .. hi - 1 (indices outside [0, n) extend the face's plane)."""
    hi = n if hi is None else hi
    return np.tan(-math.pi / 4 + (np.arange(lo, hi) + 0.5) * (math.pi / 2) / n)


def cell_vectors(n: int, lo: int = 0, hi: int | None = None) -> np.ndarray:
    """Unit vectors [6, rows, cols, 3] of the cell centres (rows and columns over indices lo .. hi - 1)."""
    c, e, d = face_frames()
    t = gnomonic(n, lo, hi)
    p = c[:, None, None, :] + t[None, None, :, None] * e[:, None, None, :] + t[None, :, None, None] * d[:, None, None, :]
    return p / np.linalg.norm(p, axis=-1, keepdims=True)


def cube_latlon(n: int):
    """(lat, lon) in degrees [6, n, n] of the cell centres; lon in [0, 360)."""
    p = cell_vectors(n)
    lat = np.degrees(np.arcsin(np.clip(p[..., 2], -1.0, 1.0)))
    lon = np.degrees(np.arctan2(p[..., 1], p[..., 0])) % 360.0
    return lat, lon


def latlon_axes(cfg: DlwpConfig):
    lat = 90.0 - (180.0 / (cfg.n_lat - 1)) * np.arange(cfg.n_lat)
    lon = (360.0 / cfg.n_lon) * np.arange(cfg.n_lon)
    return lat, lon


def ll_to_cs_map(cfg: DlwpConfig, lat=None, lon=None):
    """Bilinear lat-lon -> cube map as (row, col, S): row = cube cell, col = lat-lon point i n_lon + j; rows sum to 1."""
    if lat is None:
        lat, lon = cube_latlon(cfg.face)
    lat, lon = np.asarray(lat, np.float64).ravel(), np.asarray(lon, np.float64).ravel()
    dlat, dlon = 180.0 / (cfg.n_lat - 1), 360.0 / cfg.n_lon
    r = (90.0 - lat) / dlat
    i0 = np.clip(np.floor(r).astype(np.int64), 0, cfg.n_lat - 2)
    wr = np.clip(r - i0, 0.0, 1.0)
    c = (lon % 360.0) / dlon
    j0 = np.floor(c).astype(np.int64) % cfg.n_lon
    wc = c - np.floor(c)
    j1 = (j0 + 1) % cfg.n_lon
    rows = np.repeat(np.arange(lat.size), 4)
    cols = np.stack([i0 * cfg.n_lon + j0, i0 * cfg.n_lon + j1, (i0 + 1) * cfg.n_lon + j0, (i0 + 1) * cfg.n_lon + j1], 1).ravel()
    S = np.stack([(1 - wr) * (1 - wc), (1 - wr) * wc, wr * (1 - wc), wr * wc], 1).ravel()
    return rows, cols, S


def cs_to_ll_map(cfg: DlwpConfig):
    """Bilinear cube -> lat-lon map as (row, col, S): row = lat-lon point, col = cube cell f n^2 + y n + x; rows sum to 1.  Each point
    is interpolated on the face it projects to, between the four nearest cell centres of that face (clamped at the face edge)."""
    n = cfg.face
    lat, lon = latlon_axes(cfg)
    la, lo = np.meshgrid(np.radians(lat), np.radians(lon), indexing="ij")
    p = np.stack([np.cos(la) * np.cos(lo), np.cos(la) * np.sin(lo), np.sin(la)], -1).reshape(-1, 3)
    c, e, d = face_frames()
    dots = p @ c.T
    f = dots.argmax(1)
    pc = dots[np.arange(len(f)), f]
    a = np.einsum("ij,ij->i", p, e[f]) / pc
    b = np.einsum("ij,ij->i", p, d[f]) / pc
    u = (np.arctan(a) + math.pi / 4) / (math.pi / 2 / n) - 0.5        # fractional column
    v = (np.arctan(b) + math.pi / 4) / (math.pi / 2 / n) - 0.5        # fractional row
    x0 = np.clip(np.floor(u).astype(np.int64), 0, n - 2)
    y0 = np.clip(np.floor(v).astype(np.int64), 0, n - 2)
    wx = np.clip(u - x0, 0.0, 1.0)
    wy = np.clip(v - y0, 0.0, 1.0)
    base = (f * n + y0) * n + x0
    rows = np.repeat(np.arange(len(f)), 4)
    cols = np.stack([base, base + 1, base + n, base + n + 1], 1).ravel()
    S = np.stack([(1 - wy) * (1 - wx), (1 - wy) * wx, wy * (1 - wx), wy * wx], 1).ravel()
    return rows, cols, S


def to_csr(rows, cols, S, n_rows: int):
    """(row_ptr int64 [n_rows + 1], col int64, S float64) sorted by row; explicit zeros are dropped."""
    rows, cols, S = np.asarray(rows, np.int64), np.asarray(cols, np.int64), np.asarray(S, np.float64)
    keep = S != 0.0
    rows, cols, S = rows[keep], cols[keep], S[keep]
    order = np.lexsort((cols, rows))
    rows, cols, S = rows[order], cols[order], S[order]
    ptr = np.zeros(n_rows + 1, dtype=np.int64)
    np.add.at(ptr, rows + 1, 1)
    return np.cumsum(ptr), cols, S


# ---- TISR -------------------------------------------------------------------------------------------------------------------------- #
def days_since_j2000(t: datetime.datetime) -> float:
    return (t - J2000).total_seconds() / 86400.0


def solar_position(days):
    """(right ascension, declination, Greenwich mean sidereal time) in radians, float64, at ``days`` since J2000.0 -- the
    sidereal-time / ecliptic-longitude form of earth2mip's zenith_angle module (Meeus mean anomaly and equation of centre, obliquity
    from 23 deg 26' 21.406'', AIAA-2006 GMST).  The kernel (ingest) evaluates the same expressions."""
    T = np.asarray(days, np.float64) / 36525.0
    M = np.radians(357.52910 + 35999.05030 * T - 0.0001559 * T * T - 0.00000048 * T * T * T)
    L0 = np.radians(280.46645 + 36000.76983 * T + 0.0003032 * T * T)
    dL = np.radians((1.914600 - 0.004817 * T - 0.000014 * T * T) * np.sin(M) + (0.019993 - 0.000101 * T) * np.sin(2 * M)
                    + 0.000290 * np.sin(3 * M))
    lam = L0 + dL
    eps = np.radians(23.0 + 26.0 / 60.0 + 21.406 / 3600.0
                     - (46.836769 * T - 0.0001831 * T ** 2 + 0.00200340 * T ** 3 - 0.576e-6 * T ** 4 - 4.34e-8 * T ** 5) / 3600.0)
    x, y, z = np.cos(lam), np.cos(eps) * np.sin(lam), np.sin(eps) * np.sin(lam)
    r = np.sqrt(1.0 - z * z)
    dec = np.arctan2(z, r)
    ra = 2.0 * np.arctan2(y, x + r)
    theta = 67310.54841 + T * (876600.0 * 3600.0 + 8640184.812866 + T * (0.093104 - T * 6.2e-5))
    gmst = np.mod(np.radians(theta / 240.0), 2.0 * np.pi)
    return ra, dec, gmst


def cos_zenith(days, lat_deg, lon_deg):
    ra, dec, gmst = solar_position(days)
    la, lo = np.radians(np.asarray(lat_deg, np.float64)), np.radians(np.asarray(lon_deg, np.float64))
    return np.sin(la) * np.sin(dec) + np.cos(la) * np.cos(dec) * np.cos(gmst + lo - ra)


def tisr(days, lat_deg, lon_deg):
    """The TISR input channel: max(cos zenith, 0) - 1 / pi."""
    return np.maximum(cos_zenith(days, lat_deg, lon_deg), 0.0) - 1.0 / math.pi


# ---- synthetic parameters and states ------------------------------------------------------------------------------------------------- #
def channel_stats(cfg: DlwpConfig):
    names = CHANNELS if cfg.channels == len(CHANNELS) else [CHANNELS[i % len(CHANNELS)] for i in range(cfg.channels)]
    return (torch.tensor([_STATS[c][0] for c in names], dtype=torch.float64),
            torch.tensor([_STATS[c][1] for c in names], dtype=torch.float64))


def _smooth(lat_rad, lon_rad, gen, terms: int = 6):
    """A smooth random field on the sphere (sum of a few low-order waves), roughly unit variance."""
    out = np.zeros(np.broadcast(lat_rad, lon_rad).shape)
    for _ in range(terms):
        k = int(torch.randint(1, 6, (1,), generator=gen))
        m = int(torch.randint(0, 5, (1,), generator=gen))
        ph1, ph2 = (torch.rand(2, generator=gen) * 2 * math.pi).tolist()
        out = out + np.cos(k * lat_rad + ph1) * np.cos(m * lon_rad + ph2)
    return out * math.sqrt(2.0 / terms) * 1.4


def init_synthetic(cfg: DlwpConfig, seed: int = 0) -> dict:
    """Seeded parameters (fan-in scaled convs, small biases), the channel stats, smooth mask and topography, the cube's cell
    coordinates and both bilinear maps (``<map>.row / .col / .S``)."""
    gen = torch.Generator().manual_seed(seed)
    n = cfg.face
    out = {}
    center, scale = channel_stats(cfg)
    lat, lon = cube_latlon(n)
    la, lo = np.radians(lat), np.radians(lon)
    for name, shape in param_spec(cfg):
        if name == "center":
            t = center
        elif name == "scale":
            t = scale
        elif name == "lsm":
            t = torch.from_numpy(np.clip(0.5 + 0.4 * _smooth(la, lo, gen), 0.0, 1.0))
        elif name == "topography":
            t = torch.from_numpy(np.maximum(4000.0 + 6000.0 * _smooth(la, lo, gen), 0.0))
        elif name == "cube_lat":
            t = torch.from_numpy(lat)
        elif name == "cube_lon":
            t = torch.from_numpy(lon)
        elif name.endswith(".bias"):
            t = 0.02 * torch.randn(shape, generator=gen, dtype=torch.float64)
        else:
            fan_in = shape[1] * shape[2] * shape[3]
            t = torch.randn(shape, generator=gen, dtype=torch.float64) * math.sqrt(1.5 / fan_in)
        out[name] = t.float().contiguous() if name not in ("cube_lat", "cube_lon") else t.contiguous()
    for key, (r, c, s) in (("ll_to_cs", ll_to_cs_map(cfg, lat, lon)), ("cs_to_ll", cs_to_ll_map(cfg))):
        out[key + ".row"], out[key + ".col"], out[key + ".S"] = torch.from_numpy(r), torch.from_numpy(c), torch.from_numpy(s)
    return out


def synthetic_state(cfg: DlwpConfig, seed: int = 0) -> torch.Tensor:
    """(channels, n_lat, n_lon) fp32 state of ERA5 magnitudes: center + scale * smooth noise."""
    gen = torch.Generator().manual_seed(seed + 7919)
    lat, lon = latlon_axes(cfg)
    la, lo = np.meshgrid(np.radians(lat), np.radians(lon), indexing="ij")
    center, scale = channel_stats(cfg)
    x = np.stack([float(center[c]) + float(scale[c]) * _smooth(la, lo, gen) for c in range(cfg.channels)])
    return torch.from_numpy(x).float().contiguous()
