"""Float64 route through the Pangu oracle, the small grids whose paddings the 49 x 192 toy never has, and the error norms of the
stage tests (tests/test_pangu_kernels_gpu.py, tests/test_pangu_reference_cpu.py).

oracle/pangu_oracle.py takes its dtype from its input, so the reference here is the oracle itself on double inputs; this file restates no
kernel.  What it adds is glue the oracle keeps inside ``forward``: the normalisation in front of PatchEmbedding, the concat and the
de-normalisation around PatchRecovery (``stage``), so that one stage can be run alone on a chosen input and in a chosen dtype.
"""
from __future__ import annotations

from functools import lru_cache
from typing import NamedTuple

import torch

from oracle import pangu_oracle as O
from skyrim_amd.pangu.spec import PanguGeometry, init_synthetic, synthetic_state


class Grid(NamedTuple):
    """One row of the geometry table: what the grid is FOR.  (pad, top) pairs are (zero rows added in all, of them above the data)."""
    n_lat: int
    n_lon: int
    pad: str
    lat_pad: tuple          # input latitude -> multiple of 4
    H1: int
    H2: int
    down_pad_row: bool      # H1 odd: the last merged row of DownSample is half zero padding
    win_pad_fine: tuple     # layers 1 / 4: H1 -> multiple of 6
    win_pad_coarse: tuple   # layers 2 / 3: H2 -> multiple of 6
    tokens: tuple           # (fine, coarse)

    @property
    def id(self):
        return f"{self.n_lat}x{self.n_lon}" + ("" if self.pad == "centre" else "-" + self.pad)


# Asserted against PanguGeometry and the oracle's Geometry in test_pangu_reference_cpu.py.
# 24: no latitude padding at all, and in layers 1 / 4 one latitude window (first AND last window type); 27 / 26 / 25: input padding of
# 1 (none on top), 2, 3 rows; 33: window paddings 3 and 1; 27 x 192: two longitude windows at the coarse level and a 336-row surface slab
# (ends on a 16-row block boundary; the 168-row slabs of the 96-wide grids end inside a block).  pad="back": lat_top = 0 with two / three
# rows cropped at the bottom.  The slabs the stage GEMMs run over (hw, 7 hw, the fine token count) are no multiple of their 64- / 128- /
# 256-row tiles on any grid; of the coarse counts 288 and 480 leave a tail tile, 384 and 768 do not.
GRIDS = (
    Grid(24, 96, "centre", (0, 0), 6, 3, False, (0, 0), (3, 1), (1152, 288)),
    Grid(25, 96, "centre", (3, 1), 7, 4, True, (5, 2), (2, 1), (1344, 384)),
    Grid(26, 96, "centre", (2, 1), 7, 4, True, (5, 2), (2, 1), (1344, 384)),
    Grid(27, 96, "centre", (1, 0), 7, 4, True, (5, 2), (2, 1), (1344, 384)),
    Grid(33, 96, "centre", (3, 1), 9, 5, True, (3, 1), (1, 0), (1728, 480)),
    Grid(27, 192, "centre", (1, 0), 7, 4, True, (5, 2), (2, 1), (2688, 768)),
    Grid(26, 96, "back", (2, 0), 7, 4, True, (5, 0), (2, 0), (1344, 384)),
    Grid(25, 96, "back", (3, 0), 7, 4, True, (5, 0), (2, 0), (1344, 384)),
)
GRID = {g.id: g for g in GRIDS}
SEED = 5
STAGES = ("embed", "down", "up", "recover")


def to64(params):
    """Every floating parameter as double (the oracle's stage functions then run in float64 unchanged)."""
    return {k: (v.double() if v.is_floating_point() else v) for k, v in params.items()}


@lru_cache(maxsize=None)
def inputs(n_lat, n_lon, seed=SEED):
    """(float32 parameters, their float64 copy, float32 state) -- shared by the two pad conventions of a grid; read-only."""
    g = PanguGeometry(n_lat, n_lon)
    params = init_synthetic(g, seed)
    return params, to64(params), synthetic_state(g, seed)


@lru_cache(maxsize=None)
def reference(n_lat, n_lon, pad="centre", seed=SEED, conventions=()):
    """Float64 taps and output of one step: (taps, y).  ``conventions``: a tuple of (name, value) pairs for pangu_oracle.Conventions
    besides ``pad``.  Computed once per argument set; callers leave it unchanged."""
    _, p64, x = inputs(n_lat, n_lon, seed)
    taps = {}
    y = O.forward(p64, x.double(), taps=taps, conv=O.Conventions(pad=pad, **dict(conventions)))
    return taps, y


def stage_inputs(taps, x):
    """The float32 tensors each stage is fed on BOTH sides: the float32 rounding of the float64 tap in front of it (the state itself
    for PatchEmbedding)."""
    def f32(name):
        return taps[name].float().contiguous()
    return {"embed": (x,), "down": (f32("layer1.block1"),), "up": (f32("layer3"),), "recover": (f32("layer1.block1"), f32("layer4"))}


SMALL = 0.05


def small_stream_inputs(taps):
    """DownSample's and UpSample's inputs scaled by SMALL: the rows their LayerNorms see then have a variance of 1e-3 .. 1e-2, where
    eps = 1e-5 carries weight (on the taps as they are a tenfold change of eps moves the result by 2e-6, which no bar here would see).
    0.05 keeps the lo planes of the fp16 hi / lo split clear of the coarse end of fp16's subnormals (|x| ~ 0.05: lo ~ 2e-5, resolved to 6e-8)."""
    return {"down": ((taps["layer1.block1"] * SMALL).float().contiguous(),), "up": ((taps["layer3"] * SMALL).float().contiguous(),)}


def stage(name, params, grid, *xs, conv=O.DEFAULT):
    """One stage outside the blocks through the oracle's own function, in the dtype of ``params`` (inputs are converted to it).
    embed: (69, n_lat, n_lon) physical state -> (N1, 192); down: (N1, 192) -> (N2, 384); up: (N2, 384) -> (N1, 192);
    recover: skip (N1, 192), x4 (N1, 192) -> (69, n_lat, n_lon) physical."""
    dt = params["norm.std"].dtype
    xs = [t.to(dt) for t in xs]
    g = O.Geometry(grid.n_lat, grid.n_lon, grid.pad)
    mean, std = params["norm.mean"][:, None, None], params["norm.std"][:, None, None]
    if name == "embed":
        upper, surface = O.split_state((xs[0] - mean) / std)
        return O.patch_embed(params, g, upper, surface, None, conv)
    if name == "down":
        return O.downsample(params, g, xs[0])
    if name == "up":
        return O.upsample(params, g, xs[0])
    if name == "recover":
        up, sf = O.patch_recover(params, g, torch.cat([xs[0], xs[1]], -1), None, conv)
        return torch.cat([up.reshape(-1, *up.shape[2:]), sf], 0) * std + mean
    raise KeyError(name)


# ---- norms ------------------------------------------------------------------------------------ #
def max_rel(got, ref):
    """(max|got - ref| / max|ref|, flat index of the worst element): the definition behind BAR3 (tests/test_fuxi_kernels_gpu.py)."""
    d = (got.detach().double().cpu() - ref.double()).abs()
    return (d.max() / ref.double().abs().max()).item(), int(d.argmax())


def sigma_err(got, ref, std):
    """(per-channel max|got - ref| / sigma_c as a (69,) double tensor, flat index of the element that is worst in those units)."""
    got = got.detach().double().cpu()
    d = (got - ref.double()).abs() / std.double().reshape(-1, 1, 1)
    return O.per_channel_sigma_err(got, ref.double(), std.double()), int(d.argmax())


# ---- where a failure sits ---------------------------------------------------------------------- #
def _fine_row_touches_pad(grid, h):
    top = grid.lat_pad[1]
    return 4 * h - top < 0 or 4 * h + 3 - top >= grid.n_lat


def locate(name, grid, flat):
    """A failure message's "where": token row (z, h, w) of a token stage's worst element, (channel, lat, lon) for recovery, and whether
    that row reads or writes a padded / cropped latitude."""
    if name == "recover":
        per = grid.n_lat * grid.n_lon
        c, lat, lon = flat // per, flat % per // grid.n_lon, flat % grid.n_lon
        h = (lat + grid.lat_pad[1]) // 4
        return f"(channel, lat, lon) = ({c}, {lat}, {lon}); token row h = {h} " + ("is partly cropped" if _fine_row_touches_pad(grid, h) else "is whole")
    fine = name in ("embed", "up")
    C, H, W = (192, grid.H1, grid.n_lon // 4) if fine else (384, grid.H2, grid.n_lon // 8)
    m, c = flat // C, flat % C
    z, h, w = m // (H * W), m % (H * W) // W, m % W
    if fine:
        pad = _fine_row_touches_pad(grid, h)
    else:
        pad = 2 * h + 1 >= grid.H1 or _fine_row_touches_pad(grid, 2 * h) or _fine_row_touches_pad(grid, min(2 * h + 1, grid.H1 - 1))
    return f"token row {m} = (z, h, w) = ({z}, {h}, {w}), column {c}; the row " + ("touches a padded latitude" if pad else "touches no padding")
