"""Float64 route through the Pangu oracle, the small grids whose paddings the 49 x 192 toy never has, the error norms of the
stage tests (tests/test_pangu_kernels_gpu.py, tests/test_pangu_reference_cpu.py), and the operands of the attention tests
(tests/test_pangu_attention_kernels_gpu.py): window table, compact bias, Q / K / V^T, softmax core, parameters with a peaked softmax.

oracle/pangu_oracle.py takes its dtype from its input, so the reference here is the oracle itself on double inputs; this file restates no
kernel.  What it adds is glue the oracle keeps inside ``forward``: the normalisation in front of PatchEmbedding, the concat and the
de-normalisation around PatchRecovery (``stage``), so that one stage can be run alone on a chosen input and in a chosen dtype.
"""
from __future__ import annotations

from functools import lru_cache
from typing import NamedTuple

import torch
import torch.nn.functional as F

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


# ---- attention operands: window table, compact bias, QKV, softmax core (tests/test_pangu_attention_kernels_gpu.py) -------------------- #
# Built from the oracle's own functions (``_centre_pad``, ``position_index``, ``shifted_window_mask`` and the pad / roll / partition lines of
# ``earth_block``); the layouts are the ones the comments of csrc/aux.hip, csrc/rowtile.hip and csrc/attention.hip give.
BEFORE = {(1, 0): "embed", (1, 1): "layer1.block0", (2, 0): "down", (2, 1): "layer2.block0"}     # the tap in front of each tested block
PEAKED_BLOCKS = tuple(BEFORE)
# Target std of the q . k logits per block.  One figure does not serve all four: layer1.block0 reads the patch embedding, whose logits are
# heavy-tailed -- at std 1.5 already 8 .. 12 % of its rows put more than half their weight on one key, and from std 2.6 on the median effective
# number of keys drops under 5 -- while the other three blocks' logits are close to normal and at std 1.5 .. 4 fewer than 1 % of their rows are
# that peaked (0 .. 0.9 % on 24 x 96).  At 5.0 they have 1.6 .. 7.7 % such rows with a median of 9 .. 22 effective keys, on every grid used
# (tests/test_pangu_reference_cpu.py asserts the condition).
PEAKED_LOGIT_STD = {(1, 0): 1.5, (1, 1): 5.0, (2, 0): 5.0, (2, 1): 5.0}
PEAKED_BIAS_GAIN = 100.0
HEAD_DIM = 32
L = O.WINDOW[0] * O.WINDOW[1] * O.WINDOW[2]


def make_grid(n_lat, n_lon, pad="centre"):
    """A ``Grid`` row for a geometry outside ``GRIDS`` (49 x 96: three / two latitude windows; 25 x 864: 18 / 9 longitude windows)."""
    g = PanguGeometry(n_lat, n_lon, pad)
    return Grid(n_lat, n_lon, pad, (g.lat_padded - g.n_lat, g.lat_pad_top), g.H1, g.H2, g.H1 % 2 == 1, (g.padded_lat(1) - g.H1, g.pad_top(1)),
                (g.padded_lat(2) - g.H2, g.pad_top(2)), (g.tokens(1), g.tokens(2)))


def conventions_of(grid, **kw):
    return O.Conventions(pad=grid.pad, **kw)


def window_shape(grid, layer, conv=O.DEFAULT):
    """(nZ, nH, nW) of a layer's window partition."""
    Z, H, W = O.Geometry(grid.n_lat, grid.n_lon, conv.pad).res(layer)
    return Z // O.WINDOW[0], O._centre_pad(H, O.WINDOW[1], conv.pad)[0] // O.WINDOW[1], W // O.WINDOW[2]


def window_table(grid, layer, rolled, conv=O.DEFAULT):
    """Window row -> stream token as an int64 vector [windows * 144], -1 on padded latitudes: the token NUMBERS sent through the pad, roll
    and partition of ``earth_block``.  Tokens are numbered in storage order (surface slab at level 0 whatever ``conv.surface`` says)."""
    Z, H, W = O.Geometry(grid.n_lat, grid.n_lon, conv.pad).res(layer)
    wz, wh, ww = O.WINDOW
    tok = torch.arange(Z * H * W).reshape(Z, H, W)
    if conv.surface == "last":                      # logical level k is storage level k + 1, the last logical level is storage level 0
        tok = torch.roll(tok, -1, 0)
    Hp, top, bot = O._centre_pad(H, wh, conv.pad)
    x = F.pad(tok, (0, 0, top, bot), value=-1)
    sg = 1 if conv.roll_sign > 0 else -1
    if rolled:
        x = torch.roll(x, shifts=(sg * (wz // 2), sg * (wh // 2), sg * (ww // 2)), dims=(0, 1, 2))
    nZ, nH, nW = Z // wz, Hp // wh, W // ww
    return x.reshape(nZ, wz, nH, wh, nW, ww).permute(0, 2, 4, 1, 3, 5).reshape(-1)


def locate_window_row(m, nH, nW):
    """(window type, w-window, z, h, w) of window row ``m``."""
    win, t = divmod(int(m), L)
    return win // nW, win % nW, t // 72, t // 12 % 6, t % 12


def _pair_cells():
    """For every (query, key) of the 144 x 144: its row (z_q + 2 z_k) 36 + (h_q + 6 h_k) and column w_k - w_q + 11 in the compact table."""
    qi, ki = torch.meshgrid(torch.arange(L), torch.arange(L), indexing="ij")
    row = (qi // 72 + 2 * (ki // 72)) * 36 + (qi // 12) % 6 + 6 * ((ki // 12) % 6)
    return row, ki % 12 - qi % 12 + 11


def full_bias(table, types, heads, nZ, nH, rolled, conv=O.DEFAULT):
    """[types][heads][query][key]: the oracle's gather of the bias table (``earth_attention``) plus the shifted-window mask when rolled."""
    assert types == nZ * nH and table.shape == (3312, types, heads)
    bias = table[O.position_index().reshape(-1)].reshape(L, L, types, heads)
    bias = bias.permute(2, 3, 0, 1) if conv.bias_index == "qk" else bias.permute(2, 3, 1, 0)
    if rolled:
        bias = bias + O.shifted_window_mask(2 * nZ, 6 * nH, 12, table.dtype, conv)[:, 0][:, None]
    return bias.contiguous()


def compact_bias(table, types, heads, nZ, nH, rolled, conv=O.DEFAULT):
    """(expected [types][heads][144][24] table in the dtype of ``table``, cells of columns 0 .. 22 that no (query, key) pair addresses, cells
    to which two pairs wrote different values).  Column 23 is zero."""
    full = full_bias(table, types, heads, nZ, nH, rolled, conv).reshape(types, heads, L * L)
    row, col = _pair_cells()
    cell = (row * 24 + col).reshape(-1).expand(types, heads, -1)
    lo = torch.full((types, heads, L * 24), float("inf"), dtype=full.dtype).scatter_reduce(2, cell, full, "amin")
    hi = torch.full((types, heads, L * 24), float("-inf"), dtype=full.dtype).scatter_reduce(2, cell, full, "amax")
    hit = torch.isfinite(lo)
    live = torch.ones(L, 24, dtype=torch.bool)
    live[:, 23] = False
    unaddressed = int((~hit & live.reshape(-1)).sum())
    assert not bool((hit & ~live.reshape(-1)).any())
    conflicts = int((hit & (lo != hi)).sum())
    return torch.where(hit, hi, torch.zeros_like(hi)).reshape(types, heads, L, 24), unaddressed, conflicts


def locate_bias_cell(flat, heads):
    """(type, head, row -> z_q, z_k, h_q, h_k, column) of a flat index into a [types][heads][144][24] table."""
    e, r, th = flat % 24, flat // 24 % L, flat // (24 * L)
    return f"type {th // heads}, head {th % heads}, row {r} -> (z_q, z_k, h_q, h_k) = ({r // 36 & 1}, {r // 36 >> 1}, {r % 36 % 6}, {r % 36 // 6}), column {e}"


def qkv_reference(pb, x, table, heads, conv=O.DEFAULT):
    """Float64 Q (scaled by 32^-0.5), K, V^T of one block in the device layouts -- q, k [win][head][144][32], vt [win][head][32][144] -- from
    the stream rows ``x`` gathered through ``table`` (zeros on -1), and with each the magnitude sum_k |x_k| |w_k| of its dot products:
    {"q": (ref, mag), "k": ..., "vt": ...}.  ``pb``: the block's float64 parameters (``O._block_params``)."""
    assert conv.qkv_order == "3hd"
    x = x.double()
    rows = torch.where((table >= 0)[:, None], x[table.clamp_min(0)], torch.zeros((), dtype=x.dtype))
    nwin, C = rows.shape[0] // L, rows.shape[1]
    w, b = pb["attn.qkv.weight"].double(), pb["attn.qkv.bias"].double()
    ref = F.linear(rows, w, b).reshape(nwin, L, 3, heads, HEAD_DIM).permute(2, 0, 3, 1, 4)       # [3][win][head][144][32]
    mag = F.linear(rows.abs(), w.abs()).reshape(nwin, L, 3, heads, HEAD_DIM).permute(2, 0, 3, 1, 4)
    s = HEAD_DIM ** -0.5
    return {"q": ((ref[0] * s).contiguous(), mag[0].contiguous()), "k": (ref[1].contiguous(), mag[1].contiguous()),
            "vt": (ref[2].transpose(-1, -2).contiguous(), mag[2].transpose(-1, -2).contiguous())}


def attention_reference(q, k, vt, bias_cmp, types, heads, nW):
    """Float64 softmax attention of the GIVEN operands (the device's own fp16 q, k, vt and compact bias, or any other): q (already scaled)
    and k [win][head][144][32], vt [win][head][32][144], win = type * nW + w-window; bias [types][heads][144][24], gathered per (query, key)
    at row (z_q + 2 z_k) 36 + (h_q + 6 h_k), column w_k - w_q + 11.  Returns o [win * 144][heads * 32] (head-major columns), the weights
    p [win][head][query][key] and D [win * 144][heads * 32] = sum_k p_k |v_kd - o_qd|, the first-order sensitivity of o to a relative
    perturbation of every weight when the perturbed weights are re-normalised."""
    nwin = types * nW
    q = q.double().reshape(nwin, heads, L, HEAD_DIM)
    k = k.double().reshape(nwin, heads, L, HEAD_DIM)
    v = vt.double().reshape(nwin, heads, HEAD_DIM, L).transpose(-1, -2)
    row, col = _pair_cells()
    bias = bias_cmp.double().reshape(types, heads, L, 24)[:, :, row, col]                       # [types][heads][q][k]
    s = q @ k.transpose(-1, -2) + bias.repeat_interleave(nW, 0)
    p = torch.softmax(s, -1)
    o = p @ v
    D = torch.empty_like(o)
    for w0 in range(0, nwin, 4):                                                               # [4 win][head][q][k][d]: ~ 100 MB at 12 heads
        sl = slice(w0, w0 + 4)
        D[sl] = (p[sl, :, :, :, None] * (v[sl, :, None, :, :] - o[sl, :, :, None, :]).abs()).sum(3)
    rows = lambda t: t.permute(0, 2, 1, 3).reshape(nwin * L, heads * HEAD_DIM)          # [win][head][q][d] -> [win * 144][head-major columns]
    return rows(o), p, rows(D)


def locate_attention_row(m, col, nW):
    """(window type, w-window, head, query -> z_q, h_q, w_q) of element (row m, column col) of the attention output."""
    win, t = divmod(int(m), L)
    return f"window type {win // nW}, w-window {win % nW}, head {int(col) // HEAD_DIM} (dim {int(col) % HEAD_DIM}), query {t} -> (z_q, h_q, w_q) = ({t // 72}, {t // 12 % 6}, {t % 12})"


def peaked_params(grid, conv=None):
    """(float32 parameters, their float64 copy) of ``inputs`` with a softmax that is NOT nearly uniform in the four tested blocks: the bias
    table times 100 (std 1.77, within +-4, every entry still distinct), and the Q rows of the qkv Linear (weight and bias) times
    gain = PEAKED_LOGIT_STD[block] / std(q . k), the logits measured in float64 from the unmodified parameters on the block's own input tap.
    Read-only, like ``inputs``."""
    return _peaked_params(grid, conv or conventions_of(grid))


@lru_cache(maxsize=None)
def _peaked_params(grid, conv):
    params, p64, _ = inputs(grid.n_lat, grid.n_lon)
    extra = tuple((f, getattr(conv, f)) for f in ("roll_sign", "mask_value", "surface", "qkv_order", "bias_index") if getattr(conv, f) != getattr(O.DEFAULT, f))
    taps, _ = reference(grid.n_lat, grid.n_lon, conv.pad, conventions=extra)
    out = {k: v.clone() for k, v in params.items()}
    for layer, i in PEAKED_BLOCKS:
        pre, heads, C = f"layer{layer}.block{i}.", O.HEADS[layer - 1], O.DIM * (1 if layer in (1, 4) else 2)
        ops = qkv_reference(O._block_params(p64, layer, i), taps[BEFORE[layer, i]].float(), window_table(grid, layer, i % 2 == 1, conv), heads, conv)
        logits = ops["q"][0] @ ops["k"][0].transpose(-1, -2)
        gain = PEAKED_LOGIT_STD[layer, i] / logits.std().item()
        out[pre + "attn.bias_table"] *= PEAKED_BIAS_GAIN
        out[pre + "attn.qkv.weight"][:C] *= gain
        out[pre + "attn.qkv.bias"][:C] *= gain
    return out, to64(out)
