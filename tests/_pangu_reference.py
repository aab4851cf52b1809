"""Float64 route through the Pangu oracle, the small grids whose paddings the 49 x 192 toy never has, the error norms of the
stage tests (tests/test_pangu_kernels_gpu.py, tests/test_pangu_reference_cpu.py), and the operands of the attention tests
(tests/test_pangu_attention_kernels_gpu.py): window table, compact bias, Q / K / V^T, softmax core, parameters with a peaked softmax; and
everything of a block after the attention, per term form, with its bar and edge parameters (tests/test_pangu_block_kernels_gpu.py).

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


# ---- everything of a block after the attention (tests/test_pangu_block_kernels_gpu.py) ------------------------------------------------ #
# csrc/fused_block.hip's header gives the operation and, per term form, where an operand is rounded on its way into a GEMM; nothing of the
# kernels is restated: Linear, LayerNorm and erf-GELU are torch's own, in the dtype of ``x``.
FORMS = ("three", "two", "one")
GELU_CLAMP = 5.9396969619669995                 # tools/gelu_fit.py U = 4.2 sqrt(2)
# tools/gelu_fit.py c1 .. c8 as csrc/common.h gelu_erf2 holds them (float32 values; c0 = 0)
GELU_COEFFS = (-1.151117682e+00, -4.591012597e-01, -5.282834917e-02, 7.545167115e-03, -4.982745158e-04, -4.273382365e-05, 1.091520153e-05, -6.177511978e-07)


def gelu_poly64(x):
    """The project's degree-8 fit of log2 erfc evaluated in float64: E = 2^Q(min(|x|, U)), GELU = x / 2 (2 - E) for x > 0 and x / 2 E otherwise."""
    x = x.double()
    a = x.abs().clamp(max=GELU_CLAMP)
    c = torch.tensor(GELU_COEFFS, dtype=torch.float32).double()
    p = torch.zeros_like(a)
    for k in range(len(GELU_COEFFS) - 1, -1, -1):
        p = (p + c[k]) * a
    e = torch.exp2(p)
    return 0.5 * x * torch.where(x > 0, 2 - e, e)


def form_of(plan, layer):
    """The term form the block kernels of ``layer`` (1 .. 4) run under term plan ``plan`` (skyrim_amd/pangu/engine.py: bits 0-3 two terms, bits 8-11 one)."""
    return "one" if (plan >> (8 + layer - 1)) & 1 else "two" if (plan >> (layer - 1)) & 1 else "three"


def inverse_window_table(table, ntok):
    """Stream token -> window row: the left inverse of ``window_table`` on every real token (each token sits in exactly one window row)."""
    rows = torch.nonzero(table >= 0).flatten()
    inv = torch.full((ntok,), -1, dtype=torch.long)
    inv[table[rows]] = rows
    return inv


def ao_tokens(planes, table, ntok, C, one):
    """The device's attention output in stream-token order, float64: ``planes`` = (hi, lo) flat planes of the blocked ``ao`` buffer (fp16 or
    bf16), un-blocked as pangu/calibration.py does and gathered through the inverse of ``table``.  hi + lo is exact in float64; ``one``: the
    hi plane alone (a one-term layer neither writes nor reads the lo plane, it holds stale bytes)."""
    from skyrim_amd.pangu.calibration import _unblock
    hi, lo = planes
    flat = hi.double() if one else hi.double() + lo.double()
    return _unblock(flat, table.numel(), C)[inverse_window_table(table, ntok)]


def stream_planes(x, bf16=False):
    """The float32 stream as the engine holds it after ``to_planes``: hi = x rounded to fp16 (bf16), lo = (x - hi) rounded; hi + lo in float64."""
    t = torch.bfloat16 if bf16 else torch.float16
    hi = x.float().to(t)
    lo = (x.float() - hi.float()).to(t)
    return hi.double() + lo.double()


def post_attention_reference(pb, x, ao_tokens, form, eps=1e-5, gelu=F.gelu, parts=False):
    """x_mid = x + LN1(ao Wp^T + bp);  out = x_mid + LN2(fc2(GELU(fc1(x_mid)))) in the dtype of ``x`` (float64: the reference; float32: the
    yardstick, same rounding points).  ``pb``: the block's parameters in any float type.  ``form``: "three" -- weights as they are; "two" --
    proj / fc1 / fc2 weights rounded to ONE fp16 plane (with nearest rounding and no calibration those ARE the engine's weights); "one" -- also
    the GEMM operands x_mid and the hidden activation rounded to fp16 where they enter a GEMM (``ao_tokens`` is then the hi plane already); the
    residual path keeps x_mid unrounded.  ``parts``: also the intermediates, as a dict."""
    assert form in FORMS
    dt = x.dtype
    p = {k: v.to(dt) for k, v in pb.items() if v.is_floating_point()}
    w = (lambda k: p[k]) if form == "three" else (lambda k: pb[k].half().to(dt))
    rnd = (lambda t: t.half().to(dt)) if form == "one" else (lambda t: t)
    C = x.shape[-1]
    a = F.linear(ao_tokens.to(dt), w("attn.proj.weight"), p["attn.proj.bias"])
    ln1 = F.layer_norm(a, (C,), p["norm1.weight"], p["norm1.bias"], eps)
    x_mid = x + ln1
    pre = F.linear(rnd(x_mid), w("mlp.fc1.weight"), p["mlp.fc1.bias"])
    hid = gelu(pre).to(dt)
    y = F.linear(rnd(hid), w("mlp.fc2.weight"), p["mlp.fc2.bias"])
    out = x_mid + F.layer_norm(y, (C,), p["norm2.weight"], p["norm2.bias"], eps)
    return dict(proj=a, ln1=ln1, x_mid=x_mid, pre=pre, hid=hid, fc2=y, out=out) if parts else out


def oracle_attention_tokens(pb, x, grid, layer, rolled, conv=O.DEFAULT):
    """The oracle's own attention output (before the projection) in stream-token order, in the dtype of ``x``: ``earth_attention`` with an
    identity projection on the rows gathered through ``window_table``."""
    heads, C = O.HEADS[layer - 1], x.shape[-1]
    nZ, nH, nW = window_shape(grid, layer, conv)
    table = window_table(grid, layer, rolled, conv)
    rows = torch.where((table >= 0)[:, None], x[table.clamp_min(0)], torch.zeros((), dtype=x.dtype)).reshape(nZ * nH, nW, L, C)
    p = dict(pb)
    p["attn.proj.weight"], p["attn.proj.bias"] = torch.eye(C, dtype=x.dtype), torch.zeros(C, dtype=x.dtype)
    mask = O.shifted_window_mask(2 * nZ, 6 * nH, 12 * nW, x.dtype, conv) if rolled else None
    o = O.earth_attention(p, rows, nZ * nH, heads, mask, None, conv).reshape(-1, C)
    return o[inverse_window_table(table, x.shape[0])]


def weight_planes(w, bf16=False):
    """A three-term weight as the engine holds it: hi + lo planes of fp16 (bf16), in float64.  The lo plane of an fp16 pair is below 2^-14
    whenever |w| < 2^-3, and fp16 resolves it to 2^-25 there whatever its size: a weight of 0.013 is held to 19 bits, one of 0.001 to 15."""
    return stream_planes(w, bf16)


def block_bar(pb, x64, ao64, form, bf16=False, eps=1e-5):
    """(ref, e32, e_gelu, e_w, bar) of one post-attention case, from the reference alone: ref = the float64 result; e32 = the float32 yardstick
    against it; e_gelu = the same float64 run with ``gelu_poly64`` against it; e_w (form "three" only, else 0) = the same float64 run with the
    proj / fc1 / fc2 weights as ``weight_planes`` against it (all as max|.| / max|ref|);
    bar = max(B, 16 k e32) + 2 e_gelu + e_w with B = BAR3 = 2e-6, k = 1 for fp16 planes and B = 64 BAR3, k = 64 for bf16."""
    ref = post_attention_reference(pb, x64, ao64, form, eps)
    f32 = post_attention_reference({k: v.float() for k, v in pb.items()}, x64.float(), ao64.float(), form, eps)
    e32 = max_rel(f32, ref)[0]
    e_gelu = max_rel(post_attention_reference(pb, x64, ao64, form, eps, gelu=gelu_poly64), ref)[0]
    e_w = 0.0
    if form == "three":
        pw = {k: (weight_planes(v, bf16) if k in ("attn.proj.weight", "mlp.fc1.weight", "mlp.fc2.weight") else v) for k, v in pb.items()}
        e_w = max_rel(post_attention_reference(pw, x64, ao64, form, eps), ref)[0]
    k = 64 if bf16 else 1
    return ref, e32, e_gelu, e_w, max(k * BLOCK_BAR3, 16 * k * e32) + 2 * e_gelu + e_w


BLOCK_BAR3 = 2e-6                               # tests/test_pangu_kernels_gpu.py BAR3
EDGES = ("zero_ao", "zero_ao_fc2", "zero_var", "eps", "gelu")
ZERO_VAR_BIAS = 0.375                           # exactly representable; 192 and 384 copies of it sum exactly in fp32 and float64
EPS_TARGET_VAR = 3e-4                           # median row variance of the two LayerNorm inputs under "eps": eps = 1e-5 is 3 % of it
GELU_SHIFT, GELU_STD = -4.0, 4.0                # fc1 pre-activations under "gelu": centred in the negative tail, 0.6 % of a normal law beyond +5.94


def edge_params(grid, edge):
    """(float32 parameters, their float64 copy) of ``peaked_params`` edited in the four tested blocks -- a block kernel always runs behind its
    attention, so an edge is reached through parameters:
      zero_ao      the V rows of attn.qkv (weight and bias) are zero: the attention output is 0 exactly, x_mid - x = LN1(proj.bias) for every token
      zero_ao_fc2  and mlp.fc2.weight = 0: out = x + LN1(bp) + LN2(b2)
      zero_var     zero_ao with attn.proj.bias = 0.375 in every channel: LayerNorm 1 sees rows of variance exactly 0 and yields norm1.bias
      eps          attn.proj and mlp.fc2 (weight and bias) scaled so that the median row variance in front of each LayerNorm is 3e-4
      gelu         mlp.fc1 scaled and shifted so that its pre-activations have mean -4, std 4: past the clamp on both sides
    The scales of ``eps`` and ``gelu`` are measured in float64 on the oracle's own attention output of the block's input tap.  Read-only."""
    assert edge in EDGES
    return _edge_params(grid, edge)


@lru_cache(maxsize=None)
def _edge_params(grid, edge):
    conv = conventions_of(grid)
    base, base64 = peaked_params(grid)
    taps, _ = reference(grid.n_lat, grid.n_lon, grid.pad)
    out = {k: v.clone() for k, v in base.items()}
    for layer, i in PEAKED_BLOCKS:
        pre, C = f"layer{layer}.block{i}.", O.DIM * (1 if layer in (1, 4) else 2)
        if edge in ("zero_ao", "zero_ao_fc2", "zero_var"):
            out[pre + "attn.qkv.weight"][2 * C:] = 0
            out[pre + "attn.qkv.bias"][2 * C:] = 0
            if edge == "zero_ao_fc2":
                out[pre + "mlp.fc2.weight"].zero_()
            if edge == "zero_var":
                out[pre + "attn.proj.bias"].fill_(ZERO_VAR_BIAS)
            continue
        x = taps[BEFORE[layer, i]].float().double()
        pb = O._block_params(base64, layer, i)
        ao = oracle_attention_tokens(pb, x, grid, layer, i % 2 == 1, conv)
        if edge == "eps":
            s1 = (EPS_TARGET_VAR / post_attention_reference(pb, x, ao, "three", parts=True)["proj"].var(-1, unbiased=False).median().item()) ** 0.5
            out[pre + "attn.proj.weight"] *= s1
            out[pre + "attn.proj.bias"] *= s1
            pb = O._block_params(to64({k: v for k, v in out.items() if k.startswith(pre)}), layer, i)
            s2 = (EPS_TARGET_VAR / post_attention_reference(pb, x, ao, "three", parts=True)["fc2"].var(-1, unbiased=False).median().item()) ** 0.5
            out[pre + "mlp.fc2.weight"] *= s2
            out[pre + "mlp.fc2.bias"] *= s2
        else:
            h = post_attention_reference(pb, x, ao, "three", parts=True)["pre"]
            gain = GELU_STD / h.std().item()
            out[pre + "mlp.fc1.weight"] *= gain
            out[pre + "mlp.fc1.bias"] = out[pre + "mlp.fc1.bias"] * gain + (GELU_SHIFT - gain * h.mean().item())
    return out, to64(out)


def locate_token(grid, layer, flat, C):
    """(token row -> z, h, w; channel) of a flat index into a [tokens][C] stream."""
    _, H, W = O.Geometry(grid.n_lat, grid.n_lon, grid.pad).res(layer)
    m, c = flat // C, flat % C
    return f"token row {m} -> (z, h, w) = ({m // (H * W)}, {m % (H * W) // W}, {m % W}), channel {c}"
