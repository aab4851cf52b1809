"""Everything of a Pangu block that follows the attention -- projection, LayerNorm + residual, fc1, GELU, fc2, LayerNorm + residual -- against
float64, per term form, on the DEVICE's OWN attention output.  Section F of tests/test_pangu_attention_kernels_gpu.py, in a file of its own.

What is compared.  One block runs on the engine (``PanguEngine.block`` on the float32 tap in front of it); the attention output ``ao`` is read
back through ``debug_buffer`` (its fp16 / bf16 planes, un-blocked and gathered through the inverse of ``R.window_table``) and the rest of the
block is evaluated by ``R.post_attention_reference`` in float64 from those operands and the same stream (``R.stream_planes``: hi + lo as
``to_planes`` splits it).  The attention's own rounding is therefore no part of the figure.  No kernel is restated: the reference is torch's
Linear, LayerNorm and erf-GELU, checked against the oracle's ``earth_block`` in tests/test_pangu_reference_cpu.py.

Kernels, by mode (csrc/fused_block.hip, csrc/api.hip ``block_planes``; the term plan's bits are two_term = bit l, block_one = bit 8 + l):
  f16x3q          proj_mlp_kernel<f16, S0> (C = 192) and <f16, S1> (C = 384), three terms
  bf16x3          proj_mlp_kernel<bf16, S0> and <bf16, S1>
  f16x2m  0x06F   proj_mlp2_kernel S02 and S12, two terms
  f16x1m  0x66F   S02 two terms in layer 1, S11 ONE term in layer 2
  f16x3q-0x10F    S01: ONE term at C = 192, which no named mode reaches (``make_config`` accepts the plan; layer 2 then runs S12)
  f16x3q-split    the tiled op_proj + op_fc1 + op_fc2, what the load-time guard trusts as its reference engine
Every case asserts the plan in effect and the stage names that ``profile_read`` saw a launch under.

Grids: 24x96 (1152 = 9 x 128 fine tokens, 288 coarse: ragged at 128 and at 64), 25x96-back (1344 = 10.5 x 128: half a workgroup dead; 384 exact),
33x96 (1728 and 480: ragged at both tile sizes).  Token counts are multiples of 64 on every valid geometry and a wave holds 16 or 32 rows, so
``live[0] != live[1]`` inside one wave cannot occur; no grid is invented for it.

Bar, per case and from the reference alone (``R.block_bar``):  bar = max(B, 16 k e32) + 2 e_gelu + e_w  in the norm max|got - ref| / max|ref|,
where e32 is the float32 run of the same function against the float64 one, e_gelu the float64 run with the project's degree-8 GELU fit
(``R.gelu_poly64``) against the one with erf-GELU, B = BAR3 = 2e-6 and k = 1 for fp16 planes, B = 64 BAR3 and k = 64 for bf16 (16 significand
bits per hi / lo pair against 22).  The factor 16 is tests/test_pangu_kernels_gpu.py's.  In the two-term form the reference's weights are the
engine's one fp16 plane (nearest rounding, no calibration), so the same bar holds.  In the ONE form the operands' roundings to fp16 are in
both yardstick runs, and both e32 and e_gelu then carry whole fp16 steps of single operands that sit on a tie: the bar comes out at
5e-4 .. 3e-3 there, some hundred times the other forms' -- it is what the formula gives, and the kernels sit at 0.03 .. 0.13 of it.
e_w is the one term added to the formula, for the three-term forms only (0 otherwise), and it was justified on the CPU before it was added:
the first run of the ``eps`` edge in f16x3q exceeded max(B, 16 e32) + 2 e_gelu in layer2.block1 (6.4e-6 and 1.12e-5 against 5.3e-6 and 6.7e-6).
The same float64 reference with the proj / fc1 / fc2 weights rounded to fp16 hi + lo planes as ``prepare`` holds them (``R.weight_planes``) is
off by 6.5e-6 and 1.13e-5 on those two cases and within 3 % of the device's own error on all eight cases of that edge -- the excess IS the weight planes:
the lo plane of a weight below 2^-3 lies under 2^-14, where fp16 resolves 2^-25 whatever the value, so a weight of 0.013 (the synthetic
ones) is held to 19 bits and one of 0.001 (the scaled ones of that edge) to 15, not to 22.  That is the number format, not the row-tile
kernels; e_w is that same float64 run against ref, per case, with factor 1.  It is 0.7 .. 1.3e-6 on the plain cases -- the larger part of
the three-term kernels' 1 .. 1.6e-6 -- and the two-term kernels, whose weights are exact in the reference, sit at 3 .. 7e-7.

Edges (25x96-back and 33x96; f16x3q, f16x2m, f16x1m; ``R.edge_params``, whose claims are asserted on the CPU): zero attention output (V rows
zero; asserted on the buffer), with fc2.weight = 0 too, a projection bias constant over the channels (LayerNorm rows of variance exactly 0),
projection and fc2 scaled until eps = 1e-5 is 3 % of the median row variance (eps = 1e-6 moves the float64 result by 1e3 bars, 5 .. 15 in
the ONE form), fc1 pre-activations of mean -4 and std 4 (0.4 .. 1.1 % beyond +5.94, 31 % below -5.94, max 19 .. 22), and one token row times
1000 -- the last token and one in the middle, under the zero-attention parameters so that ``ao`` does not change: its own row is held to the
bar and every other row is bit-identical to the run without it (row isolation across the lane-quad shuffles and the dead-row guard).
Left out: bit-equality of x_mid across rows (x_mid never reaches memory in the fused kernels; the float64 statement is asserted on the CPU),
and the dead-row bullet's bit-for-bit comparison on a rearranged geometry (the stream buffers are sized in whole tokens, so a dead row's store
has nothing to land in that a read could see, and no rearrangement exists without new API).

Measured on an MI355X (all 240 cases pass; the split form's figures equal the fused three-term kernels' to two digits).
Plain cases, err / e32 / e_gelu / bar per block (layer1.block0, layer1.block1, layer2.block0, layer2.block1):
  24x96       f16x3q       1.3e-06 3.9e-07 8.0e-08 7.7e-06   9.7e-07 4.3e-07 7.7e-08 7.8e-06   1.6e-06 5.7e-07 1.1e-07 1.1e-05   1.4e-06 4.6e-07 6.2e-08 8.5e-06
  24x96       bf16x3       8.3e-06 3.8e-07 8.0e-08 3.9e-04   1.0e-05 3.8e-07 7.7e-08 3.9e-04   1.0e-05 6.0e-07 1.1e-07 6.1e-04   1.0e-05 4.4e-07 6.2e-08 4.6e-04
  24x96       f16x2m       4.2e-07 4.1e-07 8.0e-08 6.7e-06   3.6e-07 3.9e-07 7.7e-08 6.3e-06   7.1e-07 5.0e-07 1.1e-07 8.1e-06   6.2e-07 3.8e-07 6.2e-08 6.2e-06
  24x96       f16x1m       4.2e-07 4.1e-07 8.0e-08 6.7e-06   3.6e-07 3.9e-07 7.7e-08 6.3e-06   1.5e-04 1.3e-04 3.6e-05 2.1e-03   9.5e-05 8.8e-05 2.8e-05 1.5e-03
  24x96       f16x3q-0x10F 7.6e-05 1.1e-04 2.9e-05 1.9e-03   7.6e-05 8.8e-05 2.4e-05 1.5e-03   6.9e-07 5.8e-07 1.1e-07 9.5e-06   5.8e-07 4.5e-07 6.2e-08 7.3e-06
  24x96       f16x3q-split 1.3e-06 3.9e-07 8.0e-08 7.7e-06   9.7e-07 4.3e-07 7.7e-08 7.8e-06   1.6e-06 5.7e-07 1.1e-07 1.1e-05   1.4e-06 4.6e-07 6.2e-08 8.5e-06
  25x96-back  f16x3q       1.0e-06 3.3e-07 8.3e-08 6.4e-06   8.6e-07 3.7e-07 7.0e-08 6.8e-06   1.4e-06 4.4e-07 1.2e-07 8.6e-06   8.4e-07 3.2e-07 5.4e-08 5.9e-06
  25x96-back  bf16x3       8.7e-06 3.4e-07 8.3e-08 3.5e-04   8.6e-06 4.3e-07 7.0e-08 4.4e-04   9.0e-06 4.4e-07 1.2e-07 4.6e-04   9.4e-06 3.2e-07 5.4e-08 3.3e-04
  25x96-back  f16x2m       3.8e-07 3.4e-07 8.3e-08 5.5e-06   3.3e-07 4.1e-07 7.0e-08 6.7e-06   7.3e-07 4.8e-07 1.2e-07 8.0e-06   3.4e-07 3.4e-07 5.4e-08 5.6e-06
  25x96-back  f16x1m       3.8e-07 3.4e-07 8.3e-08 5.5e-06   3.3e-07 4.1e-07 7.0e-08 6.7e-06   1.3e-04 1.1e-04 2.9e-05 1.8e-03   8.4e-05 6.8e-05 1.0e-05 1.1e-03
  25x96-back  f16x3q-0x10F 1.0e-04 8.9e-05 3.0e-05 1.5e-03   8.5e-05 1.3e-04 2.2e-05 2.1e-03   5.8e-07 6.2e-07 1.2e-07 1.0e-05   3.4e-07 2.9e-07 5.4e-08 4.7e-06
  25x96-back  f16x3q-split 1.1e-06 3.3e-07 8.3e-08 6.4e-06   8.5e-07 3.7e-07 7.0e-08 6.8e-06   1.4e-06 4.4e-07 1.2e-07 8.6e-06   8.3e-07 3.2e-07 5.4e-08 5.9e-06
  33x96       f16x3q       1.2e-06 4.1e-07 8.7e-08 7.9e-06   1.1e-06 3.8e-07 7.7e-08 7.1e-06   1.5e-06 5.1e-07 9.0e-08 9.6e-06   1.3e-06 4.6e-07 6.7e-08 8.6e-06
  33x96       bf16x3       7.8e-06 4.8e-07 8.7e-08 4.9e-04   1.1e-05 3.6e-07 7.7e-08 3.7e-04   1.1e-05 4.4e-07 9.0e-08 4.6e-04   1.0e-05 4.4e-07 6.7e-08 4.6e-04
  33x96       f16x2m       5.4e-07 4.8e-07 8.7e-08 7.9e-06   4.0e-07 4.0e-07 7.7e-08 6.5e-06   7.0e-07 5.2e-07 9.0e-08 8.5e-06   6.2e-07 4.3e-07 6.7e-08 7.0e-06
  33x96       f16x1m       5.4e-07 4.8e-07 8.7e-08 7.9e-06   4.0e-07 4.0e-07 7.7e-08 6.5e-06   1.1e-04 1.5e-04 3.7e-05 2.4e-03   8.7e-05 8.8e-05 1.3e-05 1.4e-03
  33x96       f16x3q-0x10F 1.2e-04 1.6e-04 6.2e-05 2.6e-03   1.1e-04 1.0e-04 2.4e-05 1.7e-03   6.7e-07 4.6e-07 9.0e-08 7.5e-06   6.6e-07 5.4e-07 6.7e-08 8.8e-06
  33x96       f16x3q-split 1.2e-06 4.1e-07 8.7e-08 7.9e-06   1.0e-06 3.8e-07 7.7e-08 7.1e-06   1.5e-06 5.1e-07 9.0e-08 9.6e-06   1.2e-06 4.6e-07 6.7e-08 8.6e-06
Edges (both grids, four blocks): err / bar range, bar range
  zero_ao      f16x3q  three  0.138 .. 0.220   bar 4.5e-06 .. 1.1e-05
  zero_ao_fc2  f16x3q  three  0.079 .. 0.126   bar 2.0e-06 .. 2.0e-06
  zero_var     f16x3q  three  0.123 .. 0.187   bar 4.9e-06 .. 1.0e-05
  eps          f16x3q  three  0.320 .. 0.622   bar 8.3e-06 .. 1.8e-05
  gelu         f16x3q  three  0.086 .. 0.147   bar 6.9e-06 .. 1.0e-05
  zero_ao      f16x2m  two    0.069 .. 0.126   bar 3.9e-06 .. 1.0e-05
  zero_ao_fc2  f16x2m  two    0.079 .. 0.126   bar 2.0e-06 .. 2.0e-06
  zero_var     f16x2m  two    0.071 .. 0.154   bar 4.4e-06 .. 8.6e-06
  eps          f16x2m  two    0.053 .. 0.098   bar 5.2e-06 .. 8.8e-06
  gelu         f16x2m  two    0.046 .. 0.070   bar 6.4e-06 .. 1.0e-05
  zero_ao      f16x1m  two    0.069 .. 0.079   bar 4.4e-06 .. 1.0e-05
  zero_ao      f16x1m  one    0.059 .. 0.061   bar 6.7e-04 .. 2.4e-03
  zero_ao_fc2  f16x1m  two    0.079 .. 0.100   bar 2.0e-06 .. 2.0e-06
  zero_ao_fc2  f16x1m  one    0.085 .. 0.126   bar 2.0e-06 .. 2.0e-06
  zero_var     f16x1m  two    0.071 .. 0.099   bar 5.1e-06 .. 6.1e-06
  zero_var     f16x1m  one    0.025 .. 0.056   bar 4.5e-04 .. 9.0e-04
  eps          f16x1m  two    0.053 .. 0.070   bar 5.4e-06 .. 7.5e-06
  eps          f16x1m  one    0.041 .. 0.057   bar 8.7e-04 .. 2.0e-03
  gelu         f16x1m  two    0.046 .. 0.060   bar 7.8e-06 .. 9.5e-06
  gelu         f16x1m  one    0.032 .. 0.066   bar 1.7e-03 .. 2.8e-03
  big_last     f16x3q  three  0.040 .. 0.088   bar 2.0e-06 .. 2.0e-06
  big_mid      f16x3q  three  0.045 .. 0.127   bar 2.0e-06 .. 2.0e-06
  big_last     f16x2m  two    0.044 .. 0.074   bar 2.0e-06 .. 2.0e-06
  big_mid      f16x2m  two    0.053 .. 0.105   bar 2.0e-06 .. 2.0e-06
  big_last     f16x1m  two    0.044 .. 0.074   bar 2.0e-06 .. 2.0e-06
  big_last     f16x1m  one    0.053 .. 0.092   bar 2.1e-06 .. 7.1e-06
  big_mid      f16x1m  two    0.053 .. 0.105   bar 2.0e-06 .. 2.0e-06
  big_mid      f16x1m  one    0.055 .. 0.089   bar 2.1e-06 .. 7.1e-06
Every launch claimed above did run: plan and stage names asserted per case.

Do they bite?  Four scratch builds with one injected fault each (failing new cases, err / bar; then tests/test_pangu_gpu.py::test_earth_specific_block,
14 cases at 5e-4, on the same build):
  (a) the A_lo W term of fc1 removed from proj_mlp2_kernel: every two-term case that reaches fc2 fails, 72 cases at 16 .. 33 bars (plain, zero_ao,
      zero_var, eps, gelu in f16x2m, f16x1m layer 1 and 0x10F layer 2) and 2 of the 1000-times rows at 1.3; the ONE cases have no such term.  test_earth_specific_block: 14 pass.
  (b) eps = 1e-6 in the between-phase LayerNorm of both kernels: 189 cases fail; plain 11 .. 937 bars in the three- and two-term forms (bf16x3
      1 .. 16, ONE 1.4 .. 3.3), the eps edge 669 .. 2983 bars (ONE 5 .. 18), zero_ao_fc2 2156 .. 3801 bars in every form.  test_earth_specific_block:
      f16x3q fails 5 of 7 at 5.3e-4 .. 7.5e-3; the f16x1m engine is refused by the load-time guard (1.7e-2 sigma against the split form).
  (c) the GELU clamp at 4.0: only the gelu edge fails, all 20 of its three- and two-term cases at 8.8 .. 19 bars (the ONE cases pass: their bar
      is the tie flips).  test_earth_specific_block: 14 pass.
  (d) winv read one entry off in the last 16-row block: every case with a non-zero attention output fails, 108 cases at 4e3 .. 6e4 bars (bf16x3
      104 .. 889, ONE 21 .. 331); the zero-attention edges pass, as they must.  test_earth_specific_block: f16x3q fails 7 of 7 at 3.5e-3 .. 7.5e-2,
      f16x1m is refused by the guard.
"""
from __future__ import annotations

from functools import lru_cache

import pytest
import torch

import _pangu_reference as R
from oracle import pangu_oracle as O
from skyrim_amd.pangu.spec import PanguGeometry

pytestmark = pytest.mark.gpu

MODES = {"f16x3q": ("f16x3q", {}, 0), "bf16x3": ("bf16x3", {}, 0), "f16x2m": ("f16x2m", {}, 0x6F), "f16x1m": ("f16x1m", {}, 0x66F),
         "f16x3q-0x10F": ("f16x3q", dict(term_plan=0x10F), 0x10F), "f16x3q-split": ("f16x3q", dict(mlp="split"), 0)}
GRIDS = ("24x96", "25x96-back", "33x96")
EDGE_GRIDS, EDGE_MODES = ("25x96-back", "33x96"), ("f16x3q", "f16x2m", "f16x1m")
BLOCKS = R.PEAKED_BLOCKS
BIG = 1000.0


def _engine(grid, mkey):
    from skyrim_amd.pangu.engine import PanguEngine
    precision, kw, _ = MODES[mkey]
    return PanguEngine(PanguGeometry(grid.n_lat, grid.n_lon, grid.pad), precision, "cuda:0", **kw)


def _load(e, params):
    e.load_params(params, calibration="off", rounding="nearest", guard=False)       # weights: nearest fp16 of the master's; biases: the master's


def _params(grid, edge):
    return R.peaked_params(grid) if edge == "plain" else R.edge_params(grid, "zero_ao" if edge.startswith("big_") else edge)


def _input(grid, layer, i, edge):
    """The float32 tap in front of the block; ``big_last`` / ``big_mid``: its last row / a row in the middle times 1000."""
    x = R.reference(grid.n_lat, grid.n_lon, grid.pad)[0][R.BEFORE[layer, i]].float().contiguous()
    if edge.startswith("big_"):
        x = x.clone()
        x[_big_row(x.shape[0], edge)] *= BIG
    return x


def _big_row(ntok, edge):
    return ntok - 1 if edge == "big_last" else ntok // 2 + 5


def _ao_planes(e, n, bf16):
    raw = e.debug_buffer("ao", torch.uint8).view(torch.bfloat16 if bf16 else torch.float16).cpu()
    per = raw.numel() // 2
    return raw[:n].clone(), raw[per:per + n].clone()


@lru_cache(maxsize=None)
def _runs(gid, mkey):
    """Every case of one (grid, mode) on ONE engine: per parameter set one load, per block and input one ``block`` call; block output, ``ao``
    planes and launch counts on the host.  The engine is released."""
    grid = R.GRID[gid]
    edges = ("plain",) + ((*R.EDGES, "big") if gid in EDGE_GRIDS and mkey in EDGE_MODES else ())
    out = {}
    e = _engine(grid, mkey)
    try:
        for pset in edges:
            _load(e, _params(grid, "zero_ao" if pset == "big" else pset)[0])
            for layer, i in BLOCKS:
                for edge in (("big_last", "big_mid") if pset == "big" else (pset,)):
                    n = e.geom.n_windows(layer) * R.L * e.geom.dim(layer)
                    e.profile(True)
                    y = e.block(layer, i, _input(grid, layer, i, edge).cuda()).cpu()
                    launches = {s["name"]: s["launches"] for s in e.profile_read()}
                    e.profile(False)
                    out[edge, layer, i] = dict(y=y, ao=_ao_planes(e, n, mkey == "bf16x3"), launches=launches, plan=e.term_plan_in_effect, mlp=e.mlp)
    finally:
        e.release()
    return out


def _check(gid, mkey, edge, layer, i):
    """The comparison every case makes: (record, reference, input stream as float64, ``ao`` in token order, bar)."""
    grid = R.GRID[gid]
    rec = _runs(gid, mkey)[edge, layer, i]
    res = 0 if layer in (1, 4) else 1
    # the case runs the kernel it claims to: the plan, the form of the block kernels, one launch under their stage names and none under the others'
    assert rec["plan"] == MODES[mkey][2] and rec["mlp"] == MODES[mkey][1].get("mlp", "fused")
    ran = {k: rec["launches"].get(f"{k}_r{res}", 0) for k in ("proj", "proj_mlp", "fc1", "fc2")}
    assert ran == (dict(proj=1, proj_mlp=0, fc1=1, fc2=1) if rec["mlp"] == "split" else dict(proj=0, proj_mlp=1, fc1=0, fc2=0)), (mkey, rec["launches"])
    form, bf16 = R.form_of(rec["plan"], layer), mkey == "bf16x3"
    pb = O._block_params(_params(grid, edge)[1], layer, i)
    x64 = R.stream_planes(_input(grid, layer, i, edge), bf16)
    ntok, C = x64.shape
    table = R.window_table(grid, layer, i % 2 == 1, R.conventions_of(grid))
    ao = R.ao_tokens(rec["ao"], table, ntok, C, one=form == "one")
    ref, e32, e_gelu, e_w, bar = R.block_bar(pb, x64, ao, form, bf16)
    got = rec["y"]
    assert got.dtype == torch.float32 and torch.isfinite(got).all(), f"{gid} {mkey} {edge} layer{layer}.block{i}: non-finite output"
    err, flat = R.max_rel(got, ref)
    print(f"pangu block F {gid:11s} {mkey:13s} {edge:12s} layer{layer}.block{i} {form:5s}: err {err:.2e}  e32 {e32:.2e}  e_gelu {e_gelu:.2e}  e_w {e_w:.2e}  bar {bar:.2e}  err / bar {err / bar:.3f}")
    if not err <= bar:
        m, c = flat // C, flat % C
        pytest.fail(f"{gid} {mkey} {edge} layer{layer}.block{i} ({form}): err {err:.3e} above the bar {bar:.3e} (e32 {e32:.2e}, e_gelu {e_gelu:.2e}, e_w {e_w:.2e}); worst at "
                    f"{R.locate_token(grid, layer, flat, C)}: got {got[m, c].item():.8g}, expected {ref[m, c].item():.8g}; tile of 128: row {m % 128} of tile {m // 128}, "
                    f"of 64: row {m % 64} of tile {m // 64}, {ntok} tokens")
    return rec, ref, x64, ao, bar


@pytest.mark.parametrize("gid,mkey,layer,i", [(g, m, l, i) for g in GRIDS for m in MODES for l, i in BLOCKS])
def test_post_attention_against_float64(gid, mkey, layer, i):
    _check(gid, mkey, "plain", layer, i)


@pytest.mark.parametrize("gid,mkey,edge,layer,i", [(g, m, e, l, i) for g in EDGE_GRIDS for m in EDGE_MODES for e in R.EDGES for l, i in BLOCKS])
def test_post_attention_edges_against_float64(gid, mkey, edge, layer, i):
    rec, ref, x64, ao, bar = _check(gid, mkey, edge, layer, i)
    if edge in ("zero_ao", "zero_ao_fc2", "zero_var"):
        form = R.form_of(rec["plan"], layer)
        for plane in rec["ao"][:1 if form == "one" else 2]:
            assert not (plane.float() != 0).any(), f"{gid} {mkey} {edge} layer{layer}.block{i}: the attention output is not zero"
        assert not ao.bool().any()
    if edge == "eps":           # the condition on the DEVICE's attention output, as on the oracle's in the CPU test
        pb = O._block_params(R.edge_params(R.GRID[gid], edge)[1], layer, i)
        r = R.post_attention_reference(pb, x64, ao, R.form_of(rec["plan"], layer), parts=True)
        assert all(1e-4 <= r[k].var(-1, unbiased=False).median().item() <= 1e-2 for k in ("proj", "fc2"))


@pytest.mark.parametrize("gid,mkey,edge,layer,i", [(g, m, e, l, i) for g in EDGE_GRIDS for m in EDGE_MODES for e in ("big_last", "big_mid") for l, i in BLOCKS])
def test_one_token_row_times_1000_stays_in_its_row(gid, mkey, edge, layer, i):
    rec, ref, x64, ao, bar = _check(gid, mkey, edge, layer, i)        # the whole tensor in the norm of its largest row
    plain = _runs(gid, mkey)["zero_ao", layer, i]
    assert all(torch.equal(a, b) for a, b in zip(rec["ao"], plain["ao"]))
    r = _big_row(x64.shape[0], edge)
    assert x64[r].abs().max() < 65504 and x64[r].abs().max() > 100 * x64[r - 1].abs().max()
    others = torch.arange(x64.shape[0]) != r
    same = (rec["y"][others].view(torch.int32) == plain["y"][others].view(torch.int32)).all(1)
    assert same.all(), (f"{gid} {mkey} layer{layer}.block{i}: row {r} times {BIG:g} changed {int((~same).sum())} other rows, the first is row "
                        f"{int(torch.nonzero(others)[~same][0])}")
    own = ((rec["y"][r].double() - ref[r]).abs().max() / ref[r].abs().max()).item()
    assert own <= bar, f"{gid} {mkey} layer{layer}.block{i}: row {r} itself is off by {own:.3e}, bar {bar:.3e}"
