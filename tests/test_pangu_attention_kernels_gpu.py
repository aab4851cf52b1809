"""Pangu's attention tables and attention core, operand by operand, on parameters that make the softmax PEAKED.

What is compared (all through ``PanguEngine.debug_buffer``; no kernel is restated, the references are tests/_pangu_reference.py on the oracle's
own functions, checked on the CPU in tests/test_pangu_reference_cpu.py):
  A  the window gather tables ``widx{r}{roll}`` (csrc/aux.hip prep_window_index)                               -- exactly
  B  the compact earth-specific bias with the shifted-window mask folded in, ``bias_exp{b}`` (prep_bias_compact)   -- exactly, as fp16
  C  Q, K and V^T of the two-launch form (csrc/rowtile.hip rt_qkv_kernel) against float64 on the same float32 stream
  D  the attention core (csrc/attention.hip earth_attention2_kernel) against float64 softmax attention of the DEVICE's OWN fp16 q, k, vt
     and bias table, so that the roundings of C are not part of its figure
  E  the fused kernel (qkv_attention_kernel: queries walked in key order, its own LDS staging of the bias) bit for bit against D's engine.

Why peaked (``R.peaked_params``: bias table x 100, Q rows x gain): on ``init_synthetic`` parameters every attention weight is 1 / 144 to within a
few per cent, a bias entry that is misplaced, one column off or missing its mask moves a weight by 2 %, and the block's 5e-4 bar hides that.
Here the bias has std 1.77 (within +-4), the q . k logits std 1.5 (layer1.block0) or 5.0 (the other three), the median row spreads its weight
over 9 .. 22 keys and 1.6 .. 12 % of the rows put more than half of it on one key.

Grids (``R.GRIDS`` plus two):
  24x96        no latitude padding; layers 1 / 4 have ONE latitude window, which is the first and the last window type at once
  25 / 26 / 27x96, 27x192, 26x96-back, 25x96-back   (A only) window paddings 5 / 2 rows on top or all at the end, two coarse longitude windows
  33x96        latitude windows 2 (fine) / 1 (coarse), window paddings 3 and 1
  49x96        latitude windows 3 / 2: a window type that is neither first nor last; 12 fine window types, so the fused kernel's XCD map
               walks 8 + 4 and takes its ``type >= types`` exit
  25x96-back   (C, D) all padding at the end: five of the last fine window's six latitude rows are padding, whose Q / K / V are the biases alone
  25x864       18 fine / 9 coarse longitude windows per type: a wave walks several windows

Bars.  C, elementwise:  |got - ref| <= 2^-11 ((1 + onep) s sum_k |x_k| |w_k| + |ref|),  s = 32^-0.5 for Q and 1 otherwise, onep = 1 where the
term plan's QKV bit makes the weights one fp16 plane: the stream's hi plane is an 11-bit operand, one-plane weights are another, the result is
rounded to fp16 once.  Where |ref| < 2^-14 the bar has 2^-25 added: fp16 is subnormal there and NO store reaches 2^-11 |ref| (on the padding rows,
whose Q / K / V are the biases alone, the sum is 0 and the correctly rounded float64 value itself sits at up to 1.2 of the bar without it).
D, elementwise:  |got - o| <= 2 (2^-11 D + r |o| + 144 2^-25 max|v|),  D = sum_k p_k |v_kd - o_qd|, r = 2^-11 for one
output plane and 2^-21 for two: every weight is rounded to fp16 and the SAME rounded weights are summed for the normalisation (the kernel's row
of ones), weights in fp16's subnormal range carry an absolute error, and the factor 2 covers the fp32 accumulation of the scores, v_exp_f32
and v_rcp_f32.  Both bars are computed from the reference alone and carry no extra margin.

Measured on an MI355X: largest err / bar per case, columns layer1.block0, layer1.block1, layer2.block0, layer2.block1.  A, B and E hold exactly.
On the padding rows of C the sum is 0 and the bar is the final fp16 rounding alone, so the figure there is how close to a tie the worst bias lies.
C, rows that hold a stream token: q k vt (in f16x1m layer 2 runs one-plane weights, onep = 1); last column: the largest figure on padding rows
  24x96       f16x3q  0.324 0.291 0.353   0.285 0.317 0.311   0.212 0.225 0.208   0.219 0.209 0.197   | 0.971
  24x96       f16x1m  0.324 0.291 0.353   0.285 0.317 0.311   0.133 0.126 0.115   0.146 0.129 0.122   | 0.971
  33x96       f16x3q  0.321 0.383 0.298   0.316 0.317 0.314   0.232 0.254 0.226   0.217 0.241 0.232   | 0.985
  33x96       f16x1m  0.321 0.383 0.298   0.316 0.317 0.314   0.145 0.142 0.127   0.135 0.144 0.146   | 0.985
  49x96       f16x3q  0.331 0.330 0.317   0.333 0.335 0.332   0.214 0.239 0.242   0.226 0.235 0.223   | 0.989
  49x96       f16x1m  0.331 0.330 0.317   0.333 0.335 0.332   0.135 0.149 0.153   0.159 0.135 0.145   | 0.989
  25x96-back  f16x3q  0.352 0.317 0.331   0.291 0.324 0.304   0.256 0.264 0.242   0.231 0.205 0.218   | 0.974
  25x96-back  f16x1m  0.352 0.317 0.331   0.291 0.324 0.304   0.139 0.147 0.142   0.151 0.138 0.150   | 0.974
  25x864      f16x3q  0.377 0.364 0.357   0.309 0.344 0.343   0.252 0.252 0.254   0.260 0.232 0.222   | 0.972
  25x864      f16x1m  0.377 0.364 0.357   0.309 0.344 0.343   0.177 0.155 0.153   0.172 0.140 0.149   | 0.972
D (in f16x1m layer 2 writes ONE output plane, r = 2^-11)
  24x96       f16x3q  0.258   0.217   0.214   0.200
  24x96       f16x1m  0.258   0.217   0.467   0.459
  33x96       f16x3q  0.302   0.260   0.222   0.197
  33x96       f16x1m  0.302   0.260   0.464   0.477
  49x96       f16x3q  0.282   0.221   0.255   0.180
  49x96       f16x1m  0.282   0.221   0.473   0.478
  25x96-back  f16x3q  0.296   0.234   0.186   0.176
  25x96-back  f16x1m  0.296   0.234   0.453   0.479
  25x864      f16x3q  0.356   0.270   0.270   0.217
  25x864      f16x1m  0.356   0.270   0.476   0.474
Do they bite?  Three scratch builds with one placement error each, on the same tests: reading bias column 21 - e instead of 22 - e for e in
4 .. 7 fails B in 13823 .. 41470 cells per block, dropping the latitude term of the shifted-window mask fails B in 34776 cells of every rolled
block, and key offsets shifted by four entries (one aligned 8-byte read) in earth_attention2_kernel fail D at 4.5e3 .. 1.8e4 bars in layer 1 and
with non-finite rows in layer 2.  tests/test_pangu_gpu.py::test_earth_specific_block on those builds: the column error fails 5 of its 14
cases at 7.1e-4 .. 1.1e-3 against 5e-4 and passes the other 9; the missing mask term fails the 8 rolled cases at 0.04 .. 0.17.
"""
from __future__ import annotations

from functools import lru_cache

import pytest
import torch

import _pangu_reference as R
from oracle import pangu_oracle as O
from skyrim_amd.pangu.calibration import _unblock
from skyrim_amd.pangu.engine import DEFAULT_PRECISION
from skyrim_amd.pangu.spec import PanguGeometry

pytestmark = pytest.mark.gpu

GRID = {g.id: g for g in (*R.GRIDS, R.make_grid(49, 96), R.make_grid(25, 864))}
MODES = ("f16x3q", DEFAULT_PRECISION)
BLOCKS = R.PEAKED_BLOCKS
DEPTHS = O.DEPTHS
EPS1, EPS2 = 2.0 ** -11, 2.0 ** -21        # rounding to one fp16 plane; to hi + lo planes
SUBNORMAL = 2.0 ** -25                     # rounding to fp16 below 2^-14, where its spacing is 2^-24 whatever the value


def _engine(grid, mode, params, **conv):
    from skyrim_amd.pangu.engine import PanguEngine
    e = PanguEngine(PanguGeometry(grid.n_lat, grid.n_lon, grid.pad), mode, "cuda:0", **conv)
    e.load_params(params, calibration="off", rounding="nearest", guard=False)       # weights: nearest fp16 of the master's; biases: the master's
    return e


# ---- A: window tables ---------------------------------------------------------------------------------------------------------------- #
A_CASES = [(gid, {}) for gid in GRID if gid != "25x864"]
A_CASES += [(gid, conv) for gid in ("25x96", "33x96") for conv in (dict(roll_sign=+1), dict(surface="last"), dict(roll_sign=+1, surface="last"))]


@pytest.mark.parametrize("gid,conv", A_CASES, ids=lambda v: v if isinstance(v, str) else "-".join(f"{k}={x}" for k, x in v.items()) or "default")
def test_window_tables_are_exact(gid, conv):
    grid = GRID[gid]
    oc = R.conventions_of(grid, **conv)
    e = _engine(grid, "f16x3q", R.inputs(grid.n_lat, grid.n_lon)[0], **conv)
    try:
        got = {(r, roll): e.debug_buffer(f"widx{r}{roll}", torch.int32).cpu() for r in (0, 1) for roll in (0, 1)}
    finally:
        e.release()
    for (r, roll), t in got.items():
        want = R.window_table(grid, r + 1, bool(roll), oc).int()
        assert t.shape == want.shape, (gid, r, roll, t.shape, want.shape)
        if not torch.equal(t, want):
            m = int(torch.nonzero(t != want)[0])
            _, nH, nW = R.window_shape(grid, r + 1, oc)
            pytest.fail(f"{gid} {conv} widx{r}{roll}: {int((t != want).sum())} rows differ, the first is row {m} = (window type, w-window, z, h, w) = "
                        f"{R.locate_window_row(m, nH, nW)}: got {int(t[m])}, expected {int(want[m])}")


# ---- B: compact bias ------------------------------------------------------------------------------------------------------------------ #
B_CONVS = ({}, dict(roll_sign=+1), dict(bias_index="kq"), dict(roll_sign=+1, bias_index="kq", mask_value=-1000.0))


@pytest.mark.parametrize("conv", B_CONVS, ids=lambda v: "-".join(f"{k}={x}" for k, x in v.items()) or "default")
@pytest.mark.parametrize("gid", ["24x96", "33x96", "49x96"])
def test_compact_bias_is_exact(gid, conv):
    grid = GRID[gid]
    oc = R.conventions_of(grid, **conv)
    params = R.peaked_params(grid)[0]               # the tables do not depend on the conventions the engine is built with
    e = _engine(grid, "f16x3q", params, **conv)
    try:
        got = [e.debug_buffer(f"bias_exp{b}", torch.float16).cpu() for b in range(sum(DEPTHS))]
    finally:
        e.release()
    b = 0
    for layer in (1, 2, 3, 4):
        heads = O.HEADS[layer - 1]
        nZ, nH, _ = R.window_shape(grid, layer, oc)
        for i in range(DEPTHS[layer - 1]):
            want, unaddressed, conflicts = R.compact_bias(params[f"layer{layer}.block{i}.attn.bias_table"], nZ * nH, heads, nZ, nH, i % 2 == 1, oc)
            assert (unaddressed, conflicts) == (0, 0)
            want = want.half().reshape(-1)           # float32 table + float32 mask, rounded to nearest once: as the kernel does
            assert got[b].shape == want.shape, (gid, b, got[b].shape, want.shape)
            if not torch.equal(got[b], want):
                bad = torch.nonzero(got[b] != want).flatten()
                m = int(bad[0])
                pytest.fail(f"{gid} {conv} block {b} (layer{layer}.block{i}): {bad.numel()} cells differ, the first at {R.locate_bias_cell(m, heads)}: "
                            f"got {got[b][m].item()}, expected {want[m].item()}")
            b += 1


# ---- C - E: one run per (grid, mode), shared ------------------------------------------------------------------------------------------ #
CD_GRIDS = ("24x96", "33x96", "49x96", "25x96-back", "25x864")
E_GRIDS = ("24x96", "49x96", "25x864")


def _ao_planes(e, n):
    raw = e.debug_buffer("ao", torch.uint8).view(torch.float16).cpu()
    per = raw.numel() // 2
    return raw[:n].clone(), raw[per:per + n].clone()


@lru_cache(maxsize=None)
def _runs(gid, mode):
    """The four blocks on their own input taps with the peaked parameters: the two-launch engine's q, k, vt, bias table, ao planes and block
    output, and on E's grids the fused engine's ao planes, block output and launch counts.  Everything on the host; the engines are released."""
    grid = GRID[gid]
    params = R.peaked_params(grid)[0]
    taps, _ = R.reference(grid.n_lat, grid.n_lon, grid.pad)
    out = {}
    for split in (True, False) if gid in E_GRIDS else (True,):
        with pytest.MonkeyPatch.context() as mp:
            if split:
                mp.setenv("SKP_SPLIT_ATTN", "1")
            else:
                mp.delenv("SKP_SPLIT_ATTN", raising=False)
            e = _engine(grid, mode, params)
        try:
            plan = e.term_plan_in_effect
            for b, (layer, i) in enumerate(BLOCKS):
                xin = taps[R.BEFORE[layer, i]].float().contiguous()
                n = e.geom.n_windows(layer) * R.L * e.geom.dim(layer)
                e.profile(True)
                y = e.block(layer, i, xin.cuda()).cpu()
                launches = {s["name"]: s["launches"] for s in e.profile_read()}
                e.profile(False)
                rec = dict(y=y, ao=_ao_planes(e, n), launches=launches, plan=plan)
                if split:
                    rec.update({name: e.debug_buffer(name, torch.float16)[:n].cpu() for name in ("q", "k", "vt")})
                    rec["bias"] = e.debug_buffer(f"bias_exp{b}", torch.float16).cpu()
                out[split, layer, i] = rec
        finally:
            e.release()
    return out


def _case(gid, mode, layer, i):
    grid = GRID[gid]
    conv = R.conventions_of(grid)
    rec = _runs(gid, mode)[True, layer, i]
    res = 0 if layer in (1, 4) else 1
    assert rec["launches"][f"qkv_r{res}"] == 1 and rec["launches"][f"attn_r{res}"] == 1          # the two launches did run
    nZ, nH, nW = R.window_shape(grid, layer, conv)
    return grid, conv, rec, O.HEADS[layer - 1], nZ, nH, nW


CASES = pytest.mark.parametrize("gid,mode,layer,i", [(g, m, l, i) for g in CD_GRIDS for m in MODES for l, i in BLOCKS])


@CASES
def test_qkv_against_float64(gid, mode, layer, i):
    grid, conv, rec, heads, nZ, nH, nW = _case(gid, mode, layer, i)
    taps, _ = R.reference(grid.n_lat, grid.n_lon, grid.pad)
    pb = O._block_params(R.peaked_params(grid)[1], layer, i)
    table = R.window_table(grid, layer, i % 2 == 1, conv)
    ref = R.qkv_reference(pb, taps[R.BEFORE[layer, i]].float(), table, heads, conv)
    onep = (rec["plan"] >> (4 + layer - 1)) & 1
    real = (table >= 0).reshape(-1, 1, R.L, 1)                  # window rows that hold a stream token; the others are the bias alone
    worst, pads, fails = {}, {}, []
    for name in ("q", "k", "vt"):
        want, mag = ref[name]
        got = rec[name].double().reshape(want.shape)
        s = R.HEAD_DIM ** -0.5 if name == "q" else 1.0
        bar = EPS1 * ((1 + onep) * s * mag + want.abs()) + SUBNORMAL * (want.abs() < 2.0 ** -14)
        err = (got - want).abs()
        assert torch.isfinite(got).all(), (gid, mode, layer, i, name)
        ratio = err / bar
        rows = real.transpose(-1, -2) if name == "vt" else real
        worst[name] = (ratio * rows).max().item()
        pads[name] = (ratio * ~rows).max().item()
        if max(worst[name], pads[name]) > 1:
            w, h, a, c = (int(v) for v in torch.unravel_index(ratio.argmax(), ratio.shape))
            t, d = (c, a) if name == "vt" else (a, c)
            fails.append(f"{name}: err / bar {ratio.max().item():.3f} at window type {w // nW}, w-window {w % nW}, head {h}, token {t} -> (z, h, w) = ({t // 72}, {t // 12 % 6}, {t % 12}), "
                         f"dim {d}: got {got[w, h, a, c].item():.6g}, expected {want[w, h, a, c].item():.6g}; {int((ratio > 1).sum())} elements above the bar")
    print(f"pangu attention C {gid:11s} {mode} layer{layer}.block{i} onep {onep}: err / bar  q {worst['q']:.3f}  k {worst['k']:.3f}  vt {worst['vt']:.3f}"
          f"   padding rows  q {pads['q']:.3f}  k {pads['k']:.3f}  vt {pads['vt']:.3f}")
    assert not fails, f"{gid} {mode} layer{layer}.block{i}: " + "; ".join(fails)


def _ao(rec, layer, mwin, C):
    """(attention output [window rows][C] as float64, 1 where the layer's block kernels read ONE plane of it: the lo half is then stale)."""
    one = (rec["plan"] >> (8 + layer - 1)) & 1
    hi, lo = rec["ao"]
    flat = hi.double() if one else hi.double() + lo.double()
    return _unblock(flat, mwin, C), one


@CASES
def test_attention_core_against_float64_on_the_devices_operands(gid, mode, layer, i):
    grid, conv, rec, heads, nZ, nH, nW = _case(gid, mode, layer, i)
    C = heads * R.HEAD_DIM
    mwin = nZ * nH * nW * R.L
    got, one = _ao(rec, layer, mwin, C)
    assert torch.isfinite(got).all(), f"{gid} {mode} layer{layer}.block{i}: non-finite attention rows (padding rows included)"
    o, p, D = R.attention_reference(rec["q"], rec["k"], rec["vt"], rec["bias"], nZ * nH, heads, nW)
    r = EPS1 if one else EPS2
    vmax = rec["vt"].double().abs().max().item()
    bar = 2 * (EPS1 * D + r * o.abs() + R.L * 2.0 ** -25 * vmax)
    err = (got - o).abs()
    ratio = err / bar
    worst = ratio.max().item()
    print(f"pangu attention D {gid:11s} {mode} layer{layer}.block{i} planes {1 if one else 2}: err / bar {worst:.3f}  (max|err| {err.max().item():.2e}, max|o| {o.abs().max().item():.2e})")
    if worst > 1:
        m, c = (int(v) for v in torch.unravel_index(ratio.argmax(), ratio.shape))
        # the part of D that weights below 2^-14 carry: what flushing fp16 subnormals in the P operand would cost (a quantity of the reference)
        v = rec["vt"].double().reshape(-1, heads, R.HEAD_DIM, R.L)[m // R.L, c // R.HEAD_DIM, c % R.HEAD_DIM]
        pr = p[m // R.L, c // R.HEAD_DIM, m % R.L]
        small = (pr * (pr < 2.0 ** -14) * (v - o[m, c]).abs()).sum().item()
        pytest.fail(f"{gid} {mode} layer{layer}.block{i}: err / bar {worst:.3f} at {R.locate_attention_row(m, c, nW)}: got {got[m, c].item():.6g}, expected {o[m, c].item():.6g}, "
                    f"bar {bar[m, c].item():.3g} (D {D[m, c].item():.3g}); {int((ratio > 1).sum())} elements above the bar; weight mass below 2^-14 of this row: "
                    f"sum p |v - o| = {small:.3g}, largest weight {pr.max().item():.4f}")


@pytest.mark.parametrize("gid,mode,layer,i", [(g, m, l, i) for g in E_GRIDS for m in MODES for l, i in BLOCKS])
def test_fused_attention_with_a_peaked_softmax_is_bit_identical_to_the_two_launches(gid, mode, layer, i):
    runs = _runs(gid, mode)
    two, fused = runs[True, layer, i], runs[False, layer, i]
    res = 0 if layer in (1, 4) else 1
    assert two["launches"][f"qkv_r{res}"] == 1 and two["launches"][f"attn_r{res}"] == 1
    assert fused["launches"][f"attn_r{res}"] == 1
    ran = fused["launches"][f"qkv_r{res}"] == 0
    assert ran == (mode != "f16x3q" or layer == 1), (mode, layer, fused["launches"])       # fine layers in f16x3q, all four blocks in the default mode
    if not ran:
        pytest.skip(f"{mode} runs layer {layer} as the two launches: the same kernels as the other engine")
    one = (fused["plan"] >> (8 + layer - 1)) & 1
    assert fused["plan"] == two["plan"]
    assert torch.equal(fused["ao"][0], two["ao"][0]), f"{gid} {mode} layer{layer}.block{i}: hi plane of the attention output differs"
    if not one:
        assert torch.equal(fused["ao"][1], two["ao"][1]), f"{gid} {mode} layer{layer}.block{i}: lo plane of the attention output differs"
    assert torch.isfinite(fused["y"]).all() and torch.equal(fused["y"], two["y"])
