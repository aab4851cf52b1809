"""Pangu's stages outside the blocks (PatchEmbedding, DownSample, UpSample, PatchRecovery: csrc/ops_embed_recover.hip, csrc/ops_updown.hip,
merge_stats in csrc/aux.hip, the loaders and epilogues of loaders.h / epilogues.h) against the FLOAT64 oracle, on small grids whose latitude
paddings no other test runs (tests/_pangu_reference.py GRIDS: input padding 0 / 1 / 2 / 3 rows, "centre" and "back"; window paddings
0 / 1 / 3 rows), plus blocks and conventions at those window paddings.

Stage bar.  These stages run three-term fp16 hi/lo GEMMs with fp32 accumulation in every f16 mode, the arithmetic the project holds to
BAR3 = 2e-6 elsewhere (tests/test_fuxi_kernels_gpu.py).  Each stage gets the SAME float32 input on both sides (the float32 rounding of the
float64 tap in front of it), so the figure is the stage's own.  The yardstick is e32: the distance of the float32 oracle stage function
from the float64 one on that input, in the same norm -- it involves the reference alone.  bar = max(BAR3, 16 e32): operands carry 22
significand bits where float32 carries 24 (4x), two operands are split (2x), the result is split into planes again on its way out (2x).
Norms: max|err| / max|ref| for the three token stages; per channel max|err| / sigma_c (O.per_channel_sigma_err) for recovery, each channel
against its own bar.

Measured on an MI355X (mode f16x3q; err / e32 / bar; every token stage is below BAR3 itself, the bars come out at 6e-6 .. 1.4e-5 because
float32's own distance e32 is 4e-7 .. 9e-7; recovery in sigma units, each channel against its own bar -- the channels with the largest
error, 3.7 .. 4.6e-6, are geopotential / msl ones whose e32 is as large: the float32 rounding of mean + sigma y at 1e5 .. 2e5):
grid         embed  err / e32 / bar          down  err / e32 / bar           up  err / e32 / bar           recover (channel nearest its bar)  err / e32 / bar   max over channels
24x96        1.13e-06 / 3.94e-07 / 6.30e-06   1.47e-06 / 4.63e-07 / 7.40e-06   1.49e-06 / 7.67e-07 / 1.23e-05   c24  2.09e-06 / 9.28e-07 / 1.48e-05   4.39e-06
25x96        1.08e-06 / 4.13e-07 / 6.61e-06   1.15e-06 / 4.07e-07 / 6.51e-06   1.41e-06 / 7.70e-07 / 1.23e-05   c66  2.52e-06 / 9.47e-07 / 1.52e-05   3.81e-06
26x96        1.06e-06 / 3.91e-07 / 6.26e-06   1.42e-06 / 5.29e-07 / 8.46e-06   1.69e-06 / 7.44e-07 / 1.19e-05   c0   1.97e-06 / 8.04e-07 / 1.29e-05   4.17e-06
27x96        9.78e-07 / 3.99e-07 / 6.39e-06   1.33e-06 / 4.80e-07 / 7.67e-06   1.72e-06 / 8.73e-07 / 1.40e-05   c49  2.00e-06 / 9.59e-07 / 1.53e-05   4.50e-06
33x96        1.13e-06 / 4.32e-07 / 6.91e-06   1.21e-06 / 5.14e-07 / 8.22e-06   1.69e-06 / 7.96e-07 / 1.27e-05   c62  2.78e-06 / 1.32e-06 / 2.12e-05   4.56e-06
27x192       9.54e-07 / 5.20e-07 / 8.31e-06   1.45e-06 / 5.65e-07 / 9.03e-06   1.79e-06 / 8.86e-07 / 1.42e-05   c16  2.08e-06 / 9.38e-07 / 1.50e-05   4.03e-06
26x96-back   9.03e-07 / 5.00e-07 / 7.99e-06   1.46e-06 / 4.95e-07 / 7.91e-06   1.73e-06 / 8.33e-07 / 1.33e-05   c40  2.58e-06 / 1.05e-06 / 1.69e-05   4.47e-06
25x96-back   8.41e-07 / 3.96e-07 / 6.34e-06   1.37e-06 / 5.87e-07 / 9.40e-06   1.27e-06 / 7.14e-07 / 1.14e-05   c64  2.01e-06 / 8.32e-07 / 1.33e-05   3.71e-06
DownSample edge inputs on 25x96: zero stream 1.43e-06 / 2.41e-07 / 3.86e-06, constant rows 1.16e-06 / 5.72e-07 / 9.15e-06, one row 1000x
1.09e-06 / 3.68e-07 / 5.89e-06; stream x 0.05 (eps carries weight): down 1.24e-06 / 4.27e-07 / 6.84e-06, up 1.48e-06 / 6.89e-07 / 1.10e-05
(with eps = 1e-6 in the kernels, on a scratch build: 8.4e-4 and 5.8e-4, while the plain taps still pass at 2.3e-6 and 1.9e-6).  Recovery with skip = 0 / x4 = 0 on 27x96: 1.42e-06 / 5.66e-07 / 9.06e-06 (c43), 1.29e-06 / 5.11e-07 / 8.18e-06 (c60).
Blocks (max|err| / max|ref| against float64, bar 5e-4): 24x96 2.1e-5, 2.8e-5, 4.0e-5, 7.2e-5; 33x96 3.0e-5, 5.1e-5, 2.8e-5, 5.2e-5;
roll_sign = +1 on 24x96: 2.8e-5, 8.2e-5.
"""
from __future__ import annotations

import pytest
import torch
import torch.nn.functional as F

import _pangu_reference as R
from oracle import pangu_oracle as O
from skyrim_amd import ops
from skyrim_amd.pangu.spec import PanguGeometry

pytestmark = pytest.mark.gpu

BAR3 = 2e-6             # tests/test_fuxi_kernels_gpu.py BAR3: 3-term fp16 hi/lo products, fp32 accumulation, max|err| / max|ref|
BLOCK_TOL = 5e-4        # tests/test_pangu_gpu.py STAGE_TOL["f16x3q"]: one block (single-term fp16 attention inside), max|err| / max|ref|
MODE = "f16x3q"         # no term plan: load_params fits nothing; the stage kernels are the same instantiations in every f16 mode


def _engine(grid, **conv):
    from skyrim_amd.pangu.engine import PanguEngine
    e = PanguEngine(PanguGeometry(grid.n_lat, grid.n_lon, grid.pad), MODE, "cuda:0", **conv)
    e.load_params(R.inputs(grid.n_lat, grid.n_lon)[0])
    return e


@pytest.fixture(scope="module")
def rig(request):
    """(grid, engine, float32 params, float64 params, state, float64 taps, float64 output) -- one engine per geometry for the module;
    the grid comes from the test's (indirect) parameter list."""
    grid = request.param
    params, p64, x = R.inputs(grid.n_lat, grid.n_lon)
    taps, y = R.reference(grid.n_lat, grid.n_lon, grid.pad)
    e = _engine(grid)
    yield grid, e, params, p64, x, taps, y
    e.release()


def _run(e, name, xs):
    return getattr(e, {"embed": "patch_embed", "down": "downsample", "up": "upsample", "recover": "patch_recover"}[name])(*[t.cuda() for t in xs])


def on_grids(*ids):
    return pytest.mark.parametrize("rig", [R.GRID[i] for i in ids], indirect=True, ids=list(ids))


EVERY_GRID = on_grids(*R.GRID)


def check_stage(e, grid, params, p64, name, xs, label=""):
    """One stage on the float32 inputs ``xs`` against the float64 stage function on the same tensors; returns (got, ref)."""
    got = _run(e, name, xs).cpu()
    ref = R.stage(name, p64, grid, *xs)
    f32 = R.stage(name, params, grid, *xs)
    assert got.shape == ref.shape and torch.isfinite(got).all()
    if name == "recover":
        err, where = R.sigma_err(got, ref, params["norm.std"])
        e32, _ = R.sigma_err(f32, ref, params["norm.std"])
        bar = torch.clamp(16 * e32, min=BAR3)
        c = int((err / bar).argmax())
        print(f"pangu stage {grid.id} {name}{label}: err {err.max().item():.2e} sigma, e32 {e32.max().item():.2e}, bar {bar.min().item():.2e} .. {bar.max().item():.2e}; "
              f"closest channel {c}: err {err[c].item():.2e}, e32 {e32[c].item():.2e}, bar {bar[c].item():.2e}")
        assert (err <= bar).all(), (f"{grid.id} {name}{label}: channels {torch.nonzero(err > bar).flatten().tolist()} above their bars; channel {c}: "
                                    f"{err[c].item():.3e} > {bar[c].item():.3e} (e32 {e32[c].item():.3e}); worst element {R.locate(name, grid, where)}")
    else:
        err, where = R.max_rel(got, ref)
        e32, _ = R.max_rel(f32, ref)
        bar = max(BAR3, 16 * e32)
        print(f"pangu stage {grid.id} {name}{label}: err {err:.2e}, e32 {e32:.2e}, bar {bar:.2e}")
        assert err <= bar, f"{grid.id} {name}{label}: {err:.3e} > {bar:.3e} (e32 {e32:.3e}); worst element {R.locate(name, grid, where)}"
    return got, ref


@EVERY_GRID
@pytest.mark.parametrize("name", R.STAGES)
def test_stage_against_float64(rig, name):
    grid, e, params, p64, x, taps, y = rig
    check_stage(e, grid, params, p64, name, R.stage_inputs(taps, x)[name])


@EVERY_GRID
def test_stages_write_every_element(rig):
    """The ops called directly on NaN-filled outputs: every element is written (``step`` hands PatchRecovery an uninitialised state), and the
    result is bit-identical to the engine's stage methods; one whole step into a NaN-filled state likewise."""
    grid, e, params, p64, x, taps, y = rig
    xs = {k: [t.cuda() for t in v] for k, v in R.stage_inputs(taps, x).items()}
    shapes = {"embed": e.tokens(1), "down": e.tokens(2), "up": e.tokens(1), "recover": e.state_shape}
    op = {"embed": ops.hip.pangu_patch_embed, "down": ops.hip.pangu_downsample, "up": ops.hip.pangu_upsample, "recover": ops.hip.pangu_patch_recover}
    for name in R.STAGES:
        out = torch.full(shapes[name], float("nan"), dtype=torch.float32, device="cuda:0")
        op[name](e._ctx.value, *xs[name], out)
        bad = torch.nonzero(~torch.isfinite(out).flatten()).flatten()
        assert bad.numel() == 0, f"{grid.id} {name}: {bad.numel()} elements unwritten, the first at {R.locate(name, grid, int(bad[0]))}"
        assert torch.equal(out, _run(e, name, xs[name])), (grid.id, name)
    out = torch.full(e.state_shape, float("nan"), dtype=torch.float32, device="cuda:0")
    e.step(xs["embed"][0], out)
    assert torch.isfinite(out).all() and torch.equal(out, e.step(xs["embed"][0]))


# ---- DownSample's LayerNorm at its edges: 25 x 96, whose last merged row is half zero padding ---------------------------------------- #
@on_grids("25x96")
def test_downsample_of_a_zero_stream_is_the_bias_through_the_linear(rig):
    grid, e, params, p64 = rig[:4]
    x1 = torch.zeros(grid.tokens[0], 192)
    got, ref = check_stage(e, grid, params, p64, "down", (x1,), " zero stream")
    want = F.linear(p64["down.norm.bias"], p64["down.linear.weight"])           # LayerNorm of a zero row is its bias
    assert torch.allclose(ref, want.expand_as(ref), rtol=0, atol=1e-14)
    assert torch.equal(got, got[:1].expand_as(got))                              # padded and unpadded rows alike


@on_grids("25x96")
def test_downsample_of_rows_constant_across_channels(rig):
    """Each token row one constant: a merged row is four plateaus (two of them zero in the padded row), its variance entirely between them."""
    grid, e, params, p64 = rig[:4]
    gen = torch.Generator().manual_seed(11)
    x1 = torch.randn(grid.tokens[0], 1, generator=gen).expand(-1, 192).contiguous()
    check_stage(e, grid, params, p64, "down", (x1,), " constant rows")


@on_grids("25x96")
def test_downsample_with_one_token_row_1000x_the_others(rig):
    """One token of the half-padded merged row is 1000x the rest: its own row is still held to the bar, and no other row moves by a bit."""
    grid, e, params, p64 = rig[:4]
    gen = torch.Generator().manual_seed(12)
    base = torch.randn(grid.tokens[0], 192, generator=gen)
    Z, H1, W1, H2, W2 = 8, grid.H1, grid.n_lon // 4, grid.H2, grid.n_lon // 8
    z, h, w = 3, H1 - 1, 5
    big = base.clone()
    big[(z * H1 + h) * W1 + w] *= 1000.0
    got, _ = check_stage(e, grid, params, p64, "down", (big,), " 1000x row")
    plain = e.downsample(base.cuda()).cpu()
    row = (z * H2 + h // 2) * W2 + w // 2
    others = torch.arange(grid.tokens[1]) != row
    assert torch.equal(got[others], plain[others]) and not torch.equal(got[row], plain[row])


@on_grids("25x96")
@pytest.mark.parametrize("name", ["down", "up"])
def test_layernorm_epsilon_on_a_small_stream(rig, name):
    """The stream scaled by 0.05: the LayerNorm rows have a variance of 1e-3 .. 1e-2, so eps = 1e-5 carries weight -- ten times less of it moves
    the float64 result by 6 .. 8e-4 (tests/test_pangu_reference_cpu.py), some fifty bars; on the taps as they are it moves it by 2e-6 and hides."""
    grid, e, params, p64, x, taps, y = rig
    check_stage(e, grid, params, p64, name, R.small_stream_inputs(taps)[name], " small stream")


# ---- PatchRecovery reads concat(skip, x4) in that order ------------------------------------------------------------------------------ #
@on_grids("27x96")
@pytest.mark.parametrize("zero", ["skip", "x4"])
def test_recovery_channel_placement(rig, zero):
    grid, e, params, p64, x, taps, y = rig
    skip, x4 = R.stage_inputs(taps, x)["recover"]
    skip, x4 = (torch.zeros_like(skip), x4) if zero == "skip" else (skip, torch.zeros_like(x4))
    check_stage(e, grid, params, p64, "recover", (skip, x4), f" {zero} = 0")


# ---- blocks at window paddings 0, 1 and 3 ---------------------------------------------------------------------------------------------- #
BEFORE = R.BEFORE           # the tap in front of each tested block


def check_block(e, grid, p64, taps, layer, i, conv=O.DEFAULT):
    """Placement and masking, not a precision claim: attention runs single-term fp16 (tests/test_pangu_gpu.py test_earth_specific_block)."""
    xin = taps[BEFORE[layer, i]].float().contiguous()            # the oracle's true input tap, as float32 on both sides
    g = O.Geometry(grid.n_lat, grid.n_lon, grid.pad)
    want = O.earth_block(O._block_params(p64, layer, i), xin.double(), g.res(layer), O.HEADS[layer - 1], i % 2 == 1, None, conv)
    got = e.block(layer, i, xin.cuda()).cpu()
    err, where = R.max_rel(got, want)
    print(f"pangu block {grid.id} layer {layer} block {i} roll_sign {conv.roll_sign}: err {err:.2e}")
    C, (Z, H, W) = want.shape[1], g.res(layer)
    m = where // C
    assert torch.isfinite(got).all() and err < BLOCK_TOL, f"{err:.3e}; worst token row {m} = (z, h, w) = ({m // (H * W)}, {m % (H * W) // W}, {m % W})"


@on_grids("24x96", "33x96")
@pytest.mark.parametrize("layer,i", list(BEFORE))
def test_block_at_new_window_paddings(rig, layer, i):
    grid, e, params, p64, x, taps, y = rig
    check_block(e, grid, p64, taps, layer, i)


@pytest.mark.parametrize("layer,i", [(1, 1), (2, 1)])
def test_rolled_block_single_latitude_window_is_the_first_window_type(layer, i):
    """roll_sign = +1 on 24 x 96: layer 1's only latitude window is then the "first" window type, which carries the shift mask."""
    grid = R.GRID["24x96"]
    conv = O.Conventions(roll_sign=+1)
    taps, _ = R.reference(grid.n_lat, grid.n_lon, grid.pad, conventions=(("roll_sign", +1),))
    e = _engine(grid, roll_sign=+1)
    try:
        check_block(e, grid, R.inputs(grid.n_lat, grid.n_lon)[1], taps, layer, i, conv)
    finally:
        e.release()
