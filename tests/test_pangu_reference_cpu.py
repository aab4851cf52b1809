"""The float64 reference of tests/test_pangu_kernels_gpu.py, checked on the CPU: it really runs in float64, the float32 oracle agrees
with it to float32's own rounding, the stage helpers reproduce the oracle's taps, and the small grids have the paddings they were
chosen for."""
import pytest
import torch

import _pangu_reference as R
from oracle import pangu_oracle as O
from skyrim_amd.pangu.spec import PanguGeometry

F32_TOL = 1e-5      # float32 oracle against the float64 route, max|err| / max|ref| per tap: measured 4e-7 .. 1.6e-6 on these grids


@pytest.mark.parametrize("grid", R.GRIDS, ids=lambda g: g.id)
def test_geometry_table(grid):
    """The edge properties the grids were chosen for, against the engine's geometry AND the oracle's: a later change of the padding rules
    must not quietly turn the kernel tests into copies of the toy grid."""
    g = PanguGeometry(grid.n_lat, grid.n_lon, grid.pad)
    o = O.Geometry(grid.n_lat, grid.n_lon, grid.pad)
    assert (g.lat_padded - g.n_lat, g.lat_pad_top) == grid.lat_pad
    assert (o.lat_pad[1] + o.lat_pad[2], o.lat_pad[1]) == grid.lat_pad
    assert (g.H1, g.H2) == (grid.H1, grid.H2) == (o.H1, o.H2)
    assert (g.H1 % 2 == 1) == grid.down_pad_row
    assert (g.padded_lat(1) - g.H1, g.pad_top(1)) == grid.win_pad_fine == (g.padded_lat(4) - g.H1, g.pad_top(4))
    assert (g.padded_lat(2) - g.H2, g.pad_top(2)) == grid.win_pad_coarse == (g.padded_lat(3) - g.H2, g.pad_top(3))
    for layer, want in ((1, grid.win_pad_fine), (2, grid.win_pad_coarse)):
        hp, top, bot = O._centre_pad(o.res(layer)[1], O.WINDOW[1], grid.pad)
        assert (top + bot, top) == want
    assert (g.tokens(1), g.tokens(2)) == grid.tokens
    # tail tiles (csrc/tiles.h): PatchEmbedding runs 64-row tiles over the surface slab (hw rows) and the upper slabs (7 hw), PatchRecovery
    # 128- and 256-row tiles over the same, UpSample's second Linear 256-row tiles over the fine tokens: none of them divides on any grid.
    # (The coarse token counts 384 and 768 ARE multiples of DownSample's 128-row tile; 288 and 480 are not -- see the coverage test.)
    hw = g.H1 * g.W1
    assert hw % 64 and (7 * hw) % 64 and hw % 128 and (7 * hw) % 256 and grid.tokens[0] % 256
    # where the surface slab ends in the 16-row blocks of the operand layout: in mid-block on the 96-wide grids with an odd H1 (as on 721 x 1440)
    assert hw % 16 == (8 if grid.n_lon == 96 and g.H1 % 2 else 0)


def test_the_table_covers_every_padding_it_claims():
    centre = [g for g in R.GRIDS if g.pad == "centre"]
    assert {g.lat_pad for g in centre} == {(0, 0), (1, 0), (2, 1), (3, 1)}
    assert {g.win_pad_fine[0] for g in centre} | {g.win_pad_coarse[0] for g in centre} >= {0, 1, 2, 3, 5}
    assert {g.lat_pad for g in R.GRIDS if g.pad == "back"} == {(2, 0), (3, 0)}
    coarse = {g.tokens[1] for g in R.GRIDS}                             # DownSample / UpSample.linear1: 128- / 256-row tiles
    assert any(t % 128 for t in coarse) and any(t % 128 == 0 for t in coarse) and any(t % 256 for t in coarse)
    assert any(g.n_lon // 8 // 12 == 2 for g in R.GRIDS)              # two longitude windows at the coarse level


@pytest.mark.parametrize("grid", R.GRIDS, ids=lambda g: g.id)
def test_float64_route_is_float64_and_the_float32_oracle_follows_it(grid):
    params, p64, x = R.inputs(grid.n_lat, grid.n_lon)
    taps, y = R.reference(grid.n_lat, grid.n_lon, grid.pad)
    assert y.dtype == torch.float64 and taps and all(t.dtype == torch.float64 for t in taps.values())
    taps32 = {}
    y32 = O.forward(params, x, taps=taps32, conv=O.Conventions(pad=grid.pad))
    assert y32.dtype == torch.float32 and set(taps32) == set(taps)
    errs = {k: R.max_rel(taps32[k], taps[k])[0] for k in taps}
    print(grid.id, " ".join(f"{k} {v:.1e}" for k, v in errs.items() if "block" not in k))
    assert 0 < max(errs.values()) < F32_TOL, errs           # > 0: the two routes are not the same computation
    assert O.per_channel_rel_err(y32, y).max().item() < F32_TOL


@pytest.mark.parametrize("grid", R.GRIDS, ids=lambda g: g.id)
def test_stage_helpers_reproduce_the_oracles_taps(grid):
    """``stage`` on the float64 taps gives the next float64 tap exactly: the normalisation, concat and de-normalisation it carries are
    ``forward``'s own."""
    _, p64, x = R.inputs(grid.n_lat, grid.n_lon)
    taps, y = R.reference(grid.n_lat, grid.n_lon, grid.pad)
    assert torch.equal(R.stage("embed", p64, grid, x), taps["embed"])
    assert torch.equal(R.stage("down", p64, grid, taps["layer1.block1"]), taps["down"])
    assert torch.equal(R.stage("up", p64, grid, taps["layer3"]), taps["up"])
    assert torch.equal(R.stage("recover", p64, grid, taps["layer1.block1"], taps["layer4"]), y)


@pytest.mark.parametrize("name", ["down", "up"])
def test_small_stream_makes_the_layernorm_epsilon_visible(name, monkeypatch):
    """What the GPU test of the same inputs relies on: with eps ten times smaller the float64 stage moves by 6 .. 8e-4, some fifty stage
    bars (~1e-5), while on the taps as they are it moves by 2e-6 -- under every bar."""
    grid = R.GRID["25x96"]
    _, p64, x = R.inputs(grid.n_lat, grid.n_lon)
    taps, _ = R.reference(grid.n_lat, grid.n_lon, grid.pad)
    small, plain = R.small_stream_inputs(taps)[name], R.stage_inputs(taps, x)[name]
    want_small, want_plain = R.stage(name, p64, grid, *small), R.stage(name, p64, grid, *plain)
    monkeypatch.setattr(O, "LN_EPS", 1e-6)
    moved_small = R.max_rel(R.stage(name, p64, grid, *small), want_small)[0]
    moved_plain = R.max_rel(R.stage(name, p64, grid, *plain), want_plain)[0]
    print(f"{name}: eps 1e-5 -> 1e-6 moves the small stream's result by {moved_small:.1e}, the plain tap's by {moved_plain:.1e}")
    assert moved_small > 3e-4 and moved_plain < 1e-5


def test_locate_names_rows_and_padding():
    g = R.GRID["27x96"]                                     # lat_top 0: token row h = 6 holds latitudes 24 .. 27, one of them padding
    assert "(z, h, w) = (1, 6, 23), column 5" in R.locate("embed", g, ((1 * 7 + 6) * 24 + 23) * 192 + 5)
    assert "touches a padded latitude" in R.locate("embed", g, ((1 * 7 + 6) * 24 + 23) * 192 + 5)
    assert "touches no padding" in R.locate("embed", g, ((1 * 7 + 5) * 24) * 192)
    assert "touches a padded latitude" in R.locate("down", g, ((2 * 4 + 3) * 12 + 1) * 384)      # merged row 3 = fine rows 6, 7
    assert "(channel, lat, lon) = (68, 26, 95)" in R.locate("recover", g, 68 * 27 * 96 + 26 * 96 + 95)
    assert "partly cropped" in R.locate("recover", g, 26 * 96) and "is whole" in R.locate("recover", g, 23 * 96)
