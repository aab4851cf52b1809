"""The fused QKV + attention kernel (csrc/attention.hip: qkv_attention_kernel, Q / K / V in registers, Q read with the register index in
the rolled query loop) against the two-launch form (SKP_SPLIT_ATTN=1 at engine construction), which keeps Q in memory: the same products in
the same order per accumulator, so the same BITS.

The grid is 49 x 864: the fine layers (C = 192) have 18 longitude windows per window type and the coarse ones (C = 384) 9, so with eight
waves per workgroup a wave walks up to three (two) windows and some waves one fewer than their neighbours.  What a wave carries from one
window to the next -- its LDS ring, the window table entries fetched a window ahead, the Q registers -- is exercised only there: on the
49 x 192 toy grid of test_pangu_gpu.py (4 and 2 windows per type) no wave ever walks a second window.  The grid keeps the toy grid's padding
latitude rows and shifted-window blocks."""
import pytest
import torch

from skyrim_amd.pangu.engine import DEFAULT_PRECISION
from skyrim_amd.pangu.spec import PanguGeometry, init_synthetic, synthetic_state

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def wide():
    g = PanguGeometry(49, 864)
    for layer, per_type in ((1, 18), (2, 9)):
        assert g.n_windows(layer) == per_type * g.window_types(layer)
    assert g.padded_lat(1) > g.res(1)[1] or g.padded_lat(2) > g.res(2)[1]       # padding rows: tokens whose stream row is the zero row
    return g, init_synthetic(g, 0), synthetic_state(g, 0)


@pytest.mark.parametrize("precision", [DEFAULT_PRECISION, "f16x2m"])
def test_fused_attention_over_several_windows_per_wave_is_bit_identical_to_the_two_launches(wide, monkeypatch, precision):
    from skyrim_amd.pangu.engine import PanguEngine
    g, params, x = wide
    outs, launches = {}, {}
    for split in (True, False):
        if split:
            monkeypatch.setenv("SKP_SPLIT_ATTN", "1")
        else:
            monkeypatch.delenv("SKP_SPLIT_ATTN", raising=False)
        e = PanguEngine(g, precision, "cuda:0")
        e.load_params(params, calibration="off", guard=False)
        e.profile(True)
        y1 = e.step(x.cuda())
        launches[split] = {s_["name"]: s_["launches"] for s_ in e.profile_read()}
        e.profile(False)
        y2 = e.step(y1)                                # a second step, on the first one's output
        outs[split] = (y1.cpu(), y2.cpu())
        e.release()
    assert launches[True]["qkv_r0"] == 4 and launches[True]["qkv_r1"] == 12
    assert launches[False]["qkv_r0"] == 0 and launches[False]["qkv_r1"] == 0
    assert launches[False]["attn_r0"] == 4 and launches[False]["attn_r1"] == 12
    assert all(bool(torch.isfinite(y).all()) for y in outs[False])
    assert torch.equal(outs[True][0], outs[False][0])
    assert torch.equal(outs[True][1], outs[False][1])
