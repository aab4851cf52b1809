"""FuXi kernels of include/skyrim_fuxi.h at the edges the model fixtures never reach, each against a float64 restatement written here:
skfuxi_window_attention at key-tile and query-chunk edges (N = 32, 64, 65), the 2 x 2 window, one window over the whole grid, a shift
on one axis only, shifts other than half a window, mask_lon = 0, a logit scale above logit_max, zero q / k rows, a row maximum that
arrives in a late key tile and a sharp softmax over 1024 keys; skfuxi_layer_norm up to C = 1536 with and without the residual;
skfuxi_gn_stats at a large offset, with an outlier, groups = 1 and groups = C, bit for bit; skfuxi_gn_residual in place; skfuxi_conv
with stride 2 on odd grids, taps = 1 without the shuffle, two sources of different widths and group widths that are not multiples of 8;
skfuxi_resample with align_corners; one toy block and toy calls with shift_mask_lon = False and align_corners = True; the documented
argument errors.  Outputs start as a NaN sentinel with a margin past their end, so an element that is never written shows, and so does a
write past the end.  The attention restatement is checked against tests/_fuxi_reference.py on the CPU (the test without the gpu mark)."""
from __future__ import annotations

import ctypes
import datetime
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _fuxi_reference as R

GPU = pytest.mark.gpu
DEV = "cuda:0"
T0 = datetime.datetime(2024, 6, 21, 6)
BAR3 = 2e-6                    # 3-term fp16 hi/lo products, fp32 accumulation: max|err| / max|ref|
U = 2.0 ** -24                 # fp32 unit roundoff
MARGIN = 64                    # NaN elements past the end of every output
LMAX = math.log(100.0)
TOY = dict(n_lat=73, n_lon=144, channels=6, embed=128, heads=2, depth=2, window=(3, 6))


def _lib():
    from skyrim_amd.fuxi import engine
    return engine.load_library()


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


def _nan(n):
    return torch.full((n + MARGIN,), float("nan"), device=DEV)


def _dev(t):
    return t.float().contiguous().to(DEV)


# ---- window attention ---------------------------------------------------------------------------------------------------------- #
def _region(i, n, win, s):
    """The header's mask region of shifted-grid coordinate i: [0, n - win), [n - win, n - s), [n - s, n); 0 without a shift."""
    return 0 if s == 0 else (0 if i < n - win else (1 if i < n - s else 2))


def attn_ref(qkv, cpb, ls, H, W, heads, wh, ww, sh, sw, mask_lon=1, mask_value=-100.0, logit_max=LMAX, norm_eps=1e-12):
    """Swin V2 cosine window attention in float64: roll by (-sh, -sw), partition, normalise q and k, clamp the logit scale, add the
    position bias and the region mask, softmax, sum of p v, reverse, roll back.  qkv [H W][3 C] -> [H W][C]."""
    C, N = 64 * heads, wh * ww
    x = torch.roll(qkv.double().reshape(H, W, 3 * C), (-sh, -sw), (0, 1))
    win = x.reshape(H // wh, wh, W // ww, ww, 3 * C).permute(0, 2, 1, 3, 4).reshape(-1, N, 3, heads, 64).permute(2, 0, 3, 1, 4)
    q, k, v = win[0], win[1], win[2]                                                   # [nW][heads][N][64]
    qn = q / q.norm(dim=-1, keepdim=True).clamp_min(norm_eps)
    kn = k / k.norm(dim=-1, keepdim=True).clamp_min(norm_eps)
    scale = torch.exp(torch.clamp(ls.double(), max=logit_max))
    a = qn @ kn.transpose(-2, -1) * scale[None, :, None, None]
    r = torch.arange(N)
    ry, rx = r // ww, r % ww
    idx = (ry[:, None] - ry[None, :] + wh - 1) * (2 * ww - 1) + (rx[:, None] - rx[None, :] + ww - 1)
    a = a + cpb.double()[:, idx][None]
    reg_y = torch.tensor([_region(i, H, wh, sh) for i in range(H)])
    reg_x = torch.tensor([_region(i, W, ww, sw if mask_lon else 0) for i in range(W)])
    reg = (3 * reg_y[:, None] + reg_x[None, :]).reshape(H // wh, wh, W // ww, ww).permute(0, 2, 1, 3).reshape(-1, N)
    a = a + mask_value * (reg[:, :, None] != reg[:, None, :]).double()[:, None]
    o = (a.softmax(-1) @ v).permute(0, 2, 1, 3).reshape(-1, N, C)
    o = o.reshape(H // wh, W // ww, wh, ww, C).permute(0, 2, 1, 3, 4).reshape(H, W, C)
    return torch.roll(o, (sh, sw), (0, 1)).reshape(H * W, C)


def run_attn(qkv, cpb, ls, H, W, heads, wh, ww, sh, sw, mask_lon=1, mask_value=-100.0, logit_max=LMAX, norm_eps=1e-12, C=None):
    """skfuxi_window_attention on the device; returns (return code, output with its NaN margin, on the host)."""
    from skyrim_amd.fuxi.engine import AttnDesc
    C = 64 * heads if C is None else C
    q, cp, sc = _dev(qkv), _dev(cpb), _dev(ls)
    out = _nan(H * W * C)
    d = AttnDesc(q.data_ptr(), out.data_ptr(), cp.data_ptr(), sc.data_ptr(), H, W, C, heads, wh, ww, sh, sw, mask_lon, mask_value,
                 logit_max, norm_eps)
    rc = _lib().skfuxi_window_attention(ctypes.byref(d), _stream())
    torch.cuda.synchronize()
    return rc, out.cpu()


def _inputs(kind, H, W, heads, wh, ww, seed):
    gen = torch.Generator().manual_seed(seed)
    C, span = 64 * heads, (2 * wh - 1) * (2 * ww - 1)
    qkv = torch.randn(H * W, 3 * C, generator=gen, dtype=torch.float64)
    cpb = 16 * torch.sigmoid(torch.randn(heads, span, generator=gen, dtype=torch.float64))
    ls = math.log(2.0) + torch.rand(heads, generator=gen, dtype=torch.float64) * math.log(10.0)
    if kind == "clamp":                      # head 0 above logit_max (clamped to ln 100), head 1 below it
        ls = torch.tensor([LMAX + 1.5, LMAX - 3.0][:heads], dtype=torch.float64)
    elif kind == "zero":                     # zero q rows and zero k rows: |x| < norm_eps, the normalised vector is 0
        for h in range(heads):
            qkv[3 * h::7, 64 * h:64 * h + 64] = 0
            qkv[5 * h + 1::11, C + 64 * h:C + 64 * h + 64] = 0
    elif kind == "late":                     # the score grows with the key's row: every row's maximum sits in its window's last key tile
        r = torch.arange(2 * wh - 1, dtype=torch.float64) - (wh - 1)                 # dy = row(q) - row(k)
        cpb = (-2.0 * r[:, None].expand(2 * wh - 1, 2 * ww - 1)).reshape(1, -1).repeat(heads, 1) + cpb / 16
        ls = torch.zeros(heads, dtype=torch.float64)                                  # |cosine score| <= 1: the ramp decides
    return qkv.float().double(), cpb.float().double(), ls.float().double()


# (id, H, W, heads, wh, ww, sh, sw, mask_lon, kind).  Shifts other than half a window, so that a region rule that ignores s shows.
ATTN_CASES = [
    ("N32-one-key-tile", 8, 16, 2, 4, 8, 1, 5, 1, "rand"),
    ("N64-one-query-chunk", 16, 16, 1, 8, 8, 3, 2, 1, "rand"),
    ("N65-chunk-and-tile-tails", 10, 26, 1, 5, 13, 1, 4, 1, "rand"),
    ("2x2-window", 6, 8, 2, 2, 2, 1, 1, 1, "rand"),
    ("whole-grid-window", 6, 12, 1, 6, 12, 2, 7, 1, "rand"),
    ("lat-shift-only", 6, 12, 2, 3, 6, 2, 0, 1, "rand"),
    ("lon-shift-only", 6, 12, 2, 3, 6, 0, 1, 1, "rand"),
    ("mask_lon-0", 9, 18, 2, 3, 6, 1, 4, 0, "rand"),
    ("logit-scale-clamped", 6, 12, 2, 3, 6, 1, 3, 1, "clamp"),
    ("zero-q-and-k-rows", 6, 12, 2, 3, 6, 1, 2, 1, "zero"),
    ("late-row-max-N256", 16, 32, 1, 16, 16, 0, 0, 1, "late"),
]


def _attn_bar(cpb, ls, vmax):
    """max|v| (BAR3 + 16 u L): the output is a convex combination of v rows; a score of magnitude <= L = exp(min(ls, logit_max)) +
    max|cpb| carries a few fp32 roundings (the normalisation, the 64-term dot product, the bias add, expf's argument) into the weights."""
    L = torch.exp(torch.clamp(ls, max=LMAX)).max().item() + cpb.abs().max().item()
    return vmax * (BAR3 + 16 * U * L)


@GPU
@pytest.mark.parametrize("case", ATTN_CASES, ids=[c[0] for c in ATTN_CASES])
def test_window_attention_edges_against_float64(case):
    _, H, W, heads, wh, ww, sh, sw, mask_lon, kind = case
    qkv, cpb, ls = _inputs(kind, H, W, heads, wh, ww, seed=H * W + wh)
    C = 64 * heads
    ref = attn_ref(qkv, cpb, ls, H, W, heads, wh, ww, sh, sw, mask_lon)
    rc, out = run_attn(qkv, cpb, ls, H, W, heads, wh, ww, sh, sw, mask_lon)
    assert rc == 0
    assert out[H * W * C:].isnan().all(), "written past the end of the output"
    got = out[:H * W * C].double().view(H * W, C)
    assert torch.isfinite(got).all(), "an output element was not written"
    err = (got - ref).abs().max().item()
    bar = _attn_bar(cpb, ls, qkv[:, 2 * C:].abs().max().item())
    print(f"attention {case[0]}: max err {err:.3e}, bar {bar:.3e}")
    assert err <= bar


def _split_loss(p):
    """What the fp16 hi / lo split keeps of the fp32 value p, subtracted from p."""
    p32 = np.float32(p)
    h = np.float16(p32)
    lo = np.float16(np.float32(p32) - np.float32(h))
    return float(p32) - float(h) - float(lo)


def sharp_gap(n_keys):
    """A score gap g with (n_keys - 1) e^-g ~ 1/4 (the keys' weights stay small against the winner's 1) at which the fp16 split of
    p = e^-g loses the most: below 2^-3 the lo plane is subnormal and keeps only multiples of 2^-24, so up to 2^-25 of p is lost, the
    same for every key of equal weight."""
    g0 = math.log(4 * (n_keys - 1))
    gs = np.float32(g0 + np.linspace(-0.05, 0.05, 4001))
    return float(max(gs, key=lambda g: abs(_split_loss(math.exp(-float(g))))))


@GPU
def test_sharp_softmax_over_1024_keys():
    """One window of 32 x 32 = 1024 keys per query; q = 0, so every score is its position bias, exactly: the query's own key g above all
    others (p = 1), the 1023 others at p = e^-g ~ 1/4092.  Every v is positive, so what a split of P loses adds up over the keys instead
    of cancelling.  Bar as for every other case (the scores are exact, so L is generous here)."""
    H, W, heads, wh, ww = 32, 64, 1, 32, 32
    N = wh * ww
    g = sharp_gap(N)
    gen = torch.Generator().manual_seed(11)
    C = 64 * heads
    qkv = torch.randn(H * W, 3 * C, generator=gen, dtype=torch.float64)
    qkv[:, :C] = 0
    qkv[:, 2 * C:] = 1 + 0.1 * torch.rand(H * W, C, generator=gen, dtype=torch.float64)
    cpb = torch.zeros(heads, (2 * wh - 1) * (2 * ww - 1), dtype=torch.float64)
    cpb[:, (wh - 1) * (2 * ww - 1) + ww - 1] = g
    ls = torch.zeros(heads, dtype=torch.float64)
    qkv = qkv.float().double()
    ref = attn_ref(qkv, cpb, ls, H, W, heads, wh, ww, 0, 0)
    rc, out = run_attn(qkv, cpb, ls, H, W, heads, wh, ww, 0, 0)
    assert rc == 0 and out[H * W * C:].isnan().all()
    got = out[:H * W * C].double().view(H * W, C)
    err = (got - ref).abs().max().item()
    bar = _attn_bar(cpb, ls, qkv[:, 2 * C:].abs().max().item())
    print(f"sharp softmax N={N} g={g:.6f}: split loses {_split_loss(math.exp(-g)):.3e} per key; max err {err:.3e}, bar {bar:.3e}")
    assert err <= bar


@GPU
def test_window_attention_argument_errors_leave_output_untouched():
    """shift >= window (either axis) and C != 64 heads: SKFUXI_E_ARG; a window that does not tile: SKFUXI_E_WINDOW."""
    H, W, heads, wh, ww = 6, 12, 2, 3, 6
    qkv, cpb, ls = _inputs("rand", H, W, heads, wh, ww, seed=1)
    for kw, want in ((dict(sh=3, sw=0), -1), (dict(sh=0, sw=6), -1), (dict(sh=-1, sw=0), -1), (dict(sh=0, sw=0, C=96), -1),
                     (dict(sh=0, sw=0, wh=4), -3)):
        a = dict(wh=wh, ww=ww)
        a.update(kw)
        rc, out = run_attn(qkv, cpb, ls, H, W, heads, a["wh"], a["ww"], a["sh"], a["sw"], C=a.get("C"))
        assert rc == want, kw
        assert out.isnan().all(), kw


def test_attention_restatement_matches_reference():
    """attn_ref (the GPU cases' yardstick) against tests/_fuxi_reference.py's attention on a toy block: the qkv projection done here,
    the cpb table from spec.py, shifted and unshifted, with and without the longitude mask.  CPU only."""
    from skyrim_amd.fuxi.spec import FuxiConfig, cpb_table, init_synthetic, shift
    for mask_lon in (True, False):
        cfg = FuxiConfig(**TOY, shift_mask_lon=mask_lon)
        p = init_synthetic(cfg, 2)
        H, W = cfg.grid1
        x = torch.randn(H, W, cfg.embed, dtype=torch.float64, generator=torch.Generator().manual_seed(3))
        for i in (0, 1):
            b = f"short.blocks.{i}.attn."
            P = lambda n: torch.as_tensor(p[b + n]).double()          # noqa: E731,B023
            bias = torch.cat([P("q_bias"), torch.zeros(cfg.embed, dtype=torch.float64), P("v_bias")])
            qkv = x.reshape(H * W, -1) @ P("qkv.weight").T + bias
            cpb = cpb_table(cfg.window, P("cpb_mlp.0.weight"), P("cpb_mlp.0.bias"), P("cpb_mlp.2.weight"))
            sh, sw = shift(cfg, i)
            got = attn_ref(qkv, cpb, P("logit_scale").reshape(-1), H, W, cfg.heads, *cfg.window, sh, sw, int(mask_lon), cfg.mask_value,
                           cfg.logit_max, cfg.norm_eps)
            ref = R.attention(p, cfg, x, "short", i).reshape(H * W, -1)
            assert (got - ref).abs().max().item() <= 1e-12 * ref.abs().max().item()


# ---- LayerNorm ----------------------------------------------------------------------------------------------------------------- #
def _ln_rows(rows, C, seed):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, C, generator=gen, dtype=torch.float64) * torch.linspace(0.3, 3, rows, dtype=torch.float64)[:, None]
    x[3] += 1e4                                   # a large common offset: 1e4 +- 1
    x[7] = 5 + 1e-3 * x[7] / x[7].std()           # near-constant
    x[11] = 0.75                                  # constant
    x[rows - 1] -= 3e3
    return x.float()


def _ln_check(got, x, g, b, res, eps):
    xd = x.double()
    mean, var = xd.mean(1, keepdim=True), xd.var(1, unbiased=False, keepdim=True)
    rstd = 1 / torch.sqrt(var + eps)
    ref = (xd - mean) * rstd * g.double() + b.double() + (res.double() if res is not None else 0)
    assert torch.isfinite(got).all(), "a row was not written"
    err = (got - ref).abs().amax(1)
    # FCN's LayerNorm bar: 1e-5 of the row's max|ref|, plus what the fp32 mean of a row at a large offset costs (16 u |mean| rstd |gamma|)
    # and, with the residual, one rounding of the sum
    lim = 1e-5 * ref.abs().amax(1) + 16 * U * g.double().abs().max() * mean[:, 0].abs() * rstd[:, 0]
    if res is not None:
        lim = lim + U * ref.abs().amax(1)
    assert (err <= lim).all(), (err / lim).max().item()


@GPU
@pytest.mark.parametrize("res", ["none", "residual", "in-place"])
@pytest.mark.parametrize("C", [4, 132, 1028, 1536])
def test_layer_norm_against_float64(C, res):
    """4 k + 1 rows (the last workgroup's three other wavefronts idle), C = 1536 (kLnVec = 6 float4 per lane, all used), C not a multiple
    of 256 (132, 1028: lanes with a partial register set), rows at offsets 1e4 and -3e3; out = res in place (the header allows it)."""
    rows = 21
    x = _ln_rows(rows, C, C)
    gen = torch.Generator().manual_seed(C + 1)
    g, b = 1 + 0.1 * torch.randn(C, generator=gen), 0.1 * torch.randn(C, generator=gen)
    r = torch.randn(rows, C, generator=gen) * 2 if res != "none" else None
    out = _nan(rows * C)
    if res == "in-place":
        out[:rows * C] = _dev(r).reshape(-1)
        rp = out
    else:
        rp = _dev(r) if r is not None else None
    eps = 1e-5
    xd, gd, bd = _dev(x), _dev(g), _dev(b)
    rc = _lib().skfuxi_layer_norm(xd.data_ptr(), rp.data_ptr() if rp is not None else None, gd.data_ptr(), bd.data_ptr(), out.data_ptr(),
                                  rows, C, eps, _stream())
    assert rc == 0
    o = out.cpu()
    assert o[rows * C:].isnan().all(), "written past the last row"
    _ln_check(o[:rows * C].double().view(rows, C), x, g, b, r, eps)


@GPU
def test_layer_norm_refuses_c_above_1536():
    x = torch.zeros(4 * 1540, device=DEV)
    g = torch.ones(1540, device=DEV)
    out = _nan(4 * 1540)
    for C in (1540, 1538):
        assert _lib().skfuxi_layer_norm(x.data_ptr(), None, g.data_ptr(), g.data_ptr(), out.data_ptr(), 4, C, 1e-5, _stream()) == -1
    torch.cuda.synchronize()
    assert out.isnan().all()


# ---- GroupNorm ----------------------------------------------------------------------------------------------------------------- #
GN_CASES = [(1000, 64, 32, "offset"), (777, 48, 16, "outlier"), (300, 96, 1, "plain"), (129, 64, 64, "plain"), (2000, 40, 5, "offset")]


def _gn_input(rows, C, kind, seed):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, C, generator=gen, dtype=torch.float64) * 2 + 0.5
    if kind == "offset":
        x = x + 1e4
    elif kind == "outlier":
        x[0] = 5e3 * torch.tensor([1.0, -1.0] * (C // 2), dtype=torch.float64)
    return x.float()


@GPU
@pytest.mark.parametrize("rows,C,groups,kind", GN_CASES, ids=[f"{r}x{c}-g{g}-{k}" for r, c, g, k in GN_CASES])
def test_gn_stats_against_float64_and_bitwise_repeatable(rows, C, groups, kind):
    """(mean, rstd) per group: float64 sums rounded once to fp32.  mean within 2 u (|mean| + std); rstd within 2 u plus the float64
    cancellation of E[x^2] - mean^2 (n 2^-52 (mean^2 + var) / var).  Two runs give the same bits (the header's fixed order)."""
    x = _gn_input(rows, C, kind, rows + C)
    xd = x.double().reshape(rows, groups, C // groups).permute(1, 0, 2).reshape(groups, -1)
    mean, var = xd.mean(1), xd.var(1, unbiased=False)
    eps = 1e-5
    rstd = 1 / torch.sqrt(var + eps)
    xg = _dev(x)
    outs = []
    for _ in range(2):
        st = _nan(2 * groups)
        assert _lib().skfuxi_gn_stats(xg.data_ptr(), rows, C, groups, eps, st.data_ptr(), _stream()) == 0
        outs.append(st.cpu())
    assert outs[1][2 * groups:].isnan().all(), "written past the last group"
    assert torch.equal(outs[0].view(torch.int32)[:2 * groups], outs[1].view(torch.int32)[:2 * groups])
    st = outs[0][:2 * groups].double().view(groups, 2)
    n = rows * (C // groups)
    assert ((st[:, 0] - mean).abs() <= 2 * U * (mean.abs() + var.sqrt())).all()
    lim = 2 * U + n * 2.0 ** -52 * (mean ** 2 + var) / var
    err = ((st[:, 1] - rstd).abs() / rstd)
    print(f"gn_stats {rows}x{C} g{groups} {kind}: rstd rel err {err.max().item():.3e}")
    assert (err <= lim).all()


@GPU
def test_gn_residual_in_place():
    """out = x + SiLU((a - mean_g) rstd_g gamma + beta) with out == x, 3 channels per group (a float4 spans two groups).  Per element
    8 u (|x| + |pre-activation| + 1): a handful of fp32 operations and expf."""
    rows, C, groups = 101, 48, 16
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(rows, C, generator=gen).float()
    a = (torch.randn(rows, C, generator=gen) * 3 + 1).float()
    st = torch.stack([torch.randn(groups, generator=gen), 0.5 + torch.rand(groups, generator=gen)], 1).float()
    g, b = (1 + 0.2 * torch.randn(C, generator=gen)).float(), (0.1 * torch.randn(C, generator=gen)).float()
    cg = torch.arange(C) // (C // groups)
    pre = (a.double() - st[cg, 0].double()) * st[cg, 1].double() * g.double() + b.double()
    ref = x.double() + F.silu(pre)
    out = _nan(rows * C)
    out[:rows * C] = _dev(x).reshape(-1)
    sd, gd, bd, ad = _dev(st), _dev(g), _dev(b), _dev(a)
    assert _lib().skfuxi_gn_residual(out.data_ptr(), ad.data_ptr(), sd.data_ptr(), gd.data_ptr(), bd.data_ptr(), out.data_ptr(), rows, C,
                                     groups, _stream()) == 0
    o = out.cpu()
    assert o[rows * C:].isnan().all()
    got = o[:rows * C].double().view(rows, C)
    assert ((got - ref).abs() <= 8 * U * (x.double().abs() + pre.abs() + 1)).all()


# ---- conv ---------------------------------------------------------------------------------------------------------------------- #
# (id, h_in, w_in, c0, c1, taps, stride, groups (0: no GroupNorm on load), cout, shuffle)
CONV_CASES = [
    ("stride2-odd-grid-gn-cpg2", 9, 13, 16, 0, 9, 2, 8, 20, 0),
    ("stride2-odd-grid-cat", 11, 7, 8, 24, 9, 2, 0, 36, 0),
    ("taps1-no-shuffle-cat-gn-cpg4", 11, 7, 24, 16, 1, 1, 6, 36, 0),
    ("taps9-cat-gn-cpg5-N132", 10, 12, 40, 8, 9, 1, 8, 132, 0),
    ("taps1-shuffle-cat-c0-ne-c1", 5, 9, 16, 32, 1, 1, 4, 12, 1),
]


@GPU
@pytest.mark.parametrize("case", CONV_CASES, ids=[c[0] for c in CONV_CASES])
def test_conv_against_float64(case):
    """Zero padding after the GroupNorm + SiLU of the loader; channels c < c0 from src0, the rest from src1; output tails in M and N;
    the 2 x 2 pixel shuffle.  Bar: BAR3 of each output channel's max|ref|."""
    from skyrim_amd import native
    from skyrim_amd.fuxi.engine import ConvDesc
    _, h_in, w_in, c0, c1, taps, stride, groups, cout, shuffle = case
    gen = torch.Generator().manual_seed(h_in * w_in + c0)
    cin = c0 + c1
    h_out, w_out = ((h_in - 1) // stride + 1, (w_in - 1) // stride + 1) if taps == 9 else (h_in, w_in)
    N = 4 * cout if shuffle else cout
    s0 = torch.randn(h_in, w_in, c0, generator=gen).float()
    s1 = torch.randn(h_in, w_in, c1, generator=gen).float() if c1 else None
    Wm = (torch.randn(N, taps * cin, generator=gen) / math.sqrt(taps * cin)).float()
    bias = (0.1 * torch.randn(cout, generator=gen)).float()
    a0 = s0.double()
    st = gm = bt = None
    if groups:
        st = torch.stack([torch.randn(groups, generator=gen), 0.5 + torch.rand(groups, generator=gen)], 1).float()
        gm, bt = (1 + 0.2 * torch.randn(c0, generator=gen)).float(), (0.1 * torch.randn(c0, generator=gen)).float()
        cg = torch.arange(c0) // (c0 // groups)
        a0 = F.silu((a0 - st[cg, 0].double()) * st[cg, 1].double() * gm.double() + bt.double())
    A = torch.cat([a0, s1.double()], -1) if c1 else a0                               # [h_in][w_in][cin]
    if taps == 9:
        w4 = Wm.double().view(N, 3, 3, cin).permute(0, 3, 1, 2)
        acc = F.conv2d(A.permute(2, 0, 1)[None], w4, stride=stride, padding=1)[0].permute(1, 2, 0)
    else:
        acc = A @ Wm.double().T
    assert acc.shape[:2] == (h_out, w_out)
    if shuffle:                       # column n = (2 dy + dx) cout + co -> pixel (2 y + dy, 2 x + dx), channel co
        ref = acc.view(h_out, w_out, 2, 2, cout).permute(0, 2, 1, 3, 4).reshape(2 * h_out, 2 * w_out, cout) + bias.double()
    else:
        ref = acc + bias.double()
    ref = ref.reshape(-1, cout)
    W = native.HiLoWeight(torch.device(DEV), _lib().skfuxi_prepare_weight, Wm)
    dv = lambda t: _dev(t) if t is not None else None          # noqa: E731
    s0d, s1d, std_, gmd, btd, bd = dv(s0), dv(s1), dv(st), dv(gm), dv(bt), dv(bias)
    out = _nan(ref.numel())
    p = lambda t: t.data_ptr() if t is not None else None      # noqa: E731
    d = ConvDesc(p(s0d), p(s1d), p(std_), p(gmd), p(btd), W.buf.data_ptr(), W.plane, W.ldw, bd.data_ptr(), out.data_ptr(), h_in, w_in,
                 h_out, w_out, c0, c1, taps, stride, groups if groups else 1, cout, shuffle)
    assert _lib().skfuxi_conv(ctypes.byref(d), _stream()) == 0
    o = out.cpu()
    assert o[ref.numel():].isnan().all(), "written past the end of the output"
    got = o[:ref.numel()].double().view(-1, cout)
    assert torch.isfinite(got).all(), "an output element was not written"
    err = ((got - ref).abs().amax(0) / ref.abs().amax(0)).max().item()
    print(f"conv {case[0]}: per-channel rel err {err:.3e}")
    assert err <= BAR3


# ---- bilinear resample --------------------------------------------------------------------------------------------------------- #
@GPU
@pytest.mark.parametrize("align", [0, 1])
@pytest.mark.parametrize("hs,ws,ho,wo", [(20, 36, 21, 36), (7, 5, 16, 11), (12, 40, 5, 9)])
def test_resample_against_interpolate(hs, ws, ho, wo, align):
    """out = mean + std bilinear(src) as F.interpolate(align_corners) computes it: up and down, both flags.  Per element: the fp32 source
    coordinate is good to ~2 n_in u, which moves a sample by at most that times the largest neighbour difference (2 max|src|); plus 8 u
    for the two-level lerp and the affine."""
    from skyrim_amd.fuxi.engine import ResampleDesc
    C = 3
    gen = torch.Generator().manual_seed(hs * ws + align)
    src = torch.randn(C, hs, ws, generator=gen).float()
    mean, std = torch.tensor([250.0, -3.0, 0.5]), torch.tensor([20.0, 4.0, 0.01])
    ref = F.interpolate(src.double()[None], size=(ho, wo), mode="bilinear", align_corners=bool(align))[0]
    ref = ref * std.double()[:, None, None] + mean.double()[:, None, None]
    sd, md, vd = _dev(src), _dev(mean), _dev(std)
    out = _nan(C * ho * wo)
    d = ResampleDesc(sd.data_ptr(), md.data_ptr(), vd.data_ptr(), out.data_ptr(), C, hs, ws, ho, wo, align)
    assert _lib().skfuxi_resample(ctypes.byref(d), _stream()) == 0
    o = out.cpu()
    assert o[C * ho * wo:].isnan().all()
    got = o[:C * ho * wo].double().view(C, ho, wo)
    lim = (8 + 4 * max(hs, ws)) * U * src.abs().amax((1, 2)).double() * std.double() + 8 * U * mean.double().abs()
    assert ((got - ref).abs().amax((1, 2)) <= lim).all()


# ---- toy block and calls with the UNVERIFIED alternatives ------------------------------------------------------------------------ #
def _toy_cfg(**kw):
    from skyrim_amd.fuxi.spec import FuxiConfig
    return FuxiConfig(**{**TOY, **kw})


def _engine(cfg, p):
    from skyrim_amd.fuxi.engine import FuxiEngine
    eng = FuxiEngine(cfg, DEV)
    eng.load_params(p)
    return eng


@GPU
def test_shifted_block_without_longitude_mask():
    """shift_mask_lon = False (the kernel's mask_lon = 0): a shifted block on the toy grid against the restatement (1e-5)."""
    from skyrim_amd.fuxi.spec import init_synthetic
    cfg = _toy_cfg(shift_mask_lon=False)
    p = init_synthetic(cfg, 5)
    eng = _engine(cfg, p)
    g1 = cfg.grid1
    x = torch.randn(g1[0], g1[1], cfg.embed, dtype=torch.float64, generator=torch.Generator().manual_seed(4))
    ref = R.swin_block(p, cfg, x, "short", 1)
    xd = _dev(x)
    eng.swin_block(1, "short", x=xd)
    assert R.token_err(xd, ref).max().item() <= 1e-5


@GPU
@pytest.mark.parametrize("kw", [dict(shift_mask_lon=False), dict(align_corners=True)], ids=["shift_mask_lon-False", "align_corners-True"])
def test_toy_call_with_unverified_alternative(kw):
    from skyrim_amd.fuxi.spec import init_synthetic, synthetic_state
    cfg = _toy_cfg(**kw)
    p = init_synthetic(cfg, 3)
    eng = _engine(cfg, p)
    x0, x1 = synthetic_state(cfg, 0), synthetic_state(cfg, 1)
    y = eng.call(_dev(x0), _dev(x1), T0, "medium")
    assert R.per_channel_err(y, R.call(p, cfg, x0, x1, T0, "medium")).max().item() <= 1e-4
