"""FengWu kernels of include/skyrim_fengwu.h at the edges the model fixtures never reach, each against a float64 restatement written here:
skfw_window_attention with 1024-token windows (16 query chunks), latitude padding tokens under both pad values, a shift in the
modality axis alone, types_y = 2 over one row of windows, per-window tables (types_z = nwz, types_y = nwy), non-zero fz / fw front
offsets, batch entries with their own tables, a row maximum in a late key tile and a sharp softmax over 1024 keys; skfw_linear with the
two-source loader split off a tile boundary, the residual aliasing the output, M and N tails and the patch expand with front 0 and 1 at
an odd h_out; skfw_layer_norm up to C = 1536 with and without the merge gather; a toy call with pad = "back"; the documented argument
errors.  Outputs start as a NaN sentinel with a margin past their end, so an element that is never written shows, and so does a write
past the end.  The attention restatement is checked against tests/_fengwu_reference.py on the CPU (the test
without the gpu mark)."""
from __future__ import annotations

import ctypes
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _fengwu_reference as R

GPU = pytest.mark.gpu
DEV = "cuda:0"
BAR3 = 2e-6                    # 3-term fp16 hi/lo products, fp32 accumulation: max|err| / max|ref|
U = 2.0 ** -24                 # fp32 unit roundoff
MARGIN = 64                    # NaN elements past the end of every output
MASK = -100.0
TOY = dict(n_lat=33, n_lon=64, modalities=(("surface", 2), ("z", 3), ("q", 3), ("u", 3), ("v", 3), ("t", 3)), dims=(64, 128),
           heads=(2, 4), enc_depths=(2, 2), dec_depths=(2, 2), fuser_depth=2, window2d=(4, 4), window3d=(2, 4, 4))


def _lib():
    from skyrim_amd.fengwu import engine
    return engine.load_library()


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


def _nan(n):
    return torch.full((n + MARGIN,), float("nan"), device=DEV)


def _dev(t):
    return t.float().contiguous().to(DEV)


# ---- window attention ---------------------------------------------------------------------------------------------------------- #
def _type(n_types, n_win, i):
    """The header's table type of window row i: i itself with one type per row, the last row apart with two, else 0."""
    return i if n_types == n_win else ((1 if i == n_win - 1 else 0) if n_types == 2 else 0)


def fw_attn_ref(qkv, qkv_b, table, g, scale):
    """Window attention in float64.  qkv [B][Z H W][3 C], qkv_b [B][3 C], table [B][types_z types_y][heads][N][N]; g: the geometry dict.
    Pad the grid to (Zp, Hp, Wp) with the qkv bias at (fz, fh, fw), roll by -shift, partition, scores scale q k + table row of the window's
    type, softmax, sum of p v, reverse, roll back, crop -> [B][Z H W][C]."""
    B = qkv.shape[0]
    Z, H, W, Zp, Hp, Wp = g["Z"], g["H"], g["W"], g["Zp"], g["Hp"], g["Wp"]
    fz, fh, fw, (wz, wh, ww), s = g["fz"], g["fh"], g["fw"], g["win"], g["shift"]
    heads = g["heads"]
    C, N = 32 * heads, wz * wh * ww
    nz, ny, nx = Zp // wz, Hp // wh, Wp // ww
    out = []
    for b in range(B):
        P = qkv_b[b].double().expand(Zp, Hp, Wp, 3 * C).clone()
        P[fz:fz + Z, fh:fh + H, fw:fw + W] = qkv[b].double().reshape(Z, H, W, 3 * C)
        P = torch.roll(P, tuple(-v for v in s), (0, 1, 2))
        win = P.reshape(nz, wz, ny, wh, nx, ww, 3 * C).permute(0, 2, 4, 1, 3, 5, 6).reshape(nz, ny, nx, N, 3, heads, 32)
        q, k, v = (win[..., i, :, :].transpose(-3, -2) for i in range(3))          # [nz][ny][nx][heads][N][32]
        a = scale * q @ k.transpose(-2, -1)
        bias = torch.stack([torch.stack([table[b][_type(g["types"][0], nz, za) * g["types"][1] + _type(g["types"][1], ny, yb)]
                                         for yb in range(ny)]) for za in range(nz)]).double()    # [nz][ny][heads][N][N]
        a = a + bias[:, :, None]
        o = (a.softmax(-1) @ v).transpose(-3, -2).reshape(nz, ny, nx, wz, wh, ww, C)
        o = o.permute(0, 3, 1, 4, 2, 5, 6).reshape(Zp, Hp, Wp, C)
        o = torch.roll(o, tuple(s), (0, 1, 2))
        out.append(o[fz:fz + Z, fh:fh + H, fw:fw + W].reshape(Z * H * W, C))
    return torch.stack(out)


def run_fw_attn(qkv, qkv_b, table, g, scale, heads=None, C=None):
    """skfw_window_attention on the device; returns (return code, output with its NaN margin, on the host)."""
    from skyrim_amd.fengwu.engine import AttnDesc
    B = qkv.shape[0]
    heads = g["heads"] if heads is None else heads
    C = 32 * heads if C is None else C
    q, qb, t = _dev(qkv), _dev(qkv_b), _dev(table)
    n_out = B * g["Z"] * g["H"] * g["W"] * C
    out = _nan(n_out)
    tsb = table[0].numel()
    d = AttnDesc(q.data_ptr(), qb.data_ptr(), t.data_ptr(), out.data_ptr(), tsb, B, g["Z"], g["H"], g["W"], g["Zp"], g["Hp"], g["Wp"],
                 g["fz"], g["fh"], g["fw"], *g["win"], *g["shift"], *g["types"], C, heads, scale)
    rc = _lib().skfw_window_attention(ctypes.byref(d), _stream())
    torch.cuda.synchronize()
    return rc, out.cpu(), n_out


def _geom(B, Z, H, W, Zp, Hp, Wp, fz, fh, fw, win, shift, types, heads):
    return dict(B=B, Z=Z, H=H, W=W, Zp=Zp, Hp=Hp, Wp=Wp, fz=fz, fh=fh, fw=fw, win=win, shift=shift, types=types, heads=heads)


def _fw_inputs(g, kind, seed):
    gen = torch.Generator().manual_seed(seed)
    C, N = 32 * g["heads"], math.prod(g["win"])
    T = g["types"][0] * g["types"][1]
    ntok = g["Z"] * g["H"] * g["W"]
    qkv = torch.randn(g["B"], ntok, 3 * C, generator=gen, dtype=torch.float64)
    qkv_b = torch.randn(g["B"], 3 * C, generator=gen, dtype=torch.float64) * 2 + 1          # padding tokens stand apart
    table = torch.randn(g["B"], T, g["heads"], N, N, generator=gen, dtype=torch.float64) * 2
    table = table + 3 * torch.arange(T, dtype=torch.float64)[None, :, None, None, None]      # types differ in more than noise
    table[torch.rand(table.shape, generator=gen) < 0.2] = MASK                               # shift-mask entries
    idx = torch.arange(N)
    table[..., idx, idx] = table[..., idx, idx].clamp_min(0)                                 # every query keeps an unmasked key
    if kind == "late":                       # a score ramp along the key index: every row's maximum sits in its last key tile
        qkv[..., :C] *= 0.1
        table = 0.05 * idx.double().expand(N, N).expand_as(table).clone()
    return qkv.float().double(), qkv_b.float().double(), table.float().double()


def _fw_bar(qkv, qkv_b, table, g, scale):
    """max|v| (BAR3 + 16 u L), L = scale max|q| max|k| + max|table| over unmasked entries: the output is a convex combination of v rows and
    a score of magnitude <= L carries a few fp32 roundings (dot product, table add, expf's argument) into the weights."""
    C = 32 * g["heads"]
    rows = torch.cat([qkv.reshape(-1, 3 * C), qkv_b.reshape(-1, 3 * C)])
    qm = rows[:, :C].reshape(-1, g["heads"], 32).norm(dim=-1).max().item()
    km = rows[:, C:2 * C].reshape(-1, g["heads"], 32).norm(dim=-1).max().item()
    L = scale * qm * km + table[table > MASK / 2].abs().max().item()
    return rows[:, 2 * C:].abs().max().item() * (BAR3 + 16 * U * L)


# (id, geometry, kind)
FW_ATTN_CASES = [
    ("N1024-16-query-chunks", _geom(1, 1, 30, 64, 1, 32, 64, 0, 1, 0, (1, 32, 32), (0, 5, 16), (1, 2), 1), "rand"),
    ("pad-centre-batch2", _geom(2, 1, 10, 16, 1, 12, 16, 0, 1, 0, (1, 4, 8), (0, 2, 4), (1, 2), 2), "rand"),
    ("pad-back-batch2", _geom(2, 1, 10, 16, 1, 12, 16, 0, 0, 0, (1, 4, 8), (0, 2, 4), (1, 2), 2), "rand"),
    ("modality-shift-only", _geom(1, 4, 6, 8, 4, 6, 8, 0, 0, 0, (2, 3, 4), (1, 0, 0), (2, 1), 2), "rand"),
    ("types_y2-one-window-row", _geom(1, 1, 4, 8, 1, 4, 8, 0, 0, 0, (1, 4, 4), (0, 2, 2), (1, 2), 1), "rand"),
    ("per-window-tables-batch2", _geom(2, 4, 10, 8, 4, 12, 8, 0, 1, 0, (2, 4, 4), (1, 2, 2), (2, 3), 2), "rand"),
    ("front-offsets-fz-fw", _geom(1, 3, 6, 12, 4, 8, 16, 1, 2, 2, (2, 4, 8), (1, 1, 3), (2, 2), 2), "rand"),
    ("late-row-max-N256", _geom(1, 1, 16, 32, 1, 16, 32, 0, 0, 0, (1, 16, 16), (0, 0, 0), (1, 1), 1), "late"),
]


@GPU
@pytest.mark.parametrize("case", FW_ATTN_CASES, ids=[c[0] for c in FW_ATTN_CASES])
def test_window_attention_edges_against_float64(case):
    """Padding tokens read the qkv bias as keys and values; a padded query has no place in the output, so the check is that every real
    token is written and equals the reference (with two batch entries, a stray write of entry 1 lands in entry 0)."""
    _, g, kind = case
    scale = 1 / math.sqrt(32)
    qkv, qkv_b, table = _fw_inputs(g, kind, seed=g["H"] * g["W"] + g["Z"])
    ref = fw_attn_ref(qkv, qkv_b, table, g, scale)
    rc, out, n = run_fw_attn(qkv, qkv_b, table, g, scale)
    assert rc == 0
    assert out[n:].isnan().all(), "written past the end of the output"
    got = out[:n].double().view(ref.shape)
    assert torch.isfinite(got).all(), "an output element was not written"
    err = (got - ref).abs().max().item()
    bar = _fw_bar(qkv, qkv_b, table, g, scale)
    print(f"attention {case[0]}: max err {err:.3e}, bar {bar:.3e}")
    assert err <= bar


def _split_loss(p):
    p32 = np.float32(p)
    h = np.float16(p32)
    lo = np.float16(np.float32(p32) - np.float32(h))
    return float(p32) - float(h) - float(lo)


@GPU
def test_sharp_softmax_over_1024_keys():
    """One 1 x 32 x 32 window of 1024 keys per query; q = 0, so every score is its table entry, exactly: the query's own key g above the
    others (p = 1), the 1023 others at p = e^-g ~ 1/4092, chosen where the fp16 hi / lo split of p loses the most (up to 2^-25: the lo
    plane is subnormal below 2^-3).  Every v is positive, so the losses add up over the keys."""
    g = _geom(1, 1, 32, 64, 1, 32, 64, 0, 0, 0, (1, 32, 32), (0, 0, 0), (1, 1), 1)
    N, C = 1024, 32
    g0 = math.log(4 * (N - 1))
    gap = float(max(np.float32(g0 + np.linspace(-0.05, 0.05, 4001)), key=lambda x: abs(_split_loss(math.exp(-float(x))))))
    gen = torch.Generator().manual_seed(12)
    qkv = torch.randn(1, 32 * 64, 3 * C, generator=gen, dtype=torch.float64)
    qkv[..., :C] = 0
    qkv[..., 2 * C:] = 1 + 0.1 * torch.rand(1, 32 * 64, C, generator=gen, dtype=torch.float64)
    qkv_b = torch.zeros(1, 3 * C, dtype=torch.float64)
    table = torch.zeros(1, 1, 1, N, N, dtype=torch.float64)
    table[..., torch.arange(N), torch.arange(N)] = gap
    qkv = qkv.float().double()
    scale = 1 / math.sqrt(32)
    ref = fw_attn_ref(qkv, qkv_b, table, g, scale)
    rc, out, n = run_fw_attn(qkv, qkv_b, table, g, scale)
    assert rc == 0 and out[n:].isnan().all()
    err = (out[:n].double().view(ref.shape) - ref).abs().max().item()
    bar = _fw_bar(qkv, qkv_b, table, g, scale)
    print(f"sharp softmax N={N} g={gap:.6f}: split loses {_split_loss(math.exp(-gap)):.3e} per key; max err {err:.3e}, bar {bar:.3e}")
    assert err <= bar


@GPU
def test_window_attention_argument_errors_leave_output_untouched():
    """C != 32 heads, N > 1024, a shift >= its window: SKFW_E_ARG; a window that does not tile the padded grid: SKFW_E_WINDOW."""
    base = _geom(1, 1, 33, 32, 1, 33, 32, 0, 0, 0, (1, 3, 4), (0, 0, 0), (1, 1), 2)
    scale = 1 / math.sqrt(32)
    for kw, want in ((dict(C=96), -1), (dict(win=(1, 33, 32)), -1), (dict(shift=(0, 3, 0)), -1), (dict(shift=(1, 0, 0)), -1),
                     (dict(shift=(0, 0, 4)), -1), (dict(win=(1, 4, 4)), -3)):
        g = dict(base)
        g.update({k: v for k, v in kw.items() if k != "C"})
        # inputs sized for the refused geometry itself (a table of N x N, rows of 3 C), so that nothing could be read out of bounds
        qkv, qkv_b, table = _fw_inputs(g, "rand", seed=3)
        if "C" in kw:
            qkv, qkv_b = torch.zeros(1, qkv.shape[1], 3 * kw["C"]), torch.zeros(1, 3 * kw["C"])
        rc, out, _ = run_fw_attn(qkv, qkv_b, table, g, scale, C=kw.get("C"))
        assert rc == want, kw
        assert out.isnan().all(), kw


@pytest.mark.parametrize("bias", ["relative", "earth_specific"])
@pytest.mark.parametrize("where", ["s0", "fuser"])
def test_attention_restatement_matches_reference(where, bias):
    """fw_attn_ref (the GPU cases' yardstick) against tests/_fengwu_reference.py's attention: a shifted toy block of an encoder (latitude
    padding in front) and of the fuser (the modality axis), both bias conventions; the qkv projection done here, the dense table from
    spec.py.  CPU only."""
    from skyrim_amd.fengwu.spec import FengwuConfig, bias_table, block_geometry, block_shift, init_synthetic, pad_to, window_types
    cfg = FengwuConfig(**TOY, bias=bias)
    p = init_synthetic(cfg, 4)
    grid, win, D, heads = block_geometry(cfg, where)
    if where == "fuser":
        Z, (H, W), prefix = cfg.n_mod, cfg.grid2, "fuser.1"
    else:
        Z, (H, W), prefix = 1, cfg.grid1, "enc.z.s0.1"
    s = block_shift(win, 1)
    x = torch.randn(Z, H, W, D, dtype=torch.float64, generator=torch.Generator().manual_seed(5))
    P = lambda n: torch.as_tensor(p[f"{prefix}.attn.{n}"]).double()          # noqa: E731
    qkv = (x.reshape(-1, D) @ P("qkv.weight").T + P("qkv.bias"))[None]
    types = window_types(cfg, grid, win, s)
    table = bias_table(cfg, P("bias_table"), grid, win, s)[None]
    g = _geom(1, Z, H, W, *grid, 0, pad_to(H, win[1], cfg.pad)[1], 0, win, s, types, heads)
    got = fw_attn_ref(qkv, P("qkv.bias")[None], table, g, 1 / math.sqrt(D // heads))
    ref = R.attention(p, cfg, prefix, x, where, 1).reshape(1, -1, D)
    assert (got - ref).abs().max().item() <= 1e-12 * ref.abs().max().item()


# ---- linear -------------------------------------------------------------------------------------------------------------------- #
# (id, batch, M, N, K, lda, k_split (0: one source), lda2, act, bias, res ("none" | "separate" | "alias"), expand (w_tok, h_out, front))
LIN_CASES = [
    ("cat-ksplit40-MN-tails-res-alias", 2, 130, 52, 104, 48, 40, 64, 1, True, "alias", None),
    ("cat-ksplit8-res-separate", 1, 77, 20, 24, 8, 8, 24, 0, False, "separate", None),
    ("one-source-lda-gt-K", 2, 129, 132, 40, 48, 0, 0, 1, True, "none", None),
    ("expand-front0-odd-h_out", 2, 20, 48, 32, 32, 0, 0, 0, True, "none", (5, 7, 0)),
    ("expand-front1-odd-h_out", 1, 30, 64, 40, 40, 0, 0, 0, False, "none", (6, 9, 1)),
]


@GPU
@pytest.mark.parametrize("case", LIN_CASES, ids=[c[0] for c in LIN_CASES])
def test_linear_against_float64(case):
    """skfw_linear over its loaders and epilogues: ALCat's second source from k_split (40: inside the second 32-wide k-step), the residual
    read from the output it overwrites, M and N tails, GELU, the patch expand's 2 x 2 shuffle with its row crop at odd h_out.  Bar: BAR3
    of max|ref| (GELU's slope is <= 1.13: x 1.2), plus one rounding of the residual add."""
    from skyrim_amd import native
    from skyrim_amd.fengwu.engine import LinearDesc
    _, B, M, N, K, lda, ks, lda2, act, has_bias, res, expand = case
    gen = torch.Generator().manual_seed(M * N + K)
    a = torch.randn(B, M, lda, generator=gen).float()
    a2 = torch.randn(B, M, lda2, generator=gen).float() if ks else None
    w = (torch.randn(B, N, K, generator=gen) / math.sqrt(K)).float()
    bias = (0.1 * torch.randn(B, N, generator=gen)).float() if has_bias else None
    A = torch.cat([a[..., :ks], a2[..., :K - ks]], -1).double() if ks else a[..., :K].double()
    acc = torch.einsum("bmk,bnk->bmn", A, w.double()) + (bias.double()[:, None, :] if has_bias else 0)
    if expand:
        w_tok, h_out, front = expand
        Co = N // 4
        h_tok = M // w_tok
        y = acc.view(B, h_tok, w_tok, 2, 2, Co).permute(0, 1, 3, 2, 4, 5).reshape(B, 2 * h_tok, 2 * w_tok, Co)
        ref = y[:, front:front + h_out].reshape(B, -1)
        o_sb = h_out * 2 * w_tok * Co
    else:
        ref = F.gelu(acc) if act else acc
        o_sb = M * N
    r = torch.randn(B, o_sb, generator=gen).float() if res != "none" else None
    if r is not None:
        ref = ref.reshape(B, -1) + r.double()
    ref = ref.reshape(B, -1)
    W = native.HiLoWeight(torch.device(DEV), _lib().skfw_prepare_weight, w)
    out = _nan(B * o_sb)
    if res == "alias":
        out[:B * o_sb] = _dev(r).reshape(-1)
    rd = out if res == "alias" else (_dev(r) if r is not None else None)
    ad, a2d = _dev(a), (_dev(a2) if ks else None)
    bd = _dev(bias) if has_bias else None
    p = lambda t: t.data_ptr() if t is not None else None          # noqa: E731
    w_tok, h_out, front = expand or (0, 0, 0)
    d = LinearDesc(ad.data_ptr(), p(a2d), W.buf.data_ptr(), W.plane, W.w_sb, W.ldw, p(bd), p(rd), out.data_ptr(), M * lda, M * lda2, o_sb,
                   N, B, M, N, K, lda, lda2, ks, act, 1 if expand else 0, w_tok, h_out, front)
    assert _lib().skfw_linear(ctypes.byref(d), _stream()) == 0
    o = out.cpu()
    assert o[B * o_sb:].isnan().all(), "written past the end of the output (a cropped row, or past the last one)"
    got = o[:B * o_sb].double().view(B, -1)
    assert torch.isfinite(got).all(), "an output element was not written"
    err = ((got - ref).abs().max() / ref.abs().max()).item()
    print(f"linear {case[0]}: rel err {err:.3e}")
    assert err <= 1.2 * BAR3 + U


# ---- LayerNorm ----------------------------------------------------------------------------------------------------------------- #
@GPU
@pytest.mark.parametrize("merge", [0, 1])
@pytest.mark.parametrize("C", [16, 144, 1040, 1536])
def test_layer_norm_against_float64(C, merge):
    """Two batch entries with their own gamma / beta, 21 rows each (4 k + 1), C up to 1536 (kLnVec's limit) and not a multiple of 256;
    rows at offsets 1e4 and -3e3.  merge = 1: the 2 x 2 gather from a 12 x 6 grid with one zero row in front and one behind.  FCN's bar:
    1e-5 of the row's max|ref| plus 16 u |mean| rstd max|gamma|."""
    from skyrim_amd.fengwu.engine import LnDesc
    B, rows, eps = 2, 21, 1e-5
    gen = torch.Generator().manual_seed(C + merge)
    if merge:
        h_src, w_src, front = 12, 6, 1
        cs = C // 4
        src = torch.randn(B, h_src, w_src, cs, generator=gen, dtype=torch.float64)
        src[0, 4, 2] += 1e4
        src[1, 7, :] -= 3e3
        src = src.float()
        xp = F.pad(src.double(), (0, 0, 0, 0, front, 2 * (rows // (w_src // 2)) - h_src - front))
        x = torch.cat([xp[:, 0::2, 0::2], xp[:, 1::2, 0::2], xp[:, 0::2, 1::2], xp[:, 1::2, 1::2]], -1).reshape(B, rows, C)
        xin = src
    else:
        h_src = w_src = front = 0
        x = torch.randn(B, rows, C, generator=gen, dtype=torch.float64) * torch.linspace(0.3, 3, rows, dtype=torch.float64)[:, None]
        x[0, 3] += 1e4
        x[1, 7] = 5 + 1e-3 * x[1, 7] / x[1, 7].std()
        x[1, 11] = 0.75
        x[0, rows - 1] -= 3e3
        x = x.float().double()
        xin = x
    g, b = 1 + 0.1 * torch.randn(B, C, generator=gen), 0.1 * torch.randn(B, C, generator=gen)
    g, b = g.float().double(), b.float().double()
    mean, var = x.mean(-1, keepdim=True), x.var(-1, unbiased=False, keepdim=True)
    rstd = 1 / torch.sqrt(var + eps)
    ref = (x - mean) * rstd * g[:, None] + b[:, None]
    xd, gd, bd = _dev(xin), _dev(g), _dev(b)
    out = _nan(B * rows * C)
    d = LnDesc(xd.data_ptr(), gd.data_ptr(), bd.data_ptr(), out.data_ptr(), rows, B, C, merge, h_src, w_src, front, eps)
    assert _lib().skfw_layer_norm(ctypes.byref(d), _stream()) == 0
    o = out.cpu()
    assert o[B * rows * C:].isnan().all(), "written past the last row"
    got = o[:B * rows * C].double().view(B, rows, C)
    assert torch.isfinite(got).all()
    err = (got - ref).abs().amax(-1)
    lim = 1e-5 * ref.abs().amax(-1) + 16 * U * g.abs().amax(-1)[:, None] * mean[..., 0].abs() * rstd[..., 0]
    assert (err <= lim).all(), (err / lim).max().item()


@GPU
def test_layer_norm_refuses_c_above_1536():
    from skyrim_amd.fengwu.engine import LnDesc
    x = torch.zeros(4 * 1552, device=DEV)
    g = torch.ones(1552, device=DEV)
    out = _nan(4 * 1552)
    for C, merge in ((1540, 0), (1552, 1)):
        d = LnDesc(x.data_ptr(), g.data_ptr(), g.data_ptr(), out.data_ptr(), 2, 1, C, merge, 4 if merge else 0, 2 if merge else 0, 0, 1e-5)
        assert _lib().skfw_layer_norm(ctypes.byref(d), _stream()) == -1
    torch.cuda.synchronize()
    assert out.isnan().all()


# ---- a toy call with pad = "back" ---------------------------------------------------------------------------------------------- #
@GPU
def test_toy_call_with_back_padding():
    """pad = "back": the input's 3 zero rows, the window padding and the merge's odd row all go behind the grid (front 0 everywhere).
    Against the restatement at the toy call's bar (1e-4)."""
    from skyrim_amd.fengwu.engine import FengwuEngine
    from skyrim_amd.fengwu.spec import FengwuConfig, init_synthetic, synthetic_state
    cfg = FengwuConfig(**TOY, pad="back")
    assert cfg.lat_pad == (36, 0) and cfg.merge_pad[1] == 0
    p = init_synthetic(cfg, 3)
    eng = FengwuEngine(cfg, DEV)
    eng.load_params(p)
    x0, x1 = synthetic_state(cfg, 0), synthetic_state(cfg, 1)
    y = eng.call(_dev(x0), _dev(x1))
    assert R.per_channel_err(y, R.call(p, cfg, x0, x1)).max().item() <= 1e-4
