"""FourCastNet v1 kernels of include/skyrim_fcn.h at the edges the step configs never reach, each against a float64 restatement: the
spectral filter (skfcn_spectral_run) on odd h, odd w, a kept Nyquist column, km = 1 and 768 channels; skfcn_layer_norm across widths,
ragged row counts, large offsets and a near-constant row; patch embedding and head at patch 8 with 26 channels; the spectral MLP at the
production shape (8 blocks, 46 modes, h = 90) with strides of a sub-array; the token MLP at tiny row counts.  Outputs start as a NaN
sentinel, so unwritten elements show."""
from __future__ import annotations

import pytest
import torch
import torch.nn.functional as F

import _fcn_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _engine(cfg, seed):
    from skyrim_amd.fcn.engine import FcnEngine
    from skyrim_amd.fcn.spec import init_synthetic
    p = init_synthetic(cfg, seed)
    eng = FcnEngine(cfg, DEV)
    eng.load_params(p)
    return eng, p


def _rel(a, b):
    return ((a.double() - b.double()).abs().max() / b.double().abs().max()).item()


# ---- the spectral filter ------------------------------------------------------------------------------------------------------- #
def _spectral_cfgs():
    from skyrim_amd.fcn.spec import FcnConfig
    return {
        "odd_h": FcnConfig(n_lat=36, n_lon=64, patch=4, embed_dim=192, depth=1, num_blocks=2),                        # h 9, w 16, km 5
        "odd_w": FcnConfig(n_lat=32, n_lon=100, patch=4, embed_dim=192, depth=1, num_blocks=2, kept_lon_modes=13),    # w 25: every mode
        "nyquist": FcnConfig(n_lat=32, n_lon=96, patch=4, embed_dim=192, depth=1, num_blocks=2, kept_lon_modes=13),   # w 24, m = 12 kept
        "km1": FcnConfig(n_lat=28, n_lon=48, patch=4, embed_dim=192, depth=1, num_blocks=2, kept_lon_modes=1),        # h 7, w 12
        "c768": FcnConfig(n_lat=40, n_lon=88, patch=8, embed_dim=768, depth=1, num_blocks=8, kept_lon_modes=6),       # h 5, w 11, nb 8
    }


@pytest.mark.parametrize("name", ["odd_h", "odd_w", "nyquist", "km1", "c768"])
def test_spectral_filter_against_float64(name):
    """FcnEngine.spectral (-> skfcn_spectral_run): t <- t + u + irfft2(MLP(rfft2(u))), u = LayerNorm1(t), in place.  The filter's part
    is checked on its own as well (got - t - u against the restatement's filter), so that a wrong mode cannot hide under the skips."""
    cfg = _spectral_cfgs()[name]
    if name == "nyquist":
        assert cfg.w % 2 == 0 and cfg.km == cfg.w // 2 + 1
    eng, p = _engine(cfg, 3)
    gen = torch.Generator().manual_seed(len(name))
    t = torch.randn(cfg.h, cfg.w, cfg.embed_dim, generator=gen) * 2 + 0.5
    td = t.to(DEV).reshape(-1).contiguous()
    eng.spectral(0, td)
    got = td.cpu().double().reshape(cfg.h, cfg.w, -1)
    q = {k: v.double() for k, v in p.items()}
    u = F.layer_norm(t.double(), (cfg.embed_dim,), q["blocks.0.norm1.weight"], q["blocks.0.norm1.bias"], cfg.eps)
    f = R.afno_filter(u, q["blocks.0.filter.w1"], q["blocks.0.filter.b1"], q["blocks.0.filter.w2"], q["blocks.0.filter.b2"], cfg)
    ref = t.double() + u + f
    assert torch.isfinite(got).all()
    assert _rel(got, ref) < 1e-5
    # the filter alone: what the fp32 rounding of the output (|t + u| ~ 10, half an ulp ~ 5e-7) leaves, relative to the filter's range
    err_f = (got - t.double() - u - f).abs().max().item()
    assert err_f < 1e-5 * f.abs().max().item() + 1e-6 * ref.abs().max().item(), (err_f, f.abs().max().item())


# ---- LayerNorm ----------------------------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize("C", [4, 192, 260, 768, 1024])
def test_layer_norm_against_float64(C):
    """Rows: random, a large common offset (1e3 +- 1), a near-constant row (5 +- 1e-3) and an exactly constant one; 4 rows per workgroup,
    so 4 k + 1 rows leave three wavefronts of the last workgroup idle.  Bar per row: 1e-5 max|ref| + 1e-6 |gamma| |mean| rstd: the fp32
    mean of a row at 1e3 is itself only good to ~6e-8 of 1e3."""
    from skyrim_amd import ops
    gen = torch.Generator().manual_seed(C)
    rows = 4 * 5 + 1
    x = torch.randn(rows, C, generator=gen, dtype=torch.float64) * torch.linspace(0.3, 3, rows, dtype=torch.float64)[:, None]
    x[3] += 1e3
    x[7] = 5 + 1e-3 * x[7] / x[7].std()
    x[11] = 0.75
    x = x.float()
    g, b = 1 + 0.1 * torch.randn(C, generator=gen), 0.1 * torch.randn(C, generator=gen)
    out = torch.full((rows + 1, C), float("nan"), device=DEV)
    ops.hip.fcn_layer_norm(x.to(DEV), g.to(DEV), b.to(DEV), out, rows, C, 1e-6)
    got = out.cpu().double()
    assert got[rows].isnan().all(), "a row beyond `rows` was written"
    got = got[:rows]
    xd = x.double()
    mean, var = xd.mean(1, keepdim=True), xd.var(1, unbiased=False, keepdim=True)
    rstd = 1 / torch.sqrt(var + 1e-6)
    ref = (xd - mean) * rstd * g.double() + b.double()
    assert torch.isfinite(got).all()
    err = (got - ref).abs().amax(1)
    lim = 1e-5 * ref.abs().amax(1) + 1e-6 * g.double().abs().max() * mean[:, 0].abs() * rstd[:, 0]
    assert (err <= lim).all(), (err / lim)
    assert torch.allclose(got[11], b.double(), rtol=0, atol=1e-6)      # a constant row normalises to beta


# ---- patch embedding and head at patch 8 --------------------------------------------------------------------------------------- #
@pytest.fixture(scope="module")
def p8():
    from skyrim_amd.fcn.spec import FcnConfig
    cfg = FcnConfig(n_lat=32, n_lon=64, patch=8, embed_dim=192, depth=1, num_blocks=2)
    assert cfg.in_chans == cfg.out_chans == 26
    eng, p = _engine(cfg, 13)
    return cfg, p, eng


def test_patch_embed_patch8_26_channels(p8):
    """K = 26 x 8 x 8 = 1664: every k-chunk of 8 is one patch row (the loader's P == 8 gather), raw state of physical magnitudes."""
    from skyrim_amd.fcn.spec import synthetic_state
    cfg, p, eng = p8
    x = synthetic_state(cfg, 2)
    out = torch.full((cfg.tokens * cfg.embed_dim + 5,), float("nan"), device=DEV)
    eng.patch_embed(x.to(DEV), out)
    got = out.cpu()
    assert got[cfg.tokens * cfg.embed_dim:].isnan().all()
    q = {k: v.double() for k, v in p.items()}
    xn = (x.double() - q["norm.mean"][:, None, None]) / q["norm.std"][:, None, None]
    ref = F.conv2d(xn[None], q["patch_embed.proj.weight"], q["patch_embed.proj.bias"], stride=cfg.patch)[0].permute(1, 2, 0).reshape(cfg.tokens, -1)
    ref = ref + q["pos_embed"].reshape(cfg.tokens, -1)
    assert _rel(got[:cfg.tokens * cfg.embed_dim].reshape(cfg.tokens, -1), ref) < 1e-5


def test_head_patch8_26_channels(p8):
    """N = 8 x 8 x 26 = 1664 columns scattered into (26, 32, 64), de-normalisation folded in; every output element written."""
    cfg, p, eng = p8
    g = torch.Generator().manual_seed(7)
    t = torch.randn(cfg.tokens, cfg.embed_dim, generator=g)
    y = torch.full((cfg.out_chans, cfg.n_lat, cfg.n_lon), float("nan"), device=DEV)
    eng.head(t.to(DEV).contiguous(), y)
    q = {k: v.double() for k, v in p.items()}
    P, co = cfg.patch, cfg.out_chans
    r = F.linear(t.double(), q["head.weight"]).reshape(cfg.h, cfg.w, P, P, co).permute(4, 0, 2, 1, 3).reshape(co, cfg.n_lat, cfg.n_lon)
    ref = r * q["norm.std"][:, None, None] + q["norm.mean"][:, None, None]
    got = y.cpu()
    assert torch.isfinite(got).all()
    # per channel, relative to the channel's spread around its mean (the mean ~1e5 of pressure would hide the product otherwise)
    err = (got.double() - ref).abs().flatten(1).amax(1) / (r * q["norm.std"][:, None, None]).abs().flatten(1).amax(1)
    assert err.max().item() < 1e-5, err


# ---- the spectral MLP at the production shape ---------------------------------------------------------------------------------- #
def _spectral_mlp_case(lam):
    from skyrim_amd import ops
    from skyrim_amd.fcn.engine import _Pairs, FcnEngine, complex_block_matrices
    from skyrim_amd.fcn.spec import FcnConfig
    g = torch.Generator().manual_seed(11)
    nb, bs, h, km = 8, 96, 90, 46
    C = nb * bs
    w1, w2 = 0.03 * torch.randn(2, nb, bs, bs, generator=g), 0.05 * torch.randn(2, nb, bs, bs, generator=g)
    b1, b2 = 0.05 * torch.randn(2, nb, bs, generator=g), 0.05 * torch.randn(2, nb, bs, generator=g)
    # the modes of a sub-array: z[f][ri][m][C + 8] with the channels at offset 4 of each row (sm = C + 8, sm2 = 2 km (C + 8),
    # im_off = km (C + 8)); the padding around them must stay untouched
    sm = C + 8
    z = torch.randn(h, 2, km, sm, generator=g)
    z0 = z.clone()
    eng = FcnEngine(FcnConfig(n_lat=720, n_lon=1440, patch=8, embed_dim=C, num_blocks=nb, depth=1), DEV)
    w1e, b1e = complex_block_matrices(w1, b1)
    w2e, b2e = complex_block_matrices(w2, b2)
    pr = _Pairs(eng, w1e, w2e)
    zd = z.to(DEV).contiguous()
    flat = zd.view(-1)[4:]
    ops.hip.fcn_spectral_mlp(flat, pr.w1f, pr.w2f, b1e.float().to(DEV), b2e.float().to(DEV), [h * km, km, sm, 2 * km * sm, km * sm, nb], lam)
    got = zd.cpu()
    U = torch.complex(z0[:, 0, :, 4:4 + C].double(), z0[:, 1, :, 4:4 + C].double()).reshape(h, km, nb, bs)
    S = R.spectral_mlp(U, w1.double(), b1.double(), w2.double(), b2.double(), lam).reshape(h, km, C)
    pad = torch.ones(sm, dtype=torch.bool)
    pad[4:4 + C] = False
    assert torch.equal(got[..., pad], z0[..., pad]), "the padding around the channels was written"
    S0 = R.spectral_mlp(U, w1.double(), b1.double(), w2.double(), b2.double(), 0.0).reshape(h, km, C)
    return got[:, 0, :, 4:4 + C], got[:, 1, :, 4:4 + C], S, S0


@pytest.mark.parametrize("lam", [0.0, 0.08])
def test_spectral_mlp_production_shape(lam):
    re, im, S, S0 = _spectral_mlp_case(lam)
    zeroed = ((S.real == 0).double().mean() + (S.imag == 0).double().mean()).item() / 2
    if lam > 0:
        assert 0.1 < zeroed < 0.9, zeroed             # softshrink zeroes a visible fraction
    else:
        assert zeroed == 0.0
    scale = max(S.real.abs().max().item(), S.imag.abs().max().item())
    assert (re.double() - S.real).abs().max().item() < 1e-5 * scale and (im.double() - S.imag).abs().max().item() < 1e-5 * scale
    if lam > 0:                                         # softshrink gives exact zeros where the value is well inside the threshold
        inside = S0.real.abs() < 0.5 * lam
        assert inside.any() and (re.double()[inside] == 0).all()


# ---- the token MLP at tiny row counts ------------------------------------------------------------------------------------------ #
@pytest.mark.parametrize("C", [192, 768])
@pytest.mark.parametrize("rows", [1, 15, 17])
def test_token_mlp_small_row_counts(C, rows):
    from skyrim_amd import ops
    from skyrim_amd.fcn.engine import _Pairs, FcnEngine
    from skyrim_amd.fcn.spec import FcnConfig
    g = torch.Generator().manual_seed(C + rows)
    hid = 4 * C
    x = torch.randn(rows, C, generator=g) * 3 + 1
    w1, w2 = torch.randn(hid, C, generator=g) * C ** -0.5, torch.randn(C, hid, generator=g) * hid ** -0.5
    b1, b2 = torch.randn(hid, generator=g) * 0.1, torch.randn(C, generator=g) * 0.1
    gm, bt = 1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    eng = FcnEngine(FcnConfig(n_lat=16, n_lon=48, patch=4, embed_dim=C, num_blocks=C // 96), DEV)
    pr = _Pairs(eng, w1, w2)
    out = torch.full((rows + 16, C), float("nan"), device=DEV)
    ops.hip.fcn_mlp(x.to(DEV), pr.w1f, pr.w2f, b1.to(DEV), b2.to(DEV), gm.to(DEV), bt.to(DEV), out, rows, C, hid, 1e-6)
    got = out.cpu()
    assert got[rows:].isnan().all(), "a row beyond `rows` was written"
    xd = x.double()
    v = F.layer_norm(xd, (C,), gm.double(), bt.double(), 1e-6)
    ref = xd + F.linear(F.gelu(F.linear(v, w1.double(), b1.double())), w2.double(), b2.double())
    assert _rel(got[:rows], ref) < 1e-5
