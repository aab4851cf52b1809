"""``ensemble_forecast(perturbation="spherical")`` end to end on the MI355X: Pangu at 49 x 192 and FuXi at its toy size (two history
levels), the control member, the lead-0 members against the float64 restatement of the field, batching and seeds, ``perturb_channels``,
white noise unchanged, FourCastNet's 720-row style crop, and the scores."""
from __future__ import annotations

import datetime

import numpy as np
import pytest
import torch

import _noise_reference as NR
from skyrim_amd import noise as N

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T0 = datetime.datetime(2024, 5, 13, 18, 0)
FUXI_TOY = dict(n_lat=73, n_lon=144, channels=6, embed=128, heads=2, depth=2, window=(3, 6))
SCALE = 1e-3


@pytest.fixture(scope="module")
def pangu(toy):
    from skyrim_amd.core.models.pangu import PanguModel
    g, params, _ = toy
    return PanguModel(ic_source="gfs", geom=g, params=params)


@pytest.fixture(scope="module")
def fuxi():
    from skyrim_amd.core.models.fuxi import FuxiModel
    from skyrim_amd.fuxi.spec import FuxiConfig, init_synthetic
    cfg = FuxiConfig(**FUXI_TOY, cascade_steps=(1, 2))
    return FuxiModel(ic_source="synthetic", cfg=cfg, params=init_synthetic(cfg, 11), device=DEV)


def _spherical(m, **kw):
    kw = dict(dict(n_steps=1, n_members=5, seed=3, keep_members=True, perturbation="spherical"), **kw)
    return m.ensemble_forecast(T0, **kw)


def _lead0_check(m, ens, lmax, members=(1, 4)):
    """x_m - x_0 at lead 0 against g[c] y with y from the float64 restatement: within g times (the synthesis bound + the coefficients' bound
    carried through the synthesis) plus the one rounding of the fma, 2^-24 |x_m|."""
    from skyrim_amd import ensemble as E
    loop = m.model
    names_in, names_out = list(loop.in_channel_names), ens.members.channel.values.tolist()
    C, L = len(names_in), loop.n_history_levels
    n_lat, n_lon = len(loop.grid.lat), len(loop.grid.lon)
    n_full = N.full_grid(loop.grid.lat, loop.grid.lon)
    sigma = N.spectrum(lmax)
    e = N.scale_exponent(sigma)
    table = (sigma * 2.0 ** e).astype(np.float32)
    std = E.channel_std(loop).cpu().numpy().astype(np.float64)
    g = (std * SCALE * 2.0 ** -e).astype(np.float32).astype(np.float64)
    P = NR.legendre(lmax, n_full, n_lat)
    mem = np.asarray(ens.members.values)[:, 0].astype(np.float64)              # (M, C_out, H, W) at lead 0
    common = [c for c in names_out if c in names_in]
    assert len(common) >= min(C, len(names_out)) // 2
    fields = np.array([(L - 1) * C + names_in.index(c) for c in common])       # the newest history level is what lead 0 shows
    worst = 0.0
    for k in members:
        a, b = NR.coefficients(ens.seed, k, fields, lmax, table)
        y, S, Q = NR.synthesize(a, P, n_lon)
        Sb = NR.synthesize(b, P, n_lon)[1]
        for i, c in enumerate(common):
            gc = g[names_in.index(c)]
            d = mem[k, names_out.index(c)] - mem[0, names_out.index(c)]
            bound = gc * (NR.U * (NR.k_bound(lmax) * S[i] + Q[i]) + Sb[i]) + NR.U * np.abs(mem[k, names_out.index(c)])
            err = np.abs(d - gc * y[i])
            worst = max(worst, float((err / bound).max()))
            assert np.all(err <= bound), (k, c, float((err / bound).max()))
    print(f"{ens.model_name} lead 0: x_m - x_0 against g y, max err / bound {worst:.3f}")
    return std, common, names_in, names_out, sigma, n_full


def _spread_check(ens, std, common, names_in, names_out, sigma, n_full, n_lat, n_lon):
    """Area mean of the lead-0 spread^2 per channel.  Members are x_0 (the control, d_0 = 0) and x_0 + d_m, d_m = g y_m iid: per point
    M spread^2 = sum_m (d_m - dbar)^2 = g^2 (chi^2_{M-2} + chi^2_1 / M), between g^2 chi^2_{M-2} and g^2 chi^2_{M-1}.  The area mean over a
    correlated field counts n_eff = 1 / sum_pq w_p w_q C(gamma_pq)^2 independent points (Isserlis: the variance of a weighted mean of squares
    of a unit Gaussian field is 2 sum w w C^2), from the exact covariance on this grid.  Bars: the 1e-6 quantiles of chi^2 with
    (M - 2) n_eff degrees of freedom below and (M - 1) n_eff above."""
    M = ens.n_members
    w = np.repeat(NR.area_weights(n_full, n_lat) / n_lon, n_lon)
    n_eff = 1.0 / NR.square_mean_variance(sigma, n_full, n_lat, n_lon)
    lo = NR.chi2_quantiles((M - 2) * n_eff)[0] * (M - 2)
    hi = NR.chi2_quantiles((M - 1) * n_eff)[1] * (M - 1)
    sp = np.asarray(ens.spread.values)[0].astype(np.float64)
    for c in common:
        amp = SCALE * std[names_in.index(c)]
        T = M * float((w * (sp[names_out.index(c)] ** 2).reshape(-1)).sum()) / amp ** 2
        assert lo <= T <= hi, (c, T, lo, hi, n_eff)
    print(f"{ens.model_name}: lead-0 spread within the chi^2 bars ({lo:.3f} .. {hi:.3f} of (perturb_scale sigma_c)^2 / M, n_eff {n_eff:.1f})")


@pytest.mark.parametrize("which", ["pangu", "fuxi"])
def test_spherical_members(which, request):
    m = request.getfixturevalue(which)
    before = np.array(m.forecast(T0, n_steps=1).values)
    ens = _spherical(m, products=("mean", "spread"))
    loop = m.model
    n_lat, n_lon = len(loop.grid.lat), len(loop.grid.lon)
    lmax = N.default_lmax(N.full_grid(loop.grid.lat, loop.grid.lon), n_lon)
    assert (ens.perturbation, ens.lmax, ens.length_scale_km, ens.alpha) == ("spherical", lmax, 500.0, 2.0)
    mem = np.asarray(ens.members.values)
    assert np.array_equal(mem[0], before)                                      # the control member: forecast, bit for bit
    assert all(not np.array_equal(mem[k], mem[0]) for k in range(1, 5)) and np.isfinite(mem).all()
    info = _lead0_check(m, ens, lmax)
    _spread_check(ens, *info, n_lat, n_lon)
    eight = np.asarray(_spherical(m, n_members=8).members.values)
    assert np.array_equal(eight[3], mem[3]) and np.array_equal(eight[:5], mem)   # a member's bits do not depend on the ensemble size
    assert np.array_equal(np.asarray(_spherical(m).members.values), mem)        # one seed: the same bits
    other = np.asarray(_spherical(m, seed=4).members.values)
    assert np.array_equal(other[0], mem[0]) and all(not np.array_equal(other[k], mem[k]) for k in range(1, 5))
    after = np.array(m.forecast(T0, n_steps=1).values)
    assert np.array_equal(after, before)


@pytest.mark.parametrize("kind", ["spherical", "white"])
def test_perturb_channels(pangu, kind):
    names = list(pangu.model.in_channel_names)
    one = names[5]
    ens = pangu.ensemble_forecast(T0, n_steps=0, n_members=4, keep_members=True, perturbation=kind, perturb_channels=[one])
    mem = np.asarray(ens.members.values)[:, 0]
    out = ens.members.channel.values.tolist()
    for c in out:
        same = [np.array_equal(mem[k, out.index(c)], mem[0, out.index(c)]) for k in range(1, 4)]
        assert all(same) if c != one else not any(same), c


def test_white_noise_is_unchanged(pangu):
    kw = dict(n_steps=1, n_members=3, seed=2, keep_members=True, products=("mean", "spread"))
    plain = pangu.ensemble_forecast(T0, **kw)
    white = pangu.ensemble_forecast(T0, perturbation="white", length_scale_km=123.0, lmax=5, **kw)
    assert np.array_equal(np.asarray(plain.members.values), np.asarray(white.members.values))
    assert np.array_equal(plain.spread.values, white.spread.values) and white.perturbation == "white" and white.lmax is None
    every = pangu.ensemble_forecast(T0, perturb_channels=list(pangu.model.in_channel_names), **kw)
    assert np.array_equal(np.asarray(plain.members.values), np.asarray(every.members.values))


def test_cropped_grid_and_lmax(pangu):
    """The crop path end to end needs a model on the first rows of a pole-to-pole grid; the toys of this suite are all pole-to-pole, so the
    crop runs through ``Perturber`` on a 48-row state of the 49-row grid (FourCastNet's 720 of 721), and ``lmax`` through the model."""
    from skyrim_amd.core.models.pangu import PanguModel   # noqa: F401
    ens = _spherical(pangu, n_steps=0, n_members=2, lmax=12, length_scale_km=1500.0)
    assert ens.lmax == 12 and ens.length_scale_km == 1500.0
    x0 = torch.randn(1, 2, 3, 48, 192, device=DEV)
    std = torch.tensor([1.0, 10.0, 0.01], device=DEV)
    model = type("M", (), dict(grid=type("G", (), dict(lat=[90.0 - 3.75 * i for i in range(48)], lon=[1.875 * j for j in range(192)])),
                               in_channel_names=["a", "b", "c"]))
    p = N.plan(model, "spherical", lmax=20)
    assert (p.n_lat, p.n_lat_full) == (48, 49)
    pert = N.Perturber(p, x0, std, 1e-2, 1)
    out = torch.empty_like(x0)
    pert.member(0, out)
    assert torch.equal(out, x0)
    pert.member(2, out)
    d = (out - x0).double().cpu().numpy()[0]                                    # (L, C, 48, 192)
    table = (p.sigma * 2.0 ** p.e).astype(np.float32)
    a, b = NR.coefficients(1, 2, np.arange(6), 20, table)
    P = NR.legendre(20, 49, 48)
    y, S, Q = NR.synthesize(a, P, 192)
    Sb = NR.synthesize(b, P, 192)[1]
    g = np.tile((std.cpu().numpy().astype(np.float64) * 1e-2 * 2.0 ** -p.e).astype(np.float32).astype(np.float64), 2)
    bound = g[:, None, None] * (NR.U * (NR.k_bound(20) * S + Q) + Sb) + NR.U * np.abs(out.double().cpu().numpy()[0].reshape(6, 48, 192))
    assert np.all(np.abs(d.reshape(6, 48, 192) - g[:, None, None] * y) <= bound)


def test_scores_with_spherical_noise(pangu):
    ens = _spherical(pangu, n_members=4, keep_members=False, products=(), scores=True)
    table = ens.scores.table
    ssr = table.values[table.metric.values.tolist().index("ssr")]              # (time, channel)
    assert np.isfinite(ssr[1:]).all() and (ssr[1:] > 0).all()
