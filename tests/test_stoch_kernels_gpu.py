"""The stochastic-perturbation kernels on the MI355X against tests/_stoch_reference.py: ``stoch_coeffs`` (draw 0 is ``noise_coeffs`` bit
for bit; later draws element by element within the bound of include/skyrim_noise.h, bits independent of batching), ``stoch_evolve`` bit
for bit over a chain of draws, the statistics of the evolving state against derived bars, and ``stoch_apply`` bit for bit on both paths."""
from __future__ import annotations

import math

import numpy as np
import pytest
import torch

import _noise_reference as NR
import _stoch_reference as SR
from skyrim_amd import noise as N
from skyrim_amd import stochastic as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _table(lmax: int):
    """(float32 table sigma_l 2^e as the device holds it, e) of the default spectrum; lmax 1 has degree 0 alone."""
    if lmax < 2:
        return np.zeros(1, np.float32), 0
    s = N.spectrum(lmax)
    e = N.scale_exponent(s)
    return (s * 2.0 ** e).astype(np.float32), e


def _coeffs(table, F, seed, member_first, n, draw, f_first=0):
    from skyrim_amd import ops
    lmax = len(table)
    out = torch.full((n * lmax * lmax * 2 * F,), float("nan"), dtype=torch.float32, device=DEV)      # the kernel writes its zeros itself
    ops.hip.stoch_coeffs(out, torch.from_numpy(table).to(DEV), F, f_first, seed, member_first, draw)
    return out.cpu().numpy().reshape(n, lmax, lmax, 2, F)


# ---- skstoch_coeffs ----------------------------------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize("F,lmax", SR.COEFF_SHAPES + ((70, 8),))
def test_draw_0_is_noise_coeffs(F, lmax):
    table, _ = _table(lmax)
    ref = torch.full((2 * lmax * lmax * 2 * F,), float("nan"), dtype=torch.float32, device=DEV)
    N.coeffs(ref, torch.from_numpy(table).to(DEV), F, 3, 9, 1)
    got = _coeffs(table, F, 9, 1, 2, 0, f_first=3)
    assert np.array_equal(got.reshape(-1).view(np.uint32), ref.cpu().numpy().view(np.uint32))


@pytest.mark.parametrize("F,lmax", SR.COEFF_SHAPES)
def test_coeffs_against_the_restatement(F, lmax):
    table, _ = _table(lmax)
    worst, seen = 0.0, []
    for draw in SR.DRAWS:
        got = _coeffs(table, F, 9, 1, 2, draw)
        for j, member in enumerate((1, 2)):
            ref, bound = SR.coefficients(9, member, np.arange(F), lmax, table, draw)
            dead = bound == 0
            assert np.all(got[j].view(np.uint32)[dead] == 0)                   # l = 0, m > l, Im a_l0: +0, bit for bit
            err = np.abs(got[j].astype(np.float64) - ref)
            assert np.all(err[~dead] <= bound[~dead])
            if (~dead).any():
                worst = max(worst, float((err[~dead] / bound[~dead]).max()))
                assert np.all(got[j][~dead] != 0)
        if lmax > 1:
            assert all(not np.array_equal(got, o) for o in seen)                # different draws differ
        seen.append(got)
    print(f"coeffs F={F} lmax={lmax}: max err / bound {worst:.3f}")


@pytest.mark.parametrize("draw", [1, 2 ** 32 - 2])
def test_coeff_bits_do_not_depend_on_batching(draw):
    table, _ = _table(32)
    F = 7
    six = _coeffs(table, F, 4, 1, 6, draw)
    parts = np.concatenate([_coeffs(table, F, 4, 1, 1, draw), _coeffs(table, F, 4, 2, 2, draw), _coeffs(table, F, 4, 4, 3, draw)])
    assert np.array_equal(six.view(np.uint32), parts.view(np.uint32))
    fields = np.concatenate([_coeffs(table, 3, 4, 1, 6, draw), _coeffs(table, 4, 4, 1, 6, draw, f_first=3)], axis=-1)
    assert np.array_equal(six.view(np.uint32), fields.view(np.uint32))
    small = _coeffs(table[:9].copy(), F, 4, 1, 6, draw)                         # a caller with a smaller lmax: the common coefficients
    assert np.array_equal(small.view(np.uint32), six[:, :9, :9].view(np.uint32))
    assert not np.array_equal(_coeffs(table, F, 5, 1, 1, draw), six[:1]) and not np.array_equal(six[0], six[1])


# ---- skstoch_evolve ----------------------------------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize("F,lmax", SR.COEFF_SHAPES)
def test_evolve_is_one_fma_per_element(F, lmax):
    """A chain of three draws for two members, batched in one call and member by member: after every step the state is
    fma32(phi, p, fl32(psi * fresh)) of the state before, bit for bit, with ``fresh`` the device's own ``coeffs`` of that draw."""
    from skyrim_amd import ops
    table, _ = _table(lmax)
    sig = torch.from_numpy(table).to(DEV)
    phi, psi = S.ar1(6.0, 6.0)
    p = torch.from_numpy(_coeffs(table, F, 9, 1, 2, 1).reshape(-1)).to(DEV)
    single = p[p.numel() // 2:].clone()                                        # member 2 alone, through its own calls
    host = p.cpu().numpy()
    dead = np.broadcast_to(~SR.live_mask(lmax)[None, :, :, :, None], (2, lmax, lmax, 2, F)).reshape(-1)
    for draw in (2, 3, 2 ** 32 - 2):
        fresh = _coeffs(table, F, 9, 1, 2, draw).reshape(-1)
        ops.hip.stoch_evolve(p, sig, F, 0, 9, 1, draw, phi, psi)
        ops.hip.stoch_evolve(single, sig, F, 0, 9, 2, draw, phi, psi)
        want = SR.evolve(host, fresh, phi, psi)
        got = p.cpu().numpy()
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), draw
        assert np.all(got.view(np.uint32)[dead] == 0)                           # structural zeros stay +0
        assert np.array_equal(single.cpu().numpy().view(np.uint32), got[got.size // 2:].view(np.uint32))
        if lmax > 1:
            assert not np.array_equal(got, host) and np.all(got[~dead] != 0)
        host = got
    fresh = _coeffs(table, F, 9, 1, 2, 7).reshape(-1)
    ops.hip.stoch_evolve(p, sig, F, 0, 9, 1, 7, 0.0, 1.0)                      # tau = 0: the fresh draw itself
    got = p.cpu().numpy()
    assert np.all(got == fresh) and np.all(got.view(np.uint32)[dead] == 0)
    ops.hip.stoch_evolve(p, sig, F, 0, 9, 1, 8, -0.5, 0.0)                     # a negative phi keeps the zeros +0 as well
    assert np.all(p.cpu().numpy().view(np.uint32)[dead] == 0)


def test_evolving_state_statistics():
    """33 x 64 grid's lmax 32, F = 64 fields of one member, 8 steps at phi = fl32(e^-1) (seed fixed: deterministic).  Bars derived, at
    1e-6 per comparison:
    * every live coefficient of step 7 against the same one of step 8, each divided by its own standard deviation (sigma_l 2^e, times
      sqrt(1/2) for m >= 1): N = (lmax^2 - 1) F independent pairs of unit normals with correlation phi exactly (p_8 = phi p_7 + psi a,
      phi^2 + psi^2 = 1), so atanh of the sample correlation lies within ``fisher_bar(N)`` of atanh(phi);
    * per degree l, the Hermitian-weighted power of step 8 summed over orders and fields is sigma_l^2 (2^e)^2 chi^2 with (2 l + 1) F
      degrees of freedom: the stationary variance is that of a draw.
    The fp32 roundings of the state (2^-24 relative per step) are four orders of magnitude below either bar."""
    from skyrim_amd import ops
    lmax, F, seed, steps = 32, 64, 2025, 8
    table, e = _table(lmax)
    sig = torch.from_numpy(table).to(DEV)
    phi, psi = S.ar1(1.0, 1.0)
    p = torch.empty(lmax * lmax * 2 * F, dtype=torch.float32, device=DEV)
    ops.hip.stoch_coeffs(p, sig, F, 0, seed, 1, 1)
    prev = None
    for k in range(2, steps + 1):
        prev = p.cpu().numpy().astype(np.float64).reshape(lmax, lmax, 2, F)
        ops.hip.stoch_evolve(p, sig, F, 0, seed, 1, k, phi, psi)
    last = p.cpu().numpy().astype(np.float64).reshape(lmax, lmax, 2, F)
    live = SR.live_mask(lmax)
    sd = table.astype(np.float64)[:, None, None] * np.where(np.arange(lmax) == 0, 1.0, math.sqrt(0.5))[None, :, None] * np.ones((1, 1, 2))
    sd = np.where(live, sd, 1.0)
    a, b = (prev / sd[..., None])[live].reshape(-1), (last / sd[..., None])[live].reshape(-1)
    n = a.size
    assert n == (lmax * lmax - 1) * F
    a, b = a - a.mean(), b - b.mean()
    r = float((a * b).sum() / math.sqrt((a * a).sum() * (b * b).sum()))
    bar = NR.fisher_bar(n)
    print(f"lag-1 correlation {r:.5f} against phi {phi:.5f}: |d atanh| / bar {abs(math.atanh(r) - math.atanh(phi)) / bar:.3f} (N = {n})")
    assert abs(math.atanh(r) - math.atanh(phi)) <= bar
    power = (last ** 2).sum(axis=2)                                             # [l][m][F]
    tot = power[:, 0].sum(axis=-1) + 2.0 * power[:, 1:].sum(axis=(1, 2))
    worst = 0.0
    for l in range(1, lmax):
        nu = (2 * l + 1) * F
        lo, hi = NR.chi2_quantiles(nu)
        ratio = tot[l] / (nu * float(table[l]) ** 2)
        worst = max(worst, (ratio - 1) / (hi - 1), (1 - ratio) / (1 - lo))
        assert lo <= ratio <= hi, (l, ratio, lo, hi)
    assert tot[0] == 0
    print(f"variance per degree at step {steps}: worst use of the chi^2 bar {worst:.3f} (e = {e})")


# ---- skstoch_apply ------------------------------------------------------------------------------------------------------------------------ #
@pytest.mark.parametrize("kind", ["sppt", "additive", "both"])
@pytest.mark.parametrize("offset", [0, 1, 3])
@pytest.mark.parametrize("L,C,hw", SR.APPLY_SHAPES)
def test_apply_against_the_restatement(L, C, hw, offset, kind):
    from skyrim_amd import ops
    xp, xn, r, y, gs, ga = SR.apply_inputs(L, C, hw)
    n = xn.size
    off = np.repeat(np.tile((gs == 0) & (ga == 0), L), hw)                      # channels with both amplitudes 0 ...
    y = y.copy()
    y[off] = np.nan                                                             # ... are bit copies whatever y holds
    if kind == "sppt":
        y = ga = None
    if kind == "additive":
        r = gs = None
    if r is not None:
        if hw >= 500:                                                           # the clip is active on both sides for a known share:
            w = np.tile(gs, L)[:, None] * r[None, :]                            # fl32(gs r) ~ N(0, 0.6^2), so P(w > 0.9) = P(z > 1.5) = 6.7 %
            on = np.tile(gs, L) != 0
            hi, lo = float((w[on] > SR.LIM).mean()), float((w[on] < -SR.LIM).mean())
            assert 0.04 <= hi <= 0.10 and 0.04 <= lo <= 0.10, (hi, lo)
        r = r.copy()
        r[::97] = np.nan                # whatever the pattern holds: a bit copy where gs is 0, and w = -lim elsewhere (fmaxf drops the NaN)
    want = SR.apply(xp, xn, r, y, gs, ga, SR.LIM, C, hw)
    assert np.isfinite(want).all()
    dev = lambda a: None if a is None else torch.cat([torch.zeros(offset, dtype=torch.float32), torch.from_numpy(a)]).to(DEV)[offset:]      # noqa: E731
    dxp, dy, dr = dev(xp), dev(y), dev(r)
    dgs, dga = (None if g is None else torch.from_numpy(g).to(DEV) for g in (gs, ga))
    out = torch.full((offset + n + 4,), float("nan"), dtype=torch.float32, device=DEV)
    ops.hip.stoch_apply(dxp if r is not None else None, dev(xn), dr, dy, dgs, dga, SR.LIM, out[offset:offset + n], hw)
    got = out.cpu().numpy()
    assert np.array_equal(got[offset:offset + n].view(np.uint32), want.view(np.uint32))
    assert np.isnan(got[:offset]).all() and np.isnan(got[offset + n:]).all()    # nothing outside the range is written
    both_off = off if kind == "both" else np.repeat(np.tile((gs if kind == "sppt" else ga) == 0, L), hw)
    assert np.array_equal(got[offset:offset + n][both_off].view(np.uint32), xn[both_off].view(np.uint32))
    assert C < 3 or both_off.any()
    inplace = torch.cat([torch.zeros(offset, dtype=torch.float32), torch.from_numpy(xn), torch.full((4,), float("nan"))]).to(DEV)
    ops.hip.stoch_apply(dxp if r is not None else None, inplace[offset:offset + n], dr, dy, dgs, dga, SR.LIM, inplace[offset:offset + n], hw)
    res = inplace.cpu().numpy()
    assert np.array_equal(res[offset:offset + n].view(np.uint32), want.view(np.uint32)) and np.isnan(res[offset + n:]).all()     # out == xn


def test_apply_refuses_what_the_header_refuses():
    x = torch.zeros(12, dtype=torch.float32, device=DEV)
    one, g = torch.zeros(4, dtype=torch.float32, device=DEV), torch.ones(3, dtype=torch.float32, device=DEV)
    with pytest.raises(ValueError, match="xp"):
        S.apply(x, x.clone(), one, None, g, None, 0.9, x, 4)                   # out is xp
    with pytest.raises(ValueError, match="lim"):
        S.apply(x, x.clone(), one, None, g, None, 1.5, x.clone(), 4)
    with pytest.raises(ValueError, match="one of the two terms"):
        S.apply(x, x.clone(), None, None, None, None, 0.9, x.clone(), 4)
    with pytest.raises(ValueError, match="draw"):
        S.coeffs(torch.zeros(8, dtype=torch.float32, device=DEV), torch.ones(2, dtype=torch.float32, device=DEV), 1, 0, 0, 1, 2 ** 32 - 1)
