"""``ensemble_forecast(stochastic=...)`` end to end on the MI355X, on the toy Pangu (49 x 192): ``stochastic=None``, the control member,
spread from the stochastic terms alone, seeds, a member's step re-derived from the device's own states for each kind, ``channels``, the
scores, and breeding together with it."""
from __future__ import annotations

import datetime

import numpy as np
import pytest
import torch

import _stoch_reference as SR
from skyrim_amd import noise as N
from skyrim_amd import stochastic as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T0 = datetime.datetime(2024, 5, 13, 18, 0)
SCALE = 1e-3
KW = dict(n_steps=2, n_members=3, seed=3, keep_members=True, perturb_scale=SCALE)
KINDS = ("sppt", "additive", "both")


@pytest.fixture(scope="module")
def pangu(toy):
    from skyrim_amd.core.models.pangu import PanguModel
    g, params, _ = toy
    return PanguModel(ic_source="gfs", geom=g, params=params)


@pytest.fixture(scope="module")
def before(pangu):
    return np.array(pangu.forecast(T0, n_steps=2).values)


@pytest.fixture(scope="module")
def runs(pangu, before):
    """One stochastic ensemble per kind, shared (and left unchanged) by the tests below."""
    out = {}
    for kind in KINDS:
        ens = pangu.ensemble_forecast(T0, stochastic=dict(kind=kind), **KW)
        mem = np.asarray(ens.members.values)
        mem.setflags(write=False)
        out[kind] = (ens, mem)
    return out


def _step(pangu, time, state):
    """The model's own lead 1 from the host state (C, H, W), as the rollout takes it."""
    from skyrim_amd.breeding import step_once
    loop = pangu.model
    loop._resident_state = None
    x = torch.from_numpy(np.array(state, np.float32)).to(DEV)[None, None]        # (a copy: the shared members are read-only)
    out = step_once(loop, time, x, "test").cpu().numpy()
    loop._resident_state = None
    return out


def test_none_is_the_argument_left_out(pangu):
    kw = dict(n_steps=1, n_members=3, seed=2, keep_members=True, products=("mean", "spread"))
    plain = pangu.ensemble_forecast(T0, **kw)
    none = pangu.ensemble_forecast(T0, stochastic=None, **kw)
    assert np.array_equal(np.asarray(plain.members.values), np.asarray(none.members.values))
    assert np.array_equal(plain.spread.values, none.spread.values) and np.array_equal(plain.mean.values, none.mean.values)
    assert none.stochastic is None and plain.stochastic is None


@pytest.mark.parametrize("kind", KINDS)
def test_control_and_record(pangu, before, runs, kind):
    ens, mem = runs[kind]
    assert np.array_equal(mem[0], before)                                      # member 0: the deterministic forecast at every lead, bit for bit
    assert np.isfinite(mem).all()
    plain = np.asarray(pangu.ensemble_forecast(T0, **KW).members.values)
    for m in (1, 2):
        assert np.array_equal(mem[m, 0], plain[m, 0])                           # lead 0: the initial perturbation alone
        assert not np.array_equal(mem[m, 1], plain[m, 1]) and not np.array_equal(mem[m, 2], plain[m, 2])
    assert ens.stochastic == dict(kind=kind, amplitude=0.3, clip=0.9, additive_scale=SCALE, tau_h=6.0, length_scale_km=500.0, alpha=2.0,
                                  lmax=49, channels=None)
    assert np.array_equal(np.array(pangu.forecast(T0, n_steps=2).values), before)      # the model afterwards: as before


def test_spread_from_sppt_alone(pangu):
    ens = pangu.ensemble_forecast(T0, n_steps=1, n_members=4, seed=1, perturb_scale=0.0, products=("spread",), stochastic=dict(kind="sppt"))
    spread = np.asarray(ens.spread.values)
    assert np.all(spread[0] == 0) and np.isfinite(spread).all()
    assert np.all(spread[1].reshape(spread.shape[1], -1).max(axis=1) > 0)       # every channel's tendency is multiplied


@pytest.mark.parametrize("kind", ["sppt", "additive"])
def test_seeds(pangu, runs, kind):
    _, mem = runs[kind]
    again = np.asarray(pangu.ensemble_forecast(T0, stochastic=dict(kind=kind), **KW).members.values)
    assert np.array_equal(again, mem)                                           # one seed: the same bits
    other = np.asarray(pangu.ensemble_forecast(T0, stochastic=dict(kind=kind), **dict(KW, seed=4)).members.values)
    assert np.array_equal(other[0], mem[0]) and all(not np.array_equal(other[m, 1:], mem[m, 1:]) for m in (1, 2))
    five = np.asarray(pangu.ensemble_forecast(T0, stochastic=dict(kind=kind), **dict(KW, n_members=5)).members.values)
    assert np.array_equal(five[:3], mem)                                        # a member's bits do not depend on the ensemble size


@pytest.mark.parametrize("kind", KINDS)
def test_step_rederived_from_the_devices_own_states(pangu, runs, kind):
    """Member 1's lead-2 state: its lead-1 state stepped once by the model, the patterns synthesised from coeffs(draw 1) -> evolve(draw 2)
    with the field indices of the rollout (additive 0 .. C - 1, SPPT C), and the NumPy restatement of ``stoch_apply``: the same bits.
    Lead 1 likewise, from coeffs(draw 1) alone."""
    from skyrim_amd import ensemble as E
    _, mem = runs[kind]
    loop = pangu.model
    p = S.plan(loop, dict(kind=kind), SCALE)
    s = p.spectrum
    C, H, W = mem.shape[2:]
    hw, m, seed = H * W, 1, KW["seed"]
    synth = N.synthesis(DEV, s.n_lat, s.n_lat_full, s.n_lon, s.lmax)
    sigma = torch.from_numpy((s.sigma * 2.0 ** s.e).astype(np.float32)).to(DEV)
    std = E.channel_std(loop).cpu().numpy().astype(np.float64)
    gs = np.full(C, np.float32(0.3 * 2.0 ** -s.e), np.float32) if p.sppt else None
    ga = (SCALE * std * 2.0 ** -s.e).astype(np.float32) if p.additive else None
    state, field = {}, {}
    for name, F, f_first in ([("sppt", 1, C)] if p.sppt else []) + ([("additive", C, 0)] if p.additive else []):
        nc, nt, ny = synth.sizes(F)
        state[name] = (torch.empty(nc, dtype=torch.float32, device=DEV), torch.empty(nt, dtype=torch.float32, device=DEV),
                       torch.empty(ny, dtype=torch.float32, device=DEV), F, f_first)
    for k in (1, 2):
        for name, (coef, t, y, F, f_first) in state.items():
            if k == 1:
                S.coeffs(coef, sigma, F, f_first, seed, m, 1)
            else:
                S.evolve(coef, sigma, F, f_first, seed, m, k, p.phi, p.psi)
            synth.run(coef, t, y, F)
            field[name] = y.cpu().numpy()
        xp = mem[m, k - 1]
        xn = _step(pangu, T0 + (k - 1) * loop.time_step, xp)
        want = SR.apply(xp.reshape(-1), xn.reshape(-1), field.get("sppt"), field.get("additive"), gs, ga, p.clip, C, hw)
        assert not np.array_equal(want, xn.reshape(-1))
        assert np.array_equal(want.view(np.uint32), np.ascontiguousarray(mem[m, k]).reshape(-1).view(np.uint32)), (kind, k)
    if p.sppt:                                                                  # the multiplier's pattern: unit-variance-like, clipped somewhere or not
        w = gs[0] * field["sppt"]
        print(f"{kind}: SPPT pattern at lead 2: std {w.std():.3f}, |w| max {np.abs(w).max():.3f}")
        assert 0.1 < w.std() < 0.6


def test_channels(pangu):
    """``channels=[one]``: every other channel of a member's step is the model's own step from the same state, bit for bit."""
    names = list(pangu.model.in_channel_names)
    one = names[5]
    ens = pangu.ensemble_forecast(T0, stochastic=dict(kind="both", channels=[one]), **dict(KW, n_steps=1))
    mem = np.asarray(ens.members.values)
    out = ens.members.channel.values.tolist()
    for m in (1, 2):
        own = _step(pangu, T0, mem[m, 0])
        for c in out:
            same = mem[m, 1, out.index(c)].tobytes() == own[out.index(c)].tobytes()
            assert same if c != one else not same, (m, c)
    assert ens.stochastic["channels"] == [one]


def test_scores_with_stochastic_members(pangu):
    ens = pangu.ensemble_forecast(T0, stochastic=dict(kind="both"), **dict(KW, n_members=4, keep_members=False, products=(), scores=True))
    table = ens.scores.table
    ssr = table.values[table.metric.values.tolist().index("ssr")]              # (time, channel)
    assert np.isfinite(ssr[1:]).all() and (ssr[1:] > 0).all()


def test_breeding_and_spherical_seeds_together_with_it(pangu, before):
    kw = dict(KW, n_steps=1, perturbation="spherical", breeding={"cycles": 1})
    bred = pangu.ensemble_forecast(T0, **kw)
    both = pangu.ensemble_forecast(T0, stochastic=dict(kind="sppt", tau_h=0.0), **kw)
    a, b = np.asarray(bred.members.values), np.asarray(both.members.values)
    assert np.array_equal(a[:, 0], b[:, 0]) and np.array_equal(b[0], before[:2])        # the same bred initial states, the same control
    assert all(not np.array_equal(a[m, 1], b[m, 1]) for m in (1, 2)) and np.isfinite(b).all()
    assert both.breeding == dict(cycles=1, norm="total", paired=False) and both.stochastic["kind"] == "sppt" and both.stochastic["tau_h"] == 0.0
    assert np.array_equal(both.breeding_growth, bred.breeding_growth, equal_nan=True)
