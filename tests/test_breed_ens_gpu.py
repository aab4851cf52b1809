"""``ensemble_forecast(breeding=...)`` end to end on the MI355X, on the toy Pangu (49 x 192): the control member, ``breeding=None``, the
cycle re-derived from the device's own states, the factor tables, the amplitude at lead 0, ensemble size, seeds, ``perturb_channels``,
pairs, the growth record, the scores, and the model's state afterwards."""
from __future__ import annotations

import datetime

import numpy as np
import pytest
import torch

import _breed_reference as BR
from skyrim_amd import breeding as B

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T0 = datetime.datetime(2024, 5, 13, 18, 0)
SCALE = 1e-3
U = 2.0 ** -24
KW = dict(n_steps=1, n_members=5, seed=3, keep_members=True, perturb_scale=SCALE, breeding={"cycles": 2})


@pytest.fixture(scope="module")
def pangu(toy):
    from skyrim_amd.core.models.pangu import PanguModel
    g, params, _ = toy
    return PanguModel(ic_source="gfs", geom=g, params=params)


@pytest.fixture(scope="module")
def before(pangu):
    return np.array(pangu.forecast(T0, n_steps=1).values)


@pytest.fixture(scope="module")
def runs(pangu, before):
    """One bred ensemble per seed kind, shared (and left unchanged) by the tests below."""
    out = {}
    for kind in ("white", "spherical"):
        ens = pangu.ensemble_forecast(T0, perturbation=kind, **KW)
        mem = np.asarray(ens.members.values)
        mem.setflags(write=False)
        out[kind] = (ens, mem)
    return out


def _geometry(pangu):
    from skyrim_amd import ensemble as E
    from skyrim_amd.verify import area_weights
    loop = pangu.model
    w = area_weights(np.asarray(loop.grid.lat, np.float64))
    std = E.channel_std(loop).cpu().numpy().astype(np.float64)
    return w, std, len(loop.grid.lon)


def _area_mean_square(d, w, n_lon):
    """(..., C): sum_j w_j sum_i d^2 / (sum_j w_j n_lon) of float64 fields (..., C, H, W)."""
    return np.einsum("...chw,h->...c", d * d, w) / (w.sum() * n_lon)


@pytest.mark.parametrize("kind", ["white", "spherical"])
def test_control_shape_and_record(pangu, before, runs, kind):
    ens, mem = runs[kind]
    assert np.array_equal(mem[0], before)                                      # the control member: forecast, bit for bit
    assert np.isfinite(mem).all() and all(not np.array_equal(mem[k, 0], mem[0, 0]) for k in range(1, 5))
    assert ens.breeding == dict(cycles=2, norm="total", paired=False) and ens.perturbation == kind
    g = ens.breeding_growth
    C = mem.shape[2]
    assert g.shape == (2, 5, C) and g.dtype == np.float64
    assert np.isnan(g[:, 0]).all() and np.isfinite(g[:, 1:]).all() and (g[:, 1:] > 0).all()


@pytest.mark.parametrize("kind", ["white", "spherical"])
def test_amplitude_at_lead_0(pangu, runs, kind):
    """norm="total": the sigma-normalised area RMS of x_m - x_0 over the channels is perturb_scale.  x_m - x_0 = f t + e with
    |e| <= u |f t| + u |x_m| per element (the product's and the final addition's rounding, u = 2^-24) and f within u of its float64
    value (its one rounding to fp32); the normalised RMS N is a norm, so |N(x_m - x_0) - perturb_scale| <= perturb_scale (2 u + 2^-40)
    + u N(x_m): the triangle inequality, 2^-40 for the float64 arithmetic of the norms and factors."""
    ens, mem = runs[kind]
    w, std, n_lon = _geometry(pangu)
    x = mem[:, 0].astype(np.float64)
    worst = 0.0
    for k in range(1, 5):
        amp = np.sqrt((_area_mean_square(x[k] - x[0], w, n_lon) / std ** 2).mean())
        bound = SCALE * (2 * U + 2.0 ** -40) + U * np.sqrt((_area_mean_square(x[k], w, n_lon) / std ** 2).mean())
        worst = max(worst, abs(amp - SCALE) / bound)
        assert abs(amp - SCALE) <= bound, (k, amp, bound)
    print(f"{kind}: |amplitude - perturb_scale| / bound <= {worst:.3f}")


def test_amplitude_per_channel(pangu):
    ens = pangu.ensemble_forecast(T0, **dict(KW, n_steps=0, n_members=3, breeding=dict(cycles=2, norm="channel")))
    w, std, n_lon = _geometry(pangu)
    x = np.asarray(ens.members.values)[:, 0].astype(np.float64)
    for k in (1, 2):
        amp = np.sqrt(_area_mean_square(x[k] - x[0], w, n_lon)) / std
        bound = SCALE * (2 * U + 2.0 ** -40) + U * np.sqrt(_area_mean_square(x[k], w, n_lon)) / std
        assert np.all(np.abs(amp - SCALE) <= bound), (k, float((np.abs(amp - SCALE) / bound).max()))
    assert ens.breeding["norm"] == "channel"


def test_no_breeding_is_unchanged(pangu):
    kw = dict(n_steps=1, n_members=3, seed=2, keep_members=True, products=("mean", "spread"))
    plain = pangu.ensemble_forecast(T0, **kw)
    none = pangu.ensemble_forecast(T0, breeding=None, **kw)
    assert np.array_equal(np.asarray(plain.members.values), np.asarray(none.members.values))
    assert np.array_equal(plain.spread.values, none.spread.values) and none.breeding is None and none.breeding_growth is None


@pytest.mark.parametrize("kind", ["white", "spherical"])
def test_size_seed_and_afterwards(pangu, before, runs, kind):
    ens, mem = runs[kind]
    eight = np.asarray(pangu.ensemble_forecast(T0, perturbation=kind, **dict(KW, n_members=8)).members.values)
    assert np.array_equal(eight[3], mem[3]) and np.array_equal(eight[:5], mem)      # a member's bits do not depend on the ensemble size
    again = pangu.ensemble_forecast(T0, perturbation=kind, **KW)
    assert np.array_equal(np.asarray(again.members.values), mem)                     # one seed: the same bits
    assert np.array_equal(again.breeding_growth, ens.breeding_growth, equal_nan=True)
    other = np.asarray(pangu.ensemble_forecast(T0, perturbation=kind, **dict(KW, seed=4)).members.values)
    assert np.array_equal(other[0], mem[0]) and all(not np.array_equal(other[k], mem[k]) for k in range(1, 5))
    assert np.array_equal(np.array(pangu.forecast(T0, n_steps=1).values), before)    # the model afterwards: as before


@pytest.mark.parametrize("norm,paired", [("total", False), ("channel", False), ("total", True)])
def test_cycle_rederived_from_the_devices_own_states(pangu, norm, paired):
    """Driving ``Breeder`` directly (white seeds, batches of two so that the batches show): every cycle's x_m is the restatement applied to
    the device's own y states and factor tables, bit for bit; the tables are within one fp32 ulp of ``factors`` restated from the device's
    S; the growth record is the ratio of the S tables."""
    from skyrim_amd import ensemble as E
    from skyrim_amd.datasource import get_initial_condition_for_model
    loop = pangu.model
    x0 = get_initial_condition_for_model(loop, pangu.data_source, T0).to(DEV, torch.float32).contiguous()
    std = E.channel_std(loop)
    hw = x0.shape[-2] * x0.shape[-1]
    M, K, C = 6, 2, x0.shape[2]
    mask = np.ones(C, bool)
    mask[::3] = False
    std_seed = torch.where(torch.from_numpy(mask).to(DEV), std, torch.zeros_like(std))

    def seeder(m, out):
        E.perturb(x0, std_seed, out, hw, SCALE, 7, m)

    br = B.Breeder(loop, B.Plan(K, norm, paired), x0, std, SCALE, 7, T0, seeder, mask=mask, batch=2, trace=True)
    loop._resident_state = None
    br.run(M)
    loop._resident_state = None
    w, std64, n_lon = _geometry(pangu)
    x0h, y0h = x0[0, 0].cpu().numpy(), br.y0.cpu().numpy()
    assert np.array_equal(br.member(0).cpu().numpy(), x0.cpu().numpy())
    bred = [m for m in range(1, M) if not paired or m % 2 == 1]
    assert sorted(m for t in br.trace for m in t["members"] if t["cycle"] == 1) == bred
    finals = {}
    for t in br.trace:
        k, ids = t["cycle"], t["members"]
        y, x = np.stack(t["y"]), np.stack(t["x"])
        f = br.factors_used[k - 1][ids]
        assert BR.apply(x0h, y0h, y, f).tobytes() == x.tobytes(), (k, ids)
        S_ref, T_ref = BR.norms(y0h, y, w)
        assert np.all(np.abs(br.S[k][ids] - S_ref) <= B.bound_k(C, *x0h.shape[1:]) * BR.U53 * T_ref)
        f_ref = BR.factors(br.S[k][ids], std64.astype(np.float32), SCALE, norm, mask, w.sum(), n_lon)
        assert np.all(np.abs(f.astype(np.float64) - f_ref) <= np.spacing(np.abs(f_ref)).astype(np.float64)), (k, ids)
        assert np.all(f[:, ~mask] == 0) and np.all(f[:, mask] > 0)
        if k == K:
            finals.update({m: (x[i], y[i], f[i]) for i, m in enumerate(ids)})
    for m in bred:
        assert np.array_equal(br.member(m)[0, 0].cpu().numpy(), finals[m][0])
    if paired:
        for m in (2, 4):
            xa, y, f = finals[m - 1]
            assert np.array_equal(br.factors_used[:, m], -br.factors_used[:, m - 1])
            xb = br.member(m)[0, 0].cpu().numpy()
            assert BR.apply(x0h, y0h, y[None], -f[None])[0].tobytes() == xb.tobytes()
            s = (xa.astype(np.float64) - x0h) + (xb.astype(np.float64) - x0h)       # the pair is symmetric about x_0 to two roundings
            assert np.all(np.abs(s) <= U * (np.abs(xa.astype(np.float64)) + np.abs(xb.astype(np.float64))))
            assert np.array_equal(br.growth[:, m], br.growth[:, m - 1], equal_nan=True)
        assert np.all(br.factors_used[:, 5][:, mask] > 0)                       # member 5 has no partner: bred as itself
    assert br.growth.shape == (K, M, C) and br.S.shape == (K + 1, M, C)
    with np.errstate(all="ignore"):
        ratio = np.sqrt(br.S[1:] / br.S[:-1])
    live = br.S[:-1] != 0
    assert np.allclose(br.growth[live], ratio[live], rtol=4 * 2.0 ** -53, atol=0) and np.isnan(br.growth[~live]).all()      # (a division and a root)
    assert np.isnan(br.growth[:, 0]).all() and np.isfinite(br.growth[:, 1:][:, :, mask]).all()
    assert np.all(br.S[0][1:][:, ~mask] == 0) and np.isnan(br.growth[0][1:][:, ~mask]).all()   # the seed leaves masked channels alone


@pytest.mark.parametrize("kind", ["white", "spherical"])
def test_perturb_channels(pangu, kind):
    names = list(pangu.model.in_channel_names)
    one = names[5]
    ens = pangu.ensemble_forecast(T0, perturbation=kind, perturb_channels=[one], **dict(KW, n_steps=0, n_members=4))
    mem = np.asarray(ens.members.values)[:, 0]
    out = ens.members.channel.values.tolist()
    for c in out:
        same = [mem[k, out.index(c)].tobytes() == mem[0, out.index(c)].tobytes() for k in range(1, 4)]
        assert all(same) if c != one else not any(same), c
    g = ens.breeding_growth
    assert np.isfinite(g[:, 1:, names.index(one)]).all()


def test_pairs_through_the_ensemble(pangu, runs):
    ens = pangu.ensemble_forecast(T0, **dict(KW, breeding=dict(cycles=2, paired=True)))
    mem = np.asarray(ens.members.values)[:, 0].astype(np.float64)
    assert ens.breeding["paired"] is True
    for j in (1, 2):
        a, b = mem[2 * j - 1], mem[2 * j]
        s = (a - mem[0]) + (b - mem[0])
        assert np.all(np.abs(s) <= U * (np.abs(a) + np.abs(b))), j
        assert not np.array_equal(a, b)
    assert np.array_equal(mem[1], runs["white"][1][1, 0].astype(np.float64))     # member 1 is bred as itself: pairing does not change it


def test_scores_with_bred_members(pangu):
    ens = pangu.ensemble_forecast(T0, **dict(KW, n_members=4, keep_members=False, products=(), scores=True))
    table = ens.scores.table
    ssr = table.values[table.metric.values.tolist().index("ssr")]              # (time, channel)
    assert np.isfinite(ssr[1:]).all() and (ssr[1:] > 0).all()
