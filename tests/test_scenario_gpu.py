"""Ensemble scenarios end to end on the MI355X with the Pangu toy model (49 x 192): ``ensemble_forecast(scenarios=...)`` against the
restatements of tests/_scenario_reference.py made from the kept members -- the Gram matrices within the header's bound carried through
the centring, the clusters, sizes, representatives and variance fractions, with the margin of every discrete decision asserted -- the
cluster means against ``ens_stats`` bit for bit, the EOF patterns against the centred members, the energy score, ``from_members`` on the
kept members, and that nothing else of the forecast changes."""
from __future__ import annotations

import datetime

import numpy as np
import pytest
import torch

import _scenario_reference as R
from skyrim_amd import ensemble as E
from skyrim_amd import scenarios as S
from skyrim_amd.verify import area_weights

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T0 = datetime.datetime(2024, 5, 13, 18, 0)
M = 6
# (seed and kind of perturbation chosen for their margins: the least merge gap of the three lead times is 2.6e-3 of the total sum of
# squares, the bound on a merge cost 7e-6 of it; most seeds have one near-tie among their twelve merges)
KW = dict(n_steps=2, n_members=M, keep_members=True, products=("mean",), perturb_scale=0.05, seed=0, perturbation="spherical")
SPEC = {"channels": ["z500", "msl"], "region": (20, 70, 300, 40), "n_clusters": 2, "n_eofs": M - 1, "normalise": "spread"}
MARGIN = 100.0                                             # every discrete decision is this many error bounds from going the other way


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def pangu(toy):
    from skyrim_amd.core.models.pangu import PanguModel
    g, params, _ = toy
    return PanguModel(ic_source="gfs", geom=g, params=params)


@pytest.fixture(scope="module")
def plain(pangu):
    return pangu.ensemble_forecast(T0, **KW)


@pytest.fixture(scope="module")
def ens(pangu):
    """The ensemble with scenarios: computed once, shared, left unchanged."""
    return pangu.ensemble_forecast(T0, scenarios=SPEC, **KW)


def grid_of(pangu):
    lat, lon = np.asarray(pangu.model.grid.lat, np.float64), np.asarray(pangu.model.grid.lon, np.float64)
    return lat, lon, area_weights(lat), S.region_index(lat, lon, SPEC["region"])


def reference(members, truth, index, region, w, normalise="spread"):
    """Per channel the centred area-mean Gram matrix and the bound on its entries; the anomalies of the reference's own algebra."""
    Mm = len(members)
    Gd, Sabs = R.gram(members, truth, index, region, w)
    area = w[region[0]:region[0] + region[1]].sum() * region[3]
    Mp = Gd.shape[-1]
    J = np.eye(Mp)
    J[:Mm, :] -= 1.0 / Mm
    Gc = np.stack([J.T @ g @ J for g in Gd]) / area
    lim = np.stack([np.abs(J).T @ (S.bound_factor() * s) @ np.abs(J) for s in Sabs]) / area      # the bound through the linear centring
    A, ay = R.anomalies(members, truth, index, region, w, normalise)
    return Gc, lim, A, ay


def test_without_scenarios_nothing_changes(plain, ens):
    assert plain.scenarios is None and ens.scenarios is not None
    for p in ("mean", "members"):
        assert not np.any(bits(getattr(plain, p).values) != bits(getattr(ens, p).values)), p


def test_gram_clusters_representatives_and_variance_fractions_equal_the_reference(pangu, ens):
    lat, lon, w, region = grid_of(pangu)
    assert region[2] + region[3] > lon.size                                     # the box crosses Greenwich: the columns wrap
    sc = ens.scenarios
    names = ens.members.channel.values.tolist()
    index = [names.index(c) for c in SPEC["channels"]]
    assert sc.channels == SPEC["channels"] and sc.region == region and sc.n_members == M and len(sc.times) == 3
    assert sc.gram.shape == (3, 2, M, M) and sc.combined.shape == (3, M, M) and sc.pcs.shape == (3, M, M - 1)
    mem = np.asarray(ens.members.values)
    for t in range(3):
        members = [np.ascontiguousarray(mem[m, t]) for m in range(M)]
        Gc, lim, A, _ = reference(members, None, index, region, w)
        err = np.abs(sc.gram[t] - Gc)
        assert (err <= lim).all(), f"time {t}: worst entry at {float((err / lim).max()):.3f} of the bound"
        # the bound of an entry of the combined matrix relative to the total sum of squares, and of a squared distance or merge cost
        scale = np.array([np.trace(g) / (M - 1) for g in Gc])
        rel = 4.0 * float((lim / scale[:, None, None]).sum(axis=0).max()) / float((A ** 2).sum())
        gaps = []
        labels = R.ward(A, SPEC["n_clusters"], gaps)
        ref = R.summarise(A, labels)
        assert min(gaps) > MARGIN * rel and R.representative_gap(A, labels) > MARGIN * rel
        c = sc.clusters_at[t]
        assert np.array_equal(c["labels"], labels) and c["sizes"].tolist() == ref["sizes"].tolist()
        assert c["representative"].tolist() == ref["representative"].tolist() and np.allclose(c["probability"], ref["probability"])
        for k in ("within", "explained", "total"):
            assert abs(c[k] - ref[k]) <= 10 * rel * ref["total"], k
        frac, pcs, _ = R.eofs(A, M - 1)
        assert np.abs(sc.variance_fraction[t] - frac).max() <= 10 * rel and abs(sc.variance_fraction[t].sum() - 1) < 1e-12
        assert np.allclose(sc.scale[t], scale, rtol=1e-4)
    # trajectory scenarios: host only, from the stored matrices
    whole = sc.clusters(2)
    assert whole["sizes"].sum() == M and np.array_equal(sc.clusters(2, times=[1])["labels"], sc.clusters_at[1]["labels"])


def test_cluster_means_equal_ens_stats_of_the_labelled_members_bit_for_bit(ens):
    sc = ens.scenarios
    names = ens.members.channel.values.tolist()
    cm = sc.cluster_mean
    assert cm.dims == ("time", "cluster", "channel", "lat", "lon") and cm.values.shape[:3] == (3, 2, 2) and cm.values.dtype == np.float32
    mem = np.asarray(ens.members.values)
    for t in range(3):
        for c in range(2):
            idx = np.nonzero(sc.clusters_at[t]["labels"] == c)[0]
            for cc, ch in enumerate(SPEC["channels"]):
                sub = [torch.from_numpy(np.ascontiguousarray(mem[m, t, names.index(ch)])).to(DEV) for m in idx]
                out = torch.empty(sub[0].numel(), dtype=torch.float32, device=DEV)
                E.stats(sub, E.member_table(sub), 0, sub[0].numel(), mean=out)
                assert not np.any(bits(cm.values[t, c, cc].reshape(-1)) != bits(out.cpu().numpy())), (t, c, ch)


def test_eof_patterns_rebuild_the_centred_members_from_the_pcs(ens):
    sc = ens.scenarios
    names = ens.members.channel.values.tolist()
    pat = np.asarray(sc.eof_pattern.values, np.float64)                         # (time, eof, channel, lat, lon)
    assert sc.eof_pattern.dims == ("time", "eof", "channel", "lat", "lon") and pat.shape[:3] == (3, M - 1, 2)
    mem = np.asarray(ens.members.values)
    for t in range(3):
        for cc, ch in enumerate(SPEC["channels"]):
            x = mem[:, t, names.index(ch)].astype(np.float64)
            anom = x - x.mean(axis=0)
            rebuilt = np.einsum("mk,kji->mji", sc.pcs[t], pat[t, :, cc])
            spread = np.sqrt((anom ** 2).mean())
            assert np.abs(rebuilt - anom).max() <= 1e-5 * spread, (t, ch, float(np.abs(rebuilt - anom).max() / spread))


def test_energy_score_and_from_members(pangu, ens):
    from skyrim_amd import verify
    lat, lon, w, region = grid_of(pangu)
    spec = {"channels": ["z500"], "region": SPEC["region"], "n_clusters": 2, "n_eofs": 2, "normalise": "none"}
    scored = pangu.ensemble_forecast(T0, scenarios=spec, scores=True, **KW)
    sc = scored.scenarios
    assert not np.any(bits(scored.members.values) != bits(ens.members.values))
    names = scored.members.channel.values.tolist()
    k = names.index("z500")
    tf = verify._Fields(verify.default_truth(pangu), "truth", lat, lon)
    mem = np.asarray(scored.members.values)
    assert sc.gram.shape == (3, 1, M + 1, M + 1) and sc.energy_score.shape == (3,) and np.isfinite(sc.energy_score).all()
    for t, time in enumerate(sc.times):
        members = [np.ascontiguousarray(mem[m, t]) for m in range(M)]
        y = np.zeros_like(members[0])
        y[k] = tf.at(time, ["z500"])[0]
        Gc, lim, A, ay = reference(members, y, [k], region, w, "none")
        assert (np.abs(sc.gram[t] - Gc) <= lim).all()
        want = R.energy_score(A, ay)
        # a norm sqrt(D2) moves by at most min(sqrt(e), e / sqrt(D2)) when D2 moves by e, the bound of the four entries it is made of
        # (at the first lead time the truth IS the control member: that norm is 0 and only sqrt(e) holds)
        E4 = lim[0] + lim[0].T
        e = np.diag(lim[0])[:, None] + np.diag(lim[0])[None, :] + E4
        D = np.sqrt(S.distances(Gc[0]))
        with np.errstate(divide="ignore", invalid="ignore"):
            move = np.where(D > 0, np.minimum(np.sqrt(e), e / D), np.sqrt(e))
        off = ~np.eye(M, dtype=bool)
        tol = move[:M, M].mean() + move[:M, :M][off].sum() / (2.0 * M * (M - 1))
        assert abs(sc.energy_score[t] - want) <= tol
        labels = R.ward(A, 2)
        assert np.array_equal(sc.clusters_at[t]["labels"], labels) and sc.nearest_cluster[t] == R.nearest_cluster(A, ay, labels)
    # the same members uploaded again: ``from_members`` gives what the forecast path gave, bit for bit
    dev = [torch.from_numpy(np.ascontiguousarray(mem[m])).to(DEV) for m in range(M)]             # (T, C, H, W) each
    again = S.from_members(dev, lat, lon, names=names, channels=SPEC["channels"], region=SPEC["region"], n_clusters=2, n_eofs=M - 1,
                           times=ens.scenarios.times)
    first = ens.scenarios
    assert np.array_equal(again.gram, first.gram) and np.array_equal(again.pcs, first.pcs)
    assert all(np.array_equal(a["labels"], b["labels"]) and a["representative"].tolist() == b["representative"].tolist()
               for a, b in zip(again.clusters_at, first.clusters_at))
    assert not np.any(bits(again.cluster_mean.values) != bits(first.cluster_mean.values))
    assert not np.any(bits(again.eof_pattern.values) != bits(first.eof_pattern.values))
    one = S.from_members([d[1] for d in dev], lat, lon, names=names, channels=["msl"], n_clusters=3, n_eofs=0)
    assert one.gram.shape == (1, 1, M, M) and one.eof_pattern is None and one.clusters_at[0]["sizes"].sum() == M


def test_refusals_come_before_the_device(pangu, monkeypatch):
    import skyrim_amd.datasource as ds
    monkeypatch.setattr(ds, "get_initial_condition_for_model", lambda *a, **k: pytest.fail("the device was reached"))
    for kw, msg in ((dict(scenarios={"channels": ["tp06"]}), "tp06"), (dict(scenarios={"channels": ["ws10m"]}, derived=["ws10m"]), "raw channels"),
                    (dict(scenarios={**SPEC, "region": (70, 20, 0, 10)}), "empty"), (dict(scenarios=SPEC, n_members=1), "at least 2"),
                    (dict(scenarios={**SPEC, "n_clusters": 7}), "n_clusters"), (dict(scenarios={**SPEC, "n_eofs": 6}), "n_eofs")):
        args = dict(n_steps=1, n_members=M)
        args.update(kw)
        with pytest.raises(ValueError, match=msg):
            pangu.ensemble_forecast(T0, **args)
