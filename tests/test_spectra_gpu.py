"""Zonal spectra end to end on the MI355X with the Pangu toy model (49 x 192): ``ensemble_forecast(spectra=...)`` against ``from_members``
and the float64 restatement on the kept members, the labels, a flat spread spectrum for white and a red one for spherical perturbations
at lead 0, that ``spectra=None`` changes nothing, and ``spectrum_forecast`` against ``spectra_prediction`` on the files of the same
rollout."""
from __future__ import annotations

import datetime

import numpy as np
import pytest
import torch

import _spectra_reference as R
from skyrim_amd import spectra as S
from skyrim_amd import verify
from skyrim_amd.verify import area_weights

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T0 = datetime.datetime(2024, 5, 13, 18, 0)
M = 3
CH = ["z500", "u850", "v850"]
KW = dict(n_steps=2, n_members=M, keep_members=True, products=("mean",), seed=0)
SPEC = {"channels": CH}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def pangu(toy):
    from skyrim_amd.core.models.pangu import PanguModel
    g, params, _ = toy
    return PanguModel(ic_source="gfs", geom=g, params=params)


@pytest.fixture(scope="module")
def plain(pangu):
    return pangu.ensemble_forecast(T0, scores=True, **KW)


@pytest.fixture(scope="module")
def ens(pangu):
    """The scored ensemble with spectra: computed once, shared, left unchanged."""
    return pangu.ensemble_forecast(T0, spectra=SPEC, scores=True, **KW)


def test_without_spectra_nothing_changes(plain, ens):
    assert plain.spectra is None and ens.spectra is not None
    for p in ("mean", "members"):
        assert not np.any(bits(getattr(plain, p).values) != bits(getattr(ens, p).values)), p
    assert np.array_equal(plain.scores.sums.values, ens.scores.sums.values, equal_nan=True)
    assert np.array_equal(plain.scores.rank_counts.values, ens.scores.rank_counts.values)


def test_power_is_labelled_and_equals_from_members_and_the_reference_on_the_kept_members(pangu, ens):
    sp = ens.spectra
    lat, lon = np.asarray(pangu.model.grid.lat, np.float64), np.asarray(pangu.model.grid.lon, np.float64)
    K = lon.size // 2 + 1
    assert sp.power.dims == ("time", "channel", "band", "kind", "wavenumber") and sp.power.values.shape == (3, 3, 4, 6, K)
    assert sp.power.channel.values.tolist() == CH and sp.power.band.values.tolist() == ["nh_mid", "tropics", "sh_mid", "globe"]
    assert sp.power.kind.values.tolist() == list(S.KINDS) and sp.power.wavenumber.values.tolist() == list(range(K))
    assert len(sp.times) == 3
    assert sp.n_members == M and sp.model_name.endswith(f"-ens{M}") and np.isfinite(sp.power.values).all()
    names = ens.members.channel.values.tolist()
    index = [names.index(c) for c in CH]
    tf = verify._Fields(verify.default_truth(pangu), "truth", lat, lon)
    mem = np.asarray(ens.members.values)                                       # (M, T, C, H, W)
    truth = np.zeros_like(mem[0])
    for t, time in enumerate(sp.times):
        truth[t, index] = tf.at(time, CH)
    # the same members uploaded again: the kernel gives the forecast path's bits
    dev = [torch.from_numpy(np.ascontiguousarray(mem[m])).to(DEV) for m in range(M)]
    again = S.from_members(dev, lat, lon, names=names, channels=CH, truth=torch.from_numpy(truth).to(DEV), times=sp.times)
    assert np.array_equal(again.power.values, sp.power.values) and again.bands == sp.bands and again.rows == sp.rows
    w = area_weights(lat)
    worst = 0.0
    for t in range(3):
        out, lim = R.spectra([mem[m, t] for m in range(M)], truth[t], index, sp.rows, w)
        err = np.abs(sp.power.values[t] - out)
        assert (err <= lim).all(), f"time {t}: worst entry at {float((err[lim > 0] / lim[lim > 0]).max()):.3f} of the bound"
        worst = max(worst, float((err[lim > 0] / lim[lim > 0]).max()))
    print(f"spectra end to end: worst error / bound = {worst:.4f}")
    assert sp.kinetic_energy(850).shape == (3, 4, K) and sp.spread_skill("z500", "globe").shape == (3, K)
    assert sp.wavelength_km("nh_mid")[1] < sp.wavelength_km("tropics")[1]


def test_derived_fields_go_through_the_derivers_buffer_next_to_raw_channels(pangu):
    lat, lon = np.asarray(pangu.model.grid.lat, np.float64), np.asarray(pangu.model.grid.lon, np.float64)
    bands = {"tropics": (-20, 20), "globe": None}
    ens = pangu.ensemble_forecast(T0, n_steps=1, n_members=M, keep_members=True, products=("mean",), seed=0, derived=["ws850"],
                                  spectra={"channels": ["ws850", "z500"], "bands": bands})
    sp = ens.spectra
    assert sp.channels == ["ws850", "z500"] and sp.kinds == ["member", "mean", "spread"] and sp.power.values.shape == (2, 2, 2, 3, 97)
    for k, (name, kept) in enumerate((("ws850", ens.derived.members), ("z500", ens.members))):
        names = kept.channel.values.tolist()
        dev = [torch.from_numpy(np.ascontiguousarray(np.asarray(kept.values)[m])).to(DEV) for m in range(M)]
        again = S.from_members(dev, lat, lon, names=names, channels=[name], bands=bands, times=sp.times)
        assert np.array_equal(again.power.values[:, 0], sp.power.values[:, k]), name
    assert (sp.power.values[:, 0, :, 0].sum(axis=-1) > 0).all()                 # a wind speed's mean square


def chi2_factor(weights, M, p=1e-6):
    """The ratio of the (1 - p) and p quantiles of one bin of a white spread spectrum.  Member 0 is the unperturbed control, so per row and
    bin (0 < k < W/2) the sum of the members' squared anomalies is sigma^2 / 2 times [chi2_{2 (M - 2)} + chi2_2 / M] (the eigenvalues of
    I - 11'/M on the M - 1 perturbed members: M - 2 ones and 1/M); the band mean adds the rows with their weights.  The weighted sum of
    chi-squares is matched by g chi2_nu with nu = 2 (sum c)^2 / sum c^2 (Satterthwaite: the same mean and variance)."""
    from scipy.stats import chi2
    c = np.concatenate([np.repeat(weights, M - 2), weights / M])               # coefficients of independent chi2_2 variables
    nu = 2.0 * c.sum() ** 2 / (c ** 2).sum()
    return float(chi2.ppf(1.0 - p, nu) / chi2.ppf(p, nu)), nu


def test_white_perturbations_give_a_flat_spread_spectrum_and_spherical_ones_a_red_one_at_lead_0(pangu):
    lat = np.asarray(pangu.model.grid.lat, np.float64)
    w = area_weights(lat)
    kw = dict(n_steps=0, n_members=M, products=(), seed=3, perturb_scale=0.05, spectra={"channels": CH, "bands": {"globe": None}})
    white = pangu.ensemble_forecast(T0, perturbation="white", **kw).spectra
    factor, nu = chi2_factor(w, M)
    spread = white.power.values[0, :, 0, 2, 1:-1]                              # (channel, k): 0 < k < W/2 (the Nyquist bin has c_k = 1)
    ratio = spread.max(axis=-1) / spread.min(axis=-1)
    print(f"white spread spectrum: max / min = {ratio.tolist()}, allowed {factor:.2f} (nu = {nu:.1f})")
    assert (spread > 0).all() and (ratio <= factor).all()
    red = pangu.ensemble_forecast(T0, perturbation="spherical", **kw).spectra
    spread = red.power.values[0, :, 0, 2, 1:-1]
    third = spread.shape[-1] // 3
    low, high = spread[:, :third].mean(axis=-1), spread[:, -third:].mean(axis=-1)
    print(f"spherical spread spectrum: low-k third / high-k third = {(low / high).tolist()}")
    assert (low > factor * high).all()                                         # red by more than the white spectrum's scatter


def test_spectrum_forecast_matches_spectra_prediction_on_the_files_of_the_same_rollout(pangu, tmp_path):
    src = pangu.data_source
    spec = {"channels": ["z500", "t850"], "bands": {"nh_mid": (30, 60), "globe": None}}
    own = pangu.spectrum_forecast(T0, n_steps=2, spectra=spec, truth=src)
    assert own.n_members == 1 and own.kinds == list(S.KINDS) and own.power.values.shape == (3, 2, 2, 6, 97)
    assert not own.power.values[:, :, :, 2].any()                              # one member: no spread
    assert not own.power.values[0, :, :, 4].any()                              # lead 0: the truth source is the IC source
    assert np.array_equal(own.power.values[:, :, :, 0], own.power.values[:, :, :, 1])
    _, paths = pangu.rollout(T0, n_steps=2, save=True, save_config={"output_dir": str(tmp_path), "file_type": "netcdf"})
    disk = S.spectra_prediction(list(paths), truth=src, channels=spec["channels"], bands=spec["bands"], device=DEV)
    assert [np.datetime64(t, "s") for t in disk.times] == [np.datetime64(t, "s") for t in own.times] and disk.channels == own.channels
    a, b = own.power.values, disk.power.values
    total = a.sum(axis=-1, keepdims=True)                                      # the band's mean square
    assert (np.abs(a - b) <= 1e-5 * np.maximum(a, b) + 1e-12 * total).all()
    none = pangu.spectrum_forecast(T0, n_steps=1, spectra=spec)
    assert none.kinds == ["member", "mean", "spread"] and np.array_equal(none.power.values[:, :, :, 0], own.power.values[:2, :, :, 0])
    path = own.save(tmp_path / "own.json")
    assert np.array_equal(S.Spectra.load(path).power.values, own.power.values)
