"""Zonal spectra without a GPU: Parseval, a pure wave and the exact identities between the slots in the float64 restatement
(tests/_spectra_reference.py), the host algebra of ``spectra.Spectra`` (wavelengths, kinetic energy, effective resolution on a spectrum
with a known knee, the spread/skill ratio, JSON, ``merge``), the refusals of ``check_request`` and of ``ensemble_forecast(spectra=...)``
that need no device, the C ABI of include/skyrim_spec.h -- exports, constants, twiddles and every argument error -- and the command
line's options."""
from __future__ import annotations

import ctypes
import math
import re
from pathlib import Path

import numpy as np
import pytest

import _spectra_reference as R
from skyrim_amd import spectra as S
from skyrim_amd.verify import area_weights

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "skyrim_spec.h"
BUILT = (ROOT / "skyrim_amd" / "lib" / "libskyrim_spec.so").exists()
needs_lib = pytest.mark.skipif(not BUILT, reason="libskyrim_spec.so is not built")
E_ARG = -1
FAKE = 0x10000                                                                 # never dereferenced: every call below is refused first


def grid(n_lat, n_lon):
    return np.linspace(90.0, -90.0, n_lat), np.arange(n_lon) * (360.0 / n_lon)


# ---- the definition ---------------------------------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize("W", [30, 45, 64, 1440])
def test_parseval_the_bins_sum_to_the_row_mean_square(W):
    rng = np.random.default_rng(W)
    rows = 5.5e4 + R.red_rows(rng, (3,), W, 1e3) + rng.standard_normal((3, W))
    power = R.c_k(W) * np.abs(R.coeffs(rows)) ** 2
    ms = (rows ** 2).mean(axis=-1)
    assert np.abs(power.sum(axis=-1) - ms).max() <= 4e-15 * ms.max()
    assert power.shape[-1] == W // 2 + 1 == S.n_bins(W)


@pytest.mark.parametrize("W,k0", [(48, 5), (45, 7), (64, 32)])
def test_a_pure_wave_puts_half_its_squared_amplitude_at_its_wavenumber(W, k0):
    H = 6
    lam = 2.0 * np.pi * np.arange(W) / W
    a = np.linspace(1.0, 3.0, H)
    field = (a[:, None] * np.cos(k0 * lam[None, :] + 0.3)).astype(np.float32)
    w = np.linspace(0.2, 1.0, H)
    out, _ = R.spectra([field[None]], None, [0], [(0, H), (2, 5)], w)
    for b, (j0, j1) in enumerate([(0, H), (2, 5)]):
        nyquist = 2 * k0 == W
        want = (w[j0:j1] * (a[j0:j1] * np.cos(0.3)) ** 2).sum() / w[j0:j1].sum() if nyquist else (w[j0:j1] * a[j0:j1] ** 2 / 2).sum() / w[j0:j1].sum()
        got = out[0, b, 0]
        assert abs(got[k0] - want) <= 1e-6 * want, (got[k0], want)               # (the field is rounded to fp32)
        rest = np.delete(got, k0)
        assert rest.max() <= 1e-12 * want


@pytest.mark.parametrize("M", [2, 3, 7])
def test_the_exact_identities_between_the_slots_hold_in_the_reference(M):
    members, y = R.case(45, 4, M, True)
    out, _ = R.spectra(members, y, [0, 1], [(0, 4), (1, 2)], np.array([0.5, 1.0, 0.7, 0.2]))
    k = {n: i for i, n in enumerate(R.KINDS)}
    # the reference subtracts float64 fields of size 5.5e4: a coefficient of a difference is exact to a few 2^-53 * 5.5e4 = 6e-12, so
    # |G|^2 to 2 |G| times that; 1e-10 allows sixteen such roundings
    scale = np.abs(out[:, :, k["member"]]).max()
    assert np.abs(out[:, :, k["member"]] - out[:, :, k["mean"]] - (M - 1) / M * out[:, :, k["spread"]]).max() <= 1e-14 * scale
    tol = 2.0 * np.sqrt(np.abs(out[:, :, k["error_member"]]).max()) * 1e-10
    assert np.abs(out[:, :, k["error_member"]] - out[:, :, k["error_mean"]] - (M - 1) / M * out[:, :, k["spread"]]).max() <= tol


def test_the_reference_gives_a_single_member_zero_spread_and_three_slots_without_a_truth():
    members, _ = R.case(30, 3, 1, False)
    out, lim = R.spectra(members, None, [0], [(0, 3)], np.ones(3))
    assert out.shape == (1, 1, 3, 16) and not out[0, 0, 2].any() and not lim[0, 0, 2].any()
    assert np.array_equal(out[0, 0, 0], out[0, 0, 1])


# ---- the host algebra -------------------------------------------------------------------------------------------------------------------- #
def synthetic(knee=10, M=4, W=64, times=2):
    lat, lon = grid(33, W)
    req = S.check_request(["z500", "u850", "v850"], lat, lon, M, {"channels": ["z500", "u850", "v850"], "bands": {"nh_mid": (30, 60), "globe": None}})
    K = S.n_bins(W)
    k = np.arange(K, dtype=np.float64)
    truth = np.where(k > 0, np.maximum(k, 1.0) ** -3.0, 5.0)
    power = np.zeros((times, 3, 2, 6, K))
    for t in range(times):
        kn = knee - 3 * t                                                      # the forecast loses its small scales with lead time
        power[t, :, :, 0] = np.where(k <= kn, truth, 0.1 * truth)              # member: a knee at kn
        power[t, :, :, 3] = truth
        power[t, :, :, 2] = 0.25 * truth                                       # spread
        power[t, :, :, 4] = truth                                              # error of the mean
    power[:, 1] *= 2.0
    power[:, 2] *= 4.0
    return S.Spectra(list(range(times)), req["channels"], req["bands"], req["rows"], lat, W, M, power, "toy", "fid"), lat, truth


def test_wavelength_is_the_circumference_at_the_bands_mean_latitude_over_k():
    sp, lat, _ = synthetic()
    w = area_weights(lat)
    j0, j1 = S.band_rows(lat, (30, 60))
    phi = (w[j0:j1] * lat[j0:j1]).sum() / w[j0:j1].sum()
    assert 30 < phi < 60 and sp.band_latitude("nh_mid") == pytest.approx(phi)
    lam = sp.wavelength_km("nh_mid")
    assert np.isinf(lam[0]) and lam[1] == pytest.approx(2 * math.pi * 6371.0 * math.cos(math.radians(phi)))
    assert np.allclose(lam[1:] * np.arange(1, lam.size), lam[1])
    assert abs(sp.band_latitude("globe")) < 1e-9 and sp.wavelength_km("globe")[4] == pytest.approx(2 * math.pi * 6371.0 / 4)
    with pytest.raises(ValueError, match="band 'tropics' was not requested"):
        sp.wavelength_km("tropics")


def test_kinetic_energy_effective_resolution_ratio_and_spread_skill():
    sp, _, truth = synthetic(knee=10, M=4)
    ke = sp.kinetic_energy(850)
    assert ke.shape == (2, 2, 33) and np.allclose(ke[0, 0, :11], 0.5 * (2 + 4) * truth[:11])
    with pytest.raises(ValueError, match="u500"):
        sp.kinetic_energy(500)
    lam = sp.wavelength_km("nh_mid")
    assert sp.effective_resolution("z500", "nh_mid").tolist() == [lam[10], lam[7]]          # the knee, per lead time
    assert sp.effective_resolution("z500", "nh_mid", ratio=0.05).tolist() == [lam[-1], lam[-1]]      # never below 0.05: resolved to the grid
    assert np.isinf(sp.effective_resolution("z500", "nh_mid", ratio=1.5)).all()                       # already wavenumber 1 falls short
    r = sp.ratio("member", "truth")
    assert r.shape == (2, 3, 2, 33) and np.allclose(r[0, 0, 0, 1:11], 1.0) and np.allclose(r[0, 0, 0, 11:], 0.1)
    ss = sp.spread_skill("z500", "globe")
    assert ss.shape == (2, 33) and np.allclose(ss, math.sqrt(5 / 4 * 0.25))
    with pytest.raises(ValueError, match="no 'power' spectrum"):
        sp.ratio("power", "truth")


def test_power_is_labelled_and_survives_json(tmp_path):
    sp, _, _ = synthetic()
    assert sp.power.dims == ("time", "channel", "band", "kind", "wavenumber")
    assert sp.power.kind.values.tolist() == list(S.KINDS) and sp.power.band.values.tolist() == ["nh_mid", "globe"]
    assert sp.power.wavenumber.values.tolist() == list(range(33)) and sp.power.values.dtype == np.float64
    sp.power.values[0, 0, 0, 0, 3] = np.nan
    path = sp.save(tmp_path)
    assert path.endswith("fid/toy-spectra.json")
    back = S.Spectra.load(path)
    assert np.array_equal(back.power.values, sp.power.values, equal_nan=True) and back.bands == sp.bands and back.rows == sp.rows
    assert back.n_members == 4 and back.kinds == sp.kinds and np.array_equal(back.wavelength_km("nh_mid"), sp.wavelength_km("nh_mid"))
    without = S.Spectra([0], ["a"], ["globe"], [(0, 33)], np.linspace(90, -90, 33), 64, 1, np.zeros((1, 1, 1, 3, 33)))
    assert without.kinds == ["member", "mean", "spread"]
    with pytest.raises(ValueError, match="needs a truth"):
        without.ratio("member", "truth")


# ---- the request ------------------------------------------------------------------------------------------------------------------------- #
def test_check_request_normalises_and_maps_degrees_to_rows():
    lat, lon = grid(721, 1440)
    req = S.check_request(["z500", "t2m"], lat, lon, 50, {"channels": ["t2m"]})
    assert req["bands"] == ["nh_mid", "tropics", "sh_mid", "globe"] and req["index"] == [1]
    assert req["rows"] == [(120, 241), (280, 441), (480, 601), (0, 721)]       # lat_s <= lat <= lat_n, the convention of scenarios.region_index
    up = S.check_request(["z500"], lat[::-1], lon, 1, {"channels": ["z500"], "bands": {"nh_mid": (30, 60)}})
    assert up["rows"] == [(480, 601)]


def test_check_request_refusals():
    lat, lon = grid(49, 192)
    names = ["z500", "t2m"]
    ok = {"channels": ["z500"]}
    for spec, M, msg in (
            ({"channels": ["q700"]}, 3, "channel 'q700' is not an output channel"),
            ({"channels": []}, 3, "0 channels"),
            ({"channels": ["z500", "z500"]}, 3, "named twice"),
            ({"channels": ["z500"], "bands": {"x": (40, 30)}}, 3, "is empty"),
            ({"channels": ["z500"], "bands": {"x": (31, 32)}}, 3, "holds no row"),
            ({"channels": ["z500"], "bands": {"x": (30, 95)}}, 3, "outside the grid"),
            ({"channels": ["z500"], "bands": {}}, 3, "1 to 8 named latitude ranges"),
            ({"channels": ["z500"], "bands": {str(k): None for k in range(9)}}, 3, "1 to 8 named latitude ranges"),
            ({"channels": ["z500"], "region": None}, 3, "unknown keys"),
            (ok, 0, "n_members = 0"), (ok, 65, "n_members = 65")):
        with pytest.raises(ValueError, match=msg):
            S.check_request(names, lat, lon, M, spec)
    for other in ("ws10m", "t2m_max_24h"):                                     # names of other products the caller cannot serve are refused by name
        with pytest.raises(ValueError, match="regridded or aggregated"):
            S.check_request(names, lat, lon, 3, {"channels": [other]}, other=["ws10m", "t2m_max_24h"])
    with pytest.raises(ValueError, match="2\\^a 3\\^b 5\\^c"):
        S.check_request(names, lat, np.arange(14) * (360 / 14), 3, ok)
    with pytest.raises(ValueError, match="a dict"):
        S.check_request(names, lat, lon, 3, ["z500"])
    with pytest.raises(ValueError, match="not among the scored channels"):
        S.check_scored(["z500", "t2m"], ["z500"])


def test_merge_puts_raw_and_derived_spectra_in_the_requested_order():
    sp, lat, _ = synthetic()
    other = S.Spectra(sp.times, ["ws10m"], sp.bands, sp.rows, lat, 64, 4, 7.0 * sp.power.values[:, :1], "toy", "fid")
    both = S.merge([sp, other], ["u850", "ws10m", "z500", "v850"])
    assert both.channels == ["u850", "ws10m", "z500", "v850"] and both.power.values.shape == (2, 4, 2, 6, 33)
    assert np.array_equal(both.power.values[:, 1], 7.0 * sp.power.values[:, 0]) and np.array_equal(both.power.values[:, 2], sp.power.values[:, 0])
    assert S.merge([sp], sp.channels) is sp
    with pytest.raises(ValueError, match="same times, bands and kinds"):
        S.merge([sp, S.Spectra([5, 6], ["ws10m"], sp.bands, sp.rows, lat, 64, 4, sp.power.values[:, :1])], ["z500", "ws10m"])


def test_ensemble_validate_refuses_a_bad_spectra_request_before_the_device():
    from test_ens_cpu import T0, _Model
    from skyrim_amd import ensemble as E
    m = _Model()                                                               # channels u1000, v1000, t2m on a 9 x 96 grid; its loop must not start
    ok = {"channels": ["t2m"], "bands": {"tropics": (-20, 20), "globe": None}}
    assert E.validate(m.model, 2, 3, 0, (), None, None, None, 1, False, spectra=ok)[3] == [0, 1, 2]
    both = {"channels": ["ws1000", "t2m"]}                                     # a derived field next to a raw channel
    assert E.validate(m.model, 2, 3, 0, (), None, None, None, 1, False, spectra=both, derived=["ws1000"])[3] == [0, 1, 2]
    for kw, msg in ((dict(spectra={"channels": ["msl"]}), "not an output channel"),
                    (dict(spectra={"channels": ["ws1000"]}), "not an output channel"),          # a derived field that was not asked for
                    (dict(spectra={"channels": ["t2m_max_12h"]}, aggregates=["t2m:max:12h"]), "regridded or aggregated"),
                    (dict(spectra={**ok, "bands": {"x": (50, 40)}}), "empty"), (dict(spectra={**ok, "bands": {"x": (0, 100)}}), "outside"),
                    (dict(spectra={**ok, "bands": {"x": (1, 2)}}), "no row"), (dict(spectra=ok, n_members=65), "members")):
        args = dict(n_steps=2, n_members=3)
        args.update(kw)
        with pytest.raises(ValueError, match=msg):
            m.ensemble_forecast(T0, **args)
    assert E.EnsembleForecast("m", 1, 0, 0.0).spectra is None
    with pytest.raises(ValueError, match="not an output channel"):
        m.spectrum_forecast(T0, n_steps=1, spectra={"channels": ["msl"]})


def test_factor_and_bound_factor():
    assert S.factor(1440) == [4, 4, 2, 3, 3, 5] == R.factor(1440) and S.factor(45) == [3, 3, 5] and S.factor(64) == [4, 4, 4] and S.factor(2) == [2]
    assert S.factor(7) == [] and S.factor(14) == [] and S.factor(4100) == [] and S.factor(1) == [] and S.factor(8192) == []
    for W in (30, 45, 48, 64, 1440, 4096):
        assert S.bound_factor(W) == pytest.approx(R.c_w(W), rel=1e-15)
    assert 60 < S.bound_factor(1440) < 70                                      # the header's 64.6; one changed value moves a coefficient by 1.2e4 u rms
    assert S.bound(1440, 3.0, 4.0) == pytest.approx(S.bound_factor(1440) * 2.0 ** -24 * 5.0)


# ---- the library ------------------------------------------------------------------------------------------------------------------------- #
@needs_lib
def test_library_exports_every_symbol_of_the_header_and_the_constants_match():
    text = HEADER.read_text()
    declared = re.findall(r"^(?:int|void|size_t|double)\s+(skspec_\w+)\s*\(", text, re.M)
    assert sorted(declared) == sorted(S.EXPORTS) == ["skspec_abi_version", "skspec_bound_factor", "skspec_run", "skspec_twiddles", "skspec_workspace_bytes"]
    lib = S.load_library()
    for name in declared:
        assert hasattr(lib, name)
    assert lib.skspec_abi_version() == S.ABI_VERSION == int(re.search(r"#define SKSPEC_ABI_VERSION (\d+)", text).group(1))
    for macro, value in (("MAX_MEMBERS", S.MAX_MEMBERS), ("MAX_CHANNELS", S.MAX_CHANNELS), ("MAX_BANDS", S.MAX_BANDS), ("MIN_W", S.MIN_W),
                         ("MAX_W", S.MAX_W), ("MAX_H", S.MAX_H), ("CHUNK", S.CHUNK), ("SLOTS", S.SLOTS)):
        assert int(re.search(rf"#define SKSPEC_{macro} (\d+)", text).group(1)) == value
    assert len(S.KINDS) == S.SLOTS and [re.search(rf"slot {i}\s+(\w+)", text).group(1) for i in range(6)] == list(S.KINDS)
    for W in (2, 30, 45, 1440, 4096):
        assert lib.skspec_bound_factor(W) == pytest.approx(S.bound_factor(W), rel=1e-15)
    assert lib.skspec_bound_factor(7) == 0.0 and "c_1440 (4, 4, 2, 3, 3, 5) = 64.6" in text
    from skyrim_amd import ops
    assert "zonal_spectra" in ops.OP_NAMES


@needs_lib
def test_twiddles_are_the_float64_values_rounded_once():
    for W in (45, 64, 1440):
        n = np.arange(W)
        tw = S.twiddles(W)
        assert tw.dtype == np.float32 and tw.shape == (W, 2)
        assert np.array_equal(tw[:, 0], np.cos(2 * np.pi * n / W).astype(np.float32))
        assert np.array_equal(tw[:, 1], (-np.sin(2 * np.pi * n / W)).astype(np.float32))
    lib = S.load_library()
    buf = np.zeros(64, np.float32)
    for W in (7, 14, 4100, 1, 0):
        assert lib.skspec_twiddles(W, buf.ctypes.data_as(ctypes.c_void_p)) == E_ARG
    assert lib.skspec_twiddles(8, None) == E_ARG and not buf.any()


BANDS = [(0, 33), (4, 12), (8, 9)]


def good_run():
    d = S.describe(5, 6, 33, 48, [0, 5, 5], BANDS, truth=True)                 # overlapping bands, a one-row band, a repeated channel
    d.members, d.truth, d.lat_weight, d.twiddles, d.out, d.workspace = FAKE, 5 * FAKE, 2 * FAKE, 6 * FAKE, 3 * FAKE, 4 * FAKE
    d.workspace_bytes = S.workspace_bytes(5, 33, 48, 3, BANDS, True)
    return d


@needs_lib
def test_workspace_bytes_and_its_refusals():
    # segments [0, 4), [4, 8), [8, 9), [9, 12), [12, 33): 2 + 2 + 1 + 1 + 7 chunks of at most min(8, nc) = 3 rows; 6 slots of 25 bins
    assert S.workspace_bytes(5, 33, 48, 3, BANDS, True) == 3 * 13 * 6 * 25 * 8
    assert S.workspace_bytes(5, 33, 48, 3, BANDS, False) == 3 * 13 * 3 * 25 * 8
    assert S.workspace_bytes(5, 33, 48, 8, BANDS, True) == S.workspace_bytes(5, 33, 48, 32, BANDS, True) // 4 == 8 * 7 * 6 * 25 * 8
    assert S.workspace_bytes(50, 721, 1440, 8, [(120, 241), (280, 441), (480, 601), (0, 721)], True) == 8 * 93 * 6 * 721 * 8
    assert S.workspace_bytes(1, 5, 45, 1, [(1, 3)], False) == 1 * 2 * 3 * 23 * 8                      # rows outside every band cost nothing
    for kw in (dict(M=0), dict(M=65), dict(W=7), dict(W=14), dict(W=4100), dict(W=1), dict(nc=0), dict(nc=33), dict(H=0), dict(H=4097)):
        args = dict(M=5, H=33, W=48, nc=3)
        args.update(kw)
        assert S.workspace_bytes(args["M"], args["H"], args["W"], args["nc"], BANDS, True) == 0, kw
    for bands in ([], [(0, 33)] * 9, [(4, 4)], [(5, 4)], [(-1, 3)], [(0, 34)]):
        assert S.workspace_bytes(5, 33, 48, 3, bands, True) == 0, bands


@needs_lib
def test_run_refuses_bad_arguments_without_a_gpu():
    lib = S.load_library()
    assert lib.skspec_run(None, None) == E_ARG and lib.skspec_workspace_bytes(None) == 0

    def refused(**kw):
        d = good_run()
        for k, v in kw.items():
            setattr(d, k, v)
        return lib.skspec_run(ctypes.byref(d), None) == E_ARG
    assert refused(members=None) and refused(lat_weight=None) and refused(twiddles=None) and refused(out=None) and refused(workspace=None)
    assert refused(members=FAKE + 4) and refused(lat_weight=2 * FAKE + 4) and refused(twiddles=6 * FAKE + 4) and refused(out=3 * FAKE + 4)
    assert refused(workspace=4 * FAKE + 4) and refused(truth=5 * FAKE + 2)     # 8-byte tables and doubles, 4-byte states
    assert refused(M=0) and refused(M=65)
    assert refused(W=7) and refused(W=14) and refused(W=4100) and refused(W=1)
    assert refused(nc=0) and refused(nc=33) and refused(nb=0) and refused(nb=9)
    assert refused(C=0) and refused(H=0) and refused(H=4097) and refused(C=69, H=4096, W=4096)
    assert refused(workspace_bytes=S.workspace_bytes(5, 33, 48, 3, BANDS, True) - 1)
    d = good_run()
    d.truth = None                                                             # three slots: a smaller workspace is enough
    d.workspace_bytes = S.workspace_bytes(5, 33, 48, 3, BANDS, False) - 1
    assert lib.skspec_run(ctypes.byref(d), None) == E_ARG
    for b, (j0, j1) in ((1, (12, 12)), (1, (12, 4)), (2, (8, 34)), (0, (-1, 33))):      # j1 <= j0, j1 > H, j0 < 0
        d = good_run()
        d.j0[b], d.j1[b] = j0, j1
        assert lib.skspec_run(ctypes.byref(d), None) == E_ARG
    for bad in (-1, 6):
        d = good_run()
        d.channels[1] = bad
        assert lib.skspec_run(ctypes.byref(d), None) == E_ARG


# ---- the command line -------------------------------------------------------------------------------------------------------------------- #
def test_command_line_options_and_refusals():
    from click.testing import CliRunner
    from skyrim_amd import spectra_cli as cli
    assert cli.parse_band("nh_mid=30,60") == ("nh_mid", (30.0, 60.0)) and cli.parse_band("all=globe") == ("all", None)
    for bad in ("30,60", "x=30", "x=a,b", "=1,2", "x=1,2,3"):
        with pytest.raises(ValueError, match="NAME=LAT_S,LAT_N"):
            cli.parse_band(bad)
    assert cli.request(("z500", "u850"), ("nh_mid=30,60", "all=globe"), 3, "out.json") == dict(
        channels=["z500", "u850"], bands={"nh_mid": (30.0, 60.0), "all": None})
    assert cli.request(("z500",), (), 1, "") == dict(channels=["z500"])           # the default bands are check_request's
    for args, msg in ((((), (), 1, ""), "--channel"), ((("z500",), (), 0, ""), "--members"), ((("z500",), (), 65, ""), "--members"),
                      ((("z500",), (), 1, "out.csv"), ".json"), ((("z500",), ("a=1,2", "a=3,4"), 1, ""), "named twice"),
                      ((("z500",), tuple(f"b{k}=globe" for k in range(9)), 1, ""), "at most 8"), ((("z500",), ("a",), 1, ""), "NAME=LAT_S")):
        with pytest.raises(ValueError, match=msg):
            cli.request(*args)
    with pytest.raises(ValueError, match="n_steps"):
        cli.request(("z500",), (), 1, "", n_steps=-1)
    run = CliRunner().invoke
    for argv in ([], ["--channel", "z500", "--members", "0"], ["--channel", "z500", "--band", "1,2"], ["--channel", "z500", "--perturbation", "x"],
                 ["--channel", "z500", "--output", "x.txt"], ["--channel", "z500", "--modal"]):
        res = run(cli.spectra, argv)
        assert res.exit_code == 2, (argv, res.output)
    assert {"channels", "bands", "members", "n_steps", "output", "truth", "model_name", "date", "time", "lead_time",
            "initial_conditions"} <= {o.name for o in cli.spectra.params}
    assert cli.ranges(33) == [(1, 4), (4, 10), (10, 30), (30, 33)] and cli.ranges(3) == [(1, 3)]
    sp, _, _ = synthetic()
    out = cli.lines(sp)
    assert len(out) == 2 * 3 * 2 * 7 and out[0].startswith("0 z500 nh_mid member [k1-3 k4-9 k10-29 k30-32]: ")
    assert out[6].startswith("0 z500 nh_mid effective resolution: ") and out[6].endswith(" km")
