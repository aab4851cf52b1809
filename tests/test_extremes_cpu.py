"""Climate-relative extremes without a GPU: the binding of libskyrim_clim.so against its header, every SKCLIM_E_ARG path, the host
tables, ``Climate`` (slices, files), every refusal of ``extremes.check_request`` in its order, and the float32 restatement against the
float64 formula and a direct quadrature of the integral."""
import ctypes
import datetime
import math
import re
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

import _extremes_reference as R
from skyrim_amd import climate as K
from skyrim_amd import extremes as X
from skyrim_amd import native

ROOT = Path(__file__).resolve().parents[1]
E_ARG = -1
PTR = 0x7F0000001000                          # a 16-byte aligned address that is never read: every refusal comes before the GPU


# ---- the binding ------------------------------------------------------------------------------------------------------------------------- #
def test_header_binding_and_build_line():
    text = (ROOT / "include/skyrim_clim.h").read_text()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(skclim_[a-z0-9_]+)\s*\(", code))
    lib = K.load_library()
    assert declared == set(K.EXPORTS) and all(hasattr(lib, s) for s in declared)
    assert lib.skclim_abi_version() == K.ABI_VERSION == int(re.search(r"#define SKCLIM_ABI_VERSION (\d+)", text).group(1))
    assert K.SPEC.env == "SKYRIM_CLIM_LIB"
    for name, value in (("MEMBERS", K.MAX_MEMBERS), ("FIELDS", K.MAX_FIELDS), ("LEVELS", K.MAX_LEVELS), ("SOT", K.MAX_SOT),
                        ("PROB", K.MAX_PROB), ("SAMPLES", K.MAX_SAMPLES)):
        assert f"#define SKCLIM_MAX_{name} {value}\n" in text
    assert (K.MAX_MEMBERS, K.MAX_FIELDS, K.MAX_LEVELS, K.MAX_SOT, K.MAX_PROB, K.MAX_SAMPLES) == (64, 16, 128, 4, 8, 2048)
    assert "#define SKCLIM_E_ARG (-1)" in text and "#define SKCLIM_E_HIP (-2)" in text
    assert ctypes.sizeof(K.SotReq) == 16 and ctypes.sizeof(K.ProbReq) == 8
    # members, six ints, channels, clim, Q, four level tables, floor, n_sot + requests, n_prob + requests, padding, three outputs
    assert ctypes.sizeof(K.ExtremesDesc) == 8 + 6 * 4 + 64 + 8 + 4 + 4 * 512 + 64 + 4 + 64 + 4 + 64 + 4 + 3 * 8
    assert ctypes.sizeof(K.QuantilesDesc) == 8 + 5 * 4 + 64 + 4 + 512 + 512 + 8
    make = (ROOT / "skyrim_amd/csrc/Makefile").read_text()
    assert "-ffp-contract=off -shared -o $@ clim_ops.hip" in make and "$(LIB_CLIM)" in make.split("all:")[1].splitlines()[0]
    assert "$(LIB_CLIM)" in make.split("clean:")[1]
    for doc in (native.__doc__, make.splitlines()[0]):
        assert ",clim," in doc
    from skyrim_amd import ops
    assert {"clim_extremes", "clim_quantiles"} <= set(ops.OP_NAMES)
    assert [K.tile_points(n) for n in (0, 1, 64, 128, 129, 1000, 2048, 2049)] == [0, 256, 256, 256, 128, 32, 16, 0]


def good_extremes():
    d = K.describe_extremes(7, 16, 5, 9, 12, [0, 4, 2], np.linspace(0, 1, 11), [-math.inf, 0.0, 1.0],
                            [(3, 0.25, 9, 5)], [(3, False), (9, True)])
    d.members, d.clim, d.efi, d.sot, d.prob = PTR, PTR, PTR, PTR, PTR
    return d


def good_quantiles():
    d = K.describe_quantiles(100, 3, 9, 12, [0, 2], np.linspace(0, 1, 11))
    d.samples, d.clim = PTR, PTR
    return d


def test_extremes_refuses_bad_arguments_without_a_gpu():
    lib = K.load_library()
    assert lib.skclim_extremes(None, None) == E_ARG

    def refused(edit=None, **kw):
        d = good_extremes()
        for k, v in kw.items():
            setattr(d, k, v)
        if edit is not None:
            edit(d)
        return lib.skclim_extremes(ctypes.byref(d), None) == E_ARG
    assert refused(members=None) and refused(clim=None) and refused(members=PTR + 4) and refused(clim=PTR + 2)
    assert refused(M=0) and refused(M=65) and refused(member_align=8) and refused(nf=0) and refused(nf=17)
    assert refused(Q=1) and refused(Q=129) and refused(C=0) and refused(H=0) and refused(W=0)
    assert refused(n_sot=5) and refused(n_sot=-1) and refused(n_prob=9) and refused(n_prob=-1)
    assert refused(sot=None) and refused(prob=None) and refused(n_sot=0) and refused(n_prob=0)      # a count and its pointer disagree
    assert refused(efi=None, sot=None, prob=None, n_sot=0, n_prob=0)                                   # nothing asked for
    assert refused(efi=PTR + 1) and refused(sot=PTR + 2) and refused(prob=PTR + 3)
    assert refused(C=1 << 15, H=1 << 8, W=1 << 8) and refused(C=5, H=1 << 13, W=1 << 13)              # C H W, nf Q H W > 2^30
    for i, bad in ((1, -1), (1, 5)):
        assert refused(lambda d: d.channels.__setitem__(i, bad))
    assert refused(lambda d: d.p.__setitem__(0, -0.1)) and refused(lambda d: d.p.__setitem__(10, 1.5))
    assert refused(lambda d: d.p.__setitem__(4, d.p[3])) and refused(lambda d: d.p.__setitem__(4, float("nan")))
    for tab in ("A", "B", "rdp"):
        for bad in (0.0, -1.0, math.inf, math.nan):
            assert refused(lambda d: getattr(d, tab).__setitem__(2, bad)), (tab, bad)
    assert refused(lambda d: d.floor.__setitem__(1, math.nan))
    for field, bad in (("q_index", -1), ("q_index", 7), ("q_frac", 1.0), ("q_frac", -0.1), ("q_frac", math.nan), ("k_ref", 11), ("k_ref", -1),
                       ("k_base", 11), ("k_base", -1)):
        assert refused(lambda d: setattr(d.sot_req[0], field, bad)), (field, bad)
    assert refused(lambda d: setattr(d.prob_req[1], "k", 11)) and refused(lambda d: setattr(d.prob_req[0], "k", -1))
    with pytest.raises(NotImplementedError):
        import torch
        torch.ops.skyrim_hip.clim_quantiles([torch.zeros(1, 2, 2)], torch.zeros(1, dtype=torch.int64), [0], [0.5], torch.zeros(1, 1, 2, 2))


def test_quantiles_refuses_bad_arguments_without_a_gpu():
    lib = K.load_library()
    assert lib.skclim_quantiles(None, None) == E_ARG

    def refused(edit=None, **kw):
        d = good_quantiles()
        for k, v in kw.items():
            setattr(d, k, v)
        if edit is not None:
            edit(d)
        return lib.skclim_quantiles(ctypes.byref(d), None) == E_ARG
    assert refused(samples=None) and refused(clim=None) and refused(samples=PTR + 4) and refused(clim=PTR + 1)
    assert refused(N=0) and refused(N=2049) and refused(Q=0) and refused(Q=129) and refused(nf=0) and refused(nf=17)
    assert refused(C=0) and refused(H=0) and refused(W=0) and refused(C=3, H=1 << 14, W=1 << 14)
    assert refused(lambda d: d.channels.__setitem__(0, 3)) and refused(lambda d: d.channels.__setitem__(1, -1))
    assert refused(lambda d: d.q_index.__setitem__(5, 100)) and refused(lambda d: d.q_index.__setitem__(5, -1))
    assert refused(lambda d: d.q_frac.__setitem__(5, 1.0)) and refused(lambda d: d.q_frac.__setitem__(5, math.nan))


def test_every_sample_count_gives_a_descriptor_the_library_takes():
    """``h = (N - 1) level`` can fall just below an integer in double (100 * 0.29 = 28.999999999999996): its fraction would round to
    1.0f, which the library refuses.  ``positions`` hands it the next index with fraction 0: every N from 1 to 2048 with the default
    levels passes the library's own argument check (``skclim_quantiles_check``: no launch, the pointers are never read)."""
    lev = np.linspace(0, 1, 101)
    lib = K.load_library()
    for N in range(1, 2049):
        qi, qf = K.positions(lev, N)
        f32 = qf.astype(np.float32)
        assert np.all((qi >= 0) & (qi < N)) and np.all((f32 >= 0) & (f32 < 1)), N
        assert np.all(np.diff(qi + qf) >= 0) and np.all(np.abs((qi + qf) - (N - 1) * lev) <= 1e-9), N
        d = K.describe_quantiles(N, 3, 9, 12, [0, 2], lev)
        d.samples, d.clim = PTR, PTR
        assert lib.skclim_quantiles_check(ctypes.byref(d)) == 0, N
    qi, qf = K.positions(lev, 101)
    assert (qi[29], qf[29]) == (29, 0.0) and qi.tolist() == list(range(101))
    d = K.describe_quantiles(101, 3, 9, 12, [0, 2], lev)
    d.samples, d.clim = PTR, PTR
    d.q_frac[29] = 1.0                                                       # what 100 * 0.29 used to give: refused by the check and the call
    assert lib.skclim_quantiles_check(ctypes.byref(d)) == E_ARG and lib.skclim_quantiles(ctypes.byref(d), None) == E_ARG
    assert lib.skclim_quantiles_check(None) == E_ARG and lib.skclim_extremes_check(None) == E_ARG
    # the members' quantile of a SOT tail goes through the same normalisation: every M, tails that fall just below an integer included
    lev11 = np.linspace(0, 1, 11)
    for M in range(2, 65):
        for q in (0.29, 0.57, 0.58, 0.07, 0.93, 0.9, 0.1):
            k, f = K._position([(M - 1) * q], M - 1)
            assert 0 <= k[0] < M and 0 <= np.float32(f[0]) < 1 and abs(k[0] + f[0] - (M - 1) * q) <= 1e-9
            e = K.describe_extremes(M, 16, 5, 9, 12, [0], lev11, None, [(int(k[0]), float(f[0]), 9, 5)], [])
            e.members, e.clim, e.sot = PTR, PTR, PTR
            assert lib.skclim_extremes_check(ctypes.byref(e)) == 0, (M, q)
    assert any(np.float32((M - 1) * q - math.floor((M - 1) * q)) >= 1 for M in range(2, 65) for q in (0.29, 0.57, 0.58, 0.07, 0.93))


# ---- the host tables --------------------------------------------------------------------------------------------------------------------- #
def test_host_tables():
    for levels in (np.linspace(0, 1, 101), np.linspace(0, 1, 2), [0.0, 0.01, 0.3, 0.99, 1.0], np.linspace(0, 1, 128)):
        t = K.tables(levels)
        assert abs(math.fsum(t["B"]) - math.pi / 2) <= 4 * np.spacing(math.pi) and abs(math.fsum(t["A"]) - math.pi) <= 4 * np.spacing(math.pi)
        assert np.all(t["A"] > 0) and np.all(t["B"] > 0) and np.allclose(t["rdp"] * np.diff(t["p"]), 1.0, rtol=1e-15)
    d = K.describe_extremes(3, 4, 1, 2, 2, [0], np.linspace(0, 1, 101))
    t = K.tables(np.linspace(0, 1, 101))
    assert d.Q == 101 and np.array_equal(np.array(d.B[:100]), t["B"].astype(np.float32)) and d.floor[0] == -math.inf
    for bad in ([0.5, 0.5], [0.6, 0.5], [-0.1, 0.5], [0.5, 1.1], [0.1, math.nan], []):
        with pytest.raises(ValueError, match="strictly increasing"):
            K.check_levels(bad)
    qi, qf = K.positions([0.0, 0.25, 0.5, 1.0], 10)
    assert qi.tolist() == [0, 2, 4, 9] and qf.tolist() == [0.0, 0.25, 0.5, 0.0]
    lev = np.linspace(0, 1, 101)
    k, frac, ref, base = K.sot_request(lev, 0.9, 51)
    assert (k, ref, base) == (45, 99, 90) and 0 <= frac < 1e-12 and K.sot_request(lev, 0.1, 51)[2:] == (1, 10)
    with pytest.raises(ValueError, match=r"no level 0\.995"):
        K.sot_request(lev, 0.95, 51)
    assert K.field_groups(20, 101, 721 * 1440) == [list(range(0, 10)), list(range(10, 20))]
    assert K.field_groups(3, 11, 49 * 192) == [[0, 1, 2]] and K.field_groups(17, 2, 4) == [list(range(16)), [16]]


# ---- the climate ------------------------------------------------------------------------------------------------------------------------- #
LAT, LON = np.linspace(90, -90, 5), np.arange(8) * 45.0
LEV = np.array([0.0, 0.01, 0.1, 0.5, 0.9, 0.99, 1.0])


def planes(seed, fields=2):
    rng = np.random.default_rng(seed)
    return np.sort(rng.standard_normal((LEV.size, fields, LAT.size, LON.size)).astype(np.float32), axis=0)


def test_climate_at_year_wrap_hours_and_gap():
    c = K.Climate(LEV, ["t2m", "ws10m"], LAT, LON, {(12, 28, 0): planes(0), (12, 28, 12): planes(1), (1, 10, 0): planes(2), (1, 10, 12): planes(3),
                                                     (7, 1, 0): planes(4), (7, 1, 12): planes(5)})
    at = lambda *a: c.at(datetime.datetime(*a))[0]      # noqa: E731
    assert at(2023, 12, 31, 0) == (12, 28, 0) and at(2024, 1, 2, 12) == (12, 28, 12)              # across the year's end
    assert at(2024, 1, 5, 0) == (1, 10, 0) and at(2024, 7, 10, 12) == (7, 1, 12)
    assert c.at(np.datetime64("2024-01-05T00:00:00"))[1] is c.slices[(1, 10, 0)]
    with pytest.raises(ValueError, match="no slice for hour 06"):
        at(2024, 1, 5, 6)
    with pytest.raises(ValueError, match=r"nearest slice .* is 07-01, 16 days away \(max_gap_days = 15\)"):
        at(2024, 7, 17, 0)
    assert at(2024, 7, 16, 0) == (7, 1, 0)
    one = K.Climate(LEV, ["t2m"], LAT, LON, planes(0, 1))
    assert one.at(datetime.datetime(2031, 3, 3, 7))[0] is None
    daily = K.Climate(LEV, ["t2m"], LAT, LON, {(2, 29, None): planes(0, 1), (3, 20, None): planes(1, 1)})
    assert daily.at(datetime.datetime(2023, 3, 1, 17))[0] == (2, 29, None)                         # the 366-day circle holds Feb 29


def test_climate_refusals_each_with_its_own_text():
    with pytest.raises(ValueError, match="strictly increasing"):
        K.Climate([0.0, 0.5, 0.5], ["a"], LAT, LON, planes(0, 1)[:3])
    bad = planes(0)
    bad[3, 1, 2, 2] = bad[2, 1, 2, 2] - 1
    with pytest.raises(ValueError, match="decrease with the level"):
        K.Climate(LEV, ["a", "b"], LAT, LON, bad)
    ok = planes(0)
    ok[3, 1, 2, 2] = np.nan                                                   # non-decreasing wherever finite
    c = K.Climate(LEV, ["a", "b"], LAT, LON, ok)
    with pytest.raises(ValueError, match="has shape"):
        K.Climate(LEV, ["a"], LAT, LON, planes(0))
    with pytest.raises(ValueError, match="not the forecast's grid"):
        c.check_grid(LAT, LON + 1.0)
    c.check_grid(LAT, LON)
    with pytest.raises(ValueError, match="distinct names"):
        K.Climate(LEV, ["a", "a"], LAT, LON, planes(0))
    with pytest.raises(ValueError, match="either every slice carries an hour or none"):
        K.Climate(LEV, ["a", "b"], LAT, LON, {(1, 1, 0): planes(0), (1, 2, None): planes(1)})


def test_climate_save_open_round_trip_is_bit_exact(tmp_path):
    a, b = planes(7), planes(8)
    a[2, 0, 1, 1] = -0.0
    a[:, 1, 4, 7] = np.nan
    c = K.Climate(LEV, ["t2m", "ws10m_max_24h"], LAT, LON, {(2, 29, 6): a, (12, 1, 18): b}, n_samples=620, half_window_days=15)
    paths = c.save(tmp_path / "clim")
    assert sorted(Path(p).name for p in paths) == ["climate_0229_06.nc", "climate_1201_18.nc"]
    d = K.Climate.open(tmp_path / "clim")
    assert d.fields == c.fields and np.array_equal(d.levels, c.levels) and np.array_equal(d.lat, LAT) and np.array_equal(d.lon, LON)
    assert (d.n_samples, d.half_window_days) == (620, 15) and sorted(d.slices) == sorted(c.slices)
    for key in c.slices:
        assert np.array_equal(R.bits(d.slices[key]), R.bits(c.slices[key])), key
    one = K.Climate(LEV, ["t2m"], LAT, LON, planes(0, 1))
    one.save(tmp_path / "one")
    assert list(K.Climate.open(tmp_path / "one").slices) == [None]
    with pytest.raises(ValueError, match="no climate"):
        K.Climate.open(tmp_path / "none")


def test_calendar_groups_and_the_sample_limit():
    times = [datetime.datetime(2020 + y, 1, 1, h) + datetime.timedelta(days=d) for y in range(3) for d in range(40) for h in (0, 12)]
    g = K.calendar_groups(times, 5, hours=[0, 12], keys=[(1, 10)])
    assert sorted(g) == [(1, 10, 0), (1, 10, 12)] and all(len(v) == 3 * 11 for v in g.values())
    assert all(times[i].hour == 12 and abs(times[i].day - 10) <= 5 for i in g[(1, 10, 12)])
    assert len(K.calendar_groups(times, 0)) == 40                               # the days the times fall on, without hours
    from skyrim_amd.labeled import DataArray
    many = DataArray(np.zeros((2049, 1, 5, 8), np.float32), ["time", "channel", "lat", "lon"],
                     dict(time=[datetime.datetime(2000, 1, 1) + datetime.timedelta(hours=h) for h in range(2049)], channel=["t2m"], lat=LAT, lon=LON))
    with pytest.raises(ValueError, match=r"slice \(1, 15, None\) would take 2049 samples; at most 2048"):
        K.build_from_files(many, ["t2m"], half_window_days=200, keys=[(1, 15)])
    with pytest.raises(ValueError, match="neither channels of the files nor derived"):
        K.build_from_files(many, ["ws10m"])


# ---- the request ------------------------------------------------------------------------------------------------------------------------- #
def test_check_request_refuses_in_its_order():
    names, clim = ["t2m", "u10m", "v10m", "msl"], K.Climate(LEV, ["t2m", "ws10m", "ws10m_max_24h"], LAT, LON, planes(0, 3))
    check = lambda x, M=5, **kw: X.check_request(names, LAT, LON, M, x, **kw)      # noqa: E731
    full = dict(climate=clim, fields=["t2m", "ws10m"], efi=True, sot=[0.9, 0.1], above=[0.99], below=[0.01], floor={"ws10m": 0.0})
    r = check(full, derived=["ws10m"])
    assert (r.fields, r.efi, r.sot, r.prob, r.floor) == (["t2m", "ws10m"], True, [0.9, 0.1], [("above", 0.99), ("below", 0.01)], {"ws10m": 0.0})
    assert check(r) is r
    # each refusal with everything AFTER it in the order also wrong: the earlier one speaks
    later = dict(fields=["nope"], sot=[0.8], floor={"msl": 0.0})
    with pytest.raises(ValueError, match="a dict"):
        check(None)
    with pytest.raises(ValueError, match=r"unknown keys \['efo'\]"):
        check(dict(full, efo=True, **later))
    with pytest.raises(ValueError, match=r"fields \['nope'\] are neither"):
        check(dict(full, **later))
    with pytest.raises(ValueError, match=r"fields \['ws10m'\] are neither"):
        check(full)                                                            # a derived field the request does not make
    with pytest.raises(ValueError, match=r"the climate has no field \['msl'\]"):
        check(dict(full, fields=["t2m", "msl"], sot=[0.8], floor={"u10m": 0.0}))
    with pytest.raises(ValueError, match=r"sot: the climate has no level 0\.8\b"):
        check(dict(full, fields=["t2m"], sot=[0.8], above=[0.5] * 9, floor={"msl": 0.0}))
    with pytest.raises(ValueError, match=r"sot: the climate has no level 0\.95\b"):
        check(dict(full, fields=["t2m"], sot=[0.5], floor={}))                 # the reference level of the 0.5 tail: 1 - 0.5 / 10
    with pytest.raises(ValueError, match=r"above: the climate has no level 0\.95\b"):
        check(dict(full, fields=["t2m"], above=[0.95], floor={"msl": 0.0}))
    with pytest.raises(ValueError, match=r"below: the climate has no level 0\.0100001\b"):
        check(dict(full, fields=["t2m"], below=[0.0100001], floor={}))
    assert check(dict(full, fields=["t2m"], below=[0.01 + 1e-10], floor={})).prob[-1] == ("below", 0.01 + 1e-10)
    with pytest.raises(ValueError, match="5 SOT tails and 2 percentiles; at most 4 and 8"):
        check(dict(full, fields=["t2m"], sot=[0.9, 0.1, 0.9, 0.1, 0.9], floor={"msl": 0.0}))
    with pytest.raises(ValueError, match="2 SOT tails and 9 percentiles"):
        check(dict(full, fields=["t2m"], above=[0.5] * 8, floor={"msl": 0.0}))
    with pytest.raises(ValueError, match=r"floor names \['msl'\]"):
        check(dict(full, fields=["t2m"], floor={"msl": 0.0}), M=65)
    with pytest.raises(ValueError, match="1 to 64 members"):
        check(dict(full, fields=["t2m"], floor={}), M=65)
    with pytest.raises(ValueError, match="one state has none"):
        check(dict(full, fields=["t2m"], floor={}), M=1)
    with pytest.raises(ValueError, match="nothing asked for"):
        check(dict(climate=clim, fields=["t2m"], efi=False))
    with pytest.raises(ValueError, match="not the forecast's grid"):
        X.check_request(names, LAT[:4], LON, 5, dict(full, fields=["t2m"], floor={}))
    agg = check(dict(climate=clim, fields=["ws10m_max_24h"]), aggregates=["ws10m_max_24h"])
    assert agg.fields == ["ws10m_max_24h"] and agg.efi and not agg.sot and not agg.prob
    assert check(dict(climate=clim), derived=["ws10m"], aggregates=["ws10m_max_24h"]).fields == clim.fields      # default: every field of the climate


def test_ensemble_plan_takes_the_keyword_and_refuses_through_check_request():
    import inspect
    from skyrim_amd import ensemble as E
    from skyrim_amd.core.models.base import GlobalModel
    model = SimpleNamespace(out_channel_names=["t2m", "u10m", "v10m", "msl"], in_channel_names=["t2m", "u10m", "v10m", "msl"],
                            grid=SimpleNamespace(lat=LAT, lon=LON), time_step=datetime.timedelta(hours=6))
    clim = K.Climate(LEV, ["t2m"], LAT, LON, planes(0, 1))
    args = (model, 2, 3, 0, ("mean",), None, None, None, 1, False)
    assert E.validate(*args) == E.validate(*args, extremes=dict(climate=clim))
    assert E.plan_request(*args).extremes is None and E.plan_request(*args, extremes=dict(climate=clim, sot=[0.9])).extremes.sot == [0.9]
    with pytest.raises(ValueError, match="unknown keys"):
        E.validate(*args, extremes=dict(climate=clim, efy=1))
    for fn in (E.run, GlobalModel.ensemble_forecast, E.validate, E.plan_request):
        assert inspect.signature(fn).parameters["extremes"].default is None
    assert E.EnsembleForecast("pangu", 3, 0, 1e-3).extremes is None


# ---- the restatement --------------------------------------------------------------------------------------------------------------------- #
def test_restatement_against_float64_and_quadrature():
    rng = np.random.default_rng(5)
    for Q, M in ((2, 1), (3, 7), (11, 2), (101, 50), (128, 64)):
        lev = np.linspace(0, 1, Q)
        c = np.sort(rng.standard_normal((Q, 300)).astype(np.float32), axis=0)
        x = (rng.standard_normal((M, 300)) * 1.3 + 0.2).astype(np.float32)
        sot = [(int((M - 1) * 0.5), (M - 1) * 0.5 - int((M - 1) * 0.5), Q - 1, 0)] if M > 1 else []
        a, b = R.extremes32(x, c, lev, sot=sot), R.extremes64(x, c, lev, sot=sot)
        assert np.all(np.abs(a["efi"] - b["efi"]) <= b["efi_bound"]) and np.all(np.abs(a["efi"]) <= 1)
        assert np.all(np.abs(a["sot"] - b["sot"]) <= b["sot_bound"])
        assert np.all(R.extremes32(x * 0 + 100, c, lev)["efi"] == np.float32(1))                 # above the top level: exactly 1
        low = R.extremes32(x * 0 - 100, c, lev)["efi"]
        assert np.all(low >= -1) and np.all(low <= np.float32(-1) + 2 * b["efi_bound"].max())
    lev = np.linspace(0, 1, 101)
    for seed in range(4):                                                      # a few points against the integral itself
        r = np.random.default_rng(seed)
        c, x = np.sort(r.standard_normal(101)).astype(np.float32), (r.standard_normal(50) + 0.4 * seed).astype(np.float32)
        e = R.extremes32(x[:, None], c[:, None], lev)["efi"][0]
        assert abs(e - R.efi_quadrature(x, c, lev)) <= 1e-4
    # the floor leaves out the intervals at or below it; a non-finite input is the one quiet NaN
    c = np.sort(rng.standard_normal((11, 6)).astype(np.float32), axis=0)
    x = rng.standard_normal((5, 6)).astype(np.float32)
    lev = np.linspace(0, 1, 11)
    assert np.all(R.bits(R.extremes32(x, c, lev, floor=c.max() + 1)["efi"]) == 0)
    x[2, 3] = np.nan
    out = R.extremes32(x, c, lev, prob=[(4, False)])
    assert R.bits(out["efi"])[3] == 0x7FC00000 and R.bits(out["prob"])[0, 3] == 0x7FC00000 and np.isfinite(np.delete(out["efi"], 3)).all()
    # the builder's restatement: numpy's linear method within the header's bound, planes non-decreasing
    s = R.field(257, 3, 2, 5, 1)[:, 1].reshape(257, -1)
    q = R.quantiles32(s, np.linspace(0, 1, 101))
    exact, bound = R.quantile_bound(s, np.linspace(0, 1, 101))
    assert np.all(np.abs(q - exact) <= bound) and np.all(np.diff(q, axis=0) >= 0)
