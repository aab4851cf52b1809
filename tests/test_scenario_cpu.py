"""Ensemble scenarios without a GPU: the exports, descriptors and argument checks of libskyrim_gram.so, the region parser, the host
algebra of skyrim_amd/scenarios.py (centring, channel combination, Ward's clustering, representatives, EOFs, the energy score) against
restatements made directly from the members' fields (tests/_scenario_reference.py), planted clusters, a rank-2 spread, the tie rules,
the refusals of ``ensemble_forecast(scenarios=...)`` that come before the device, and the command line's options."""
from __future__ import annotations

import ctypes
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import _scenario_reference as R
from skyrim_amd import scenarios as S
from skyrim_amd.verify import area_weights

ROOT = Path(__file__).resolve().parents[1]
E_ARG = -1
FAKE = 0x10000                                                                 # never dereferenced: every call below is refused first


def grid(n_lat, n_lon):
    return np.linspace(90.0, -90.0, n_lat), np.arange(n_lon) * (360.0 / n_lon)


# ---- the library ------------------------------------------------------------------------------------------------------------------------ #
def test_library_exports_every_symbol_of_the_header_and_the_abi_matches():
    text = (ROOT / "include" / "skyrim_gram.h").read_text()
    declared = re.findall(r"^(?:int|void|size_t)\s+(skgram_\w+)\s*\(", text, re.M)
    assert sorted(declared) == sorted(S.EXPORTS) == ["skgram_abi_version", "skgram_combine", "skgram_run", "skgram_workspace_bytes"]
    lib = S.load_library()
    for name in declared:
        assert hasattr(lib, name)
    assert lib.skgram_abi_version() == S.ABI_VERSION == int(re.search(r"#define SKGRAM_ABI_VERSION (\d+)", text).group(1))
    for macro, value in (("MAX_MEMBERS", S.MAX_MEMBERS), ("MAX_CHANNELS", S.MAX_CHANNELS), ("MAX_OUT", S.MAX_OUT), ("TILE", S.TILE),
                         ("CHAIN", S.CHAIN), ("GROUPS", S.GROUPS)):
        assert int(re.search(rf"#define SKGRAM_{macro} (\d+)", text).group(1)) == value
    assert S.bound_factor() == (S.CHAIN + 3) * 2.0 ** -24 + 2.0 ** -40 and "(SKGRAM_CHAIN + 3) u + 2^-40" in text
    from skyrim_amd import ops
    assert {"gram", "member_combine"} <= set(ops.OP_NAMES)


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not installed")
def test_descriptor_layouts_match_the_header(tmp_path):
    probes = []
    for struct, cls in (("skgram_desc", S.GramDesc), ("skgram_combine_desc", S.CombineDesc)):
        fields = [n for n, _ in cls._fields_]
        probes.append((struct, cls, fields))
    src = tmp_path / "layout.cpp"
    body = ""
    for struct, _, fields in probes:
        body += f'  printf(" %zu", sizeof({struct}));\n' + "".join(f'  printf(" %zu", offsetof({struct}, {f}));\n' for f in fields)
    src.write_text('#include <cstdio>\n#include <cstddef>\n#include "skyrim_gram.h"\nint main() {\n' + body + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    r = subprocess.run(["hipcc", "-x", "c++", "-std=c++17", f"-I{ROOT / 'include'}", str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    for _, cls, fields in probes:
        assert got[0] == ctypes.sizeof(cls)
        assert got[1:1 + len(fields)] == [getattr(cls, f).offset for f in fields]
        got = got[1 + len(fields):]
    assert not got


def good_run():
    d = S.describe(5, 6, 33, 64, [0, 5, 5], (2, 20, 60, 10))                   # a box across the date line, a repeated channel
    d.members, d.lat_weight, d.out, d.workspace = FAKE, 2 * FAKE, 3 * FAKE, 4 * FAKE
    d.workspace_bytes = S.workspace_bytes(5, 3, 20, 10)
    return d


def test_workspace_bytes_and_its_refusals():
    assert S.workspace_bytes(5, 3, 20, 10) == 3 * 20 * 1 * 1024 * 8            # one tile per row, one block of 32 x 32 doubles
    assert S.workspace_bytes(33, 1, 721, 1440) == 1 * S.GROUPS * 3 * 1024 * 8  # 4326 tiles: the cap on the workgroups, three blocks
    assert S.workspace_bytes(32, 2, 1, 257) == 2 * 2 * 1024 * 8
    for args in ((1, 1, 1, 1), (65, 1, 1, 1), (5, 0, 1, 1), (5, 33, 1, 1), (5, 1, 0, 1), (5, 1, 1, 0), (5, 1, (1 << 21) + 1, 1),
                 (5, 1, (1 << 20) + 1, 257)):
        assert S.workspace_bytes(*args) == 0, args


def test_run_refuses_bad_arguments_without_a_gpu():
    lib = S.load_library()
    assert lib.skgram_run(None, None) == E_ARG

    def refused(**kw):
        d = good_run()
        for k, v in kw.items():
            setattr(d, k, v)
        return lib.skgram_run(ctypes.byref(d), None) == E_ARG
    assert refused(members=None) and refused(lat_weight=None) and refused(out=None) and refused(workspace=None)
    assert refused(members=FAKE + 4) and refused(lat_weight=2 * FAKE + 4) and refused(out=3 * FAKE + 4) and refused(workspace=4 * FAKE + 4)
    assert refused(truth=5 * FAKE + 2)                                         # 4-byte alignment of a state
    assert refused(M=1) and refused(M=65) and refused(M=64, truth=5 * FAKE)    # the truth is column 65
    assert refused(nc=0) and refused(nc=33)
    assert refused(C=0) and refused(H=0) and refused(W=0) and refused(C=69, H=4096, W=4096)
    assert refused(j0=-1) and refused(nj=0) and refused(j0=14, nj=20) and refused(nj=34)
    assert refused(i0=-1) and refused(i0=64) and refused(ni=0) and refused(ni=65)
    assert refused(workspace_bytes=S.workspace_bytes(5, 3, 20, 10) - 1) and refused(out_stride=24)
    d = good_run()
    d.truth, d.M, d.out_stride = 5 * FAKE, 32, 33 * 33                         # M' = 33: three blocks, a workspace three times as large
    assert lib.skgram_run(ctypes.byref(d), None) == E_ARG
    for bad in (-1, 6):
        d = good_run()
        d.channels[1] = bad
        assert lib.skgram_run(ctypes.byref(d), None) == E_ARG


def test_a_truth_column_with_enough_workspace_is_not_refused_for_its_count():
    """M' = M + 1 is what the limits apply to: 63 members and a truth pass the count check (and fail only on the workspace here)."""
    lib = S.load_library()
    d = good_run()
    d.M, d.truth, d.out_stride, d.workspace_bytes = 63, 5 * FAKE, 64 * 64, S.workspace_bytes(64, 3, 20, 10) - 8
    assert S.workspace_bytes(64, 3, 20, 10) > 0 and lib.skgram_run(ctypes.byref(d), None) == E_ARG


def test_combine_refuses_bad_arguments_without_a_gpu():
    lib = S.load_library()
    assert lib.skgram_combine(None, None) == E_ARG

    def good():
        d = S.describe_combine(5, 6, 33, 64, [0, 5], 3)
        d.members, d.coef, d.b, d.out = FAKE, 2 * FAKE, 3 * FAKE, 4 * FAKE
        return d

    def refused(**kw):
        d = good()
        for k, v in kw.items():
            setattr(d, k, v)
        return lib.skgram_combine(ctypes.byref(d), None) == E_ARG
    assert refused(members=None) and refused(coef=None) and refused(b=None) and refused(out=None)
    assert refused(members=FAKE + 4) and refused(coef=2 * FAKE + 2) and refused(b=3 * FAKE + 1) and refused(out=4 * FAKE + 2)
    assert refused(M=1) and refused(M=65) and refused(K=0) and refused(K=9) and refused(nc=0) and refused(nc=33)
    assert refused(C=0) and refused(H=0) and refused(W=0) and refused(C=69, H=4096, W=4096)
    assert refused(C=40, H=4096, W=4096, K=8, nc=32)                           # K nc H W > 2^30
    d = good()
    d.channels[0] = 6
    assert lib.skgram_combine(ctypes.byref(d), None) == E_ARG


# ---- the region ------------------------------------------------------------------------------------------------------------------------- #
def test_region_rows_columns_and_the_date_line():
    lat, lon = grid(721, 1440)
    assert S.region_index(lat, lon, None) == (0, 721, 0, 1440)
    j0, nj, i0, ni = S.region_index(lat, lon, (30, 75, -80, 40))
    assert (lat[j0], lat[j0 + nj - 1]) == (75.0, 30.0) and nj == 181
    assert lon[i0] == 280.0 and ni == 481 and lon[(i0 + ni - 1) % 1440] == 40.0
    assert S.region_index(lat, lon, (30, 75, 280, 40)) == (j0, nj, i0, ni)      # eastward around from 280 to 40
    assert S.region_index(lat, lon, (-10, 10, 170, 190)) == (320, 81, 680, 81)  # across the date line
    assert S.region_index(lat, lon, (-90, 90, -180, 180)) == (0, 721, 0, 1440)
    assert S.region_index(lat, lon, (0, 0, 10, 10)) == (360, 1, 40, 1)
    assert S.region_index(lat[::-1], lon, (30, 75, 0, 10))[:2] == (480, 181)   # an ascending axis
    for bad, msg in (((75, 30, 0, 10), "empty"), ((30.1, 30.2, 0, 10), "no row"), ((30, 40, 0.1, 0.2), "no column"), ((-95, 0, 0, 10), "outside"),
                     ((0, 95, 0, 10), "outside"), ((0, 10, 0), "region is"), ((0, np.nan, 0, 10), "outside")):
        with pytest.raises(ValueError, match=msg):
            S.region_index(lat, lon, bad)
    with pytest.raises(ValueError, match="no row"):
        S.region_index(lat[:600], lon, (-80, -70, 0, 10))                      # south of a grid without its southern rows


# ---- the host algebra ------------------------------------------------------------------------------------------------------------------- #
def planted(seed=0, sizes=(7, 4, 2), C=2, H=6, W=20, noise=0.3, order=None):
    rng = np.random.default_rng(seed)
    centres = rng.normal(size=(len(sizes), C, H, W)) * 5
    group = [g for g, n in enumerate(sizes) for _ in range(n)]
    group = [group[i] for i in (rng.permutation(len(group)) if order is None else order)]
    members = [(centres[g] + rng.normal(size=(C, H, W)) * noise).astype(np.float32) for g in group]
    truth = (centres[1] + rng.normal(size=(C, H, W)) * noise).astype(np.float32)
    return members, truth, np.asarray(group)


def setup(members, truth, channels, region_spec, normalise="spread", std=None):
    C, H, W = members[0].shape
    lat, lon = grid(H, W)
    w = area_weights(lat)
    region = S.region_index(lat, lon, region_spec)
    Gd, _ = R.gram(members, truth, channels, region, w)
    area = w[region[0]:region[0] + region[1]].sum() * region[3]
    A, ay = R.anomalies(members, truth, channels, region, w, normalise, std)
    return Gd, area, A, ay


def test_centring_equals_the_directly_centred_gram():
    members, truth, _ = planted()
    M = len(members)
    for normalise, std in (("none", None), ("spread", None), ("std", [2.0, 0.5])):
        Gd, area, A, ay = setup(members, truth, [0, 1], (-50, 60, 300, 40), normalise, std)
        Gc = np.stack([S.centre(g, M) for g in Gd]) / area
        Gf, scale = S.combine_channels(Gc, M, normalise, std)
        want = np.block([[A @ A.T, (A @ ay)[:, None]], [(A @ ay)[None, :], np.array([[ay @ ay]])]])
        # (the reference differences are fp32 as on the device, the anomalies float64 of the same fp32 fields: both are exact here
        # because x_m - x_0 of nearby fp32 values rounds by at most 2^-24 of the spread; 1e-12 would need exact differences)
        Gx = exact_gram(members, truth, [0, 1], (-50, 60, 300, 40))
        Gcx = np.stack([S.centre(g, M) for g in Gx]) / area
        Gfx, _ = S.combine_channels(Gcx, M, normalise, std)
        assert np.abs(Gfx - want).max() <= 1e-12 * np.abs(want).max()
        assert np.abs(Gf - want).max() <= 1e-6 * np.abs(want).max()            # with the fp32 differences of the device
        assert np.allclose(Gfx[:M, :M].sum(axis=0), 0, atol=1e-12 * np.abs(want).max())      # centred: rows sum to 0
    with pytest.raises(ValueError, match="normalise"):
        S.combine_channels(Gc, M, "variance")
    with pytest.raises(ValueError, match="sigma"):
        S.combine_channels(Gc, M, "std", [1.0, 0.0])


def exact_gram(members, truth, channels, region_spec):
    """Gd from float64 differences of the fp32 fields: what the centring identity is exact for."""
    C, H, W = members[0].shape
    lat, lon = grid(H, W)
    w = area_weights(lat)
    j0, nj, i0, ni = S.region_index(lat, lon, region_spec)
    cols = R.columns(i0, ni, W)
    out = []
    for c in channels:
        x = np.stack([m[c, j0:j0 + nj][:, cols].astype(np.float64) for m in members + [truth]])
        d = x - x[0]
        out.append(np.einsum("mji,nji,j->mn", d, d, w[j0:j0 + nj]))
    return np.stack(out)


def test_planted_clusters_are_recovered_with_sizes_representatives_and_probabilities():
    members, truth, group = planted()
    M = len(members)
    Gd, area, A, ay = setup(members, truth, [0, 1], None)
    a = S.analyse(Gd, M, area, 3, 3)
    c = a["clusters"]
    assert c["sizes"].tolist() == [7, 4, 2] and np.allclose(c["probability"], [7 / 13, 4 / 13, 2 / 13])
    assert np.array_equal(c["labels"], group)                                  # planted group g has the g-th largest size
    gaps = []
    want = R.ward(A, 3, gaps)
    assert np.array_equal(c["labels"], want) and min(gaps) > 1e-9
    ref = R.summarise(A, want)
    assert c["representative"].tolist() == ref["representative"].tolist()
    assert all(c["labels"][r] == k for k, r in enumerate(c["representative"]))
    for k in ("within", "total", "explained"):
        assert abs(c[k] - ref[k]) <= 1e-6 * ref["total"], k
    assert c["explained"] > 0.99 * c["total"]
    assert a["nearest_cluster"] == R.nearest_cluster(A, ay, want) == 1          # the truth was drawn from group 1
    # fewer and more clusters, every count down to one member each
    for n in (1, 2, 5, 13):
        assert np.array_equal(S.ward(S.distances(a["combined"][:M, :M]), n), R.ward(A, n)), n
    assert S.ward(S.distances(a["combined"][:M, :M]), 13).tolist() == list(range(13))
    for bad in (0, 14):
        with pytest.raises(ValueError, match="n_clusters"):
            S.ward(S.distances(a["combined"][:M, :M]), bad)


def test_a_rank_two_spread_has_two_variance_fractions_and_orthogonal_pcs():
    rng = np.random.default_rng(3)
    C, H, W, M = 1, 5, 16, 9
    p1, p2 = rng.normal(size=(2, C, H, W))
    base = rng.normal(size=(C, H, W)) * 10
    c1, c2 = rng.normal(size=(2, M))
    members = [base + c1[m] * p1 + 0.3 * c2[m] * p2 for m in range(M)]          # float64 fields: the rank is exact
    lat, lon = grid(H, W)
    w = area_weights(lat)
    x = np.stack([m[0] for m in members])
    d = x - x[0]
    Gd = np.einsum("mji,nji,j->mn", d, d, w)[None]
    a = S.analyse(Gd, M, w.sum() * W, 2, 4, "none")
    f = a["variance_fraction"]
    assert f[0] >= f[1] > 0 and f[2] == 0 and f[3] == 0 and abs(f[0] + f[1] - 1) < 1e-12
    pcs = a["pcs"]
    assert abs(pcs[:, 0] @ pcs[:, 1]) < 1e-9 * np.linalg.norm(pcs[:, 0]) * np.linalg.norm(pcs[:, 1]) and not pcs[:, 2:].any()
    assert np.allclose(pcs.sum(axis=0), 0, atol=1e-9) and not a["coef"][2:].any()
    for k in range(2):
        assert pcs[int(np.argmax(np.abs(pcs[:, k]))), k] > 0                    # the sign rule
    # the patterns made of the members by ``coef`` rebuild the anomalies from the PCs
    anom = (x - x.mean(axis=0)).reshape(M, -1)
    pat = a["coef"][:2] @ anom
    assert np.abs(pcs[:, :2] @ pat - anom).max() < 1e-9 * np.abs(anom).max()
    frac, rp, _ = R.eofs(anom * np.sqrt(np.repeat(w, W) / (w.sum() * W)), 2)
    assert np.allclose(f[:2], frac, rtol=1e-9) and np.allclose(pcs[:, :2], rp, rtol=1e-7, atol=1e-9 * np.abs(rp).max())


def test_energy_score_equals_the_pairwise_norm_formula():
    members, truth, _ = planted(seed=5)
    M = len(members)
    for normalise in ("spread", "none"):
        Gx = exact_gram(members, truth, [0, 1], (-60, 60, 350, 30))
        lat, lon = grid(6, 20)
        w = area_weights(lat)
        j0, nj, i0, ni = S.region_index(lat, lon, (-60, 60, 350, 30))
        a = S.analyse(Gx, M, w[j0:j0 + nj].sum() * ni, 3, 0, normalise)
        _, _, A, ay = setup(members, truth, [0, 1], (-60, 60, 350, 30), normalise)
        assert abs(a["energy_score"] - R.energy_score(A, ay)) <= 1e-12 * abs(R.energy_score(A, ay))
    # a truth equal to a member of an ensemble of identical members: every norm is 0
    same = [members[0]] * 4
    Gd, area, _, _ = setup(same, members[0], [0], None)
    assert S.analyse(Gd, 4, area, 1, 0)["energy_score"] == 0


def test_tie_rules_are_deterministic():
    # four members at the corners of a square: every first merge costs the same, and so does every choice of a representative
    e = np.zeros((4, 1, 1, 4), np.float32)
    for m, (a, b) in enumerate(((0, 0), (1, 0), (0, 1), (1, 1))):
        e[m, 0, 0, :2] = (a, b)
    lat, lon = np.array([0.0]), np.arange(4) * 90.0
    Gd, _ = R.gram(list(e), None, [0], (0, 1, 0, 4), np.ones(1))
    runs = [S.analyse(Gd, 4, 4.0, 2, 2, "none") for _ in range(3)]
    for r in runs:
        assert r["clusters"]["labels"].tolist() == [0, 0, 1, 1]                # (0, 1) is the lowest pair among the equal ones
        assert r["clusters"]["representative"].tolist() == [0, 2] and r["clusters"]["sizes"].tolist() == [2, 2]
        assert np.array_equal(r["pcs"], runs[0]["pcs"])
    # equal sizes are numbered by lowest member; identical members merge first
    d = np.array([[0, 9, 0, 9], [9, 0, 9, 0], [0, 9, 0, 9], [9, 0, 9, 0]], np.float64)
    assert S.ward(d, 2).tolist() == [0, 1, 0, 1]
    assert S.summarise(np.eye(3) - 1 / 3, np.zeros(3, int))["representative"].tolist() == [0]
    assert lat.size == 1 and lon.size == 4


# ---- the request ------------------------------------------------------------------------------------------------------------------------ #
def test_check_request_normalises_and_refuses():
    lat, lon = grid(721, 1440)
    names = ["z500", "t850", "msl"]
    r = S.check_request(names, lat, lon, 50, {"channels": ["msl", "z500"], "region": (30, 75, -80, 40)})
    assert r["index"] == [2, 0] and r["region"] == (60, 181, 1120, 481) and (r["n_clusters"], r["n_eofs"], r["normalise"]) == (3, 3, "spread")
    assert S.check_request(names, lat, lon, 2, {"channels": ["msl"], "n_clusters": 2, "n_eofs": 1})["region"] == (0, 721, 0, 1440)
    base = {"channels": ["z500"]}
    for spec, M, scores, other, msg in (
            ({"channels": ["q700"]}, 5, False, (), "not an output channel"), ({"channels": ["ws10m"]}, 5, False, ["ws10m"], "raw channels"),
            ({"channels": ["t2m_max_24h"]}, 5, False, ["t2m_max_24h"], "raw channels"), ({"channels": []}, 5, False, (), "channels"),
            ({"channels": ["msl", "msl"]}, 5, False, (), "twice"), ({**base, "region": (75, 30, 0, 10)}, 5, False, (), "empty"),
            ({**base, "region": (-95, 30, 0, 10)}, 5, False, (), "outside"), ({**base, "region": (30.1, 30.2, 0, 10)}, 5, False, (), "no row"),
            (base, 1, False, (), "n_members"), (base, 65, False, (), "n_members"), (base, 64, True, (), "truth needs a column"),
            ({**base, "n_clusters": 0}, 5, False, (), "n_clusters"), ({**base, "n_clusters": 6}, 5, False, (), "n_clusters"),
            ({**base, "n_eofs": -1}, 5, False, (), "n_eofs"), ({**base, "n_eofs": 5}, 5, False, (), "n_eofs"),
            ({**base, "n_eofs": 9}, 50, False, (), "n_eofs"), ({**base, "normalise": "variance"}, 5, False, (), "normalise"),
            ({**base, "clusters": 3}, 5, False, (), "unknown keys"), (["z500"], 5, False, (), "a dict")):
        with pytest.raises(ValueError, match=msg):
            S.check_request(names, lat, lon, M, spec, scores, other)
    assert S.check_request(names, lat, lon, 64, base, False)["n_eofs"] == 3 and S.check_request(names, lat, lon, 63, base, True)


def test_the_public_entry_point_refuses_before_the_device():
    from test_ens_cpu import T0, _Model
    from skyrim_amd import ensemble as E
    m = _Model()                                                               # channels u1000, v1000, t2m on a 9 x 96 grid; its loop must not start
    ok = {"channels": ["t2m"], "n_clusters": 2, "n_eofs": 2}
    assert E.validate(m.model, 2, 3, 0, (), None, None, None, 1, False, scenarios=ok)[3] == [0, 1, 2]
    for kw, msg in ((dict(scenarios={"channels": ["msl"]}), "not an output channel"),
                    (dict(scenarios={"channels": ["ws1000"]}, derived=["ws1000"]), "raw channels on the model's own grid only"),
                    (dict(scenarios={"channels": ["t2m_max_12h"]}, aggregates=["t2m:max:12h"]), "raw channels on the model's own grid only"),
                    (dict(scenarios={**ok, "region": (50, 40, 0, 10)}), "empty"), (dict(scenarios={**ok, "region": (0, 100, 0, 10)}), "outside"),
                    (dict(scenarios={**ok, "region": (1, 2, 0, 10)}), "no row"), (dict(scenarios=ok, n_members=1), "at least 2"),
                    (dict(scenarios={**ok, "n_clusters": 4}), "n_clusters"), (dict(scenarios={**ok, "n_eofs": 3}), "n_eofs"),
                    (dict(scenarios=ok, n_members=64, scores=True), "truth needs a column")):
        args = dict(n_steps=2, n_members=3)
        args.update(kw)
        with pytest.raises(ValueError, match=msg):
            m.ensemble_forecast(T0, **args)
    assert E.EnsembleForecast("m", 1, 0, 0.0).scenarios is None
    # with scores=True the truth is a column of the matrix: a truth without a scenario channel is refused before the device, too
    from skyrim_amd.labeled import DataArray
    grid_ = m.model.grid
    truth = DataArray(np.zeros((1, len(grid_.lat), len(grid_.lon)), np.float32), ["channel", "lat", "lon"],
                      dict(channel=["u1000"], lat=np.asarray(grid_.lat), lon=np.asarray(grid_.lon)))
    with pytest.raises(ValueError, match="t2m.*not among the scored channels"):
        m.ensemble_forecast(T0, n_steps=1, n_members=3, scenarios=ok, scores=True, truth=truth)
    S.check_scored(["a"], ["b", "a"])
    with pytest.raises(RuntimeError, match="GPU"):                             # everything valid: the work itself needs the device
        m.ensemble_forecast(T0, n_steps=1, n_members=3, scenarios=ok)


def test_scenarios_clusters_over_several_lead_times_is_host_only():
    members, truth, group = planted()
    M = len(members)
    parts = []
    for seed in (0, 1):
        mem, _, _ = planted(seed=seed, order=np.argsort(np.argsort(group, kind="stable"), kind="stable"))
        Gd, area, _, _ = setup(mem, None, [0, 1], None)
        parts.append(S.analyse(Gd, M, area, 3, 2))
    sc = S.Scenarios(["a", "b"], ["t0", "t1"], (0, 6, 0, 20), "spread", M, np.stack([p["gram"] for p in parts]),
                     np.stack([p["combined"] for p in parts]), np.stack([p["scale"] for p in parts]), [p["clusters"] for p in parts])
    both = sc.clusters(3)
    assert both["sizes"].tolist() == [7, 4, 2] and np.array_equal(both["labels"], parts[0]["clusters"]["labels"])
    assert np.array_equal(sc.clusters(3, times=["t1"])["labels"], parts[1]["clusters"]["labels"])
    assert np.array_equal(sc.clusters(3, times=[0])["labels"], parts[0]["clusters"]["labels"])
    assert abs(both["total"] - (parts[0]["clusters"]["total"] + parts[1]["clusters"]["total"])) < 1e-9 * both["total"]
    with pytest.raises(ValueError, match="at least one"):
        sc.clusters(2, times=[])


# ---- the command line -------------------------------------------------------------------------------------------------------------------- #
def test_command_line_options_and_refusals():
    from click.testing import CliRunner
    from skyrim_amd import scenario_cli as cli
    assert cli.parse_region("30,75,-80,40") == (30.0, 75.0, -80.0, 40.0) and cli.parse_region("") is None
    for bad in ("30,75,-80", "a,b,c,d", "1,2,3,4,5"):
        with pytest.raises(ValueError, match="LAT_S"):
            cli.parse_region(bad)
    assert cli.request(("z500",), "30,75,-80,40", 3, 2, "spread", 10, "out.json") == dict(
        channels=["z500"], region=(30.0, 75.0, -80.0, 40.0), n_clusters=3, n_eofs=2, normalise="spread")
    for args, msg in ((((), "", 3, 3, "spread", 10, ""), "--channel"), ((("z500",), "", 3, 3, "spread", 1, ""), "--members"),
                      ((("z500",), "", 11, 3, "spread", 10, ""), "--clusters"), ((("z500",), "", 3, 9, "spread", 10, ""), "--eofs"),
                      ((("z500",), "", 2, 2, "spread", 2, ""), "--eofs"), ((("z500",), "", 3, 3, "spread", 10, "out.csv"), ".json"),
                      ((("z500",), "1,2", 3, 3, "spread", 10, ""), "LAT_S")):
        with pytest.raises(ValueError, match=msg):
            cli.request(*args)
    with pytest.raises(ValueError, match="n_steps"):
        cli.request(("z500",), "", 3, 3, "spread", 10, "", n_steps=-1)
    run = CliRunner().invoke
    for argv in ([], ["--channel", "z500", "--members", "1"], ["--channel", "z500", "--region", "1,2"], ["--channel", "z500", "--normalise", "x"],
                 ["--channel", "z500", "--output", "x.txt"], ["--channel", "z500", "--modal"]):
        res = run(cli.scenario, argv)
        assert res.exit_code == 2, (argv, res.output)
    assert {"channels", "region", "clusters", "eofs", "normalise", "members", "n_steps", "output", "model_name", "date", "time", "lead_time",
            "initial_conditions"} <= {o.name for o in cli.scenario.params}
    members, _, _ = planted()
    Gd, area, _, _ = setup(members, None, [0, 1], None)
    a = S.analyse(Gd, 13, area, 3, 2)
    sc = S.Scenarios(["a", "b"], ["t0"], (0, 6, 0, 20), "spread", 13, a["gram"][None], a["combined"][None], a["scale"][None], [a["clusters"]],
                     variance_fraction=a["variance_fraction"][None], pcs=a["pcs"][None])
    out = cli.lines(sc)
    assert len(out) == 4 and out[0].startswith("t0 cluster 0: p=0.538 size=7 representative=") and out[3].startswith("t0 eof variance fractions: ")
    doc = cli.document(sc)
    assert doc["times"][0]["sizes"] == [7, 4, 2] and doc["n_members"] == 13 and len(doc["times"][0]["labels"]) == 13
