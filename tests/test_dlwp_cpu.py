"""DLWP without a GPU: the padding table against the cube geometry, the synthetic maps, TISR, the C ABI surface and argument checks,
op registration, the converter, the time contract of the TimeLoop and the data source, the model registry, and the refusals of
zero-step predictions and mixed-step ensembles."""
from __future__ import annotations

import ctypes
import datetime
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import _dlwp_reference as R

ROOT = Path(__file__).resolve().parent.parent


def _toy():
    from skyrim_amd.dlwp.spec import DlwpConfig
    return DlwpConfig(n_lat=33, n_lon=64, face=8)


# ---- geometry ------------------------------------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize("n", [4, 8])
def test_padding_matches_geometry(n):
    """Every non-corner halo cell takes the neighbouring face's cell whose centre is nearest to the halo cell's position extended on
    the face's own gnomonic plane; checked on a field that is distinct in every cell."""
    from skyrim_amd.dlwp.spec import cell_vectors
    field = torch.arange(6 * n * n, dtype=torch.float64).reshape(6, 1, n, n)
    padded = R.pad(field)[:, 0]
    ext = cell_vectors(n, -1, n + 1)                    # [6][n+2][n+2][3] on each face's plane
    cells = cell_vectors(n).reshape(-1, 3)
    checked = 0
    for f in range(6):
        for py in range(n + 2):
            for px in range(n + 2):
                yin, xin = 1 <= py <= n, 1 <= px <= n
                if yin == xin:                          # interior (checked below) or corner
                    continue
                nearest = int(np.argmax(cells @ ext[f, py, px]))
                assert nearest // (n * n) != f
                assert padded[f, py, px].item() == nearest, (f, py, px)
                checked += 1
    assert checked == 6 * 4 * n
    assert torch.equal(padded[:, 1:-1, 1:-1], field[:, 0])
    # corners: the mean of the two halo cells next to them
    assert padded[0, 0, 0].item() == 0.5 * (padded[0, 0, 1].item() + padded[0, 1, 0].item())


def test_pad_table_is_an_involution_of_edges():
    """If face f's side s comes from face g, one of g's sides comes from f (every cube edge is shared by exactly two faces)."""
    from skyrim_amd.dlwp.spec import PAD
    for f in range(6):
        for g, _ in PAD[f]:
            assert g != f and f in [h for h, _ in PAD[g]]


def test_synthetic_maps_rows_sum_to_one():
    from skyrim_amd.dlwp.spec import cs_to_ll_map, ll_to_cs_map, to_csr
    cfg = _toy()
    for (r, c, s), rows, cols in ((ll_to_cs_map(cfg), cfg.cells, cfg.points), (cs_to_ll_map(cfg), cfg.points, cfg.cells)):
        ptr, col, S = to_csr(r, c, s, rows)
        assert col.min() >= 0 and col.max() < cols and (S > 0).all()
        sums = np.add.reduceat(S, ptr[:-1]) if len(S) else np.zeros(rows)
        assert np.allclose(sums, 1.0, atol=1e-12) and (np.diff(ptr) > 0).all()


def test_cube_latlon_covers_the_sphere():
    from skyrim_amd.dlwp.spec import cube_latlon
    lat, lon = cube_latlon(16)
    assert lat[4].min() > 35 and lat[5].max() < -35 and abs(lat[:4]).max() < 45.1
    assert 0 <= lon.min() and lon.max() < 360
    # face f of the equator is centred on longitude 90 f, its columns run east
    for f in range(4):
        east, west = (((lon[f, 8, 8] - 90 * f + 180) % 360) - 180), (((lon[f, 8, 7] - 90 * f + 180) % 360) - 180)
        assert 0 < east < 6 and east == pytest.approx(-west, abs=1e-9)


# ---- TISR ----------------------------------------------------------------------------------------------------------------------------- #
def test_solar_declination_and_subsolar_point():
    from skyrim_amd.dlwp.spec import cos_zenith, days_since_j2000, solar_position, tisr
    ra, dec, gmst = solar_position(days_since_j2000(datetime.datetime(2024, 6, 20, 20, 51)))
    assert abs(np.degrees(dec) - 23.44) < 0.01
    _, dec_eq, _ = solar_position(days_since_j2000(datetime.datetime(2024, 3, 20, 3, 6)))
    assert abs(np.degrees(dec_eq)) < 0.01
    # subsolar point: latitude = declination, longitude = RA - GMST
    days = days_since_j2000(datetime.datetime(2024, 6, 21, 12))
    ra, dec, gmst = solar_position(days)
    assert cos_zenith(days, np.degrees(dec), np.degrees(ra - gmst)) == pytest.approx(1.0, abs=1e-12)
    lat, lon = np.meshgrid(np.linspace(-90, 90, 37), np.linspace(0, 359, 60), indexing="ij")
    t = tisr(days, lat, lon)
    assert t.min() >= -1 / np.pi - 1e-15 and t.max() <= 1 - 1 / np.pi + 1e-12 and t.max() > 0.6


# ---- C ABI and ops -------------------------------------------------------------------------------------------------------------------- #
def _lib():
    from skyrim_amd.dlwp import engine
    return engine.load_library()


def test_header_symbols_equal_exports_and_library_has_them():
    from skyrim_amd.dlwp import engine
    hdr = (ROOT / "include" / "skyrim_dlwp.h").read_text()
    names = set(re.findall(r"^(?:int|const char\*) (skdlwp_\w+)\(", hdr, re.M))
    assert names == set(engine.EXPORTS)
    lib = _lib()
    assert lib.skdlwp_abi_version() == 1
    assert lib.skdlwp_error_string(-1) == b"invalid argument" and lib.skdlwp_error_string(-2) == b"HIP runtime error"


def test_argument_errors_without_gpu():
    from skyrim_amd.dlwp import engine
    lib = _lib()
    assert lib.skdlwp_prepare_weight(None, 1, 1, 4, 4, None, 16, 8, None) == -1
    assert lib.skdlwp_ingest(None, None) == -1
    assert lib.skdlwp_conv(None, None) == -1
    assert lib.skdlwp_egress(None, None) == -1
    d = engine.IngestDesc(16, 16, 16, 16, 16, 16, 16, 16, 16, 16, 0.0, 0.0, 16, 9, 10, 10, 24)           # 9 channels: more than compiled
    assert lib.skdlwp_ingest(ctypes.byref(d), None) == -1
    c = engine.ConvDesc(16, None, 16, 16, 2 * 64 * 216, 64 * 216, 216, 16, 16, 8, 18, 0, 0, 9, 64, 64, 1, 5, 0.1, 10.0)   # c0 not a multiple of 8
    assert lib.skdlwp_conv(ctypes.byref(c), None) == -1
    c = engine.ConvDesc(16, None, 16, 16, 2 * 64 * 216, 64 * 216, 216, 16, 16, 7, 24, 0, 2, 9, 64, 64, 1, 5, 0.1, 10.0)    # upsampling an odd face
    assert lib.skdlwp_conv(ctypes.byref(c), None) == -1
    c = engine.ConvDesc(16, None, 16, 16, 2 * 64 * 216, 64 * 100, 216, 16, 16, 8, 24, 0, 0, 9, 64, 64, 1, 5, 0.1, 10.0)    # polar set overlaps
    assert lib.skdlwp_conv(ctypes.byref(c), None) == -1
    e = engine.EgressDesc(16, 16, 16, 16, 16, 16, 16, 16, 7, 10, 10, 14)                                  # ld_y not a multiple of 4
    assert lib.skdlwp_egress(ctypes.byref(e), None) == -1


def test_dlwp_ops_have_no_cpu_kernel():
    from skyrim_amd import ops
    assert {n for n in ops.OP_NAMES if n.startswith("dlwp_")} == {"dlwp_ingest", "dlwp_conv", "dlwp_egress"}
    with pytest.raises(NotImplementedError):
        ops.hip.dlwp_egress(torch.zeros(16), torch.zeros(2, dtype=torch.int32), torch.zeros(1, dtype=torch.int32), torch.zeros(1),
                            torch.zeros(7), torch.ones(7), torch.zeros(7), torch.zeros(7), 7, 16)


# ---- the network restatement --------------------------------------------------------------------------------------------------------- #
def test_spec_sizes():
    from skyrim_amd.dlwp.spec import DlwpConfig, convs, flops_per_call, n_parameters
    cfg = DlwpConfig()
    assert cfg.in_ch == 18 and cfg.out_ch == 14 and cfg.cells == 24576
    assert [(c[2], c[3]) for c in convs(cfg)] == [(18, 64), (64, 64), (64, 128), (128, 128), (128, 256), (256, 128), (256, 128),
                                                 (128, 64), (128, 64), (64, 64), (64, 14)]
    assert 2.6e6 < n_parameters(cfg) < 2.8e6 and 16e9 < flops_per_call(cfg) < 18e9


def test_polar_mirror_is_a_row_flipped_kernel():
    """Mirroring the flip face around its conv equals the kernel flipped in rows on the unmirrored, padded face (what the loader does)."""
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(0)
    x = torch.randn(6, 3, 8, 8, generator=g, dtype=torch.float64)
    w = torch.randn(4, 3, 3, 3, generator=g, dtype=torch.float64)
    b = torch.zeros(4, dtype=torch.float64)
    y = R.cube_conv(x, w, b, w, b, flip=5)
    direct = F.conv2d(R.pad(x)[5:6], torch.flip(w, [-2]), b)
    assert torch.allclose(y[5:6], direct, atol=1e-12) and not torch.allclose(y[4:5], F.conv2d(R.pad(x)[4:5], torch.flip(w, [-2]), b))


# ---- checkpoint ----------------------------------------------------------------------------------------------------------------------- #
def _write_nc(path, **vars_):
    from scipy.io import netcdf_file
    with netcdf_file(str(path), "w") as f:
        for name, a in vars_.items():
            a = np.asarray(a)
            dims = tuple(f"{name}_d{i}" for i in range(a.ndim))
            for d, s in zip(dims, a.shape):
                f.createDimension(d, s)
            v = f.createVariable(name, a.dtype if a.dtype != np.int64 else np.int32, dims)
            v[:] = a


def test_checkpoint_round_trip_and_unplaced_keys(tmp_path):
    import tarfile
    from skyrim_amd.dlwp import checkpoint
    from skyrim_amd.dlwp.spec import init_synthetic
    cfg = _toy()
    p = init_synthetic(cfg, 5)
    sd = {"module." + k: v.clone() for k, v in p.items() if k.startswith(("equatorial_", "polar_"))}
    buf = tmp_path / "model.pt"
    torch.save(sd, buf)
    with tarfile.open(tmp_path / "dlwp_cubesphere.mdlus", "w") as tar:
        tar.add(buf, arcname="model.pt")
    buf.unlink()
    np.save(tmp_path / "global_means.npy", p["center"].numpy().reshape(1, -1, 1, 1))
    np.save(tmp_path / "global_stds.npy", p["scale"].numpy().reshape(1, -1, 1, 1))
    _write_nc(tmp_path / "land_sea_mask_rs_cs.nc", lsm=p["lsm"].numpy())
    _write_nc(tmp_path / "geopotential_rs_cs.nc", z=p["topography"].numpy())
    _write_nc(tmp_path / "latlon_grid_field_rs_cs.nc", latgrid=p["cube_lat"].numpy(), longrid=p["cube_lon"].numpy())
    for name, fname in checkpoint.map_files(cfg).items():
        _write_nc(tmp_path / fname, row=p[name + ".row"].numpy() + 1, col=p[name + ".col"].numpy() + 1, S=p[name + ".S"].numpy())
    got = checkpoint.load_package(str(tmp_path), cfg)
    assert set(got) == set(p)
    for k in p:
        assert torch.allclose(got[k].double(), p[k].double(), rtol=0, atol=1e-6 * max(1.0, p[k].double().abs().max().item())), k
    # the torch file of the slot dict is read as it is
    from skyrim_amd.dlwp.timeloop import DlwpTimeLoop
    torch.save(p, tmp_path / "slots.pt")
    loop = DlwpTimeLoop.__new__(DlwpTimeLoop)
    loop.cfg = cfg
    assert set(loop._load(str(tmp_path / "slots.pt"))) == set(p)
    # a renamed key is named, nothing partial comes back
    sd["module.equatorial_upsample.9.weight"] = sd.pop("module.equatorial_upsample.3.weight")
    statics = {k: p[k].numpy() for k in checkpoint.STATIC_FILES}
    maps = {m: (p[m + ".row"], p[m + ".col"], p[m + ".S"]) for m in ("ll_to_cs", "cs_to_ll")}
    with pytest.raises(ValueError, match=r"equatorial_upsample\.9\.weight.*equatorial_upsample\.3\.weight"):
        checkpoint.convert(sd, cfg, p["center"], p["scale"], statics, maps)


def test_netcdf4_file_is_refused_with_the_conversion(tmp_path):
    from skyrim_amd.dlwp import checkpoint
    f = tmp_path / "map.nc"
    f.write_bytes(b"\x89HDF\r\n\x1a\n" + bytes(64))
    with pytest.raises(ValueError, match="netCDF-4.*nccopy -k classic"):
        checkpoint.read_netcdf(str(f), ["S"])


# ---- time contract, registry, refusals -------------------------------------------------------------------------------------------------- #
def test_time_contract_and_ic_levels():
    from skyrim_amd.datasource import get_initial_condition_for_model
    from skyrim_amd.dlwp.timeloop import DlwpTimeLoop
    assert DlwpTimeLoop.time_step == datetime.timedelta(hours=12) and DlwpTimeLoop.n_history_levels == 2
    assert DlwpTimeLoop.history_time_step == datetime.timedelta(hours=6)

    class Source:
        asked = []

        def __getitem__(self, t):
            self.asked.append(t)
            return np.zeros((7, 3, 4), dtype=np.float32)

    loop = DlwpTimeLoop.__new__(DlwpTimeLoop)
    loop.engine = type("E", (), {"device": torch.device("cpu")})()
    t = datetime.datetime(2024, 1, 1, 12)
    x = get_initial_condition_for_model(loop, Source(), t)
    assert tuple(x.shape) == (1, 2, 7, 3, 4)
    assert Source.asked == [t - datetime.timedelta(hours=6), t]


def test_ic_array_must_hold_levels_six_hours_apart():
    from skyrim_amd.core.models.utils import _check_history_spacing
    from skyrim_amd.dlwp.timeloop import DlwpTimeLoop
    from skyrim_amd.labeled import DataArray
    loop = DlwpTimeLoop.__new__(DlwpTimeLoop)
    t = datetime.datetime(2024, 1, 1, 12)

    def da(times):
        return DataArray(np.zeros((len(times), 7, 2, 2), np.float32), dims=["time", "channel", "lat", "lon"],
                         coords=dict(time=times, channel=list("abcdefg"), lat=np.arange(2.0), lon=np.arange(2.0)))

    _check_history_spacing(loop, da([t - datetime.timedelta(hours=6), t]))
    with pytest.raises(ValueError, match="cannot be restarted from"):
        _check_history_spacing(loop, da([t - datetime.timedelta(hours=12), t]))


def test_dlwp_is_a_registered_model_and_cli_choice():
    from skyrim_amd import common, forecast
    from skyrim_amd.core import Skyrim, models
    from skyrim_amd.core.models.dlwp import CHANNELS, DLWPModel
    assert "dlwp" in Skyrim.list_available_models()
    assert "dlwp" in common.AVAILABLE_MODELS and models.MODELS["dlwp"] is DLWPModel
    opt = next(p for p in forecast.main.params if p.name == "model_name")
    assert "dlwp" in opt.type.choices
    assert CHANNELS == ["t850", "z1000", "z700", "z500", "z300", "tcwv", "t2m"]
    assert common.AVAILABLE_MODELS == ["pangu", "fourcastnet", "fourcastnet_v2", "graphcast", "dlwp"]


def test_zero_step_predict_is_refused():
    from skyrim_amd.core.skyrim import Skyrim
    s = Skyrim.__new__(Skyrim)
    s.model_names = ("dlwp",)
    s.model = type("M", (), {"time_step": datetime.timedelta(hours=12),
                             "rollout": lambda *a, **k: pytest.fail("rollout must not run with zero steps")})()
    with pytest.raises(ValueError, match="shorter than one 12-h step"):
        s.predict("20240101", "0000", lead_time=6)


def test_ensemble_with_mixed_time_steps_is_refused():
    from skyrim_amd.core.models.ensemble import GlobalEnsemble
    with pytest.raises(ValueError, match="share one time step"):
        GlobalEnsemble(["pangu", "dlwp"], ic_source="synthetic")
    assert GlobalEnsemble(["pangu", "fourcastnet"], ic_source="synthetic").time_step == datetime.timedelta(hours=6)
