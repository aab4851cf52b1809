"""DLWP package (earth2mip's ``dlwp``) -> the engine's parameter slots.

The reference obtains the model through ``earth2mip.networks.dlwp.load(registry.get_model("e2mip://dlwp"))`` (the reference's
skyrim/core/models/dlwp.py:25): a package directory with modulus's checkpoint of ``DLWP`` (``*.mdlus``, a tar archive holding
``model.pt``, or a bare ``*.pt`` / ``*.pth`` state dict), ``global_means.npy`` / ``global_stds.npy``, the static fields on the cube
(land-sea mask, geopotential of the surface, cell latitudes / longitudes) and the two TempestRemap maps (``S``, 1-based ``row`` /
``col``).  The file and variable names below are UNVERIFIED against the real package (it is not obtainable offline), so
``convert`` follows fcn/checkpoint.py's rule: nothing is returned partial or shape-mismatched, and every key it cannot place is named.

The ``.nc`` files are read with ``scipy.io.netcdf_file``, which reads netCDF-3 only; a netCDF-4 (HDF5) file is refused with the command
that converts it.
"""
from __future__ import annotations

import io
import os
import re
import tarfile

import numpy as np
import torch

from .. import weights
from .spec import MAP_SLOTS, DlwpConfig, param_spec

# slot -> (file, variable) of the static fields
STATIC_FILES = {"lsm": ("land_sea_mask_rs_cs.nc", "lsm"), "topography": ("geopotential_rs_cs.nc", "z"),
                "cube_lat": ("latlon_grid_field_rs_cs.nc", "latgrid"), "cube_lon": ("latlon_grid_field_rs_cs.nc", "longrid")}


def map_files(cfg: DlwpConfig) -> dict:
    return {"ll_to_cs": f"map_LL{cfg.n_lat}x{cfg.n_lon}_CS{cfg.face}.nc", "cs_to_ll": f"map_CS{cfg.face}_LL{cfg.n_lat}x{cfg.n_lon}.nc"}


def read_netcdf(path: str, names: list[str]) -> dict:
    """{name: array} of the named variables of a netCDF-3 file."""
    with open(path, "rb") as f:
        magic = f.read(4)
    if magic[:3] != b"CDF":
        kind = "netCDF-4 (HDF5)" if magic == b"\x89HDF" else "not netCDF"
        raise ValueError(f"{path} is {kind}; this build reads netCDF-3 only.  Convert it once, e.g. `nccopy -k classic {path} out.nc` "
                         "(netCDF tools) or `xarray.open_dataset(path).to_netcdf(out, format='NETCDF3_64BIT')`, and put the result in its place")
    from scipy.io import netcdf_file
    with netcdf_file(path, "r", mmap=False) as f:
        missing = [n for n in names if n not in f.variables]
        if missing:
            raise ValueError(f"{path}: variables {missing} not found (has {sorted(f.variables)})")
        return {n: np.array(f.variables[n][:]) for n in names}


def _strip(key: str) -> str:
    return re.sub(r"^(module\.)+", "", key)


def convert(state_dict: dict, cfg: DlwpConfig, center, scale, statics: dict, maps: dict) -> dict:
    """``state_dict``: DLWP's state dict; ``center`` / ``scale``: one value per channel (any shape of that size); ``statics``: {slot:
    array of 6 face^2 values} for lsm, topography (raw geopotential), cube_lat, cube_lon (degrees); ``maps``: {map: (row, col, S)} with
    0-based indices.  -> the engine's parameter dict."""
    want = dict(param_spec(cfg))
    out, unplaced = {}, []
    for key, val in state_dict.items():
        slot = _strip(key)
        if slot not in want or not slot.startswith(("equatorial_", "polar_")):
            unplaced.append(key)
            continue
        t = (val if torch.is_tensor(val) else torch.as_tensor(np.asarray(val))).detach().float()
        if tuple(t.shape) != tuple(want[slot]):
            raise ValueError(f"checkpoint key {key!r} -> slot {slot}: shape {tuple(t.shape)} != expected {want[slot]}")
        out[slot] = t.contiguous()
    for slot, val in (("center", center), ("scale", scale)):
        t = torch.as_tensor(np.asarray(val, dtype=np.float32)).flatten()
        if t.numel() != cfg.channels:
            raise ValueError(f"{slot}: {t.numel()} values, expected {cfg.channels}")
        out[slot] = t
    for slot, val in statics.items():
        a = np.asarray(val, dtype=np.float64)
        if a.size != 6 * cfg.face * cfg.face:
            raise ValueError(f"{slot}: {a.size} values, expected 6 x {cfg.face} x {cfg.face}")
        out[slot] = torch.from_numpy(a.reshape(6, cfg.face, cfg.face).copy())
        if slot not in ("cube_lat", "cube_lon"):
            out[slot] = out[slot].float()
    for name, (row, col, S) in maps.items():
        out[name + ".row"] = torch.from_numpy(np.asarray(row, np.int64).ravel())
        out[name + ".col"] = torch.from_numpy(np.asarray(col, np.int64).ravel())
        out[name + ".S"] = torch.from_numpy(np.asarray(S, np.float64).ravel())
    missing = [s for s in want if s not in out] + [f"{m}.{p}" for m in MAP_SLOTS for p in ("row", "col", "S") if f"{m}.{p}" not in out]
    if unplaced or missing:
        raise ValueError(f"checkpoint does not match the DLWP layout: unplaced keys {sorted(unplaced)}, missing slots {missing}")
    return out


def read_state_dict(path: str) -> dict:
    """A modulus ``.mdlus`` archive (its ``model.pt``) or a torch file (bare, or under ``model_state`` / ``state_dict``)."""
    if tarfile.is_tarfile(path):
        with tarfile.open(path) as tar:
            member = next((m for m in tar.getmembers() if m.name.endswith("model.pt")), None)
            if member is None:
                raise ValueError(f"{path}: tar archive without model.pt")
            sd = torch.load(io.BytesIO(tar.extractfile(member).read()), map_location="cpu", weights_only=False)
    else:
        sd = torch.load(path, map_location="cpu", weights_only=False)
    for key in ("model_state", "state_dict"):
        if isinstance(sd, dict) and key in sd:
            sd = sd[key]
    return sd


def load(path: str, cfg: DlwpConfig) -> dict:
    return weights.load_slots(path, lambda d: load_package(d, cfg))


def load_package(path: str, cfg: DlwpConfig) -> dict:
    names = sorted(n for n in os.listdir(path) if n.endswith((".mdlus", ".pt", ".pth")))
    if len(names) != 1:
        raise ValueError(f"{path}: expected exactly one checkpoint (*.mdlus / *.pt / *.pth), found {names}")
    statics = {}
    for slot, (fname, var) in STATIC_FILES.items():
        statics[slot] = read_netcdf(os.path.join(path, fname), [var])[var]
    maps = {}
    for name, fname in map_files(cfg).items():
        v = read_netcdf(os.path.join(path, fname), ["row", "col", "S"])
        maps[name] = (v["row"].astype(np.int64) - 1, v["col"].astype(np.int64) - 1, v["S"])      # TempestRemap: 1-based
    return convert(read_state_dict(os.path.join(path, names[0])), cfg, np.load(os.path.join(path, "global_means.npy")),
                   np.load(os.path.join(path, "global_stds.npy")), statics, maps)
