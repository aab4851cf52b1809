"""FourCastNet v1 checkpoint (earth2mip's ``fcn`` package) -> the engine's parameter slots.

The reference obtains the weights through ``earth2mip.networks.fcn.load(registry.get_model("e2mip://fcn"))`` (the reference's
skyrim/core/models/fourcastnet.py:24-25): a weights archive holding the published ``AFNONet`` state dict -- bare or as
``{"model_state": ...}``, keys possibly prefixed ``module.`` -- plus ``global_means.npy`` / ``global_stds.npy``.  The key names below are
those of the published module structure (patch_embed.proj, pos_embed, blocks[i].{norm1, filter, norm2, mlp.fc1, mlp.fc2}, head) and are
UNVERIFIED against the real file (it is not obtainable offline), so ``convert`` follows sfno/checkpoint.py's rule: nothing is returned
partial or shape-mismatched, and every key it cannot place is reported by name.
"""
from __future__ import annotations

import os
import re

import numpy as np
import torch

from .. import weights
from .spec import FcnConfig, param_spec

# keys of the published model that the forward does not read: tolerated, never placed
IGNORED = [r"blocks\.\d+\.filter\.scale", r"head\.bias"]


def _strip(key: str) -> str:
    return re.sub(r"^(module\.)+", "", key)


def convert(state_dict: dict, cfg: FcnConfig, means, stds) -> dict:
    """``state_dict``: the model's state dict (tensors or arrays); ``means`` / ``stds``: arrays with one value per input channel
    (any shape of that size, e.g. (1, C, 1, 1)).  -> {slot: float32 tensor} for every slot of ``param_spec(cfg)``."""
    want = dict(param_spec(cfg))
    out, unplaced = {}, []
    for key, val in state_dict.items():
        slot = _strip(key)
        if slot not in want or slot.startswith("norm."):
            if not any(re.fullmatch(p, slot) for p in IGNORED):
                unplaced.append(key)
            continue
        t = torch.as_tensor(np.asarray(val)) if not torch.is_tensor(val) else val
        t = t.detach().float()
        if tuple(t.shape) != tuple(want[slot]):
            raise ValueError(f"checkpoint key {key!r} -> slot {slot}: shape {tuple(t.shape)} != expected {want[slot]}")
        out[slot] = t.contiguous()
    means = torch.as_tensor(np.asarray(means, dtype=np.float32)).flatten()
    stds = torch.as_tensor(np.asarray(stds, dtype=np.float32)).flatten()
    if means.numel() != cfg.in_chans or stds.numel() != cfg.in_chans:
        raise ValueError(f"normalisation arrays have {means.numel()} / {stds.numel()} values, expected {cfg.in_chans}")
    out["norm.mean"], out["norm.std"] = means, stds
    missing = [s for s in want if s not in out]
    if unplaced or missing:
        raise ValueError(f"checkpoint does not match the AFNONet layout: unplaced keys {sorted(unplaced)}, missing slots {missing}")
    return out


def load(path: str, cfg: FcnConfig) -> dict:
    return weights.load_slots(path, lambda d: load_package(d, cfg))


def load_files(weights_path: str, cfg: FcnConfig, means_path: str, stds_path: str) -> dict:
    sd = torch.load(weights_path, map_location="cpu", weights_only=False)
    if isinstance(sd, dict) and "model_state" in sd:
        sd = sd["model_state"]
    return convert(sd, cfg, np.load(means_path), np.load(stds_path))


def load_package(path: str, cfg: FcnConfig) -> dict:
    """A package directory: the one weights archive (``*.tar`` / ``*.pt`` / ``*.pth``) plus ``global_means.npy`` / ``global_stds.npy``."""
    names = sorted(n for n in os.listdir(path) if n.endswith((".tar", ".pt", ".pth")))
    if len(names) != 1:
        raise ValueError(f"{path}: expected exactly one weights archive (*.tar / *.pt / *.pth), found {names}")
    return load_files(os.path.join(path, names[0]), cfg, os.path.join(path, "global_means.npy"), os.path.join(path, "global_stds.npy"))
