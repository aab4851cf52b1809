"""FengWu weights -> the engine's parameter mapping (``spec.full_param_spec``).

``SKYRIM_FENGWU_WEIGHTS`` names either
  * a torch file of the parameter dict (keys ``norm.mean``, ``norm.std`` and the network's slots), or
  * a directory holding one ``*.onnx`` graph (its external-data files next to it) plus the input affine: ``global_means.npy`` and
    ``global_stds.npy`` (69 values each, any shape -- the files earth2studio's FengWu package ships), or ``norm.json``
    ({"mean": [69], "std": [69]}).

The graph is read with the dependency-free reader (pangu/onnx_weights.py), external data opted in with the directory as base.  Its
initializers are mapped onto ``spec.param_spec`` by shape in order of use (``auto_map_slots``) unless ``fengwu.map.json`` in the directory
gives the mapping explicitly ({slot: onnx_name | [onnx_name, transform]}); every slot left unresolved is reported.  The z, q, u, v and t
stacks have identical shapes, so the assumed order of use (spec.param_spec) is all that tells them apart (UNVERIFIED).
"""
from __future__ import annotations

import glob
import json
import os

import numpy as np
import torch

from ..pangu.onnx_weights import _apply, auto_map_slots, read_model
from .spec import FengwuConfig, param_spec, shape_source

MAP_FILE = "fengwu.map.json"


def load(path: str, cfg: FengwuConfig) -> dict:
    if os.path.isdir(path):
        return load_onnx_dir(path, cfg)
    return torch.load(path, map_location="cpu")


def graph_mapping(model, cfg: FengwuConfig, explicit: dict | None = None) -> tuple[dict, list]:
    """{slot: [onnx_name, transform]} and the list of unresolved slots."""
    slots = param_spec(cfg)
    if explicit is not None:
        mapping = {k: (v if isinstance(v, list) else [v, "id"]) for k, v in explicit.items()}
        return mapping, [s for s, _ in slots if s not in mapping]
    return auto_map_slots(model, slots)


def _affine(path: str, cfg: FengwuConfig) -> tuple:
    npy = [os.path.join(path, f) for f in ("global_means.npy", "global_stds.npy")]
    if all(os.path.exists(f) for f in npy):
        mean, std = (np.load(f).astype(np.float64).reshape(-1) for f in npy)
    elif os.path.exists(os.path.join(path, "norm.json")):
        with open(os.path.join(path, "norm.json")) as f:
            n = json.load(f)
        mean, std = np.asarray(n["mean"], dtype=np.float64).reshape(-1), np.asarray(n["std"], dtype=np.float64).reshape(-1)
    else:
        raise ValueError(f"{path}: the input affine is missing (global_means.npy + global_stds.npy, or norm.json)")
    if mean.size != cfg.channels or std.size != cfg.channels:
        raise ValueError(f"{path}: the input affine holds {mean.size} / {std.size} values, the config's modalities {cfg.channels} channels")
    return torch.tensor(mean, dtype=torch.float32), torch.tensor(std, dtype=torch.float32)


def load_onnx_dir(path: str, cfg: FengwuConfig) -> dict:
    graphs = sorted(glob.glob(os.path.join(path, "*.onnx")))
    if len(graphs) != 1:
        raise ValueError(f"{path}: expected exactly one *.onnx graph, found {len(graphs)}")
    out = {}
    out["norm.mean"], out["norm.std"] = _affine(path, cfg)
    model = read_model(graphs[0], base_dir=path)
    mp = os.path.join(path, MAP_FILE)
    explicit = None
    if os.path.exists(mp):
        with open(mp) as fh:
            explicit = json.load(fh)
    mapping, unresolved = graph_mapping(model, cfg, explicit)
    if unresolved:
        raise ValueError(f"{graphs[0]}: {len(unresolved)} parameter slots unresolved: {unresolved}; write {MAP_FILE} "
                         "({slot: onnx_name | [onnx_name, transform]}) next to it")
    shapes = dict(param_spec(cfg))
    for slot, (name, how) in mapping.items():
        if slot not in shapes:
            raise KeyError(f"{MAP_FILE}: {slot!r} is not a parameter slot of this config")
        if name not in model.initializers:
            raise KeyError(f"{slot}: initializer {name!r} not in {graphs[0]}")
        try:
            out[slot] = torch.from_numpy(_apply(model.initializers[name].array().astype(np.float32), how, shapes[slot]))
        except ValueError as e:
            raise ValueError(f"{graphs[0]}: slot {slot} (shape from FengwuConfig.{shape_source(slot)}): initializer {name!r}: {e}") from None
    return out
