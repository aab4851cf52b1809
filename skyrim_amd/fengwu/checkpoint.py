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
import os

import numpy as np
import torch

from .. import weights
from ..pangu.onnx_weights import load_graph_slots, map_slots, read_norm_json
from .spec import FengwuConfig, param_spec, shape_source

MAP_FILE = "fengwu.map.json"


def load(path: str, cfg: FengwuConfig) -> dict:
    return weights.load_slots(path, lambda d: load_onnx_dir(d, cfg))


def graph_mapping(model, cfg: FengwuConfig, explicit: dict | None = None) -> tuple[dict, list]:
    """{slot: [onnx_name, transform]} and the list of unresolved slots."""
    return map_slots(model, param_spec(cfg), explicit)


def _affine(path: str, cfg: FengwuConfig) -> tuple:
    npy = [os.path.join(path, f) for f in ("global_means.npy", "global_stds.npy")]
    if all(os.path.exists(f) for f in npy):
        mean, std = (torch.tensor(np.load(f).astype(np.float64).reshape(-1), dtype=torch.float32) for f in npy)
    else:
        norm = read_norm_json(path)
        if norm is None:
            raise ValueError(f"{path}: the input affine is missing (global_means.npy + global_stds.npy, or norm.json)")
        mean, std = norm[0].reshape(-1), norm[1].reshape(-1)
    if mean.numel() != cfg.channels or std.numel() != cfg.channels:
        raise ValueError(f"{path}: the input affine holds {mean.numel()} / {std.numel()} values, the config's modalities {cfg.channels} channels")
    return mean, std


def load_onnx_dir(path: str, cfg: FengwuConfig) -> dict:
    graphs = sorted(glob.glob(os.path.join(path, "*.onnx")))
    if len(graphs) != 1:
        raise ValueError(f"{path}: expected exactly one *.onnx graph, found {len(graphs)}")
    out = {}
    out["norm.mean"], out["norm.std"] = _affine(path, cfg)
    out.update(load_graph_slots(graphs[0], param_spec(cfg), os.path.join(path, MAP_FILE), source=lambda slot: f"FengwuConfig.{shape_source(slot)}"))
    return out
