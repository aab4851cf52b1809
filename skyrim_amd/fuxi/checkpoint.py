"""FuXi weights -> the engine's parameter mapping (``spec.full_param_spec``).

``SKYRIM_FUXI_WEIGHTS`` names either
  * a torch file of the parameter dict (keys ``norm.mean``, ``norm.std`` and ``<stage>.<name>``), or
  * a directory of FuXi's release: ``short.onnx``, ``medium.onnx``, ``long.onnx``, each with its external-data file next to it.

The ONNX graphs are read with the dependency-free reader (pangu/onnx_weights.py), external data opted in with the directory as base.
Each stage's initializers are mapped onto ``spec.param_spec`` by shape in order of use (``auto_map_slots``) unless ``<stage>.map.json``
in the directory gives the mapping explicitly ({slot: onnx_name | [onnx_name, transform]}); every slot left unresolved is reported.
The input affine is not a graph initializer this reader can place: ``norm.json`` ({"mean": [70], "std": [70]}) supplies it (UNVERIFIED,
DESIGN.md 15: whether the graphs normalise internally -- then norm.json holds the graph's own constants).
"""
from __future__ import annotations

import json
import os

import numpy as np
import torch

from ..pangu.onnx_weights import _apply, auto_map_slots, read_model
from .spec import STAGES, FuxiConfig, param_spec


def load(path: str, cfg: FuxiConfig) -> dict:
    if os.path.isdir(path):
        return load_onnx_dir(path, cfg)
    return torch.load(path, map_location="cpu")


def stage_mapping(model, cfg: FuxiConfig, explicit: dict | None = None) -> tuple[dict, list]:
    """{slot: [onnx_name, transform]} for one stage and the list of unresolved slots."""
    slots = param_spec(cfg)
    if explicit is not None:
        mapping = {k: (v if isinstance(v, list) else [v, "id"]) for k, v in explicit.items()}
        return mapping, [s for s, _ in slots if s not in mapping]
    return auto_map_slots(model, slots)


def load_onnx_dir(path: str, cfg: FuxiConfig) -> dict:
    out = {}
    norm = os.path.join(path, "norm.json")
    if not os.path.exists(norm):
        raise ValueError(f"{path}: norm.json missing -- the input affine ({{\"mean\": [{cfg.channels}], \"std\": [{cfg.channels}]}}) of the graphs")
    with open(norm) as f:
        n = json.load(f)
    out["norm.mean"] = torch.tensor(n["mean"], dtype=torch.float32)
    out["norm.std"] = torch.tensor(n["std"], dtype=torch.float32)
    shapes = dict(param_spec(cfg))
    for st in STAGES:
        f = os.path.join(path, f"{st}.onnx")
        if not os.path.exists(f):
            raise ValueError(f"{path}: {st}.onnx missing (the directory holds short.onnx, medium.onnx and long.onnx)")
        model = read_model(f, base_dir=path)
        mp = os.path.join(path, f"{st}.map.json")
        explicit = None
        if os.path.exists(mp):
            with open(mp) as fh:
                explicit = json.load(fh)
        mapping, unresolved = stage_mapping(model, cfg, explicit)
        if unresolved:
            raise ValueError(f"{f}: {len(unresolved)} parameter slots unresolved: {unresolved}; write {st}.map.json "
                             "({slot: onnx_name | [onnx_name, transform]}) next to it")
        for slot, (name, how) in mapping.items():
            if name not in model.initializers:
                raise KeyError(f"{slot}: initializer {name!r} not in {f}")
            out[f"{st}.{slot}"] = torch.from_numpy(_apply(model.initializers[name].array().astype(np.float32), how, shapes[slot]))
    return out
