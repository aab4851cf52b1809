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

import os

from .. import weights
from ..pangu.onnx_weights import load_graph_slots, map_slots, read_norm_json
from .spec import STAGES, FuxiConfig, param_spec


def load(path: str, cfg: FuxiConfig) -> dict:
    return weights.load_slots(path, lambda d: load_onnx_dir(d, cfg))


def stage_mapping(model, cfg: FuxiConfig, explicit: dict | None = None) -> tuple[dict, list]:
    """{slot: [onnx_name, transform]} for one stage and the list of unresolved slots."""
    return map_slots(model, param_spec(cfg), explicit)


def load_onnx_dir(path: str, cfg: FuxiConfig) -> dict:
    norm = read_norm_json(path)
    if norm is None:
        raise ValueError(f"{path}: norm.json missing -- the input affine ({{\"mean\": [{cfg.channels}], \"std\": [{cfg.channels}]}}) of the graphs")
    out = {"norm.mean": norm[0], "norm.std": norm[1]}
    for st in STAGES:
        f = os.path.join(path, f"{st}.onnx")
        if not os.path.exists(f):
            raise ValueError(f"{path}: {st}.onnx missing (the directory holds short.onnx, medium.onnx and long.onnx)")
        stage = load_graph_slots(f, param_spec(cfg), os.path.join(path, f"{st}.map.json"))
        out.update({f"{st}.{slot}": t for slot, t in stage.items()})
    return out
