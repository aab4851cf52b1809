"""The shell the ctypes-bound engines share (skyrim_amd/engine.py), on a stand-in subclass without a GPU: what ``release()`` keeps and
drops, the refusal of a wrong state tensor, the refusal of an unprepared engine under each engine's name, the input affine and the
shape-checking parameter view."""
from __future__ import annotations

import pytest
import torch

from skyrim_amd.engine import CheckedParams, Engine


class _Toy(Engine):
    keep = ("convs", "_label")

    def __init__(self):
        self.cfg, self.convs, self._label = "cfg", [1, 2], "gemm"
        self._bind("lib", "cpu", [2, 3, 4])


def test_bind_and_release_keep_the_declared_attributes_only():
    e = _Toy()
    assert (e.lib, e.device, e.state_shape, e.prepared) == ("lib", torch.device("cpu"), (2, 3, 4), False)
    e.buf, e.stages, e.prepared = torch.zeros(4), {"short": 1}, True
    e.release()
    assert vars(e) == dict(cfg="cfg", convs=[1, 2], _label="gemm", lib="lib", device=torch.device("cpu"), state_shape=(2, 3, 4), prepared=False)
    e.release()                                                              # twice is the same
    assert not e.prepared and e.convs == [1, 2]


def test_what_each_engine_keeps():
    from skyrim_amd.dlwp.engine import DlwpEngine
    from skyrim_amd.fcn.engine import FcnEngine
    from skyrim_amd.fengwu.engine import FengwuEngine
    from skyrim_amd.fuxi.engine import FuxiEngine
    from skyrim_amd.graphcast.engine import GraphcastEngine
    from skyrim_amd.sfno.engine import SfnoEngine
    assert FuxiEngine.keep == FengwuEngine.keep == FcnEngine.keep == ()
    assert DlwpEngine.keep == ("convs",) and SfnoEngine.keep == ("terms", "fused", "_label", "profiling")
    assert GraphcastEngine.keep == ("rank", "world", "reduce_fn", "gather_fn", "sf")
    for cls, extra in ((SfnoEngine, dict(chain=None, _events=[])), (GraphcastEngine, dict(_events=[]))):
        e = cls.__new__(cls)
        e.cfg, e.lib, e.device, e.state_shape, e.work = "cfg", "lib", torch.device("cpu"), (1, 2, 3), torch.zeros(3)
        for k in cls.keep:
            setattr(e, k, k)
        e.release()
        assert vars(e) == dict(cfg="cfg", lib="lib", device=torch.device("cpu"), state_shape=(1, 2, 3), prepared=False,
                               **{k: k for k in cls.keep}, **extra)


def test_check_state_names_what_is_wrong():
    e = _Toy()
    e.check_state(torch.zeros(2, 3, 4))
    e.check_state(torch.zeros(2, 3, 4), "x0")
    want = "expected a contiguous float32 tensor of shape (2, 3, 4) on cpu"
    for bad in (torch.zeros(2, 3, 5), torch.zeros(2, 3, 4, dtype=torch.float64), torch.zeros(2, 4, 3).transpose(1, 2), torch.zeros(2, 3, 4, device="meta")):
        with pytest.raises(ValueError) as err:
            e.check_state(bad)
        assert str(err.value) == want
        with pytest.raises(ValueError) as err:
            e.check_state(bad, "x1")
        assert str(err.value) == "x1: " + want


@pytest.mark.parametrize("path, method", [("fuxi.engine:FuxiEngine", "call"), ("fengwu.engine:FengwuEngine", "call"), ("dlwp.engine:DlwpEngine", "call"),
                                          ("fcn.engine:FcnEngine", "step"), ("sfno.engine:SfnoEngine", "step"), ("graphcast.engine:GraphcastEngine", "step")])
def test_an_unprepared_engine_is_refused_under_its_name(path, method):
    import importlib
    module, name = path.split(":")
    cls = getattr(importlib.import_module(f"skyrim_amd.{module}"), name)
    e = cls.__new__(cls)
    e.prepared = False
    n_args = {"fuxi": 3, "fengwu": 2, "dlwp": 3, "fcn": 1, "sfno": 1, "graphcast": 3}[module.split(".")[0]]
    with pytest.raises(RuntimeError) as err:
        getattr(e, method)(*[None] * n_args)                                 # refused before an argument is looked at
    assert str(err.value) == f"{name}.{method} before load_params: not prepared"
    e.prepared = True
    e.require_prepared(method)


def test_upload_affine_and_its_refusal():
    e = _Toy()
    e.upload_affine([1.0, 2.0, 3.0], torch.tensor([2.0, 4.0, 0.5]), 3)
    assert torch.equal(e.mean, torch.tensor([1.0, 2.0, 3.0])) and torch.equal(e.std, torch.tensor([2.0, 4.0, 0.5]))
    assert torch.equal(e.inv_std, torch.tensor([0.5, 0.25, 2.0])) and e.inv_std.dtype == e.mean.dtype == torch.float32
    for bad in (torch.tensor([1.0, 0.0, 1.0]), torch.ones(4), torch.ones(1, 3)):
        with pytest.raises(ValueError, match="^norm.std must hold 3 non-zero values$"):
            e.upload_affine(torch.zeros(3), bad, 3)


def test_checked_params_messages():
    params = {"short.embed.bias": torch.zeros(4), "head.weight": [[0.0, 1.0]]}
    stage = CheckedParams(params, {"embed.bias": (5,)}, prefix="short.")
    with pytest.raises(ValueError) as err:
        stage["embed.bias"]
    assert str(err.value) == "parameter short.embed.bias: expected shape (5,), got (4,)"
    assert CheckedParams(params, {"embed.bias": (4,)}, prefix="short.")["embed.bias"] is params["short.embed.bias"]
    sourced = CheckedParams(params, {"head.weight": (2, 1)}, source=lambda name: f"ToyConfig.dims of {name}")
    with pytest.raises(ValueError) as err:
        sourced["head.weight"]
    assert str(err.value) == "parameter head.weight: expected shape (2, 1) (from ToyConfig.dims of head.weight), got (1, 2)"
    assert torch.equal(CheckedParams(params, {"head.weight": (1, 2)})["head.weight"], torch.tensor([[0.0, 1.0]]))
    with pytest.raises(KeyError):
        stage["embed.weight"]
