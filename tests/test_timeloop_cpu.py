"""The TimeLoop protocol of the two-level models (FuXi, FengWu, DLWP) without a GPU: the real loops, built through their real ``__init__``
on toy configurations, over a CPU stand-in for the engine that records what it is handed.  The state is (C, 3, 4) and one network call is
``newer + 1`` (DLWP: t + 6 h = ``newer + 1``, t + 12 h = ``newer + 2``), so every yield, every argument and every step number below follows
from the loops' contract: first yield = the input's newest level, then one call per yield."""
from __future__ import annotations

import datetime
import importlib
from types import SimpleNamespace

import pytest
import torch

T0 = datetime.datetime(2024, 1, 1, 12)
H6 = datetime.timedelta(hours=6)
INF = float("inf")


class _Stub:
    """An engine on the CPU: ``call`` = newer + 1; the ``bad``-th call of its life returns a state with one inf."""
    pair = False

    def __init__(self, cfg, device):
        self.cfg, self.device, self.state_shape = cfg, torch.device("cpu"), (cfg.channels, 3, 4)
        self.loaded, self.calls, self.outs, self.released, self.bad = [], [], [], 0, None

    def load_params(self, params):
        self.loaded.append(params)

    def release(self):
        self.released += 1

    def call(self, *args):
        self.calls.append(args)
        y = args[1] + 1
        if len(self.calls) == self.bad:
            y[0, 0, 0] = INF
        out = (y, y + 1) if self.pair else y
        self.outs.append(out)
        return out


class _PairStub(_Stub):
    pair = True


def _substitute_engine(monkeypatch, cls, stub):
    """The loop class builds ``stub`` where it would build its HIP engine."""
    monkeypatch.setattr(cls, "engine_class", stub)


def _fuxi():
    from skyrim_amd.fuxi.spec import FuxiConfig
    from skyrim_amd.fuxi.timeloop import FuxiTimeLoop
    return FuxiTimeLoop, FuxiConfig(n_lat=73, n_lon=144, channels=6, embed=128, heads=2, depth=2, window=(3, 6), cascade_steps=(1, 4))


def _fengwu():
    from skyrim_amd.fengwu.spec import FengwuConfig
    from skyrim_amd.fengwu.timeloop import FengwuTimeLoop
    return FengwuTimeLoop, FengwuConfig(n_lat=33, n_lon=64, modalities=(("surface", 4), ("z", 5), ("q", 5), ("u", 5), ("v", 5), ("t", 5)),
                                        dims=(64, 128), heads=(2, 4), enc_depths=(1, 1), dec_depths=(1, 1), fuser_depth=2, window2d=(4, 4),
                                        window3d=(2, 4, 4))


def _dlwp():
    from skyrim_amd.dlwp.spec import DlwpConfig
    from skyrim_amd.dlwp.timeloop import DlwpTimeLoop
    return DlwpTimeLoop, DlwpConfig(n_lat=33, n_lon=64, face=8)


#        name: (loop class and toy config, key of channel_std, engine stand-in, hours per yield, name in the guard's hint, weight variable)
MODELS = {"fuxi": (_fuxi, "norm.std", _Stub, 6, "FuXi", "SKYRIM_FUXI_WEIGHTS"),
          "fengwu": (_fengwu, "norm.std", _Stub, 6, "FengWu", "SKYRIM_FENGWU_WEIGHTS"),
          "dlwp": (_dlwp, "scale", _PairStub, 12, "DLWP", "SKYRIM_DLWP_WEIGHTS")}


def _build(monkeypatch, name, params="toy"):
    make, std_key, stub, _, _, _ = MODELS[name]
    cls, cfg = make()
    _substitute_engine(monkeypatch, cls, stub)
    if params == "toy":
        params = {std_key: torch.arange(1.0, cfg.channels + 1)}              # just the key the loop reads
    return cls(params=params, cfg=cfg, device="cpu"), cfg, params


def _x(cfg, seed=0):
    """Small whole numbers: every ``+ 1`` below is exact."""
    return torch.randint(-8, 9, (1, 2, cfg.channels, 3, 4), generator=torch.Generator().manual_seed(seed)).float()


def _take(gen, n):
    return [next(gen) for _ in range(n)]


# ---- construction ---------------------------------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize("name", list(MODELS))
def test_construction_binds_engine_weights_channels_grid_and_guard(monkeypatch, name):
    loop, cfg, params = _build(monkeypatch, name)
    eng = loop.engine
    assert loop.cfg is cfg and eng.cfg is cfg and eng.loaded == [params]
    assert loop.n_history_levels == 2 and loop.device == torch.device("cpu") and loop.to("cpu") is loop
    assert loop.time_step == datetime.timedelta(hours=MODELS[name][3])
    assert torch.equal(loop.channel_std, torch.arange(1.0, cfg.channels + 1)) and loop.channel_std.dtype == torch.float32
    real = importlib.import_module(f"skyrim_amd.{name}.spec").CHANNELS
    names = real if len(real) == cfg.channels else [f"c{i}" for i in range(cfg.channels)]       # the model's names only at its own width
    assert loop.in_channel_names == names and loop.out_channel_names == names and (name == "dlwp") == (names == real)
    assert loop.grid.shape == (cfg.n_lat, cfg.n_lon) and loop.grid.lat[0] == 90.0 and loop.grid.lat[-1] == -90.0 and loop.grid.lon[0] == 0.0
    assert loop.guard.hint == f"the {MODELS[name][4]} network produced non-finite values" and loop.take_pending_check() is None
    with pytest.raises(NotImplementedError, match="bound to one GPU"):
        loop.to("cuda:1")
    loop.release()
    assert eng.released == 1


@pytest.mark.parametrize("name", list(MODELS))
def test_parameters_come_from_the_weight_variable_or_are_refused(monkeypatch, tmp_path, name):
    std_key, env = MODELS[name][1], MODELS[name][5]
    monkeypatch.delenv(env, raising=False)
    monkeypatch.delenv("SKYRIM_SYNTHETIC_WEIGHTS", raising=False)
    with pytest.raises(RuntimeError, match=f"^{name}: no parameters given and {env} is unset"):
        _build(monkeypatch, name, params=None)
    cfg = MODELS[name][0]()[1]
    torch.save({std_key: torch.full((cfg.channels,), 2.0)}, tmp_path / "slots.pt")
    monkeypatch.setenv(env, str(tmp_path / "slots.pt"))
    loop, _, _ = _build(monkeypatch, name, params=None)                    # a torch file of the slot dict is read as it is
    assert list(loop.engine.loaded[0]) == [std_key] and torch.equal(loop.channel_std, torch.full((cfg.channels,), 2.0))


# ---- yields and call arguments ------------------------------------------------------------------------------------------------------------ #
@pytest.mark.parametrize("name", list(MODELS))
def test_first_yield_is_a_copy_of_the_newest_level_and_times_advance(monkeypatch, name):
    loop, cfg, _ = _build(monkeypatch, name)
    x = _x(cfg)
    want = x[0, 1].clone()
    restart = object()
    gen = loop(T0, x, restart)
    t, first, r = next(gen)
    x.zero_()                                                                # the loop holds copies: the caller's tensor is its own again
    assert t == T0 and r is restart and tuple(first.shape) == (1, cfg.channels, 3, 4) and torch.equal(first[0], want)
    later = _take(gen, 3)
    gen.close()
    dt = datetime.timedelta(hours=MODELS[name][3])
    assert [t for t, _, _ in later] == [T0 + dt, T0 + 2 * dt, T0 + 3 * dt] and all(r is restart for _, _, r in later)
    inc = 2 if name == "dlwp" else 1
    for k, (_, y, _) in enumerate(later, 1):
        assert torch.equal(y[0], want + inc * k)
    assert torch.equal(first[0], want)                                       # every step's output is a new tensor


def test_fengwu_call_sees_the_previous_newer_as_older(monkeypatch):
    loop, cfg, _ = _build(monkeypatch, "fengwu")
    x = _x(cfg)
    gen = loop(T0, x.clone())
    ys = _take(gen, 4)
    gen.close()
    calls = loop.engine.calls
    assert [len(c) for c in calls] == [2, 2, 2]
    assert torch.equal(calls[0][0], x[0, 0]) and torch.equal(calls[0][1], x[0, 1])
    for k in (1, 2):
        assert calls[k][0] is calls[k - 1][1] and calls[k][1] is loop.engine.outs[k - 1]
    assert ys[3][1][0].data_ptr() == loop.engine.outs[2].data_ptr()


def test_fuxi_call_also_sees_the_time_and_the_stage(monkeypatch):
    loop, cfg, _ = _build(monkeypatch, "fuxi")
    x = _x(cfg)
    gen = loop(T0, x.clone())
    _take(gen, 7)
    gen.close()
    calls = loop.engine.calls
    assert [len(c) for c in calls] == [4] * 6
    assert torch.equal(calls[0][0], x[0, 0]) and torch.equal(calls[0][1], x[0, 1])
    assert [c[2] for c in calls] == [T0 + k * H6 for k in range(6)]          # the time of the call's newest input level
    assert [c[3] for c in calls] == ["short", "medium", "medium", "medium", "long", "long"]      # cascade_steps = (1, 4)
    for k in range(1, 6):
        assert calls[k][0] is calls[k - 1][1] and calls[k][1] is loop.engine.outs[k - 1]
    assert [loop.stage_for(k) for k in (1, 2, 4, 5)] == ["short", "medium", "medium", "long"]


def test_fuxi_cascade_goes_on_from_its_own_output_and_restarts_otherwise(monkeypatch):
    loop, cfg, _ = _build(monkeypatch, "fuxi")
    gen = loop(T0, _x(cfg))
    _take(gen, 4)                                                            # three steps
    gen.close()
    loop._state_is_own_output = True                                         # what run_basic_inference sets on the resident state
    gen = loop(T0 + 3 * H6, _x(cfg, 1))
    _take(gen, 3)
    gen.close()
    assert "_state_is_own_output" not in loop.__dict__
    assert [c[3] for c in loop.engine.calls[3:]] == ["medium", "long"]       # steps 4 and 5 of the whole rollout
    gen = loop(T0, _x(cfg, 2))                                               # no mark: any other input is an initial condition
    _take(gen, 2)
    gen.close()
    assert loop.engine.calls[5][3] == "short"


def test_fengwu_step_count_continues_under_the_mark(monkeypatch):
    loop, cfg, _ = _build(monkeypatch, "fengwu")
    gen = loop(T0, _x(cfg))
    _take(gen, 4)
    gen.close()
    loop.engine.bad = 4
    loop._state_is_own_output = True
    gen = loop(T0 + 3 * H6, _x(cfg, 1))
    with pytest.raises(FloatingPointError, match="after step 4: the FengWu network produced non-finite values"):
        _take(gen, 2)
        gen.close()
    assert "_state_is_own_output" not in loop.__dict__


def test_dlwp_hands_back_the_engines_pair_and_keeps_the_history_of_the_last_yield(monkeypatch):
    loop, cfg, _ = _build(monkeypatch, "dlwp")
    x = _x(cfg)
    assert loop.history_for(x) is None                                       # before the first yield
    gen = loop(T0, x.clone())
    (_, first, _), (_, y, _), (_, z, _) = _take(gen, 3)
    calls, outs = loop.engine.calls, loop.engine.outs
    assert [len(c) for c in calls] == [3, 3] and [c[2] for c in calls] == [T0, T0 + 2 * H6]
    assert torch.equal(calls[0][0], x[0, 0]) and torch.equal(calls[0][1], x[0, 1])
    assert calls[1][0] is outs[0][0] and calls[1][1] is outs[0][1]           # exactly the two tensors the engine returned
    assert y[0].data_ptr() == outs[0][1].data_ptr() and torch.equal(z[0], x[0, 1] + 4)
    hist = loop.history_for(z)
    assert len(hist) == 2 and hist[1] is z and torch.equal(hist[0], outs[1][0][None]) and hist[0].data_ptr() == outs[1][0].data_ptr()
    assert loop.history_for(y) is None and loop.history_for(z.clone()) is None and loop.history_for(first) is None
    gen.close()
    assert loop.history_time_step == H6


@pytest.mark.parametrize("mark", [False, True])
def test_dlwp_step_count_restarts_and_leaves_the_mark(monkeypatch, mark):
    loop, cfg, _ = _build(monkeypatch, "dlwp")
    gen = loop(T0, _x(cfg))
    _take(gen, 4)
    gen.close()
    loop.engine.bad = 4
    if mark:
        loop._state_is_own_output = True
    gen = loop(T0 + 6 * H6, _x(cfg, 1))
    with pytest.raises(FloatingPointError, match="after step 1: the DLWP network produced non-finite values"):
        _take(gen, 2)
        gen.close()
    assert ("_state_is_own_output" in loop.__dict__) == mark                 # leads.forget_resident clears it, not the loop


# ---- the deferred finite check --------------------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize("name", list(MODELS))
def test_non_finite_state_is_reported_with_its_step_by_close_at_the_latest(monkeypatch, name):
    loop, cfg, _ = _build(monkeypatch, name)
    loop.engine.bad = 2
    gen = loop(T0, _x(cfg))
    with pytest.raises(FloatingPointError, match=f"after step 2: the {MODELS[name][4]} network produced non-finite values"):
        _take(gen, 3)                                                        # the flag of step 2 is pending
        gen.close()


@pytest.mark.parametrize("name", list(MODELS))
def test_a_taken_check_is_the_callers(monkeypatch, name):
    loop, cfg, _ = _build(monkeypatch, name)
    loop.engine.bad = 2
    gen = loop(T0, _x(cfg))
    _take(gen, 3)
    flag, step, hint = loop.take_pending_check()
    assert not bool(flag) and step == 2 and hint == f"the {MODELS[name][4]} network produced non-finite values"
    assert loop.take_pending_check() is None
    gen.close()                                                              # nothing left to check


@pytest.mark.parametrize("name", list(MODELS))
def test_two_open_generators_check_their_own_states(monkeypatch, name):
    loop, cfg, _ = _build(monkeypatch, name)
    loop.engine.bad = 2
    a = loop(T0, _x(cfg))
    _take(a, 3)                                                              # calls 1 and 2: a's step 2 is non-finite and pending
    b = loop(T0, _x(cfg, 1))
    _take(b, 2)                                                              # call 3
    flag, step, _ = loop.take_pending_check()                                # answers for the generator opened last
    assert bool(flag) and step == 1
    _take(b, 1)
    b.close()                                                                # b's own step 2 is finite
    with pytest.raises(FloatingPointError, match="after step 2"):
        a.close()


# ---- refusals --------------------------------------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize("name", list(MODELS))
def test_two_level_shape_refusal(monkeypatch, name):
    loop, cfg, _ = _build(monkeypatch, name)
    C = cfg.channels
    for bad in (torch.zeros(1, 1, C, 3, 4), torch.zeros(2, C, 3, 4), torch.zeros(1, 2, C, 3, 5)):
        with pytest.raises(ValueError) as e:
            next(loop(T0, bad))
        assert str(e.value) == f"expected x of shape (1, 2, {C}, 3, 4) (states at time - 6 h and time), got {tuple(bad.shape)}"
    assert loop.engine.calls == []


def test_pangu_and_graphcast_loops_keep_their_own_initial_condition_hooks():
    """``GlobalModel.build_datasource`` hands a loop's ``synthetic_state`` to the synthetic DataSource when it has one: Pangu's loop has
    none (its source makes the fields from the geometry), GraphCast's is its own."""
    from skyrim_amd.graphcast.timeloop import GraphcastTimeLoop
    from skyrim_amd.pangu.timeloop import PanguTimeLoop
    assert not hasattr(PanguTimeLoop, "synthetic_state") and not hasattr(PanguTimeLoop, "_load")
    assert "synthetic_state" in vars(GraphcastTimeLoop) and "_load" in vars(GraphcastTimeLoop)


@pytest.mark.parametrize("path", ["skyrim_amd.fcn.timeloop:FcnTimeLoop", "skyrim_amd.sfno.timeloop:SfnoTimeLoop"])
def test_single_level_loops_keep_their_call_and_refusal(path):
    mod, cls = path.split(":")
    cls = getattr(importlib.import_module(mod), cls)
    loop = cls.__new__(cls)
    loop.engine = SimpleNamespace(state_shape=(2, 3, 4), device=torch.device("cpu"), step=lambda s: s + 1)
    assert cls.n_history_levels == 1 and cls.time_step == H6 and not hasattr(loop, "guard") and not hasattr(loop, "take_pending_check")
    with pytest.raises(ValueError) as e:
        next(loop(T0, torch.zeros(1, 2, 2, 3, 4)))
    assert str(e.value) == "expected x of shape (1, 1, 2, 3, 4), got (1, 2, 2, 3, 4)"
    x = torch.zeros(1, 1, 2, 3, 4)
    gen = loop(T0, x)
    (t0, a, _), (t1, b, _) = _take(gen, 2)
    assert (t0, t1) == (T0, T0 + H6) and torch.equal(a[0], x[0, 0]) and torch.equal(b[0], x[0, 0] + 1)
