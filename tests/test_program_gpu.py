"""The prelude the five program-driven bindings share (``derived.run``, ``thermo.run``, ``vertical.run``, ``aggregate.run``,
``neighbourhood.run``): the exact text of every refusal it makes, in the order it makes them -- each call breaks one thing more than
the one before mends, so a later check that ran first would speak instead -- with no refusal reaching a launch; then one valid launch
per binding against the restatement its kernel tests use.  The messages are what the users of ``torch.ops.skyrim_hip.*_fields`` see."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import _agg_reference as RA
import _derive_reference as RD
import _nbr_reference as RN
import _thermo_reference as RT
import _vert_reference as RV
from skyrim_amd import aggregate as A
from skyrim_amd import derived as D
from skyrim_amd import neighbourhood as N
from skyrim_amd import thermo as T
from skyrim_amd import vertical as V
from skyrim_amd.members import member_table
from skyrim_amd.tracks import EARTH_RADIUS_KM
from skyrim_amd.verify import area_weights

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
M, C, H, W = 2, 6, 5, 8

_LAT, _LON = RN.grid(H, W)
_REACH, _HALF = N.discs(_LAT, _LON, 1.53 * np.deg2rad(180.0 / (H - 1)) * EARTH_RADIUS_KM)      # about a row and a half


def states():
    """M states (C, H, W) float32 that every one of the five ops can read: temperatures in kelvin"""
    rng = np.random.default_rng(7)
    return [(250.0 + 50.0 * rng.random((C, H, W))).astype(np.float32) for _ in range(M)]


# per binding: the module, the name in front of its messages, the name of its output, one valid minimal op, the call and the restatement
def _derive(members, table, ops, out):
    D.run(members, table, ops, out)


def _derive_ref(x):
    exact, S = RD.diff(x[0], x[1])
    return exact, RD.bound(RD.K_DIFF, S, RD.TINY_DIFF)


def _thermo(members, table, ops, out):
    T.run(members, table, ops, out)


def _thermo_ref(x):
    return RT.fp32.moist(x[0], x[0], 850.0, T.Q, theta_only=True)[3], None


def _vert(members, table, ops, out):
    V.run(members, table, ops, out)


VERT_OP = V.Op(V.P, (850.0, 500.0), (), (), (V.target_value(V.P, 700.0),), (V.Field(V.PLAIN, (0, 1), (), (0,)),), V.NAN)


def _vert_ref(x):
    return RV.fp32.apply(VERT_OP, x, None)[0], None


def _agg(members, table, ops, out):
    A.run(members, table, ops, out, 6.0)


def _agg_ref(x):
    acc = np.zeros((1, 1, H, W), np.float32)
    RA.update(x[None], acc, [A.Op(A.MAX, 0, 0, -1, A.FIRST)], 6.0)
    return acc[0, 0], None


def _nbr(members, table, ops, out):
    N.run(members, table, ops, [torch.from_numpy(_HALF).to(DEV)], torch.from_numpy(area_weights(_LAT)).to(DEV), out)


def _nbr_ref(x):
    return RN.one(x[0], N.MAX, _REACH, _HALF), None


CASES = {"derive": (D, "derive_fields", "out", D.Op(D.DIFF, (0, 1), (0,)), _derive, _derive_ref),
         "thermo": (T, "thermo_fields", "out", T.Op(T.MOIST, (0,), (), (), (-1, -1, -1, 0), T.Q, (850.0,)), _thermo, _thermo_ref),
         "vert": (V, "vert_fields", "out", VERT_OP, _vert, _vert_ref),
         "agg": (A, "agg_update", "acc", A.Op(A.MAX, 0, 0, -1, A.FIRST), _agg, _agg_ref),
         "nbr": (N, "nbr_fields", "out", N.Op(N.MAX, 0, 0, 0), _nbr, _nbr_ref)}


@pytest.mark.parametrize("name", list(CASES))
def test_refusals_in_order_then_one_launch(name, monkeypatch):
    mod, what, out_name, op, call, ref = CASES[name]
    host = states()
    members = [torch.from_numpy(s).to(DEV) for s in host]
    table = member_table(members)
    out = torch.zeros((M, 1, H, W), dtype=torch.float32, device=DEV)
    dev = members[0].device

    def launched():
        raise AssertionError("a refused call reached the launch")

    def refused(message, members=members, table=table, ops=(op,), out=out):
        with pytest.raises(ValueError) as e:
            call(list(members), table, list(ops), out)
        assert str(e.value) == message

    with monkeypatch.context() as mp:
        mp.setattr(mod, "load_library", launched)
        f64_member = [members[0].double()] + members[1:]
        long_table = member_table(members + members[:1])
        f64_out = out.double()
        tall_out = torch.zeros((M, 1, H + 1, W), dtype=torch.float32, device=DEV)
        more_out = torch.zeros((M + 1, 1, H, W), dtype=torch.float32, device=DEV)
        # each line keeps what the lines after it break: the earlier refusal is the one that speaks
        refused(f"{what}: 0 members; 1 to 64 are supported", members=[], ops=(), table=long_table, out=f64_out)
        refused(f"{what}: 65 members; 1 to 64 are supported", members=members[:1] * 65, ops=(), table=long_table, out=f64_out)
        refused(f"{what}: 0 ops; 1 to 16 are supported", members=f64_member, ops=(), table=long_table, out=f64_out)
        refused(f"{what}: 17 ops; 1 to 16 are supported", members=f64_member, ops=(op,) * 17, table=long_table, out=f64_out)
        refused(f"{what}: member: expected a contiguous float32 tensor on {dev}", members=f64_member, table=long_table, out=f64_out)
        refused(f"{what}: table must be member_table(members)", table=long_table, out=f64_out)
        refused(f"{what}: {out_name}: expected a contiguous float32 tensor on {dev}", out=f64_out)
        refused(f"{what}: {out_name} must be ({M}, D, {H}, {W})", out=tall_out)
        refused(f"{what}: {out_name} must be ({M}, D, {H}, {W})", out=more_out)
    assert not out.any()

    call(members, table, [op], out)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    for m in range(M):
        want, bound = ref(host[m])
        if bound is None:                                      # a restatement in float32: the same bits
            assert np.array_equal(got[m, 0].view(np.uint32), np.asarray(want, np.float32).view(np.uint32)), (name, m)
        else:                                                  # a float64 restatement and the header's bound
            assert np.all(np.abs(got[m, 0].astype(np.float64) - want) <= bound), (name, m)
