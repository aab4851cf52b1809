"""The invariant of ``leads.run_model`` on the MI355X with the Pangu toy model (49 x 192): a product run, one that ends well or one whose
call-back fails on the host at lead 1, leaves nothing behind that a plain ``rollout`` after it would continue from."""
from __future__ import annotations

import datetime

import numpy as np
import pytest

from skyrim_amd import derived as D

pytestmark = pytest.mark.gpu
T0 = datetime.datetime(2024, 5, 13, 18, 0)


def test_a_product_run_leaves_the_plain_rollout_bit_for_bit_what_it_was(toy, monkeypatch):
    from skyrim_amd.core.models.pangu import PanguModel
    g, params, _ = toy
    pangu = PanguModel(ic_source="gfs", geom=g, params=params)

    def rollout():
        pred, _ = pangu.rollout(T0, 2, save=False)
        return np.array(pred.values)

    def left_clean():
        return pangu.model._resident_state is None and "_state_is_own_output" not in pangu.model.__dict__
    first = rollout()
    assert np.isfinite(first).all() and first.std() > 0

    add, calls = D.LeadDeriver.add, []

    def failing(self, states, table=None):
        calls.append(len(calls))
        if len(calls) == 2:
            raise ValueError("lead 1 fails on the host")
        return add(self, states, table)
    with monkeypatch.context() as m:
        m.setattr(D.LeadDeriver, "add", failing)
        with pytest.raises(ValueError, match="lead 1 fails on the host") as caught:
            pangu.derive_fields(T0, 2, ["ws10m"])
        assert calls == [0, 1] and caught.value.__traceback__ is not None and left_clean()       # (while the traceback still holds the frames)
    assert np.array_equal(rollout(), first)

    da = pangu.derive_fields(T0, 2, ["ws10m"])
    assert da.shape == (3, 1, 49, 192) and np.isfinite(da.values).all() and left_clean()
    assert np.array_equal(rollout(), first)
