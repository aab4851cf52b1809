"""The shared binding code of the product libraries without a GPU (skyrim_amd/members.py, ``native.tensor_ptr``, the helpers of
skyrim_amd/common.py): everything here is refused, or done, before any device work -- a CPU tensor fails ``tensor_ptr``'s check, and
the count refusals come first."""
from __future__ import annotations

import ctypes
import datetime
import re

import numpy as np
import pytest
import torch

from skyrim_amd import (aggregate, breeding, common, derived, ensemble, events, members, native, points, regrid, scenarios, spectra, tracks,
                        verify)

STATE = torch.zeros(2, 3, 5)
TABLE = torch.zeros(1, dtype=torch.int64)


@pytest.mark.parametrize("bad", [None, np.zeros(4, np.float32), torch.zeros(4, dtype=torch.float64), torch.zeros(4, 4)[:, 1], torch.zeros(4)],
                         ids=["none", "ndarray", "dtype", "view", "cpu"])
def test_tensor_ptr_refuses_with_the_pinned_message(bad):
    with pytest.raises(ValueError, match="^" + re.escape("x: y: expected a contiguous float32 tensor on the GPU") + "$"):
        native.tensor_ptr(bad, "x: y", torch.float32)
    with pytest.raises(ValueError, match="^" + re.escape("x: expected a contiguous int32 tensor on cuda:1") + "$"):
        native.tensor_ptr(bad, "x", torch.int32, torch.device("cuda:1"))


def test_member_set_refuses_a_count_outside_its_range():
    with pytest.raises(ValueError, match=r"^p: 0 members; 1 to 8 are supported$"):
        members.member_set([], TABLE, "p", 8)
    with pytest.raises(ValueError, match=r"^p: 9 members; 1 to 8 are supported$"):
        members.member_set([STATE] * 9, TABLE, "p", 8)
    with pytest.raises(ValueError, match=r"^p: 1 members; 2 to 8 are supported$"):
        members.member_set([STATE], TABLE, "p", 8, lo=2)
    with pytest.raises(ValueError, match=r"^p: 0 members; 1 to 8 are supported$"):
        members.member_count([], "p", 8)
    assert members.member_count([STATE] * 8, "p", 8) == 8
    # past the count: the rank, then the members themselves (on the CPU here)
    with pytest.raises(ValueError, match=r"^p: states are \(C, H, W\)$"):
        members.member_set([STATE[0]], TABLE, "p", 8)
    with pytest.raises(ValueError, match=r"^p: member: expected a contiguous float32 tensor on cpu$"):
        members.member_set([STATE], TABLE, "p", 8)
    assert ensemble.member_table is members.member_table


def test_fill_channels_writes_the_count_and_the_first_entries():
    class Desc(ctypes.Structure):
        _fields_ = [("nc", ctypes.c_int), ("channels", ctypes.c_int32 * 4)]

    d = Desc()
    members.fill_channels(d, [3, 1, 2], 4)
    assert d.nc == 3 and list(d.channels) == [3, 1, 2, 0]
    members.fill_channels(d, (np.int64(7), 6, 5, 4, 9, 8), 4)            # nc counts what does not fit: the callers refuse it
    assert d.nc == 6 and list(d.channels) == [7, 6, 5, 4]


def test_common_iso_world_size_and_finish(tmp_path):
    assert common.iso(datetime.datetime(2024, 5, 13, 18, 0)) == "2024-05-13T18:00:00"
    assert common.iso(np.datetime64("2024-05-13T18:00:00.123456")) == "2024-05-13T18:00:00"
    assert common.iso(np.datetime64("2024-05-13T18")) == "2024-05-13T18:00:00"
    assert common.world_size() == 1
    assert verify._iso is common.iso is tracks._iso and verify._finish is common.finish is tracks._finish

    class Result:
        forecast_id, path = "", None

        def save(self, output_dir):
            return f"{output_dir}/{self.forecast_id}.json"

    r, cfg = Result(), {"output_dir": str(tmp_path)}
    assert common.finish(r, False, cfg) is r and r.path is None and "forecast_id" not in cfg
    assert common.finish(r, True, cfg) is r and cfg["forecast_id"] == r.forecast_id != "" and r.path == f"{tmp_path}/{r.forecast_id}.json"
    assert common.finish(Result(), True, None).path.startswith(common.OUTPUT_DIR)


_NO_MEMBERS = {
    "ens_stats": lambda: ensemble.stats([], TABLE, 0, 0),
    "score_fields": lambda: verify.score([], TABLE, STATE, None, None, None, verify.DET),
    "event_counts": lambda: events.run([], TABLE, STATE, [0], [[1.0]], None),
    "track_detect": lambda: tracks.detect([], TABLE, [0] * 7, (1, 2), [0.0] * 4, None, None, None, None, None, None, None, None),
    "derive_fields": lambda: derived.run([], TABLE, [], None),
    "regrid": lambda: regrid.run([], TABLE, [0], None, None, None),
    "agg_update": lambda: aggregate.run([], TABLE, [], None, 0.0),
    "point_gather": lambda: points.run([], TABLE, [0], None, None),
    "gram": lambda: scenarios.gram([], TABLE, None, [0], (0, 1, 0, 1), None, None, None),
    "zonal_spectra": lambda: spectra.zonal([], TABLE, None, [0], [(0, 1)], None, None, None),
    "breed_norms": lambda: breeding.norms(STATE, [], TABLE, None, None, None),
}


@pytest.mark.parametrize("what", list(_NO_MEMBERS))
def test_every_product_refuses_no_members_under_its_own_name(what):
    lo = 2 if what == "gram" else 1
    with pytest.raises(ValueError, match=rf"^{what}: 0 members; {lo} to 64 are supported$"):
        _NO_MEMBERS[what]()
