"""Which engine, tile and K slices every contraction of the models gets, and how much workspace the split-K slabs take, pinned
against tests/golden/igemm_dispatch.json -- recorded from the commit before csrc/igemm_dispatch.cpp took over launch_igemm (see
tests/golden/make_golden_dispatch.py for the cases).  The profile's detail row names carry the engine, the tile, the slices and
the problem shape, so equal {name: launches} maps mean the same decisions and the same launch counts."""
import json

import pytest

from tests.golden import make_golden_dispatch as MG

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def recorded():
    return MG.record_all()


def test_dispatch_matches_the_recorded_decisions(recorded):
    with open(MG.PATH) as f:
        want = json.load(f)
    assert sorted(recorded) == sorted(want)
    for case in sorted(want):
        got, ref = recorded[case], want[case]
        assert len(got["rows"]) < MG.ROW_CAP and len(ref["rows"]) < MG.ROW_CAP, case
        diff = {k: (ref["rows"].get(k), got["rows"].get(k)) for k in set(ref["rows"]) | set(got["rows"])
                if ref["rows"].get(k) != got["rows"].get(k)}
        assert not diff, "%s: rows (recorded, now) differ: %s" % (case, diff)
        assert got["workspace_bytes"] == ref["workspace_bytes"], case
