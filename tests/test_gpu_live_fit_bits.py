"""codd_ego_motion, codd_epipolar_check and codd_ground_plane share one statement of their fixed-order sums, Cholesky
solve, last-workgroup ticket and scratch layout (codd_amd/csrc/fit_sums.h), and reproduce, bit for bit, what the three
hand-built copies of the PARENT commit produced on the launches of tests/live_fit_cases.py: tests/golden/live_fit_bits.json
holds sha256 of the bytes of each output tensor -- the record, and every map, label plane and grid separately
(tools/parent_bits.py --cases live_fit wrote it on the GPU with that library).  A key missing from the fixture, or one the
fixture has and the tree does not, fails (tests/test_parent_bits.py, which needs no GPU)."""
import pytest

import live_fit_cases as FC
import parent_bits as P

pytestmark = pytest.mark.gpu
FIXTURE = P.load(FC.NAME)
GOLD = FIXTURE["sha256"]
GROUPS = FC.groups()


def test_fixture_is_from_another_commit():
    """parent_bits.assert_from_another_commit states the rule."""
    P.assert_from_another_commit(FIXTURE, FC.SOURCES)


@pytest.fixture(autouse=True)
def _no_autotune():
    from codd_amd import ops
    ops.enable_autotune(False)
    yield


@pytest.mark.parametrize("group", GROUPS, ids=[g[0] for g in GROUPS])
def test_launches_keep_the_parents_bits(group):
    _, keys, run = group
    got = run()
    assert list(got) == keys
    bad = P.changed(got, GOLD, keys)
    assert not bad, ("%d of %d output tensors changed bits" % (len(bad), len(keys)), bad)
