"""codd_ingest_pair, codd_ingest_frames and codd_ingest_calibrated run ONE kernel body (ingest_kernel, ingest.hip) with
one pinned bilinear blend, and reproduce, bit for bit, what the three kernels of the PARENT commit produced on the launches
of tests/ingest_cases.py -- every launch whose arithmetic is exact (map-free, identity and 1/64-pixel maps, the view
without calibration of the fused entry) plus codd_rectify_maps: tests/golden/ingest_bits.json holds sha256 of the bytes of
each output view (tools/parent_bits.py --cases ingest wrote it on the GPU with that library).  A key missing
from the fixture, or one the fixture has and the tree does not, fails (tests/test_ingest_cases.py, which needs no GPU)."""
import pytest

import ingest_cases as IC
import parent_bits as P

pytestmark = pytest.mark.gpu
FIXTURE = P.load(IC.NAME)
GOLD = FIXTURE["sha256"]
GROUPS = IC.groups()


def test_fixture_is_from_another_commit():
    """parent_bits.assert_from_another_commit states the rule."""
    P.assert_from_another_commit(FIXTURE, IC.SOURCES)


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
    assert not bad, ("%d of %d output views changed bits" % (len(bad), len(keys)), bad)
