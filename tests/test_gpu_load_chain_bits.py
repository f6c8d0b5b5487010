"""instnorm_stats / instnorm_apply / instnorm_apply_xs, se3_gn_solve and splat_gather request their loads in batches (several
in flight before the first wait, clamped addresses and selects in place of branches around loads) and reproduce, bit for
bit, what the library of the PARENT commit produced on the launches of tests/load_chain_cases.py:
tests/golden/load_chain_bits.json holds sha256 of the output bytes per launch (tools/parent_bits.py wrote it on the GPU
with that library).  A key missing from the fixture, or one the fixture has and the tree does not, fails
(tests/test_load_chain_cases.py, which needs no GPU)."""
import pytest

import load_chain_cases as LC
import parent_bits as P

pytestmark = pytest.mark.gpu
FIXTURE = P.load(LC.NAME)
GOLD = FIXTURE["sha256"]
GROUPS = LC.groups()


def test_fixture_is_from_another_commit():
    """parent_bits.assert_from_another_commit states the rule."""
    P.assert_from_another_commit(FIXTURE, LC.SOURCES)


@pytest.mark.parametrize("group", GROUPS, ids=[g[0] for g in GROUPS])
def test_launches_keep_the_parents_bits(group):
    _, keys, run = group
    got = run()
    assert list(got) == keys
    bad = P.changed(got, GOLD, keys)
    assert not bad, ("%d of %d launches changed bits" % (len(bad), len(keys)), bad)
