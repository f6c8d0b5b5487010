"""No GPU needed.  The convolution launch planner (codd_amd/ops.py: _conv_cfg, the candidate lists of _autotune and
_bf16_candidates as the library's dry run filters them, _small_footprint, _split_dims, _split_rows) decides what the planner
of the PARENT commit decided: tests/golden/conv_plan_bits.json holds one sha256 per signature of the shipped tune db, per
layer of a hand grid the db does not hold, and one for _split_rows (tests/conv_plan_cases.py says what each hashes;
tools/parent_bits.py --cases conv_plan made the fixture in a checkout of that commit, with its library)."""
import conv_plan_cases as CP
import parent_bits as P

FIXTURE = P.load(CP.NAME)


def test_fixture_is_from_another_commit_and_names_every_case():
    P.assert_from_another_commit(FIXTURE, CP.SOURCES)
    P.assert_keys(FIXTURE, P.all_keys(CP))
    assert len(FIXTURE["sha256"]) > 1200


def test_planner_decides_what_the_parent_decided():
    keys = P.all_keys(CP)
    bad = P.changed(P.all_digests(CP), FIXTURE["sha256"], keys)
    assert not bad, ("%d of %d decisions changed" % (len(bad), len(keys)), bad[:8])
