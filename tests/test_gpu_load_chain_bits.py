"""instnorm_stats / instnorm_apply / instnorm_apply_xs, se3_gn_solve and splat_gather request their loads in batches (several
in flight before the first wait, clamped addresses and selects in place of branches around loads) and reproduce, bit for
bit, what the library of the PARENT commit produced on the launches of tests/load_chain_cases.py:
tests/golden/load_chain_bits.json holds sha256 of the output bytes per launch (tools/load_chain_bits.py wrote it on the GPU
with that library).  A key missing from the fixture, or one the fixture has and the tree does not, fails
(tests/test_load_chain_cases.py, which needs no GPU)."""
import json
import os
import re
import subprocess

import pytest

import load_chain_cases as LC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = json.load(open(os.path.join(ROOT, "tests", "golden", "load_chain_bits.json")))
GOLD = FIXTURE["sha256"]
GROUPS = LC.groups()


def _git(*args):
    try:
        return subprocess.run(("git", "-C", ROOT) + args, capture_output=True, text=True, timeout=30)
    except (OSError, subprocess.TimeoutExpired):
        return None


def test_fixture_is_from_another_commit():
    """The digests were not made by the library under test (the rule of test_gpu_conv_epilogue_vec_bits.py): the fixture
    names a commit other than HEAD, or, in a work tree whose HEAD is still that commit, a motion.hip that differs from it."""
    commit = FIXTURE["library_commit"]
    assert re.fullmatch(r"[0-9a-f]{40}", commit), commit
    head = _git("rev-parse", "HEAD")
    if head is not None and head.returncode == 0 and head.stdout.strip() == commit:
        diff = _git("diff", "--quiet", commit, "--", "codd_amd/csrc/motion.hip")
        assert diff is not None and diff.returncode == 1, "the fixture was made by the library of this very commit"
    assert all(re.fullmatch(r"[0-9a-f]{64}", v) for v in GOLD.values())


@pytest.mark.parametrize("group", GROUPS, ids=[g[0] for g in GROUPS])
def test_launches_keep_the_parents_bits(group):
    _, keys, run = group
    got = run()
    assert list(got) == keys
    bad = [k for k in keys if got[k] != GOLD[k]]
    assert not bad, ("%d of %d launches changed bits" % (len(bad), len(keys)), bad)
