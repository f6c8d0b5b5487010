"""codd_ingest_pair, codd_ingest_frames and codd_ingest_calibrated run ONE kernel body (ingest_kernel, ingest.hip) with
one pinned bilinear blend, and reproduce, bit for bit, what the three kernels of the PARENT commit produced on the launches
of tests/ingest_cases.py -- every launch whose arithmetic is exact (map-free, identity and 1/64-pixel maps, the view
without calibration of the fused entry) plus codd_rectify_maps: tests/golden/ingest_bits.json holds sha256 of the bytes of
each output view (tools/load_chain_bits.py --cases ingest_cases wrote it on the GPU with that library).  A key missing
from the fixture, or one the fixture has and the tree does not, fails (tests/test_ingest_cases.py, which needs no GPU)."""
import json
import os
import re
import subprocess

import pytest

import ingest_cases as IC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = json.load(open(os.path.join(ROOT, "tests", "golden", "ingest_bits.json")))
GOLD = FIXTURE["sha256"]
GROUPS = IC.groups()
# the sources of the ingest entries, in the parent's tree and in this one
SOURCES = ("codd_amd/csrc/live.hip", "codd_amd/csrc/ingest_decode.h", "codd_amd/csrc/ingest_formats.hip",
           "codd_amd/csrc/ingest_calib.hip", "codd_amd/csrc/ingest.hip")


def _git(*args):
    try:
        return subprocess.run(("git", "-C", ROOT) + args, capture_output=True, text=True, timeout=30)
    except (OSError, subprocess.TimeoutExpired):
        return None


def test_fixture_is_from_another_commit():
    """The digests were not made by the library under test (the rule of test_gpu_load_chain_bits.py): the fixture names a
    commit other than HEAD, or, in a work tree whose HEAD is still that commit, ingest sources that differ from it."""
    commit = FIXTURE["library_commit"]
    assert re.fullmatch(r"[0-9a-f]{40}", commit), commit
    head = _git("rev-parse", "HEAD")
    if head is not None and head.returncode == 0 and head.stdout.strip() == commit:
        diff = _git("diff", "--quiet", commit, "--", *SOURCES)
        assert diff is not None and diff.returncode == 1, "the fixture was made by the library of this very commit"
    assert all(re.fullmatch(r"[0-9a-f]{64}", v) for v in GOLD.values())


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
    bad = [k for k in keys if got[k] != GOLD[k]]
    assert not bad, ("%d of %d output views changed bits" % (len(bad), len(keys)), bad)
