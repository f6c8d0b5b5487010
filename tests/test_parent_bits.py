"""No GPU needed: every parent-bits fixture under tests/golden names exactly the launches of its case module, in their
order (tests/parent_bits.py; tools/parent_bits.py writes the fixtures)."""
import importlib

import pytest

import parent_bits as P

NAMES = ("conv_epilogue", "conv_epilogue_vec", "convb_epilogue", "load_chain", "ingest", "conv_plan", "live_fit")


@pytest.mark.parametrize("name", NAMES)
def test_fixture_keys_are_the_case_list(name):
    cases = importlib.import_module(name + "_cases")
    assert cases.NAME == name and cases.SOURCES
    groups = cases.groups()
    assert len({gid for (gid, _, _) in groups}) == len(groups)
    assert all(keys and callable(run) for (_, keys, run) in groups)
    P.assert_keys(P.load(name), P.all_keys(cases))
