#!/usr/bin/env python
"""dev (GPU box): write a parent-bits fixture tests/golden/<name>_bits.json -- sha256 of the output bytes of the launches
of the case module tests/<name>_cases.py, produced by the library this process loads, with the commit that library was
built from:

    CODD_LIB_AB=ab/libcodd_hip_parent.so python tools/parent_bits.py --cases <name> --commit <id> [--out PATH]

This is how a same-bits change is fenced.  The fixture is made ONCE, with the library of the commit BEFORE the change
(built apart and loaded through CODD_LIB_AB), never with the library of the tree that holds it: a test
tests/test_gpu_<name>_bits.py then holds the in-tree library to those digests, and parent_bits.assert_from_another_commit
(tests/parent_bits.py) refuses a fixture that names the commit under test.  <name>: conv_epilogue, conv_epilogue_vec,
convb_epilogue, load_chain, ingest, live_fit, and conv_plan -- host decisions, not output bytes: no GPU, run in a checkout of the parent
commit with the case module copied in; a new fence adds its case module (NAME, SOURCES, groups()), its fixture and its test.
    --stub   no GPU: enumerate the keys only (every digest "stub"); the key list must not depend on the library."""
import argparse
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", required=True, metavar="NAME", help="the case module tests/<NAME>_cases.py")
    ap.add_argument("--commit", required=True, help="commit id of the sources the loaded library was built from")
    ap.add_argument("--out", default=None, help="default: tests/golden/<NAME>_bits.json")
    ap.add_argument("--stub", action="store_true")
    a = ap.parse_args()
    import parent_bits as P  # (tests/parent_bits.py: this file runs as __main__)
    cases = importlib.import_module(a.cases + "_cases")
    assert cases.NAME == a.cases, (cases.NAME, a.cases)
    a.out = a.out or os.path.join(ROOT, "tests", "golden", cases.NAME + "_bits.json")
    keys = P.all_keys(cases)
    if a.stub:
        digests = {k: "stub" for k in keys}
        lib = "stub"
    else:
        from codd_amd import _abi
        _abi.load()
        lib = os.path.relpath(_abi.LOADED, ROOT)
        digests = P.all_digests(cases, lambda gid, got: print("%-44s %4d digests" % (gid, len(got)), flush=True))
    assert list(digests) == keys and len(set(keys)) == len(keys), "key list"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"library_commit": a.commit, "library": lib, "sha256": digests}, f, indent=0, sort_keys=False)
        f.write("\n")
    print("%d digests (%d groups) of %s at %s -> %s" % (len(digests), len(cases.groups()), lib, a.commit, a.out))


if __name__ == "__main__":
    main()
