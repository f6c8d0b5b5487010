#!/usr/bin/env python
"""dev (GPU box): write tests/golden/load_chain_bits.json -- sha256 of the output bytes of the launches of
tests/load_chain_cases.py (instance norm, Gauss-Newton step, splat), produced by the library this process loads, with
the commit that library was built from:

    CODD_LIB_AB=ab/libcodd_hip_parent.so python tools/load_chain_bits.py --commit <id> --out /tmp/load_chain_bits.json

The fixture is made ONCE with the library of the commit BEFORE the loads of instnorm_stats / instnorm_apply /
instnorm_apply_xs / se3_gn_solve / splat_gather were re-ordered; tests/test_gpu_load_chain_bits.py then holds the in-tree
library to those bits.
    --stub   no GPU: enumerate the keys only (every digest "stub"); the key list must not depend on the library."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="commit id of the sources the loaded library was built from")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "load_chain_bits.json"))
    ap.add_argument("--stub", action="store_true")
    a = ap.parse_args()
    import load_chain_cases as LC
    if a.stub:
        digests = {k: "stub" for k in LC.all_keys()}
        lib = "stub"
    else:
        from codd_amd import _abi
        _abi.load()
        lib = os.path.relpath(_abi.LOADED, ROOT)
        digests = LC.all_digests()
    keys = LC.all_keys()
    assert list(digests) == keys and len(set(keys)) == len(keys), "key list"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"library_commit": a.commit, "library": lib, "sha256": digests}, f, indent=0, sort_keys=False)
        f.write("\n")
    print("%d digests (%d groups) of %s at %s -> %s" % (len(digests), len(LC.groups()), lib, a.commit, a.out))


if __name__ == "__main__":
    main()
