#!/usr/bin/env python
"""dev (GPU box): write tests/golden/convb_epilogue_bits.json -- sha256 of the bytes written by the launches of
tests/convb_epilogue_cases.py (the epilogues of the split-bf16 convolution kernel on every instantiated wave grid, operand
format and tile kind), produced by the library this process loads, with the commit that library was built from:

    CODD_LIB_AB=ab/libcodd_hip_parent.so python tools/convb_epilogue_bits.py --commit <id> --out /tmp/convb_epilogue_bits.json

The fixture is made ONCE with the library of the commit BEFORE the record epilogue batched its operand loads;
tests/test_gpu_convb_epilogue_bits.py then holds the in-tree library to those bits.
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
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "convb_epilogue_bits.json"))
    ap.add_argument("--stub", action="store_true")
    a = ap.parse_args()
    import convb_epilogue_cases as BC
    if a.stub:
        digests = {k: "stub" for k in BC.all_keys()}
        lib = "stub"
    else:
        from codd_amd import _abi
        _abi.load()
        lib = os.path.relpath(_abi.LOADED, ROOT)
        digests = BC.case_digests()
    keys = BC.all_keys()
    assert list(digests) == keys and len(set(keys)) == len(keys), "key list"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"library_commit": a.commit, "library": lib, "sha256": digests}, f, indent=0, sort_keys=False)
        f.write("\n")
    print("%d digests of %s at %s -> %s" % (len(digests), lib, a.commit, a.out))


if __name__ == "__main__":
    main()
