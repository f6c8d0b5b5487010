#!/usr/bin/env python
"""dev (GPU box): write tests/golden/conv_epilogue_bits.json -- sha256 of the output bytes of every exact-fp32 entry of
the shipped-configuration sweep, of one four-job multi launch and of the hand-made cases of tests/conv_epilogue_cases.py,
produced by the library this process loads, with the commit that library was built from:

    CODD_LIB_AB=ab/libcodd_hip_parent.so python tools/conv_epilogue_bits.py --commit <id> --out /tmp/conv_epilogue_bits.json

The fixture is made ONCE with the library of the commit BEFORE a change of the fp32 convolution epilogue;
tests/test_gpu_conv_epilogue_bits.py then holds the in-tree library to those bits.
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
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "conv_epilogue_bits.json"))
    ap.add_argument("--stub", action="store_true")
    a = ap.parse_args()
    import conv_epilogue_cases as E
    digests = {}
    if a.stub:
        digests = {k: "stub" for k in E.all_keys()}
        lib = "stub"
    else:
        import test_gpu_conv_fp64 as T  # the launch of the sweep and of the multi jobs is the test file's own
        from codd_amd import _abi
        _abi.load()
        lib = os.path.relpath(_abi.LOADED, ROOT)
        for L, items in E.sweep_entries().items():
            for (key, e, geom, act, operands) in items:
                digests[key] = E.sweep_digest(T, e, geom, act, operands)
            print("%-40s %3d entries" % (E.V.layer_id(L), len(items)), flush=True)
        digests.update(E.multi_digests(T))
        digests.update(E.hand_digests())
    keys = E.all_keys()
    assert list(digests) == keys and len(set(keys)) == len(keys), "key list"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"library_commit": a.commit, "library": lib, "sha256": digests}, f, indent=0, sort_keys=False)
        f.write("\n")
    print("%d digests (%d sweep, %d multi, %d hand) of %s at %s -> %s" % (
        len(digests), len(keys) - len(E.multi_keys()) - len(E.hand_keys()), len(E.multi_keys()), len(E.hand_keys()), lib,
        a.commit, a.out))


if __name__ == "__main__":
    main()
