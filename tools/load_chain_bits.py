#!/usr/bin/env python
"""dev (GPU box): write a parent-bits fixture tests/golden/<name>_bits.json -- sha256 of the output bytes of the launches
of a case module tests/<name>_cases.py (its groups() / all_keys() / all_digests()), produced by the library this process
loads, with the commit that library was built from:

    CODD_LIB_AB=ab/libcodd_hip_parent.so python tools/load_chain_bits.py --commit <id> --out /tmp/load_chain_bits.json
    CODD_LIB_AB=ab/libcodd_hip_parent.so python tools/load_chain_bits.py --cases ingest_cases --commit <id>

A fixture is made ONCE with the library of the commit BEFORE the change it fences: load_chain_cases (the default; instance
norm, Gauss-Newton step, splat) before the loads of instnorm_stats / instnorm_apply / instnorm_apply_xs / se3_gn_solve /
splat_gather were re-ordered, held by tests/test_gpu_load_chain_bits.py; ingest_cases (the live-session ingest entries
and codd_rectify_maps) before the three ingest kernels became one, held by tests/test_gpu_ingest_bits.py.
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
    ap.add_argument("--cases", default="load_chain_cases", metavar="MODULE", help="case module under tests/ (<name>_cases)")
    ap.add_argument("--out", default=None, help="default: tests/golden/<name>_bits.json")
    ap.add_argument("--stub", action="store_true")
    a = ap.parse_args()
    import importlib
    assert a.cases.endswith("_cases"), a.cases
    LC = importlib.import_module(a.cases)
    a.out = a.out or os.path.join(ROOT, "tests", "golden", a.cases[:-len("_cases")] + "_bits.json")
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
